from .losses import IouLoss  # noqa: F401
from .network import (BaseConv, Bottleneck, CspDarknet, CspLayer, Darknet, DWConv, Focus,  # noqa: F401
                      ResLayer, SPPBottleneck, YoloFpn, YoloPafpn, YoloxHead)
from .processor import Detections, YoloxProcessor  # noqa: F401
from .yolox import Yolox, YoloxModule  # noqa: F401
