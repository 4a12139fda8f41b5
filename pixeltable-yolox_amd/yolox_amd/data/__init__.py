"""Training data on device (reference yolox/data): the mosaic / mixup / affine / HSV / mirror
sample pipeline over dataset images in HBM -- all of them (``ResidentImages``) or a bounded
pool filled on demand (``StreamedImages``) -- and the COCO-format reader that feeds it from
disk (``CocoDataset``: the annotation JSON and PIL, no pycocotools or cv2).  This directory also
holds the BN calibration statistics (bn_stats_*.npz) the planner's synthetic weights use."""
from .coco import CocoDataset
from .mosaic import (AugParams, GpuMosaicDetection, MosaicBatches, ResidentImages, SyntheticDetectionDataset,
                     TrainTransform)
from .streamed import SlotTable, StreamedImages

MosaicDetection = GpuMosaicDetection  # the reference's name (datasets/mosaicdetection.py:35)

__all__ = ["AugParams", "CocoDataset", "GpuMosaicDetection", "MosaicDetection", "MosaicBatches", "ResidentImages",
           "SlotTable", "StreamedImages", "SyntheticDetectionDataset", "TrainTransform"]
