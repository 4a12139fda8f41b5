"""The id space of ``yxh_conv_desc.tile`` (tile code = 2 * id + low bit).

A static mirror of the family table in csrc/conv_tiles.hpp, importable without the
library; tests/test_conv_tiles.py checks it row by row against yxh_conv_tile_family.
The tuners' candidate lists (engine.py, train.py) are built from the names below.
``yxh_wgrad_desc.tile`` is a separate id space and is not described here.
"""
from __future__ import annotations

from typing import Iterable, NamedTuple, Optional

# flags of a row (YXH_TILE_* in include/yoloxhip.h)
BIT_SLABS = 1    # the code's low bit selects two 64-byte K slabs per stage
BIT_V16 = 2      # the code's low bit asks for conv_ws1's 16-byte-store epilogue
POST = 4         # runs a conv with a 1x1 post conv (post_weight)
GROUPS2 = 8      # runs YXH_CONV_GROUPS2
PRE = 16         # a pre_weight conv is handed to the family (only ws_fused runs one)
NO_DILATED = 32  # refuses zero-dilated (upsample == 2) sources


class Family(NamedTuple):
    name: str
    first: int
    count: int
    flags: int

    @property
    def ids(self) -> range:
        return range(self.first, self.first + self.count)


FAMILIES = (
    Family("igemm", 1, 9, BIT_SLABS),
    Family("glds", 17, 9, BIT_SLABS | NO_DILATED),
    Family("rows", 33, 19, BIT_SLABS | NO_DILATED),
    Family("pw", 65, 6, BIT_SLABS | NO_DILATED),
    Family("pwr", 81, 2, NO_DILATED),
    Family("pwf", 97, 8, NO_DILATED),
    Family("r3", 113, 48, NO_DILATED),
    Family("ws", 161, 30, GROUPS2 | NO_DILATED),
    Family("ws_fused", 191, 6, PRE | NO_DILATED),
    Family("ws1", 201, 10, BIT_V16 | PRE | NO_DILATED),
    Family("pw1f", 211, 4, PRE | NO_DILATED),
    Family("dgrad_s2", 215, 6, PRE),
    Family("ws_post", 221, 16, POST | PRE),
    Family("ws1_deep", 241, 18, BIT_V16 | PRE),
    Family("ws_wide", 261, 29, PRE),
)
(IGEMM, GLDS, ROWS, PW, PWR, PWF, R3, WS, WS_FUSED, WS1, PW1F, DGRAD_S2, WS_POST, WS1_DEEP, WS_WIDE) = FAMILIES

# Sub-ranges the tuners pick, each relative to its row
R3_BUILT = R3.ids[:40]  # the rest of the row is reserved: conv_r3's own dispatch refuses those ids
R3H_F32 = tuple(R3.first + local - 1 for local in (29, 30, 31, 32, 33, 38, 39, 40))  # conv_r3h ids built for fp32
DGRAD_S2_F32, DGRAD_S2_16 = DGRAD_S2.ids[:2], DGRAD_S2.ids[2:]  # dgrad_s2f / dgrad_s2h
# ws_wide: yolox_x / yolox_l widths, then the forms that accumulate an fp32 data gradient and the
# training step's stem conv -- inference has no use for the last two groups
WS_WIDE_16, WS_WIDE_F32GRAD, WS_WIDE_STEM = WS_WIDE.ids[:20], WS_WIDE.ids[20:28], WS_WIDE.ids[28:]


def code(tile_id: int, bit: int = 0) -> int:
    return 2 * tile_id + bit


def codes(ids: Iterable[int], bits: Iterable[int] = (0,)) -> list:
    """Tile codes of ``ids`` in order, each id with every low bit of ``bits``."""
    bits = tuple(bits)
    return [code(i, b) for i in ids for b in bits]


def family_of(tile_code: int) -> Optional[Family]:
    """The row that holds this code's id, or None for an id in a gap."""
    tile_id = tile_code >> 1
    return next((f for f in FAMILIES if f.first <= tile_id < f.first + f.count), None)
