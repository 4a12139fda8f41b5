// The id space of yxh_conv_desc.tile (tile code = 2 * id + low bit): one row per contiguous range of
// public ids, sorted by `first`.  conv2d (conv.hip) validates, constrains and routes a code through this
// table alone; yxh_conv_tile_family reports it and yolox_amd/tiles.py mirrors it (tests/test_conv_tiles.py
// holds the two together).  A new family is one row here and one in tiles.py.
#pragma once

#include "yxh_common.hpp"

namespace yxh {

struct ConvParams;  // conv_common.hpp

// Each family's dispatch; `id` is the family's own numbering (the switch table in its file)
int conv_igemm_dispatch(int dtype, int id, const ConvParams& p, int ks, hipStream_t st);  // conv.hip
// conv_igemm's tiles on the LDS-DMA loader (conv_glds.hip)
int conv_glds_dispatch(int dtype, int id, const ConvParams& p, int ks, hipStream_t st);
// Row-tiled 3x3 conv (conv_rows.hip): 2D output tiles, kx taps share one LDS row image
int conv_rows_dispatch(int dtype, int id, const ConvParams& p, int ks, hipStream_t st);
// Persistent streaming 1x1 conv (conv_pw.hip)
int conv_pw_dispatch(int dtype, int id, const ConvParams& p, int ks, hipStream_t st);
// Register-operand 1x1 conv (conv_pwr.hip)
int conv_pwr_dispatch(int dtype, int id, const ConvParams& p, hipStream_t st);
// VALU-free-loop dense 1x1 conv (conv_pwf.hip)
int conv_pwf_dispatch(int dtype, int id, const ConvParams& p, hipStream_t st);
// 3x3 conv with the branch-free buffer-LDS loader (conv_r3.hip)
int conv_r3_dispatch(int dtype, int id, const ConvParams& p, hipStream_t st);
// Weight-stationary persistent 3x3 conv (conv_ws.hip): ids 1-30 plain, 31-36 fused Bottleneck
// (pre_weight), 41-56 with a 1x1 post conv (post_weight), 61-89 wide input channels
int conv_ws_dispatch(int dtype, int id, const ConvParams& p, hipStream_t st);
// Weight-stationary persistent 1x1 conv over dense sources (conv_ws1.hip): ids 1-10, and 11-28 the deep
// row pipelines (19-22, 26: upsampled source 0; 23-28: full-width)
int conv_ws1_dispatch(int dtype, int id, const ConvParams& p, hipStream_t st);
// fp32 1x1 GEMM for the training path, k-minor MFMA operands (conv_pw1f.hip)
int conv_pw1f_dispatch(int dtype, int id, const ConvParams& p, hipStream_t st);
// Data gradient of a 3x3 s2 conv by output parity class (conv_pw1f.hip): ids 1-2 fp32 (dgrad_s2f),
// 3-6 16-bit (dgrad_s2h)
int dgrad_s2f_dispatch(int dtype, int id, const ConvParams& p, hipStream_t st);

// ... behind one signature: the families that take no slab count drop it
using TileDispatch = int (*)(int dtype, int id, const ConvParams& p, int ks, hipStream_t st);
template <int (*F)(int, int, const ConvParams&, hipStream_t)>
int no_ks(int dtype, int id, const ConvParams& p, int, hipStream_t st) { return F(dtype, id, p, st); }

struct TileFamily {
    const char* name;
    int first, count;  // public ids first .. first + count - 1
    int local_first;   // the id the family's dispatch expects for `first`
    TileDispatch fn;
    int flags;         // YXH_TILE_* (yoloxhip.h)
    constexpr int last() const { return first + count - 1; }
};

// Ids a family has withdrawn or not built yet (ws 9, 10, 37-40; ws_post 57-60; ws_wide 70, 73, 75, 77, 78;
// r3 beyond the built ones) stay inside their row and are refused by the family's own switch.
// YXH_TILE_PRE is set where conv2d hands a pre_weight conv on: only ws_fused runs one, the later rows
// refuse it in their own dispatch.  YXH_TILE_NO_DILATED: every row from glds to pw1f.
constexpr TileFamily kTileFamilies[] = {
    {"igemm", 1, 9, 1, conv_igemm_dispatch, YXH_TILE_BIT_SLABS},
    {"glds", 17, 9, 1, conv_glds_dispatch, YXH_TILE_BIT_SLABS | YXH_TILE_NO_DILATED},
    {"rows", 33, 19, 1, conv_rows_dispatch, YXH_TILE_BIT_SLABS | YXH_TILE_NO_DILATED},
    {"pw", 65, 6, 1, conv_pw_dispatch, YXH_TILE_BIT_SLABS | YXH_TILE_NO_DILATED},
    {"pwr", 81, 2, 1, no_ks<conv_pwr_dispatch>, YXH_TILE_NO_DILATED},
    {"pwf", 97, 8, 1, no_ks<conv_pwf_dispatch>, YXH_TILE_NO_DILATED},
    {"r3", 113, 48, 1, no_ks<conv_r3_dispatch>, YXH_TILE_NO_DILATED},
    {"ws", 161, 30, 1, no_ks<conv_ws_dispatch>, YXH_TILE_GROUPS2 | YXH_TILE_NO_DILATED},
    {"ws_fused", 191, 6, 31, no_ks<conv_ws_dispatch>, YXH_TILE_PRE | YXH_TILE_NO_DILATED},
    {"ws1", 201, 10, 1, no_ks<conv_ws1_dispatch>, YXH_TILE_BIT_V16 | YXH_TILE_PRE | YXH_TILE_NO_DILATED},
    {"pw1f", 211, 4, 1, no_ks<conv_pw1f_dispatch>, YXH_TILE_PRE | YXH_TILE_NO_DILATED},
    {"dgrad_s2", 215, 6, 1, no_ks<dgrad_s2f_dispatch>, YXH_TILE_PRE},
    {"ws_post", 221, 16, 41, no_ks<conv_ws_dispatch>, YXH_TILE_POST | YXH_TILE_PRE},
    {"ws1_deep", 241, 18, 11, no_ks<conv_ws1_dispatch>, YXH_TILE_BIT_V16 | YXH_TILE_PRE},
    {"ws_wide", 261, 29, 61, no_ks<conv_ws_dispatch>, YXH_TILE_PRE},
};
constexpr int kNumTileFamilies = sizeof(kTileFamilies) / sizeof(kTileFamilies[0]);

constexpr const TileFamily* find_family(int id) {
    for (const TileFamily& f : kTileFamilies)
        if (id >= f.first && id <= f.last()) return &f;
    return nullptr;
}
// The first row that carries `flag`: the row a constraint's error text names
constexpr const TileFamily& family_with(int flag) {
    for (const TileFamily& f : kTileFamilies)
        if (f.flags & flag) return f;
    return kTileFamilies[0];
}
constexpr bool families_sorted() {
    for (int i = 1; i < kNumTileFamilies; ++i)
        if (kTileFamilies[i].first <= kTileFamilies[i - 1].last()) return false;
    return true;
}
static_assert(families_sorted(), "tile families must be sorted by first and disjoint");

// By-shape defaults of the conv_ws forms the heuristic cannot pick (tile == 0), as public ids
constexpr int kTileHeadForm = 231;                                          // GROUPS2 + the head's preds
constexpr int kTilePostStride2 = 225;                                       // s2 conv + conv1 | conv2
constexpr int kTilePostChain64 = 234, kTilePostChain128 = 235;              // Bottleneck chain (POST_STORE)
constexpr int kTilePost32 = 221, kTilePost64 = 223;                         // 3x3 + CspLayer.conv3
constexpr int kTileGroups2_128 = 185, kTileGroups2_256 = 176;               // a head level's two 3x3s
constexpr int kTileFused32 = 191, kTileFused64 = 194, kTileFused128 = 195;  // fused Bottleneck

}  // namespace yxh
