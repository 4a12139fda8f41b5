// Weight gradient of Conv2d (yxh_conv_wgrad): what the six kernel families and their router
// (wgrad.hip) share.
//   dW[n][c][ky][kx] = sum over output pixels of dY[n] * X[c](tap) on MFMA, split-K over pixel
//   ranges.  Each split stores its partial dW into the workspace and wgrad_reduce sums the splits
//   in a fixed order (deterministic); without a workspace the partials go out as fp32 atomics
//   into a pre-zeroed dW.
#pragma once

#include "conv_common.hpp"

namespace yxh {

struct WgradParams {
    int in_h, in_w, out_h, out_w, cin, cout, kh, kw, stride, pad, ohw, M;
    int nsrc, src0_ch, B;
    const void* sptr[2];
    int scs[2], sw[2], sup[2];
    long long sbs[2];
    const void* dy;
    int dycs;
    long long dybs;
    float* dw;
    int cin_store;
    int sps, nst;  // stages per split, total pixel stages
    int ntc;       // channel tiles per tap
    int dych;      // channels of the dy view (loads past them read the zero chunk)
    float* ws;     // per-split partial dW (yxh_wgrad_desc.workspace), or null: atomics
    long long ws_elems;
};

// ------------------------------------------------------------------ split-K planning
// A family cuts `units` of K work (stages or pixel tiles) into equal splits for each of its `tiles`
// output tiles.  It wants about target_blocks blocks over the grid; it gets fewer where a split
// would hold less than min_units_per_split, or where the splits' partials would not fit the
// workspace (ws_capacity_in_splits; <= 0: no workspace, no cap).  The count is then re-divided so no
// split is empty.
struct SplitPlan {
    long long splits;
    int per_split;
};

constexpr SplitPlan plan_splits(long long units, long long tiles, long long target_blocks, int min_units_per_split,
                                long long ws_capacity_in_splits) {
    long long splits = (target_blocks + tiles - 1) / tiles;
    const long long max_splits = (units + min_units_per_split - 1) / min_units_per_split;
    if (splits > max_splits) splits = max_splits;
    if (ws_capacity_in_splits > 0 && splits > ws_capacity_in_splits) splits = ws_capacity_in_splits;
    if (splits < 1) splits = 1;
    const int per_split = (int)((units + splits - 1) / splits);
    return {(units + per_split - 1) / per_split, per_split};
}

// Floats of partials a launcher spends at most: 16 MiB, beyond which writing and summing the
// partials cost more than the extra blocks gain.  The nine-tap 16-bit tiles (25-30) hold all nine
// taps per split and take 64 MiB, or wide 3x3s get ~100 blocks.
constexpr long long kWsCapElems = 4LL << 20, kWsCapElemsNine16 = 16LL << 20;

// Splits whose partial dW (ne floats each) fit the workspace and the launcher's cap
constexpr long long ws_capacity(long long ws_elems, long long cap_elems, long long ne) {
    return (ws_elems < cap_elems ? ws_elems : cap_elems) / ne;
}

constexpr bool plan_is(SplitPlan s, long long splits, int per_split) {
    return s.splits == splits && s.per_split == per_split;
}
// One case per binding clamp, worked from the formulas the launchers each carried before they shared
// this one (default target 512):
// the floor: tile 1 bf16, 64 -> 64 3x3, B 2, 16x16 out: 4 stages, 9 tiles; wanted 57, 8 per split allow 1
static_assert(plan_is(plan_splits(4, 9, 512, 8, 0), 1, 4), "work-per-split floor");
// the target: tile 17, 128 -> 128 3x3 s1, B 4, 40x40, 32 MiB workspace: 200 stages, 36 tiles; wanted 15,
// the floor allows 50, the cap 4 Mi / 147 456 = 28
static_assert(ws_capacity(8LL << 20, kWsCapElems, 147456) == 28, "partials cap");
static_assert(plan_is(plan_splits(200, 36, 512, 4, 28), 15, 14), "target");
// the cap: the same conv with room for 10 partials
static_assert(plan_is(plan_splits(200, 36, 512, 4, 10), 10, 20), "partials cap");
// the re-division: 20 pixel tiles, 64 output tiles, 2 per split: wanted 8 -> 3 per split -> 7 splits
static_assert(plan_is(plan_splits(20, 64, 512, 2, 0), 7, 3), "re-division");
// a workspace below one partial: no cap (and ws_cap_splits clears p.ws: atomics)
static_assert(ws_capacity(1000, kWsCapElems, 147456) == 0, "no room for one split");
static_assert(plan_is(plan_splits(200, 36, 512, 4, 0), 15, 14), "no cap without a workspace");

// The workspace's capacity in splits for plan_splits; p.ws is cleared when not even one split fits.
inline long long ws_cap_splits(WgradParams& p, long long cap_elems) {
    if (!p.ws) return 0;
    const long long cap = ws_capacity(p.ws_elems, cap_elems, (long long)p.cout * p.cin_store * p.kh * p.kw);
    if (cap < 1) p.ws = nullptr;
    return cap;
}

inline SplitPlan plan_wgrad(WgradParams& p, long long units, long long tiles, long long target_blocks,
                            int min_units_per_split, long long cap_elems = kWsCapElems) {
    return plan_splits(units, tiles, target_blocks, min_units_per_split, ws_cap_splits(p, cap_elems));
}

// Blocks a weight-gradient grid aims for (splits x tiles): YXH_WGRAD_BLOCKS, default 512 = two per CU
int wgrad_target_blocks();

// dW += the splits' partials, summed in split order (deterministic); nothing to do without p.ws
int ws_reduce(const WgradParams& p, long long splits, hipStream_t st);

// ------------------------------------------------------------------ families
// One dispatch per kernel family, called by the router (wgrad.hip kWgradFamilies) with the public
// tile id after it has checked the row's operand types and 3x3 constraint.
int wgrad_reg_dispatch(int dtype, int tile, const WgradParams& p, hipStream_t st);          // 1-4
int wgrad_glds_dispatch(int dtype, int tile, const WgradParams& p, hipStream_t st);         // 5-10
int wgrad9_f32_dispatch(int dtype, int tile, const WgradParams& p, hipStream_t st);         // 11-16
int wgrad_kmajor_dispatch(int dtype, int tile, const WgradParams& p, hipStream_t st);       // 17-20
int wgrad9_kmajor_dispatch(int dtype, int tile, const WgradParams& p, hipStream_t st);      // 21-24
int wgrad9t_h_dispatch(int dtype, int tile, const WgradParams& p, hipStream_t st);          // 25-30

}  // namespace yxh
