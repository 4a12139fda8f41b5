// head_pred2: the per-wave form of head.hip's head_pred (one head level's three 1x1 pred convs +
// cat + sigmoid + decode in one launch), for 1-80 classes and 64 / 96 / 128 / 192 / 256 / 320 feature
// channels.  One kernel per (dtype, CIN, NCF = ceil(C / 16), MODE); the instantiations of one width
// are compiled in head2_c<CIN>.hip so the build parallelises (head2_dispatch_t).
#pragma once
#include <algorithm>

#include "conv_common.hpp"

namespace yxh {

namespace {

// The fused head runs on the 16-bit inference path only (the fp32 parity path keeps the
// decode convs and their IEEE exp / divide): hardware exp2 + reciprocal (~1 ulp each), as
// the bf16 SiLU -- the per-element exp / divide sequences were most of this kernel's VALU.
__device__ __forceinline__ float hd_exp(float v) { return __builtin_amdgcn_exp2f(v * 1.4426950408889634f); }
__device__ __forceinline__ float hd_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.0f + hd_exp(-v)); }

}  // namespace

// head_pred2: every wave an independent worker over 16-pixel groups.  head_pred
// spent 68 % of its wave cycles waiting (profiles/r04/mfma_util_r4z.txt): each tile's
// feature loads were issued and waited for before any MFMA, and two barriers per tile
// serialised the block.  Here
//  * a wave's B operands come straight from global memory into registers (lane (r, q) of
//    step s: pixel r's channels 32 s + 8 q .. + 8 -- 64-byte segments of the pixel rows), the
//    NEXT group's loads issued before this group's MFMAs, so HBM latency hides behind a whole
//    group of work;
//  * the weights of all 1 + NCF output fragments live in VGPRs for the wave's life (one LDS copy per
//    block feeds them), the biases in LDS;
//  * the decoded [16][5 + C] rows go through a per-wave LDS slot and leave as 16-byte stores of
//    the contiguous output rows -- no block barrier after the prologue.
// Same MFMA order and decode arithmetic as head_pred: bit-identical output
// (tests/test_gpu_ops.py test_head_pred_fused_level, tests/test_gpu_head_classes.py run both).
// Fragment f's accumulator sees its K steps in order whatever NCF is, and nothing in the decode
// looks at another fragment: the first 5 + C columns of a C-class launch equal those of any wider
// launch whose weight rows start with the same C rows.
// MODE = yxh_head_desc.train, fixed per instantiation (0: eval decode, 1: training rows -- decoded boxes, raw
// obj / cls logits, 2: eval raw rows -- raw boxes, sigmoid obj / cls): the decode is branch-free (every lane
// evaluates its fragment-0 candidates and selects; 32-bit pixel / image arithmetic), where the runtime mode
// tests and per-lane branches had split it into exec-masked blocks with SGPR spills (round 6)
// 8 waves per block (two per SIMD, 256 registers each) up to 128 channels; 4 (one per SIMD, 512 registers) above:
// the (1 + NCF) x CIN / 32 weight fragments and the two groups of 2 x CIN / 32 feature operands of 4 registers
// each need 264 registers at 192 x 5 fragments, ~350 at 256 (yolox_l) and 400 at 320 (yolox_x)
constexpr int head2_waves(int cin) { return cin > 128 ? 4 : 8; }

template <typename T, int CIN, int NCF, int MODE>
__global__ __launch_bounds__(64 * head2_waves(CIN)) void head_pred2(yxh_head_desc d) {
    static_assert(CIN % 32 == 0 && NCF >= 1 && NCF <= 5 && MODE >= 0 && MODE <= 2, "head_pred2 shape");
    constexpr int NW = head2_waves(CIN);
    constexpr int KS = CIN / 32;                 // K steps
    constexpr int NF = 1 + NCF;                  // output fragments: reg|obj, then cls
    constexpr int WROWS = NF * 16;
    constexpr int WRB = CIN * 2 + 16;            // LDS weight row: +16 B (odd 16-B slots: conflict-free)
    constexpr int STGF = 16 * (5 + NCF * 16);    // per-wave staging floats (>= 16 rows of 5 + C)
    static_assert((WRB / 16) % 2 == 1, "head_pred2 weight rows: an odd number of 16-byte slots");
    // ~70 KB of LDS for CIN 128, 5 fragments: one block per CU on gfx950 (160 KiB), built for that target only
    static_assert(WROWS * WRB + WROWS * 4 + NW * STGF * 4 <= 160 * 1024, "head_pred2 LDS exceeds gfx950's 160 KiB");
    __shared__ __attribute__((aligned(16))) char wl[WROWS * WRB];
    __shared__ float bl[WROWS];
    __shared__ __attribute__((aligned(16))) float stg_all[NW][STGF];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fq = lane >> 4;
    const int C = d.num_classes, hw = d.h * d.w, rowf = 5 + C, W = d.w;
    const int M = d.batch * hw;  // < 2^31 (head_pred_launch)
    const int G = (M + 15) / 16;
    const int gstride = (int)gridDim.x * NW;
    int g = (int)blockIdx.x * NW + wave;
    // ---- weights / biases -> LDS (rows past 5 reg|obj and C cls rows are zero), then VGPRs
    for (int q = tid; q < WROWS * (CIN / 8); q += 64 * NW) {
        const int r = q / (CIN / 8), c = q - (CIN / 8) * (q / (CIN / 8));
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r < 5) v = *(const uint4*)((const T*)d.w_reg + (long long)r * CIN + c * 8);
        else if (r >= 16 && r - 16 < C) v = *(const uint4*)((const T*)d.w_cls + (long long)(r - 16) * CIN + c * 8);
        *(uint4*)(wl + r * WRB + c * 16) = v;
    }
    for (int q = tid; q < WROWS; q += 64 * NW)
        bl[q] = q < 5 ? d.b_reg[q] : (q >= 16 && q - 16 < C) ? d.b_cls[q - 16] : 0.0f;
    __syncthreads();
    uint4 wr[NF][KS];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int s = 0; s < KS; ++s) wr[f][s] = *(const uint4*)(wl + (f * 16 + frow) * WRB + (s * 4 + fq) * 16);
    if (g >= G) return;  // wave-uniform; no block barrier follows

    // B operands of group g: [0..KS) reg features, [KS..2KS) cls features of pixel 16 g + frow
    auto load_b = [&](int gg, uint4 (&b)[2 * KS]) {
        int m = gg * 16 + frow;
        m = m < M ? m : M - 1;
        const int bi = m / hw, pix = m - bi * hw;
        const T* pr = (const T*)d.reg.ptr + (long long)bi * d.reg.bstride + (long long)pix * d.reg.cstride + fq * 8;
        const T* pc = (const T*)d.cls.ptr + (long long)bi * d.cls.bstride + (long long)pix * d.cls.cstride + fq * 8;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            b[s] = *(const uint4*)(pr + s * 32);
            b[KS + s] = *(const uint4*)(pc + s * 32);
        }
    };
    float* stg = stg_all[wave];
    uint4 bc[2 * KS], bn[2 * KS];
    load_b(g, bc);
    const float st = d.stride;
    for (; g < G; g += gstride) {
        const bool more = g + gstride < G;
        if (more) load_b(g + gstride, bn);
        f32x4 acc[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int f = 0; f < NF; ++f) Mma<T>::run(acc[f], wr[f][s], f == 0 ? bc[s] : bc[KS + s]);
        // ---- bias + decode -> this wave's staging rows (row = frow, the group's pixel)
        const int m0 = g * 16;
        int m = m0 + frow;
        m = m < M ? m : M - 1;
        const int img = m / hw, pix = m - img * hw;
        const int gy = pix / W, gx = pix - gy * W;
        float* row = stg + frow * rowf;
        // serving score records (ABI 18): this lane's classes (f - 1) * 16 + fq * 4 + r, in increasing
        // order, scanned as postprocess.hip's filter scans a row (class 0 -- lane fq 0 -- starts the
        // scan even when NaN, every later class replaces only on a strict '>'), from the very values
        // the row gets; a lane with no class below C keeps cbi = C ("none") through the merge
        float cbest = -INFINITY, objv = 0.0f;
        float boxv[4];  // ch 0-3 (lane fq 0): the decoded box, copied into the record
        int cbi = C;
        // fragment 0: lane row fq 0 holds ch 0-3 (the box), fq 1 ch 4 (obj); every lane evaluates both
        // candidates of its values and selects (the same arithmetic as the branchy form: bit-identical)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ch = fq * 4 + r;
            const float v = acc[0][r] + bl[ch];
            float bx = v;
            if constexpr (MODE != 2) bx = r < 2 ? (v + (float)(r == 0 ? gx : gy)) * st : hd_exp(v) * st;
            const float ob = MODE == 1 ? v : hd_sigmoid(v);
            boxv[r] = bx;
            if (r == 0) objv = ob;  // lane row fq 1: ch 4
            if (ch < 5) row[ch] = ch < 4 ? bx : ob;
        }
#pragma unroll
        for (int f = 1; f < NF; ++f) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = f * 16 + fq * 4 + r;
                const float v = acc[f][r] + bl[ch];
                const float sv = MODE == 1 ? v : hd_sigmoid(v);
                if (ch - 16 < C) {
                    row[5 + ch - 16] = sv;
                    if (ch == 16 || sv > cbest) {
                        cbest = sv;
                        cbi = ch - 16;
                    }
                }
            }
        }
        if (d.scores != nullptr) {
            // the four lanes of a pixel (fq = 0..3: lanes frow + 16 fq) merged with the filter's rules
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) {
                const float ob = __shfl_xor(cbest, off);
                const int oi = __shfl_xor(cbi, off);
                bool take;
                if (oi >= C) take = false;
                else if (cbi >= C) take = true;
                else if (cbest != cbest) take = false;  // class 0 is NaN: the serial answer
                else if (ob != ob) take = true;
                else take = ob > cbest || (ob == cbest && oi < cbi);
                if (take) { cbest = ob; cbi = oi; }
            }
            const float obj = __shfl(objv, frow + 16);  // ch 4 (obj) lives in lane fq = 1
            const int mr = m0 + frow;
            if (fq == 0 && mr < M) {
                float4* rec = (float4*)(d.scores + 8 * ((long long)img * (d.out_bstride / rowf) + d.a_off + pix));
                rec[0] = make_float4(obj * cbest, cbest, (float)cbi, obj);
                rec[1] = make_float4(boxv[0], boxv[1], boxv[2], boxv[3]);
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): every lane's rows are in LDS
        __builtin_amdgcn_wave_barrier();
        const int n = M - m0 < 16 ? M - m0 : 16;
        // ---- the group's rows are contiguous in the output (split once at an image boundary)
        int t0 = 0, bi = m0 / hw, p0 = m0 - bi * hw;
        while (t0 < n) {
            const int cnt = min(n - t0, hw - p0);
            float* dst = d.out + (long long)bi * d.out_bstride + (long long)(d.a_off + p0) * rowf;
            const float* src = stg + t0 * rowf;
            const int total4 = cnt * rowf / 4;  // cnt % 4 == 0: 16-byte runs
            for (int q = lane; q < total4; q += 64) *(float4*)(dst + 4 * q) = *(const float4*)(src + 4 * q);
            t0 += cnt;
            ++bi;
            p0 = 0;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // the staging reads are done before the next group's writes
        __builtin_amdgcn_wave_barrier();
        if (more) {
#pragma unroll
            for (int q = 0; q < 2 * KS; ++q) bc[q] = bn[q];
        }
    }
}

// grid: a block per CU at most (persistent over the level's 16-pixel groups)
template <typename T, int CIN, int NCF>
int head2_launch(const yxh_head_desc& d, hipStream_t st) {
    constexpr int nw = head2_waves(CIN);
    const long long groups = ((long long)d.batch * d.h * d.w + 15) / 16;
    const unsigned grid2 = (unsigned)std::min<long long>((groups + nw - 1) / nw, device_cus());
    if (d.train == 1) hipLaunchKernelGGL((head_pred2<T, CIN, NCF, 1>), dim3(grid2), dim3(64 * nw), 0, st, d);
    else if (d.train == 2) hipLaunchKernelGGL((head_pred2<T, CIN, NCF, 2>), dim3(grid2), dim3(64 * nw), 0, st, d);
    else hipLaunchKernelGGL((head_pred2<T, CIN, NCF, 0>), dim3(grid2), dim3(64 * nw), 0, st, d);
    YXH_CHECK_LAUNCH("head_pred2 launch");
    return YXH_OK;
}

// the (NCF, MODE) kernels of one (dtype, CIN): explicitly instantiated in head2_c<CIN>.hip
template <typename T, int CIN>
int head2_dispatch_t(const yxh_head_desc& d, hipStream_t st) {
    switch ((d.num_classes + 15) / 16) {
        case 1: return head2_launch<T, CIN, 1>(d, st);
        case 2: return head2_launch<T, CIN, 2>(d, st);
        case 3: return head2_launch<T, CIN, 3>(d, st);
        case 4: return head2_launch<T, CIN, 4>(d, st);
        case 5: return head2_launch<T, CIN, 5>(d, st);
    }
    set_error("head_pred2: %d classes (1-80: the weights of more than 5 class fragments do not fit in registers)",
              d.num_classes);
    return YXH_EUNSUPPORTED;
}

#define YXH_HEAD2_UNIT(CIN)                                                                 \
    template int head2_dispatch_t<bf16, CIN>(const yxh_head_desc& d, hipStream_t st);       \
    template int head2_dispatch_t<f16, CIN>(const yxh_head_desc& d, hipStream_t st)
#define YXH_HEAD2_EXTERN(CIN)                                                               \
    extern template int head2_dispatch_t<bf16, CIN>(const yxh_head_desc& d, hipStream_t st); \
    extern template int head2_dispatch_t<f16, CIN>(const yxh_head_desc& d, hipStream_t st)

}  // namespace yxh
