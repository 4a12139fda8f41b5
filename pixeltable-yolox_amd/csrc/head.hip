// head_pred: the three 1x1 pred convs of one YOLOX head level + cat + sigmoid + decode
// in ONE kernel (reference yolo_head.py:149-160 reg_preds / obj_preds / cls_preds,
// :185-187 cat([reg, obj.sigmoid(), cls.sigmoid()]), :205-207 flatten/permute,
// :233-251 decode_outputs), writing the level's rows of the [B, A, 5+C] fp32 output.
//
// Persistent blocks (weights loaded into LDS once) walk tiles of TM = 64 consecutive
// pixels m (image-major) of the level:
//  * the reg_feat and cls_feat tiles [64][cin] and both weight matrices ([5][cin] reg+obj,
//    [C][cin] cls, zero rows up to whole 16-row fragments) are staged in LDS (XOR-swizzled);
//  * wave w computes pixel fragment w (16 pixels) x every output-channel fragment
//    (1 reg/obj + ceil(C/16) cls) on MFMA 16x16x32 -- no block-diagonal zero work;
//  * bias + decode in registers: ch 0-1 (v + grid) * stride, ch 2-3 exp(v) * stride,
//    ch 4.. sigmoid -- hardware exp2 + reciprocal (hd_exp / hd_sigmoid, ~1 ulp each), NOT
//    the IEEE expf / divide of conv_common.hpp's fp32 decode path (test_gpu_ops.py
//    test_head_pred_fused_level: vs torch fp32 exp / sigmoid within 1e-4 abs + rel);
//  * the decoded [64][5+C] tile is staged in LDS and leaves as 16-byte stores over the
//    contiguous output rows (a level's rows of one image are consecutive; a tile
//    straddles at most one image boundary) -- instead of 4-byte scattered stores of
//    4 * (5 + C)-byte rows.
// This file: the launch (head_pred_launch: 1-80 classes, 16-bit dtypes; selects (dtype, CIN, NCF, MODE)) and
// the tile kernel head_pred (CIN 64 / 128 / 256).  The default path is the per-wave head_pred2 of head2.hpp
// (CIN 64 / 96 / 128 / 192 / 256 / 320), compiled in head2_c<CIN>.hip.
#include <stdlib.h>

#include <algorithm>

#include "head2.hpp"

namespace yxh {

// CIN: feature channels (a power of two >= 64); NCF: cls output fragments (16 rows each), 1-5
template <typename T, int CIN, int NCF>
__global__ __launch_bounds__(256) void head_pred(yxh_head_desc d) {
    constexpr int TM = 64;
    constexpr int EPC = Chunk<T>::N;
    constexpr int CPR = CIN / EPC;        // 16-byte chunks per row
    static_assert((CPR & (CPR - 1)) == 0, "head_pred: the LDS swizzle needs a power-of-two row");
    constexpr int ROWB = CIN * sizeof(T);
    constexpr int NF = 1 + NCF;           // output-channel fragments
    constexpr int WROWS = NF * 16;        // weight rows in LDS
    constexpr int XB = TM * ROWB;         // one feature tile
    constexpr int WB = WROWS * ROWB;
    constexpr int STG = TM * (5 + NCF * 16) * 4;  // staged rows, stride 5 + C (<= 5 + NCF * 16)
    __shared__ __attribute__((aligned(16))) char smem[2 * XB + WB + STG];
    char* xr = smem;            // reg_feat tile [TM][CIN] (chunks XOR-swizzled by row)
    char* xc = smem + XB;       // cls_feat tile
    char* wl = smem + 2 * XB;   // weights [WROWS][CIN]: row 0-4 reg+obj, 16.. cls
    float* stg = (float*)(smem + 2 * XB + WB);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = d.num_classes, hw = d.h * d.w;
    const int M = d.batch * hw;
    const int ntiles = (M + TM - 1) / TM;
    auto swz = [](int r, int c) { return c ^ (r & (CPR - 1)); };

    // weights once per block (the grid is persistent over pixel tiles)
    for (int q = tid; q < WROWS * CPR; q += 256) {
        const int r = q / CPR, c = q - r * CPR;
        const int cs = swz(r, c);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r < 5)
            v = *(const uint4*)((const T*)d.w_reg + (long long)r * CIN + cs * EPC);
        else if (r >= 16 && r - 16 < C)
            v = *(const uint4*)((const T*)d.w_cls + (long long)(r - 16) * CIN + cs * EPC);
        *(uint4*)(wl + q * 16) = v;
    }
    const int frow = lane & 15, fq = lane >> 4;
    const int rowf = 5 + C;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int m0 = tile * TM;
        const int b0 = m0 / hw, p0 = m0 - b0 * hw;
        // ---- feature tiles -> LDS (chunk c of row r stored at c ^ (r & (CPR - 1))): all
        // loads of the tile issued before any LDS store
        constexpr int NQ = TM * CPR / 256;  // 16-byte chunks per thread per tensor
        uint4 vr[NQ], vc[NQ];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const int q = tid + 256 * k;
            const int r = q / CPR, c = q - r * CPR;
            int pix = p0 + min(r, M - 1 - m0), b = b0;
            while (pix >= hw) {  // levels smaller than a tile: several images per tile
                pix -= hw;
                ++b;
            }
            const int cs = swz(r, c);
            vr[k] = *(const uint4*)((const T*)d.reg.ptr + (long long)b * d.reg.bstride + (long long)pix * d.reg.cstride +
                                    cs * EPC);
            vc[k] = *(const uint4*)((const T*)d.cls.ptr + (long long)b * d.cls.bstride + (long long)pix * d.cls.cstride +
                                    cs * EPC);
        }
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const int q = tid + 256 * k;
            *(uint4*)(xr + q * 16) = vr[k];
            *(uint4*)(xc + q * 16) = vc[k];
        }
        __syncthreads();

        // ---- MFMA: out[ch][pix], wave = pixel fragment
        f32x4 acc[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int pr = wave * 16 + frow;  // tile pixel of this lane's B fragment
#pragma unroll
        for (int s = 0; s < CIN / 32; ++s) {
            const int ch = s * 4 + fq;
            const uint4 br = *(const uint4*)(xr + (pr * CPR + swz(pr, ch)) * 16);
            const uint4 bc = *(const uint4*)(xc + (pr * CPR + swz(pr, ch)) * 16);
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const int wr = f * 16 + frow;
                const uint4 a = *(const uint4*)(wl + (wr * CPR + swz(wr, ch)) * 16);
                Mma<T>::run(acc[f], a, f == 0 ? br : bc);
            }
        }

        // ---- bias + decode -> staged fp32 rows
        {
            int pix = p0 + min(pr, M - 1 - m0);
            while (pix >= hw) pix -= hw;
            const int gy = pix / d.w, gx = pix - gy * d.w;
            const float st = d.stride;
            float* row = stg + pr * rowf;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ch = f * 16 + fq * 4 + r;  // fragment row
                    float v = acc[f][r];
                    if (f == 0) {
                        if (ch < 5) {
                            v += d.b_reg[ch];
                            if (ch < 4) {
                                if (d.train != 2) v = ch < 2 ? (v + (float)(ch == 0 ? gx : gy)) * st : hd_exp(v) * st;
                            } else {
                                v = d.train == 1 ? v : hd_sigmoid(v);
                            }
                            row[ch] = v;
                        }
                    } else {
                        const int c = ch - 16;
                        if (c < C) {
                            v += d.b_cls[c];
                            row[5 + c] = d.train == 1 ? v : hd_sigmoid(v);
                        }
                    }
                }
            }
        }
        __syncthreads();

        // ---- the staged rows have the output's row stride, so each piece of the tile (it
        // splits at an image boundary) is one contiguous, 16-byte aligned run in both LDS and
        // the output: a plain float4 copy
        const int n = min(TM, M - m0);
        int t0 = 0, b = b0, pix = p0;
        while (t0 < n) {
            const int cnt = min(n - t0, hw - pix);
            float* dst = d.out + (long long)b * d.out_bstride + (long long)(d.a_off + pix) * rowf;
            const float* src = stg + t0 * rowf;
            const int total = cnt * rowf;  // floats, a multiple of 4 (cnt % 4 == 0)
            for (int q = tid * 4; q < total; q += 1024) *(float4*)(dst + q) = *(const float4*)(src + q);
            t0 += cnt;
            ++b;
            pix = 0;
        }
        __syncthreads();  // staging and feature tiles are reused by the next tile
    }
}

YXH_HEAD2_EXTERN(64);
YXH_HEAD2_EXTERN(96);
YXH_HEAD2_EXTERN(128);
YXH_HEAD2_EXTERN(192);
YXH_HEAD2_EXTERN(256);
YXH_HEAD2_EXTERN(320);

namespace {

// the tile kernel's (dtype, CIN) instantiations of one class-fragment count
template <typename T, int CIN>
int head1_launch(const yxh_head_desc& d, unsigned grid, hipStream_t st) {
    switch ((d.num_classes + 15) / 16) {
        case 1: hipLaunchKernelGGL((head_pred<T, CIN, 1>), dim3(grid), dim3(256), 0, st, d); break;
        case 2: hipLaunchKernelGGL((head_pred<T, CIN, 2>), dim3(grid), dim3(256), 0, st, d); break;
        case 3: hipLaunchKernelGGL((head_pred<T, CIN, 3>), dim3(grid), dim3(256), 0, st, d); break;
        case 4: hipLaunchKernelGGL((head_pred<T, CIN, 4>), dim3(grid), dim3(256), 0, st, d); break;
        default: hipLaunchKernelGGL((head_pred<T, CIN, 5>), dim3(grid), dim3(256), 0, st, d); break;
    }
    YXH_CHECK_LAUNCH("head_pred launch");
    return YXH_OK;
}

// (dtype, CIN) -> the kernels of that pair; NCF and MODE are selected below them
template <typename T>
int head_dispatch(const yxh_head_desc& d, bool v2, unsigned grid, hipStream_t st) {
    switch (d.cin) {
        case 64: return v2 ? head2_dispatch_t<T, 64>(d, st) : head1_launch<T, 64>(d, grid, st);
        case 128: return v2 ? head2_dispatch_t<T, 128>(d, st) : head1_launch<T, 128>(d, grid, st);
        case 256: return v2 ? head2_dispatch_t<T, 256>(d, st) : head1_launch<T, 256>(d, grid, st);
        case 96: if (v2) return head2_dispatch_t<T, 96>(d, st); break;
        case 192: if (v2) return head2_dispatch_t<T, 192>(d, st); break;
        case 320: if (v2) return head2_dispatch_t<T, 320>(d, st); break;
        default:
            set_error("head_pred: %d feature channels not built (64 / 96 / 128 / 192 / 256 / 320)", d.cin);
            return YXH_EUNSUPPORTED;
    }
    set_error("head_pred: %d feature channels run on head_pred2 only (the tile kernel's LDS swizzle needs a "
              "power-of-two row): not with YXH_HEAD_V1=1 or feature rows that are not 16-byte aligned", d.cin);
    return YXH_EUNSUPPORTED;
}

}  // namespace

int head_pred_launch(const yxh_head_desc* d, hipStream_t st) {
    YXH_CHECK_ARG(d && d->out && d->cls.ptr && d->reg.ptr && d->w_reg && d->w_cls && d->b_reg && d->b_cls,
                  "head_pred: null pointer");
    YXH_CHECK_ARG(d->batch > 0 && d->h > 0 && d->w > 0, "head_pred: empty level");
    YXH_CHECK_ARG(d->train >= 0 && d->train <= 2, "head_pred: mode %d", d->train);
    YXH_CHECK_ARG(((long long)d->h * d->w) % 4 == 0 && d->a_off % 4 == 0 && d->out_bstride % 4 == 0 &&
                      ((uintptr_t)d->out & 15) == 0,
                  "head_pred: level rows must be 16-byte aligned (h*w, a_off multiples of 4)");
    YXH_CHECK_ARG(d->reg.channels == d->cin && d->cls.channels == d->cin, "head_pred: feature channels");
    const long long M = (long long)d->batch * d->h * d->w;
    YXH_CHECK_ARG(M < (1LL << 31), "head_pred: too many pixels");
    const long long tiles = (M + 63) / 64;
    const unsigned grid = (unsigned)(tiles < 512 ? tiles : 512);  // persistent: weights loaded once per block
    if (d->num_classes < 1 || d->num_classes > 80) {
        // past 5 class fragments the resident weights no longer fit in registers: the planner keeps
        // the two pred convs there
        set_error("head_pred built for 1-80 classes (got %d)", d->num_classes);
        return YXH_EUNSUPPORTED;
    }
    // head_pred2 wherever the feature rows are 16-byte aligned (YXH_HEAD_V1=1: the tile kernel, for
    // A/B and the bit-identity tests; 64 / 128 / 256 channels only)
    const char* v1e = getenv("YXH_HEAD_V1");
    const bool v1 = v1e != nullptr && v1e[0] == '1';
    const bool rows16 = ((uintptr_t)d->reg.ptr % 16) == 0 && ((uintptr_t)d->cls.ptr % 16) == 0 &&
                        d->reg.cstride % 8 == 0 && d->cls.cstride % 8 == 0 && d->reg.bstride % 8 == 0 &&
                        d->cls.bstride % 8 == 0;
    const bool cin2 = d->cin == 64 || d->cin == 96 || d->cin == 128 || d->cin == 192 || d->cin == 256 || d->cin == 320;
    const bool v2 = !v1 && rows16;
    YXH_CHECK_ARG(!d->scores || (v2 && cin2 && d->train == 0 && ((uintptr_t)d->scores % 16) == 0 &&
                                 d->out_bstride % (5 + d->num_classes) == 0),
                  "head_pred: score records need the head_pred2 path (eval decode rows, 64 / 96 / 128 / 192 / 256 / 320 "
                  "16-bit channels, 16-byte rows) and a 16-byte aligned buffer");
    if (d->dtype == YXH_BF16) return head_dispatch<bf16>(*d, v2, grid, st);
    if (d->dtype == YXH_F16) return head_dispatch<f16>(*d, v2, grid, st);
    set_error("head_pred: dtype %d not built", d->dtype);
    return YXH_EUNSUPPORTED;
}

}  // namespace yxh
