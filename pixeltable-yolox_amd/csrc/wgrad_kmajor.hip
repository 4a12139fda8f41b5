// Weight-gradient tiles 17-24 (fp32), MFMA operands read k-major straight from the pixel-major
// tensors: wgrad_f32 (17-20, any conv shape, one tap per block) and wgrad9t_f32 (21-24, 3x3 pad 1
// of stride 1 or 2, all nine taps per block).
#include "wgrad.hpp"

namespace yxh {

// ------------------------------------------------------------------ fp32 weight gradient
// dW[n][c][tap] += sum over output pixels p of dY[p][n] * X[in(p, tap)][c] for fp32 convs (any
// kh x kw, stride, pad; the 1x1 and 3x3 BaseConvs of the training step).  Both operands are
// pixel-major, which is exactly the k-major operand form of v_mfma_f32_16x16x4_f32 (lane l:
// A[l % 16][l / 16] = dY[p0 + l / 16][n0 + l % 16], B likewise from X at the tap's input pixel,
// zero outside the image): no transposes.  A block owns a TN x TC tile of ONE tap over a range of
// KP-pixel stages (split-K over pixels); per stage both slabs are staged through LDS by 16-byte
// register loads (rows padded by 16 floats: the four 16-lane row groups of a ds_read_b32 hit
// distinct banks), double-buffered.  With a workspace each split stores its partial dW plainly
// and wgrad_reduce sums the splits in a fixed order (deterministic, no cross-XCD atomics);
// without one the partials go out as fp32 atomics (dW pre-zeroed, as for conv_wgrad).
template <int TN, int TC, int WN, int WC, int KP>
__global__ __launch_bounds__(256) void wgrad_f32(WgradParams p) {
    static_assert(WN * WC == 4, "4 waves");
    constexpr int WTN = TN / WN, WTC = TC / WC, FN = WTN / 16, FC = WTC / 16;
    constexpr int TNP = TN + 16, TCP = TC + 16;
    constexpr int ASZ = KP * TNP, BSZ = KP * TCP;
    constexpr int ACH = KP * TN / 4, BCH = KP * TC / 4, AL = (ACH + 255) / 256, BL = (BCH + 255) / 256;
    __shared__ __attribute__((aligned(16))) float lds[2][ASZ + BSZ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave % WN, wc = wave / WN;
    const int taps = p.kh * p.kw;
    const int tap = (int)blockIdx.z % taps, ct = (int)blockIdx.z / taps;
    const int ty = tap / p.kw, tx = tap - ty * p.kw;
    const int n0 = blockIdx.y * TN, c0 = ct * TC;
    const int st0 = blockIdx.x * p.sps, st1 = min(p.nst, st0 + p.sps);
    const int M = p.M, ohw = p.ohw, ow = p.out_w, cout = p.cout, cin = p.cin;
    const float* dy = (const float*)p.dy;
    const bool dy_dense = p.dybs == (long long)ohw * p.dycs;

    float4 ra[AL], rb[BL];
    auto gload = [&](int st) {
        const int pb = st * KP;
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            const int q = tid + 256 * i;
            const int row = q / (TN / 4), col = q - row * (TN / 4);
            const int m = pb + row, n = n0 + col * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < ACH && m < M && n < cout) {
                long long off;
                if (dy_dense) {
                    off = (long long)m * p.dycs;
                } else {
                    const int b = m / ohw;
                    off = (long long)b * p.dybs + (long long)(m - b * ohw) * p.dycs;
                }
                v = *(const float4*)(dy + off + n);
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < BL; ++i) {
            const int q = tid + 256 * i;
            const int row = q / (TC / 4), col = q - row * (TC / 4);
            const int m = pb + row, c = c0 + col * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < BCH && m < M && c < cin) {
                const int b = m / ohw, pix = m - b * ohw;
                const int oy = pix / ow, ox = pix - oy * ow;
                const int iy = oy * p.stride + ty - p.pad, ix = ox * p.stride + tx - p.pad;
                if ((unsigned)iy < (unsigned)p.in_h && (unsigned)ix < (unsigned)p.in_w) {
                    const int s = (p.nsrc > 1 && c >= p.src0_ch) ? 1 : 0;
                    const int cc = s ? c - p.src0_ch : c;
                    const int spix = p.sup[s] ? (iy >> 1) * p.sw[s] + (ix >> 1) : iy * p.sw[s] + ix;
                    v = *(const float4*)((const float*)p.sptr[s] + (long long)b * p.sbs[s] + (long long)spix * p.scs[s] + cc);
                }
            }
            rb[i] = v;
        }
    };
    auto lstore = [&](int buf) {
        float* A = lds[buf];
        float* Bm = lds[buf] + ASZ;
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            const int q = tid + 256 * i;
            const int row = q / (TN / 4), col = q - row * (TN / 4);
            if (q < ACH) *(float4*)(A + row * TNP + col * 4) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < BL; ++i) {
            const int q = tid + 256 * i;
            const int row = q / (TC / 4), col = q - row * (TC / 4);
            if (q < BCH) *(float4*)(Bm + row * TCP + col * 4) = rb[i];
        }
    };

    f32x4 acc[FN][FC];
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FC; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kr = lane >> 4, kc = lane & 15;
    if (st0 < st1) {
        gload(st0);
        lstore(0);
        __syncthreads();
    }
    int buf = 0;
    for (int st = st0; st < st1; ++st) {
        const bool more = st + 1 < st1;
        if (more) gload(st + 1);
        const float* A = lds[buf] + wn * WTN + kc;
        const float* Bm = lds[buf] + ASZ + wc * WTC + kc;
#pragma unroll
        for (int kk = 0; kk < KP / 4; ++kk) {
            float a[FN], b[FC];
#pragma unroll
            for (int i = 0; i < FN; ++i) a[i] = A[(4 * kk + kr) * TNP + 16 * i];
#pragma unroll
            for (int j = 0; j < FC; ++j) b[j] = Bm[(4 * kk + kr) * TCP + 16 * j];
#pragma unroll
            for (int i = 0; i < FN; ++i)
#pragma unroll
                for (int j = 0; j < FC; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    // D[m][n] of fragment (i, j): lane holds rows 4 (lane / 16) + r, column lane % 16
    float* out = p.ws ? p.ws + (long long)blockIdx.x * p.cout * p.cin_store * taps : p.dw;
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FC; ++j) {
            const int c = c0 + wc * WTC + 16 * j + kc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wn * WTN + 16 * i + 4 * kr + r;
                if (n >= cout || c >= p.cin_store) continue;
                float* d = out + ((long long)n * p.cin_store + c) * taps + tap;
                if (p.ws) *d = acc[i][j][r];
                else unsafeAtomicAdd(d, acc[i][j][r]);
            }
        }
}

// fp32 3x3 weight gradient with all nine taps per block: a stage is a row segment of KP output
// pixels (image b, row oy, columns ox0 .. ox0 + KP); dY[KP][TN] and the three input rows it
// reads, X[3][(KP - 1) s + 3][TC] (zero outside the image), are staged once, and every tap's
// B operand is a shifted view of the X rows: dY and X are read once per stage instead of once
// per tap.  acc[9][FN][FC] stays in registers for the block's pixel range; partials as wgrad_f32.
template <int TN, int TC, int S, int KP>
__global__ __launch_bounds__(256) void wgrad9t_f32(WgradParams p, int nseg) {
    constexpr int WN = 2, WC = 2;
    constexpr int WTN = TN / WN, WTC = TC / WC, FN = WTN / 16, FC = WTC / 16;
    constexpr int XW = (KP - 1) * S + 3, TNP = TN + 16, TCP = TC + 16;
    constexpr int ASZ = KP * TNP, BSZ = 3 * XW * TCP;
    constexpr int ACH = KP * TN / 4, BCH = 3 * XW * TC / 4, AL = (ACH + 255) / 256, BL = (BCH + 255) / 256;
    __shared__ __attribute__((aligned(16))) float lds[2][ASZ + BSZ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave % WN, wc = wave / WN;
    const int n0 = blockIdx.y * TN, c0 = blockIdx.z * TC;
    const int st0 = blockIdx.x * p.sps, st1 = min(p.nst, st0 + p.sps);
    const int oh = p.out_h, ow = p.out_w, cout = p.cout, cin = p.cin;
    const float* dy = (const float*)p.dy;

    float4 ra[AL], rb[BL];
    auto gload = [&](int st) {
        const int seg = st % nseg, r = st / nseg;
        const int b = r / oh, oy = r - b * oh, ox0 = seg * KP;
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            const int q = tid + 256 * i;
            const int row = q / (TN / 4), col = q - row * (TN / 4);
            const int ox = ox0 + row, n = n0 + col * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < ACH && ox < ow && n < cout)
                v = *(const float4*)(dy + (long long)b * p.dybs + (long long)(oy * ow + ox) * p.dycs + n);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < BL; ++i) {
            const int q = tid + 256 * i;
            const int row = q / (TC / 4), col = q - row * (TC / 4);  // row = ty * XW + xx
            const int ty = row / XW, xx = row - ty * XW;
            const int iy = oy * S + ty - 1, ix = ox0 * S + xx - 1, c = c0 + col * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < BCH && c < cin && (unsigned)iy < (unsigned)p.in_h && (unsigned)ix < (unsigned)p.in_w) {
                const int s = (p.nsrc > 1 && c >= p.src0_ch) ? 1 : 0;
                const int cc = s ? c - p.src0_ch : c;
                const int spix = p.sup[s] ? (iy >> 1) * p.sw[s] + (ix >> 1) : iy * p.sw[s] + ix;
                v = *(const float4*)((const float*)p.sptr[s] + (long long)b * p.sbs[s] + (long long)spix * p.scs[s] + cc);
            }
            rb[i] = v;
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            const int q = tid + 256 * i;
            if (q < ACH) *(float4*)(lds[buf] + (q / (TN / 4)) * TNP + (q % (TN / 4)) * 4) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < BL; ++i) {
            const int q = tid + 256 * i;
            if (q < BCH) *(float4*)(lds[buf] + ASZ + (q / (TC / 4)) * TCP + (q % (TC / 4)) * 4) = rb[i];
        }
    };

    f32x4 acc[9][FN][FC];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FC; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kr = lane >> 4, kc = lane & 15;
    if (st0 < st1) {
        gload(st0);
        lstore(0);
        __syncthreads();
    }
    int buf = 0;
    for (int st = st0; st < st1; ++st) {
        const bool more = st + 1 < st1;
        if (more) gload(st + 1);
        const float* A = lds[buf] + wn * WTN + kc;
        const float* Bm = lds[buf] + ASZ + wc * WTC + kc;
#pragma unroll
        for (int kk = 0; kk < KP / 4; ++kk) {
            float a[FN];
#pragma unroll
            for (int i = 0; i < FN; ++i) a[i] = A[(4 * kk + kr) * TNP + 16 * i];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int xrow = (t / 3) * XW + (4 * kk + kr) * S + (t % 3);
                float b[FC];
#pragma unroll
                for (int j = 0; j < FC; ++j) b[j] = Bm[xrow * TCP + 16 * j];
#pragma unroll
                for (int i = 0; i < FN; ++i)
#pragma unroll
                    for (int j = 0; j < FC; ++j)
                        acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[t][i][j], 0, 0, 0);
            }
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    float* out = p.ws ? p.ws + (long long)blockIdx.x * p.cout * p.cin_store * 9 : p.dw;
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FC; ++j) {
            const int c = c0 + wc * WTC + 16 * j + kc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wn * WTN + 16 * i + 4 * kr + r;
                if (n >= cout || c >= p.cin_store) continue;
                float* d = out + ((long long)n * p.cin_store + c) * 9;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    if (p.ws) d[t] = acc[t][i][j][r];
                    else unsafeAtomicAdd(d + t, acc[t][i][j][r]);
                }
            }
        }
}

namespace {

// 16-byte channel chunks everywhere (conv_wgrad_launch checks the views' own)
int check_chunks(const WgradParams& p, const char* tiles) {
    if ((p.nsrc > 1 && p.src0_ch % 4) || p.dycs % 4 || p.dybs % 4 || p.cin % 4) {
        set_error("wgrad tiles %s: 16-byte channel chunks", tiles);
        return YXH_EUNSUPPORTED;
    }
    return YXH_OK;
}

template <int TN, int TC, int WN, int WC, int KP>
int launch_wgrad_f32(WgradParams p, hipStream_t st) {
    if (int rc = check_chunks(p, "17-20")) return rc;
    const int taps = p.kh * p.kw;
    const int ntn = (p.cout + TN - 1) / TN, ntc = (p.cin + TC - 1) / TC;
    p.nst = (int)(((long long)p.M + KP - 1) / KP);
    // about two blocks per CU; >= 4 stages per split
    const SplitPlan s = plan_wgrad(p, p.nst, (long long)ntn * ntc * taps, wgrad_target_blocks(), 4);
    p.sps = s.per_split;
    YXH_CHECK_ARG(ntn < 65536 && ntc * taps < 65536, "wgrad grid");
    hipLaunchKernelGGL((wgrad_f32<TN, TC, WN, WC, KP>), dim3((unsigned)s.splits, ntn, ntc * taps), dim3(256), 0, st, p);
    YXH_CHECK_LAUNCH("wgrad_f32");
    return ws_reduce(p, s.splits, st);
}

template <int TN, int TC, int S, int KP>
int launch_wgrad9t_f32(WgradParams p, hipStream_t st) {
    if (int rc = check_chunks(p, "21-24")) return rc;
    const int nseg = (p.out_w + KP - 1) / KP;
    const int ntn = (p.cout + TN - 1) / TN, ntc = (p.cin + TC - 1) / TC;
    p.nst = p.B * p.out_h * nseg;
    const SplitPlan s = plan_wgrad(p, p.nst, (long long)ntn * ntc, wgrad_target_blocks(), 4);
    p.sps = s.per_split;
    YXH_CHECK_ARG(ntn < 65536 && ntc < 65536, "wgrad grid");
    hipLaunchKernelGGL((wgrad9t_f32<TN, TC, S, KP>), dim3((unsigned)s.splits, ntn, ntc), dim3(256), 0, st, p, nseg);
    YXH_CHECK_LAUNCH("wgrad9t_f32");
    return ws_reduce(p, s.splits, st);
}

// KP1 / KP2 output pixels per stage at stride 1 / 2
template <int TN, int TC, int KP1, int KP2 = KP1>
int by_stride(const WgradParams& p, hipStream_t st) {
    return p.stride == 2 ? launch_wgrad9t_f32<TN, TC, 2, KP2>(p, st) : launch_wgrad9t_f32<TN, TC, 1, KP1>(p, st);
}

}  // namespace

// cout x cin, waves, pixels per stage
int wgrad_kmajor_dispatch(int, int tile, const WgradParams& p, hipStream_t st) {
    switch (tile) {
        case 17: return launch_wgrad_f32<64, 64, 2, 2, 32>(p, st);
        case 18: return launch_wgrad_f32<128, 128, 2, 2, 16>(p, st);
        case 19: return launch_wgrad_f32<128, 64, 2, 2, 32>(p, st);
        default: return launch_wgrad_f32<64, 128, 2, 2, 32>(p, st);
    }
}

int wgrad9_kmajor_dispatch(int, int tile, const WgradParams& p, hipStream_t st) {
    switch (tile) {
        case 21: return by_stride<64, 64, 16>(p, st);
        case 22: return by_stride<64, 64, 32, 8>(p, st);
        case 23: return by_stride<32, 64, 16>(p, st);
        default: return by_stride<64, 32, 16>(p, st);
    }
}

}  // namespace yxh
