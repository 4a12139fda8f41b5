// Weight-gradient tiles 5-10 (bf16/f16, any conv shape): conv_wgrad2.
#include "lds_tr.hpp"
#include "wgrad.hpp"

namespace yxh {

// The zero chunk invalid lanes read.  Without relocatable device code each unit needs its own
// (wgrad_reg.hip has another); an external symbol of the unit's own name, so the kernels reach it as before.
inline namespace wgrad_glds {
__device__ __attribute__((aligned(16))) uint4 g_wg_zero[4];
}

// ------------------------------------------------------------------ weight gradient, LDS-DMA + transposed reads
// bf16/f16 variant (tile ids 5-10, TN and TM in {64, 128}): both operands land in LDS in
// their natural pixel-major layout by LDS-DMA (global_load_lds_dwordx4: one 16-byte
// channel chunk per lane, the zero chunk for padding taps and the pixel tail), and the
// MFMA fragments come out pixel(K)-major through gfx950's ds_read_b64_tr_b16 -- no
// register staging and no in-register transpose, so the K loop is DMA issue + LDS reads
// + MFMA over an NBUF-deep ring with counted vmcnt waits and raw barriers.  K = linear
// output pixels, 64 per stage; each lane's DMA rows advance incrementally (no division
// in the loop).  Row images are [pixel][chunk ^ f(pixel)]: the transposed reads of a
// 32-lane half (4 consecutive rows, two blocks 8 rows apart) cover all 64 banks once.
template <int NCH>
__device__ __forceinline__ int wg2_swz(int row) {
    if constexpr (NCH == 16) return ((row & 3) << 2) | ((row >> 2) & 3);
    else return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2);
}

__device__ __forceinline__ void wg2_glds16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

template <int N>
__device__ __forceinline__ void wg2_wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void wg2_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

struct Wg2Pix {
    int b, oy, ox;
};

template <typename T, int TN, int TM, int NBUF>
__global__ __launch_bounds__(256) void conv_wgrad2(WgradParams p) {
    constexpr int KP = 64;                     // output pixels per stage (two 32-deep K slabs)
    constexpr int NCA = TN / 8, NCB = TM / 8;  // 16-byte chunks per pixel row
    constexpr int RBA = NCA * 16, RBB = NCB * 16;
    constexpr int A_BYTES = KP * RBA, B_BYTES = KP * RBB, BUF = A_BYTES + B_BYTES;
    constexpr int PWA = A_BYTES / 4096, PWB = B_BYTES / 4096;  // 1 KiB DMA pieces per wave per stage
    constexpr int PW = PWA + PWB;
    constexpr int WTN = TN / 2, WTM = TM / 2, FR = WTN / 16, FC = WTM / 16;
    static_assert(PWA >= 1 && PWB >= 1 && sizeof(T) == 2 && (NBUF == 2 || NBUF == 3), "tile");
    __shared__ __attribute__((aligned(16))) char smem[NBUF * BUF];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int n0 = blockIdx.y * TN;
    const int tap = blockIdx.z / p.ntc, c0 = (blockIdx.z - tap * p.ntc) * TM;
    const int ky = tap / p.kw, kx = tap - ky * p.kw;
    const int st0 = blockIdx.x * p.sps;
    const int nst = min(p.nst, st0 + p.sps) - st0;
    if (nst <= 0) return;

    // this lane's DMA slots: piece k of an image holds bytes [1024k, 1024k + 1024)
    int rowA[PWA], chA[PWA], rowB[PWB], chB[PWB];
#pragma unroll
    for (int a = 0; a < PWA; ++a) {
        const int byte = (wave * PWA + a) * 1024 + lane * 16;
        rowA[a] = byte / RBA;
        chA[a] = ((byte % RBA) >> 4) ^ wg2_swz<NCA>(rowA[a]);
    }
#pragma unroll
    for (int q = 0; q < PWB; ++q) {
        const int byte = (wave * PWB + q) * 1024 + lane * 16;
        rowB[q] = byte / RBB;
        chB[q] = ((byte % RBB) >> 4) ^ wg2_swz<NCB>(rowB[q]);
    }
    Wg2Pix sa[PWA], sb[PWB];
    auto init = [&](Wg2Pix& s, int row) {
        const long long m = (long long)st0 * KP + row;
        s.b = (int)(m / p.ohw);
        const int pix = (int)(m - (long long)s.b * p.ohw);
        s.oy = pix / p.out_w;
        s.ox = pix - s.oy * p.out_w;
    };
    auto adv = [&](Wg2Pix& s) {
        s.ox += KP;
        while (s.ox >= p.out_w) {
            s.ox -= p.out_w;
            if (++s.oy == p.out_h) {
                s.oy = 0;
                ++s.b;
            }
        }
    };
#pragma unroll
    for (int a = 0; a < PWA; ++a) init(sa[a], rowA[a]);
#pragma unroll
    for (int q = 0; q < PWB; ++q) init(sb[q], rowB[q]);

    const T* dyp = (const T*)p.dy;
    const void* zero = (const void*)g_wg_zero;
    auto issue = [&](int buf) {
        char* A = smem + buf * BUF;
        char* Bm = A + A_BYTES;
#pragma unroll
        for (int a = 0; a < PWA; ++a) {
            const int n = n0 + chA[a] * 8;
            const void* g = zero;
            if (sa[a].b < p.B && n < p.dych)
                g = dyp + (long long)sa[a].b * p.dybs + (long long)(sa[a].oy * p.out_w + sa[a].ox) * p.dycs + n;
            wg2_glds16(g, A + (wave * PWA + a) * 1024);
        }
#pragma unroll
        for (int q = 0; q < PWB; ++q) {
            int c = c0 + chB[q] * 8;
            const int iy = sb[q].oy * p.stride - p.pad + ky, ix = sb[q].ox * p.stride - p.pad + kx;
            const void* g = zero;
            if (sb[q].b < p.B && c < p.cin && iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w) {
                int si = 0;
                if (p.nsrc == 2 && c >= p.src0_ch) {
                    si = 1;
                    c -= p.src0_ch;
                }
                const int up = p.sup[si];
                g = (const T*)p.sptr[si] + (long long)sb[q].b * p.sbs[si] +
                    ((long long)(iy >> up) * p.sw[si] + (ix >> up)) * p.scs[si] + c;
            }
            wg2_glds16(g, Bm + (wave * PWB + q) * 1024);
        }
#pragma unroll
        for (int a = 0; a < PWA; ++a) adv(sa[a]);
#pragma unroll
        for (int q = 0; q < PWB; ++q) adv(sb[q]);
    };

    // transposed-read addresses (image-relative, K slab 0): lane 4q+p of a 16-lane group
    // supplies row q of the 4-row block, columns 4p..4p+3; it receives its own column
    const int g4 = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
    int offA[2][FR], offB[2][FC];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int row = 8 * g4 + 4 * h + q4;
#pragma unroll
        for (int i = 0; i < FR; ++i) {
            const int ch = ((wr * WTN + i * 16) >> 3) + (p4 >> 1);
            offA[h][i] = row * RBA + 16 * (ch ^ wg2_swz<NCA>(row)) + 8 * (p4 & 1);
        }
#pragma unroll
        for (int j = 0; j < FC; ++j) {
            const int ch = ((wc * WTM + j * 16) >> 3) + (p4 >> 1);
            offB[h][j] = row * RBB + 16 * (ch ^ wg2_swz<NCB>(row)) + 8 * (p4 & 1);
        }
    }

    f32x4 acc[FR][FC];
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int j = 0; j < FC; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto compute = [&](int buf) {
        const char* A = smem + buf * BUF;
        const char* Bm = A + A_BYTES;
#pragma unroll
        for (int s = 0; s < KP / 32; ++s) {
            uint4 af[FR], bf[FC];
#pragma unroll
            for (int i = 0; i < FR; ++i) {
                const uint2 lo = lds_read_tr16(A + s * 32 * RBA + offA[0][i]);
                const uint2 hi = lds_read_tr16(A + s * 32 * RBA + offA[1][i]);
                af[i] = make_uint4(lo.x, lo.y, hi.x, hi.y);
            }
#pragma unroll
            for (int j = 0; j < FC; ++j) {
                const uint2 lo = lds_read_tr16(Bm + s * 32 * RBB + offB[0][j]);
                const uint2 hi = lds_read_tr16(Bm + s * 32 * RBB + offB[1][j]);
                bf[j] = make_uint4(lo.x, lo.y, hi.x, hi.y);
            }
#pragma unroll
            for (int i = 0; i < FR; ++i)
#pragma unroll
                for (int j = 0; j < FC; ++j) Mma<T>::run(acc[i][j], af[i], bf[j]);
        }
    };

    constexpr int D = NBUF - 1;  // stages in flight ahead of the one being computed
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < nst) issue(d);
    for (int k = 0; k < nst; ++k) {
        if constexpr (D == 2) {
            if (k + 1 < nst) wg2_wait_vm<PW>();  // stage k landed; stage k+1 may still fly
            else wg2_wait_vm<0>();
        } else {
            wg2_wait_vm<0>();
        }
        wg2_barrier();  // every wave's pieces landed; compute(k-1) done -> its buffer is free
        if (k + D < nst) issue((k + D) % NBUF);
        compute(k % NBUF);
    }
    // dW (torch layout [cout][cin_store][kh][kw]) += acc
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int j = 0; j < FC; ++j) {
            const int c = c0 + wc * WTM + j * 16 + (lane & 15);
            if (c >= p.cin_store) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wr * WTN + i * 16 + (lane >> 4) * 4 + r;
                if (n < p.cout) {
                    const long long e = (((long long)n * p.cin_store + c) * p.kh + ky) * p.kw + kx;
                    if (p.ws) p.ws[(long long)blockIdx.x * p.cout * p.cin_store * p.kh * p.kw + e] = acc[i][j][r];
                    else atomicAdd(p.dw + e, acc[i][j][r]);
                }
            }
        }
}

namespace {

template <typename T, int TN, int TM, int NBUF>
int launch_wgrad2_t(WgradParams p, hipStream_t st) {
    constexpr int KP = 64;
    constexpr int LDS = NBUF * KP * (TN + TM) * 2;
    const int ntn = (p.cout + TN - 1) / TN;
    p.ntc = (p.cin + TM - 1) / TM;
    const int ntap = p.kh * p.kw;
    p.nst = (int)(((long long)p.M + KP - 1) / KP);
    // about one wave of blocks (256 CUs x the blocks whose LDS fits one); >= 4 stages per split
    const int occ = (160 * 1024) / LDS;
    const SplitPlan s = plan_wgrad(p, p.nst, (long long)ntn * ntap * p.ntc, 256LL * (occ < 1 ? 1 : occ), 4);
    p.sps = s.per_split;
    YXH_CHECK_ARG(ntap * p.ntc < 65536 && ntn < 65536, "wgrad grid");
    hipLaunchKernelGGL((conv_wgrad2<T, TN, TM, NBUF>), dim3((unsigned)s.splits, ntn, ntap * p.ntc), dim3(256), 0, st,
                       p);
    YXH_CHECK_LAUNCH("conv_wgrad2");
    return ws_reduce(p, s.splits, st);
}

// cout x cin, ring depth
template <typename T>
int wgrad_glds_tile(int tile, const WgradParams& p, hipStream_t st) {
    switch (tile) {
        case 5: return launch_wgrad2_t<T, 128, 128, 3>(p, st);
        case 6: return launch_wgrad2_t<T, 128, 128, 2>(p, st);
        case 7: return launch_wgrad2_t<T, 64, 64, 3>(p, st);
        case 8: return launch_wgrad2_t<T, 64, 64, 2>(p, st);
        case 9: return launch_wgrad2_t<T, 128, 64, 3>(p, st);
        default: return launch_wgrad2_t<T, 64, 128, 3>(p, st);
    }
}

}  // namespace

int wgrad_glds_dispatch(int dtype, int tile, const WgradParams& p, hipStream_t st) {
    // 16-bit operands only: the router refuses fp32
    return dtype == YXH_BF16 ? wgrad_glds_tile<bf16>(tile, p, st) : wgrad_glds_tile<f16>(tile, p, st);
}

}  // namespace yxh
