// Weight-gradient tiles 1-4, any operand type and conv shape (the by-shape default, tile 0, picks
// among them).
//  conv_wgrad      : dW[n][c][ky][kx] = sum_pixels dY[n] * X[c](tap) on MFMA: both
//                    operands are pixel-major (NHWC), so the loader transposes 16-byte
//                    chunks in registers (v_perm) and the LDS image is the forward
//                    kernel's [K chunk][row] layout with K = pixels; split over pixel
//                    ranges, one tap per block.
#include "wgrad.hpp"

namespace yxh {

// The zero chunk invalid lanes read.  Without relocatable device code each unit needs its own
// (wgrad_glds.hip has another); an external symbol of the unit's own name, so the kernels reach it as before.
inline namespace wgrad_reg {
__device__ __attribute__((aligned(16))) uint4 g_wg_zero[4];
}

// In-register transpose of an EPC x EPC block of T: a[e] = EPC channels of pixel e ->
// a[j] = EPC pixels of channel j.
__device__ __forceinline__ void transpose_chunks(uint4 (&a)[8]) {  // 16-bit elements
    uint32_t w[8][4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        w[e][0] = a[e].x; w[e][1] = a[e].y; w[e][2] = a[e].z; w[e][3] = a[e].w;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t sel = (j & 1) ? 0x07060302u : 0x05040100u;
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = __builtin_amdgcn_perm(w[2 * q + 1][j >> 1], w[2 * q][j >> 1], sel);
        a[j] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}
__device__ __forceinline__ void transpose_chunks(uint4 (&a)[4]) {  // 32-bit elements
    uint4 b[4];
    b[0] = make_uint4(a[0].x, a[1].x, a[2].x, a[3].x);
    b[1] = make_uint4(a[0].y, a[1].y, a[2].y, a[3].y);
    b[2] = make_uint4(a[0].z, a[1].z, a[2].z, a[3].z);
    b[3] = make_uint4(a[0].w, a[1].w, a[2].w, a[3].w);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = b[j];
}

// LDS row placement of the wgrad image: the chunk XOR of the forward kernel plus
// (r >> 3) & 7 on the low bits.  A loader lane writes 8 consecutive rows of one chunk and
// neighbouring lanes are 8 rows apart, so without the second term every lane of a
// ds_write_b128 hits the same 32-bank group; with it 8 lanes cover all banks.  A fragment
// read (16 consecutive rows, one chunk) stays a permutation of one 256-byte block.
__device__ __forceinline__ int wg_row(int r, int sw) { return r ^ sw ^ ((r >> 3) & 7); }

template <typename T, int TN, int TM, int WR, int WC, int KS>
__global__ __launch_bounds__(256) void conv_wgrad(WgradParams p) {
    constexpr int EPC = Chunk<T>::N;
    constexpr int CPR = 4 * KS;           // 16-byte chunks (of EPC pixels) per row per stage
    static_assert(CPR * EPC > 0, "stage");
    constexpr int NA = (TN / EPC) * CPR;  // transpose items: A = dY rows (cout)
    constexpr int NB = (TM / EPC) * CPR;  //                  B = X rows (cin of the tap)
    constexpr int NIT = (NA + NB + 255) / 256;
    constexpr int WTN = TN / WR, WTM = TM / WC;
    constexpr int FR = WTN / 16, FC = WTM / 16;
    constexpr int A_BYTES = TN * CPR * 16, B_BYTES = TM * CPR * 16;
    constexpr int BUF = A_BYTES + B_BYTES;
    static_assert(WR * WC == 4 && FR >= 1 && FC >= 1, "tile");
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WC, wc = wave % WC;
    const int n0 = blockIdx.y * TN;
    const int tap = blockIdx.z / p.ntc, c0 = (blockIdx.z - tap * p.ntc) * TM;
    const int ky = tap / p.kw, kx = tap - ky * p.kw;
    const int st0 = blockIdx.x * p.sps, st1 = min(p.nst, st0 + p.sps);

    uint4 rg[NIT][EPC];
    // K runs over "runs": EPC consecutive output pixels of one output row (rows padded to
    // a multiple of EPC), so a run is one (b, oy, ox0) decomposition and its input pixels
    // for the tap are one input row at stride `stride`.  Loads are branch-free: invalid
    // lanes read a zero chunk.
    const int rpr = (p.out_w + EPC - 1) / EPC, rpi = rpr * p.out_h;
    auto gload = [&](int stg) {
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int it = tid + 256 * i;
            if (it >= NA + NB) continue;
            const bool isa = it < NA;
            const int jt = isa ? it : it - NA;
            const int rows = isa ? TN : TM;
            const int ci = jt % (rows / EPC), pc = jt / (rows / EPC);
            const int R = stg * CPR + pc;
            const int b = R / rpi, rem = R - b * rpi;
            const int oy = rem / rpr, ox0 = (rem - oy * rpr) * EPC;
            const bool run_ok = b < p.B;
            const T* zero = (const T*)g_wg_zero;
            if (isa) {
                const int n = n0 + ci * EPC;
                const bool ok = run_ok && n < p.cout;
                const T* base = (const T*)p.dy + (ok ? (long long)b * p.dybs + n : 0);
                const int o0 = (oy * p.out_w + ox0) * p.dycs;
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const bool v = ok && ox0 + e < p.out_w;
                    rg[i][e] = *(const uint4*)(v ? base + o0 + e * p.dycs : zero);
                }
            } else {
                int c = c0 + ci * EPC;
                int s = 0;
                if (p.nsrc == 2 && c >= p.src0_ch) {
                    s = 1;
                    c -= p.src0_ch;
                }
                const int iy = oy * p.stride - p.pad + ky;
                const bool ok = run_ok && c0 + ci * EPC < p.cin && iy >= 0 && iy < p.in_h;
                const int up = p.sup[s], scs = p.scs[s];
                const T* base = (const T*)p.sptr[s] + (ok ? (long long)b * p.sbs[s] + c : 0);
                const int rowoff = (iy >> up) * p.sw[s];
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const int ix = (ox0 + e) * p.stride - p.pad + kx;
                    const bool v = ok && ox0 + e < p.out_w && ix >= 0 && ix < p.in_w;
                    rg[i][e] = *(const uint4*)(v ? base + (rowoff + (ix >> up)) * scs : zero);
                }
            }
        }
    };
    auto lstore = [&](int buf) {
        char* A = smem + buf * BUF;
        char* B = A + A_BYTES;
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int it = tid + 256 * i;
            if (it >= NA + NB) continue;
            transpose_chunks(rg[i]);
            const bool isa = it < NA;
            const int jt = isa ? it : it - NA;
            const int rows = isa ? TN : TM;
            const int ci = jt % (rows / EPC), pc = jt / (rows / EPC);
            const int sw_ = 2 * (pc & 3) + (pc >> 2);
            char* base = isa ? A : B;
#pragma unroll
            for (int j = 0; j < EPC; ++j) {
                const int r = ci * EPC + j;
                *(uint4*)(base + (pc * rows + wg_row(r, sw_)) * 16) = rg[i][j];
            }
        }
    };

    f32x4 acc[FR][FC];
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int j = 0; j < FC; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4;
    auto compute = [&](int buf) {
        const char* A = smem + buf * BUF;
        const char* B = A + A_BYTES;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int chunk = s * 4 + fq, sw_ = 2 * fq + s;
            uint4 af[FR], bf[FC];
#pragma unroll
            for (int i = 0; i < FR; ++i) af[i] = *(const uint4*)(A + (chunk * TN + wg_row(wr * WTN + i * 16 + frow, sw_)) * 16);
#pragma unroll
            for (int j = 0; j < FC; ++j) bf[j] = *(const uint4*)(B + (chunk * TM + wg_row(wc * WTM + j * 16 + frow, sw_)) * 16);
#pragma unroll
            for (int i = 0; i < FR; ++i)
#pragma unroll
                for (int j = 0; j < FC; ++j) Mma<T>::run(acc[i][j], af[i], bf[j]);
        }
    };

    if (st0 < st1) {
        gload(st0);
        lstore(0);
        __syncthreads();
        for (int k = st0; k < st1; ++k) {
            const int cur = (k - st0) & 1;
            if (k + 1 < st1) gload(k + 1);
            compute(cur);
            if (k + 1 < st1) lstore(cur ^ 1);
            __syncthreads();
        }
    }
    // dW (torch layout [cout][cin_store][kh][kw]) += acc
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int j = 0; j < FC; ++j) {
            const int c = c0 + wc * WTM + j * 16 + frow;
            if (c >= p.cin_store) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wr * WTN + i * 16 + fq * 4 + r;
                if (n < p.cout) {
                    const long long e = (((long long)n * p.cin_store + c) * p.kh + ky) * p.kw + kx;
                    if (p.ws) p.ws[(long long)blockIdx.x * p.cout * p.cin_store * p.kh * p.kw + e] = acc[i][j][r];
                    else atomicAdd(p.dw + e, acc[i][j][r]);
                }
            }
        }
}

namespace {

template <typename T, int TN, int TM, int WR, int WC, int KS>
int launch_wgrad_t(WgradParams p, hipStream_t st) {
    constexpr int EPC = Chunk<T>::N;
    const int ntn = (p.cout + TN - 1) / TN;
    p.ntc = (p.cin + TM - 1) / TM;
    const int ntap = p.kh * p.kw;
    p.nst = (int)(((long long)p.B * p.out_h * ((p.out_w + EPC - 1) / EPC) + 4 * KS - 1) / (4 * KS));
    // ~2 blocks per CU over the whole grid; at least 8 stages per split
    const SplitPlan s = plan_wgrad(p, p.nst, (long long)ntn * ntap * p.ntc, wgrad_target_blocks(), 8);
    p.sps = s.per_split;
    YXH_CHECK_ARG(ntap * p.ntc < 65536 && ntn < 65536, "wgrad grid");
    hipLaunchKernelGGL((conv_wgrad<T, TN, TM, WR, WC, KS>), dim3((unsigned)s.splits, ntn, ntap * p.ntc), dim3(256), 0,
                       st, p);
    YXH_CHECK_LAUNCH("conv_wgrad");
    return ws_reduce(p, s.splits, st);
}

// cout x cin, waves; 2 slabs per stage (4 for tile 1 at 16 bits: 128 pixels)
template <typename T>
int wgrad_reg_tile(int tile, const WgradParams& p, hipStream_t st) {
    switch (tile) {
        case 1: return sizeof(T) == 4 ? launch_wgrad_t<T, 64, 64, 2, 2, 2>(p, st) : launch_wgrad_t<T, 64, 64, 2, 2, 4>(p, st);
        case 2: return launch_wgrad_t<T, 128, 128, 2, 2, 2>(p, st);
        case 3: return launch_wgrad_t<T, 32, 64, 1, 4, 2>(p, st);
        default: return launch_wgrad_t<T, 16, 64, 1, 4, 2>(p, st);
    }
}

}  // namespace

int wgrad_reg_dispatch(int dtype, int tile, const WgradParams& p, hipStream_t st) {
    if (dtype == YXH_BF16) return wgrad_reg_tile<bf16>(tile, p, st);
    if (dtype == YXH_F16) return wgrad_reg_tile<f16>(tile, p, st);
    return wgrad_reg_tile<float>(tile, p, st);
}

}  // namespace yxh
