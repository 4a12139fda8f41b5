// Training-mode BatchNorm and the channel reductions of the YOLOX training step on gfx950 (MI355X).
//
//  bn_stats        : BatchNorm2d training statistics (network_blocks.py:44-49 BaseConv.bn,
//                    eps/momentum from config.py:162-166): per-channel shifted sums in a
//                    fixed-order two-stage reduction, then mean / invstd / folded
//                    scale+shift and the running-stat update (unbiased var, momentum).
//  bn_act_fwd      : y*scale+shift -> act (SiLU/ReLU/LReLU) (+ Bottleneck residual,
//                    network_blocks.py:97-99) into a channel-slice view.
//  bn_act_bwd      : act' and BatchNorm backward: dgamma = sum dz*xhat, dbeta = sum dz,
//                    dx = gamma*invstd*(dz - dbeta/M - xhat*dgamma/M).
//  channel_sum     : bias gradients of the head's pred convs.
//  bn_frozen_stats : the same stats[4][C] table from the RUNNING statistics (a BatchNorm in eval mode,
//                    utils/model_utils.py:129-154 freeze_module): no reduction, nothing updated.
//  bn_frozen_act_bwd : backward of act(y*scale + shift) with constant scale / shift:
//                    dx = dout * act'(z) * scale, elementwise.
#include <cstdlib>

#include "train_common.hpp"

namespace yxh {

// ------------------------------------------------------------------ reductions
// Stage 1: block b reduces rows [b*rpb, (b+1)*rpb) into partial[b][2][C].
// Thread = (row lane, channel chunk of EPC channels); rows stride by the row lanes.
enum { RED_STATS = 0, RED_BWD = 1, RED_SUM = 2 };

struct RedArgs {
    TView x;          // activation (T): y for STATS/BWD, x for SUM
    TView g;          // fp32 gradient (BWD)
    const float* st;  // stats [4][C] = mean, invstd, scale, shift (BWD)
    int act, M, rpb;
    float* partial;
};

template <typename T, int MODE>
__global__ __launch_bounds__(256) void chan_reduce(RedArgs a) {
    constexpr int EPC = Chunk<T>::N;
    // one staging buffer for both sums in turn (8 KiB at 16 bits): beside the side stream's weight
    // gradients (up to ~140 KiB of LDS per CU) a 16 KiB block often found no room on a CU
    __shared__ float red[256 * EPC];
    // blockIdx.y = channel group of up to 256 16-byte chunks (yolox_x fp32: 1280 channels)
    const int C = a.x.C, cg = blockIdx.y * 256 * EPC, CL = min(C - cg, 256 * EPC), nch = CL / EPC;
    const int tid = threadIdx.x;
    const int q = tid % nch, rl = tid / nch, rpi = 256 / nch;
    float s1[EPC], s2[EPC], sh[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) s1[e] = s2[e] = sh[e] = 0.0f;
    const int c0 = cg + q * EPC;
    const T* xp = (const T*)a.x.ptr;
    if (MODE == RED_STATS && rl < rpi) {
        load_f<T, EPC>(xp + c0, sh);  // shift = pixel 0 (cancellation guard)
        if (blockIdx.x == 0 && rl == 0)
#pragma unroll
            for (int e = 0; e < EPC; ++e) a.partial[(long long)gridDim.x * 2 * C + c0 + e] = sh[e];
    }
    float sc[EPC], sf[EPC], mu[EPC], is[EPC];
    if (MODE == RED_BWD) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            mu[e] = a.st[c0 + e];
            is[e] = a.st[C + c0 + e];
            sc[e] = a.st[2 * C + c0 + e];
            sf[e] = a.st[3 * C + c0 + e];
        }
    }
    const int r0 = blockIdx.x * a.rpb, r1 = min(a.M, r0 + a.rpb);
    auto accum = [&](const float (&v)[EPC], const float (&gv)[EPC]) {
        if (MODE == RED_STATS) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const float d = v[e] - sh[e];
                s1[e] += d;
                s2[e] += d * d;
            }
        } else if (MODE == RED_SUM) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) s1[e] += v[e];
        } else {
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const float z = v[e] * sc[e] + sf[e];
                const float dz = gv[e] * act_grad<sizeof(T) == 4>(z, a.act);
                s1[e] += dz;
                s2[e] += dz * ((v[e] - mu[e]) * is[e]);
            }
        }
    };
    // U rows in flight per thread: all loads first, then the rows in order (the same
    // fixed summation order as one row at a time).  BWD holds y, the fp32 gradient and four
    // coefficient rows per channel: at U = 4 the 16-bit form took 159 VGPRs (3 waves per SIMD, so
    // the 1024-block grid ran in two rounds: the slowest kernel of the configs[4] step's main
    // stream); fp32 (4 channels per 16-byte chunk) fits 91 at U = 4
    constexpr int U = MODE == RED_BWD && sizeof(T) == 2 ? 2 : 4;
    if (rl < rpi) {
        int r = r0 + rl;
        for (; r + (U - 1) * rpi < r1; r += U * rpi) {
            float v[U][EPC], gv[U][EPC] = {};
#pragma unroll
            for (int u = 0; u < U; ++u) {
                load_f<T, EPC>(xp + vofs(a.x, r + u * rpi) + c0, v[u]);
                if (MODE == RED_BWD) load_f<float, EPC>((const float*)a.g.ptr + vofs(a.g, r + u * rpi) + c0, gv[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) accum(v[u], gv[u]);
        }
        for (; r < r1; r += rpi) {
            float v[EPC], gv[EPC] = {};
            load_f<T, EPC>(xp + vofs(a.x, r) + c0, v);
            if (MODE == RED_BWD) load_f<float, EPC>((const float*)a.g.ptr + vofs(a.g, r) + c0, gv);
            accum(v, gv);
        }
    }
    // thread t < C sums channel t over the row lanes (fixed order: deterministic), Σ1 then Σ2
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (k) __syncthreads();  // every thread is done reading the Σ1 stage
#pragma unroll
        for (int e = 0; e < EPC; ++e) red[tid * EPC + e] = k ? s2[e] : s1[e];
        __syncthreads();
        for (int c = tid; c < CL; c += 256) {
            const int qq = c / EPC, e = c - qq * EPC;
            float t = 0.0f;
            for (int l = 0; l < rpi; ++l) t += red[(l * nch + qq) * EPC + e];
            a.partial[((long long)blockIdx.x * 2 + k) * C + cg + c] = t;
        }
    }
}

struct FinArgs {
    const float* partial;  // [nblk][2][C] (+ [C] shift row for STATS)
    int nblk, C, M, mode;
    const float *gamma, *beta;
    float *rmean, *rvar;
    float eps, momentum;
    float* stats;        // STATS out [4][C] = mean, invstd, scale, shift
    float *out0, *out1;  // BWD: dgamma, dbeta; SUM: out0
    const float* st_in;  // BWD: the forward's stats [4][C]
    float* coef;         // BWD out [3][C]: dx = k1*dz + k2*(y - mean) + k3
};

// 4 channels per block, a wave per channel: each lane sums its strided share of the
// per-block partials in double (eight independent chains, so the loads of eight rows are in
// flight at once: the kernel is latency-bound, <= 512 partials per channel), then a
// fixed-order tree over the lanes: deterministic.
__global__ __launch_bounds__(256) void chan_finalize(FinArgs f) {
    __shared__ double red[2][256];
    const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + j;
    // eight independent chains: the <= 512 partials of a channel (red_blocks) arrive in ONE round of
    // loads per lane instead of two dependent rounds
    constexpr int U = 8;
    double a1[U], a2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) a1[u] = a2[u] = 0.0;
    if (c < f.C) {
        const long long rs = 2LL * f.C;  // partial row stride (one block's [2][C])
        const float* p0 = f.partial + c;
        for (int b = lane; b < f.nblk; b += 64 * U) {
            float v1[U], v2[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int bb = b + 64 * u;
                v1[u] = bb < f.nblk ? p0[(long long)bb * rs] : 0.0f;
                v2[u] = bb < f.nblk ? p0[(long long)bb * rs + f.C] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                a1[u] += v1[u];
                a2[u] += v2[u];
            }
        }
    }
    red[0][threadIdx.x] = ((a1[0] + a1[1]) + (a1[2] + a1[3])) + ((a1[4] + a1[5]) + (a1[6] + a1[7]));
    red[1][threadIdx.x] = ((a2[0] + a2[1]) + (a2[2] + a2[3])) + ((a2[4] + a2[5]) + (a2[6] + a2[7]));
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if (lane < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (lane != 0 || c >= f.C) return;
    double t1, t2;
    t1 = red[0][threadIdx.x];
    t2 = red[1][threadIdx.x];
    if (f.mode == RED_STATS) {
        const double m1 = t1 / f.M;
        const double mean = (double)f.partial[(long long)f.nblk * 2 * f.C + c] + m1;
        double var = t2 / f.M - m1 * m1;
        if (var < 0) var = 0;
        const float invstd = (float)(1.0 / sqrt(var + (double)f.eps));
        const float g = f.gamma ? f.gamma[c] : 1.0f, be = f.beta ? f.beta[c] : 0.0f;
        const float scale = g * invstd;
        f.stats[c] = (float)mean;
        f.stats[f.C + c] = invstd;
        f.stats[2 * f.C + c] = scale;
        f.stats[3 * f.C + c] = be - (float)mean * scale;
        if (f.rmean) {
            const float mo = f.momentum;
            f.rmean[c] = (1.0f - mo) * f.rmean[c] + mo * (float)mean;
            const double unb = f.M > 1 ? var * f.M / (f.M - 1) : var;
            f.rvar[c] = (1.0f - mo) * f.rvar[c] + mo * (float)unb;
        }
    } else if (f.mode == RED_BWD) {
        f.out0[c] = (float)t2;  // dgamma = sum dz * xhat
        f.out1[c] = (float)t1;  // dbeta = sum dz
        const float is = f.st_in[f.C + c], inv_m = 1.0f / (float)f.M;
        const float k1 = (f.gamma ? f.gamma[c] : 1.0f) * is;
        f.coef[c] = k1;
        f.coef[f.C + c] = -k1 * is * ((float)t2 * inv_m);
        f.coef[2 * f.C + c] = -k1 * ((float)t1 * inv_m);
    } else {
        f.out0[c] = (float)t1;
    }
}

// ------------------------------------------------------------------ elementwise
template <typename T>
__global__ __launch_bounds__(256) void bn_act_fwd(TView y, const float* st, int act, TView res, TView out, int M) {
    constexpr int EPC = Chunk<T>::N;
    const int C = y.C, nch = C / EPC;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)M * nch) return;
    const int m = (int)(idx / nch), c0 = (int)(idx - (long long)m * nch) * EPC;
    float v[EPC], sc[EPC], sf[EPC];
    load_f<T, EPC>((const T*)y.ptr + vofs(y, m) + c0, v);
    load_f<float, EPC>(st + 2 * C + c0, sc);
    load_f<float, EPC>(st + 3 * C + c0, sf);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        const float z = v[e] * sc[e] + sf[e];
        // training keeps the IEEE-divide SiLU on every dtype: the SimOTA assignment
        // downstream is discrete, so the bf16/f16 step stays bit-stable across builds
        v[e] = (act == YXH_ACT_SILU && sizeof(T) != 4) ? z / (1.0f + __expf(-z)) : apply_act<sizeof(T) == 4>(z, act);
    }
    if (res.ptr) {
        float r[EPC];
        load_f<T, EPC>((const T*)res.ptr + vofs(res, m) + c0, r);
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] += r[e];
    }
    store_f<T, EPC>((T*)out.ptr + vofs(out, m) + c0, v);
}

// dx = k1*dz + k2*(y - mean) + k3 with the per-channel coefficients chan_finalize derived
// from dgamma / dbeta (BatchNorm's backward with batch statistics).
template <typename T>
__global__ __launch_bounds__(256) void bn_act_bwd_apply(TView y, TView g, const float* st, const float* coef,
                                                       int act, int M, T* dx) {
    constexpr int EPC = Chunk<T>::N;
    const int C = y.C, nch = C / EPC;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)M * nch) return;
    const int m = (int)(idx / nch), c0 = (int)(idx - (long long)m * nch) * EPC;
    float v[EPC], gv[EPC], o[EPC], mu[EPC], sc[EPC], sf[EPC], k1[EPC], k2[EPC], k3[EPC];
    load_f<T, EPC>((const T*)y.ptr + vofs(y, m) + c0, v);
    load_f<float, EPC>((const float*)g.ptr + vofs(g, m) + c0, gv);
    load_f<float, EPC>(st + c0, mu);
    load_f<float, EPC>(st + 2 * C + c0, sc);
    load_f<float, EPC>(st + 3 * C + c0, sf);
    load_f<float, EPC>(coef + c0, k1);
    load_f<float, EPC>(coef + C + c0, k2);
    load_f<float, EPC>(coef + 2 * C + c0, k3);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        const float z = v[e] * sc[e] + sf[e];
        const float dz = gv[e] * act_grad<sizeof(T) == 4>(z, act);
        o[e] = k1[e] * dz + k2[e] * (v[e] - mu[e]) + k3[e];
    }
    store_f<T, EPC>(dx + (long long)m * C + c0, o);
}

// ------------------------------------------------------------------ frozen BatchNorm (eval mode)
// One thread per channel; the operation order of chan_finalize's STATS branch (invstd from a double
// sqrt, scale = gamma * invstd, shift = beta - mean * scale in float).
__global__ __launch_bounds__(256) void bn_frozen_stats_k(const float* gamma, const float* beta, const float* rmean,
                                                         const float* rvar, float eps, int C, float* stats) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float mean = rmean[c];
    const float invstd = (float)(1.0 / sqrt((double)rvar[c] + (double)eps));
    const float g = gamma ? gamma[c] : 1.0f, be = beta ? beta[c] : 0.0f;
    const float scale = g * invstd;
    stats[c] = mean;
    stats[C + c] = invstd;
    stats[2 * C + c] = scale;
    stats[3 * C + c] = be - mean * scale;
}

// n <= N live elements at p: one 16-byte access per 16 bytes when the chunk is whole and p is 16-byte
// aligned, element by element otherwise (the last chunk of a row whose channel count is no multiple of
// the chunk, rows of a view that do not start on 16 bytes); lanes past n read nothing and hold 0.
template <typename T, int N>
__device__ __forceinline__ void load_n(const T* p, int n, float (&o)[N]) {
    if (n == N && ((uintptr_t)p & 15u) == 0) {
        load_f<T, N>(p, o);
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) o[e] = e < n ? to_f32(p[e]) : 0.0f;
    }
}

template <typename T, int N>
__device__ __forceinline__ void store_n(T* p, int n, const float (&o)[N]) {
    if (n == N && ((uintptr_t)p & 15u) == 0) {
        store_f<T, N>(p, o);
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e)
            if (e < n) p[e] = from_f32<T>(o[e]);
    }
}

// A lane per (pixel, 16-byte chunk of channels): y (T view), dout (fp32 view), scale / shift rows of the
// stats table -> dx (T, dense [M][C]).  nch = ceil(C / EPC): the last chunk of a row may be partial.
template <typename T>
__global__ __launch_bounds__(256) void bn_frozen_act_bwd_k(TView y, TView g, const float* st, int act, int M, T* dx) {
    constexpr int EPC = Chunk<T>::N;
    const int C = y.C, nch = (C + EPC - 1) / EPC;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)M * nch) return;
    const int m = (int)(idx / nch), c0 = (int)(idx - (long long)m * nch) * EPC;
    const int n = min(EPC, C - c0);
    float v[EPC], gv[EPC], sc[EPC], sf[EPC], o[EPC];
    load_n<T, EPC>((const T*)y.ptr + vofs(y, m) + c0, n, v);
    load_n<float, EPC>((const float*)g.ptr + vofs(g, m) + c0, n, gv);
    load_n<float, EPC>(st + 2 * C + c0, n, sc);
    load_n<float, EPC>(st + 3 * C + c0, n, sf);
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        const float z = v[e] * sc[e] + sf[e];
        o[e] = gv[e] * act_grad<sizeof(T) == 4>(z, act) * sc[e];
    }
    store_n<T, EPC>(dx + (long long)m * C + c0, n, o);
}

// ================================================================== host
namespace {

constexpr int kRedMaxBlocks = 1024;

// Reduction blocks: ~8 rows per thread, at most YXH_RED_BLOCKS (default 512: two 4-wave blocks
// per CU, one round; chan_finalize then reads 512 partials per channel instead of 1024 -- it is
// latency-bound on the strided partial rows and runs once per BatchNorm per pass)
int red_cap() {
    static const int cap = [] {
        const char* e = getenv("YXH_RED_BLOCKS");
        const int v = e ? atoi(e) : 512;
        return v < 1 ? 1 : v > kRedMaxBlocks ? kRedMaxBlocks : v;
    }();
    return cap;
}

int red_blocks(int M, int C, int dt, int* rpb) {
    const int nch = C / (16 / esz(dt));
    const int rpi = nch >= 256 ? 1 : 256 / nch;
    // ~8 rows per thread (2-4 in flight).  (~32 rows per thread left 4x fewer partials for chan_finalize
    // but too few blocks in flight for the mid-size fp32 maps: configs[2] 570 -> 527 img/s, round 5)
    int nblk = (int)(((long long)M + rpi * 8 - 1) / (rpi * 8));
    const int cap = red_cap();
    nblk = nblk < 1 ? 1 : (nblk > cap ? cap : nblk);
    *rpb = (M + nblk - 1) / nblk;
    return (M + *rpb - 1) / *rpb;
}

template <int MODE>
int launch_reduce(int dt, const RedArgs& a, int nblk, hipStream_t st) {
    const int per = 256 * (16 / esz(dt));  // channels per group (256 chunks)
    const dim3 grid(nblk, (a.x.C + per - 1) / per);
    if (dt == YXH_BF16) hipLaunchKernelGGL((chan_reduce<bf16, MODE>), grid, dim3(256), 0, st, a);
    else if (dt == YXH_F16) hipLaunchKernelGGL((chan_reduce<f16, MODE>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((chan_reduce<float, MODE>), grid, dim3(256), 0, st, a);
    YXH_CHECK_LAUNCH("chan_reduce");
    return YXH_OK;
}

}  // namespace

// partials [nblk][2][C] + the stats shift row [C] + the backward coefficients [3][C]
size_t reduce_workspace(int C) { return (size_t)(kRedMaxBlocks * 2 + 4) * C * sizeof(float); }

namespace {

int run_reduce(int mode, int dt, int B, const yxh_src* x, const yxh_src* g, const float* stats, int act,
               void* ws, size_t ws_bytes, FinArgs f, hipStream_t st) {
    const int C = x->channels;
    YXH_CHECK_ARG(B > 0, "batch %d", B);
    YXH_CHECK_ARG(C > 0 && C % (16 / esz(dt)) == 0, "reduction: %d channels not in 16-byte chunks", C);
    YXH_CHECK_ARG(ws && ws_bytes >= reduce_workspace(C), "reduction workspace too small");
    RedArgs a{};
    a.x = tview(x, C);
    a.g = tview(g, C);
    a.st = stats;
    a.act = act;
    const long long M = (long long)B * x->h * x->w;
    YXH_CHECK_ARG(M < (1LL << 31), "too many pixels");
    a.M = (int)M;
    const int nblk = red_blocks(a.M, C, dt, &a.rpb);
    a.partial = (float*)ws;
    int rc = mode == RED_STATS ? launch_reduce<RED_STATS>(dt, a, nblk, st)
             : mode == RED_BWD ? launch_reduce<RED_BWD>(dt, a, nblk, st)
                               : launch_reduce<RED_SUM>(dt, a, nblk, st);
    if (rc) return rc;
    f.partial = (const float*)ws;
    f.nblk = nblk;
    f.C = C;
    f.M = a.M;
    f.mode = mode;
    hipLaunchKernelGGL(chan_finalize, dim3((C + 3) / 4), dim3(256), 0, st, f);
    YXH_CHECK_LAUNCH("chan_finalize");
    return YXH_OK;
}

}  // namespace

int bn_stats(int dt, int B, const yxh_src* y, const float* gamma, const float* beta, float* rmean, float* rvar,
             float eps, float momentum, float* stats, void* ws, size_t ws_bytes, hipStream_t st) {
    if (int rc = check_view(y, dt, "bn_stats y")) return rc;
    YXH_CHECK_ARG(stats, "bn_stats: null stats");
    YXH_CHECK_ARG(!rmean == !rvar, "running mean/var must both be given or both NULL");
    FinArgs f{};
    f.gamma = gamma;
    f.beta = beta;
    f.rmean = rmean;
    f.rvar = rvar;
    f.eps = eps;
    f.momentum = momentum;
    f.stats = stats;
    return run_reduce(RED_STATS, dt, B, y, nullptr, nullptr, 0, ws, ws_bytes, f, st);
}

int bn_act_fwd_launch(int dt, int B, const yxh_src* y, const float* stats, int act, const yxh_src* res,
                      const yxh_src* out, hipStream_t st) {
    if (int rc = check_view(y, dt, "bn_act_fwd y")) return rc;
    if (int rc = check_view(out, dt, "bn_act_fwd out")) return rc;
    if (res && res->ptr)
        if (int rc = check_view(res, dt, "bn_act_fwd residual")) return rc;
    const int C = y->channels;
    YXH_CHECK_ARG(out->channels == C && out->h == y->h && out->w == y->w, "bn_act_fwd: out view shape");
    YXH_CHECK_ARG(!res || !res->ptr || (res->channels == C && res->h == y->h && res->w == y->w),
                  "bn_act_fwd: residual view shape");
    YXH_CHECK_ARG(stats && a16(stats) && B > 0, "bn_act_fwd: stats (16-byte aligned) / batch");
    const long long M = (long long)B * y->h * y->w;
    const long long total = M * (C / (16 / esz(dt)));
    TView r = tview(res && res->ptr ? res : nullptr, C);
    dim3 grid((unsigned)((total + 255) / 256));
#define YXH_BNF(T) hipLaunchKernelGGL(bn_act_fwd<T>, grid, dim3(256), 0, st, tview(y, C), stats, act, r, tview(out, C), (int)M)
    if (dt == YXH_BF16) YXH_BNF(bf16);
    else if (dt == YXH_F16) YXH_BNF(f16);
    else YXH_BNF(float);
#undef YXH_BNF
    YXH_CHECK_LAUNCH("bn_act_fwd");
    return YXH_OK;
}

int bn_act_bwd_launch(int dt, int B, const yxh_src* y, const yxh_src* dout, const float* stats, const float* gamma,
                      int act, float* dgamma, float* dbeta, void* dx, void* ws, size_t ws_bytes, hipStream_t st) {
    if (int rc = check_view(y, dt, "bn_act_bwd y")) return rc;
    if (int rc = check_view(dout, YXH_F32, "bn_act_bwd dout")) return rc;
    const int C = y->channels;
    YXH_CHECK_ARG(dout->channels == C && dout->h == y->h && dout->w == y->w, "bn_act_bwd: dout view shape");
    YXH_CHECK_ARG(stats && dgamma && dbeta && dx && a16(dx), "bn_act_bwd: null / unaligned outputs");
    YXH_CHECK_ARG(a16(stats), "bn_act_bwd: stats not 16-byte aligned");
    FinArgs f{};
    f.out0 = dgamma;
    f.out1 = dbeta;
    f.gamma = gamma;
    f.st_in = stats;
    float* coef = (float*)ws + (size_t)(kRedMaxBlocks * 2 + 1) * C;
    f.coef = coef;
    if (int rc = run_reduce(RED_BWD, dt, B, y, dout, stats, act, ws, ws_bytes, f, st)) return rc;
    const long long M = (long long)B * y->h * y->w;
    const long long total = M * (C / (16 / esz(dt)));
    dim3 grid((unsigned)((total + 255) / 256));
#define YXH_BNB(T)                                                                                                 \
    hipLaunchKernelGGL(bn_act_bwd_apply<T>, grid, dim3(256), 0, st, tview(y, C), tview(dout, C), stats, coef, act, \
                       (int)M, (T*)dx)
    if (dt == YXH_BF16) YXH_BNB(bf16);
    else if (dt == YXH_F16) YXH_BNB(f16);
    else YXH_BNB(float);
#undef YXH_BNB
    YXH_CHECK_LAUNCH("bn_act_bwd_apply");
    return YXH_OK;
}

int bn_frozen_stats_launch(const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps,
                           int C, float* stats, hipStream_t st) {
    YXH_CHECK_ARG(C > 0, "bn_frozen_stats: %d channels", C);
    YXH_CHECK_ARG(rmean && rvar && stats, "bn_frozen_stats: null running statistics / stats");
    hipLaunchKernelGGL(bn_frozen_stats_k, dim3((C + 255) / 256), dim3(256), 0, st, gamma, beta, rmean, rvar, eps, C,
                       stats);
    YXH_CHECK_LAUNCH("bn_frozen_stats");
    return YXH_OK;
}

int bn_frozen_act_bwd_launch(int dt, int B, const yxh_src* y, const yxh_src* dout, const float* stats, int act,
                             void* dx, hipStream_t st) {
    YXH_CHECK_ARG(dt == YXH_F32 || dt == YXH_BF16 || dt == YXH_F16, "bn_frozen_act_bwd: dtype %d", dt);
    YXH_CHECK_ARG(y && y->ptr && dout && dout->ptr && stats && dx, "bn_frozen_act_bwd: null view / stats / dx");
    const int C = y->channels;
    YXH_CHECK_ARG(B > 0 && C > 0 && y->h > 0 && y->w > 0, "bn_frozen_act_bwd: batch %d, %d channels, %d x %d", B, C,
                  y->h, y->w);
    YXH_CHECK_ARG(dout->channels == C && dout->h == y->h && dout->w == y->w, "bn_frozen_act_bwd: dout view shape");
    YXH_CHECK_ARG(y->upsample == 0 && dout->upsample == 0, "bn_frozen_act_bwd: upsampled views are not read here");
    // rows inside their pixel stride, images inside their batch stride: every access stays in the views
    YXH_CHECK_ARG(y->cstride >= C && dout->cstride >= C && y->bstride >= (long long)y->h * y->w * y->cstride &&
                      dout->bstride >= (long long)y->h * y->w * dout->cstride,
                  "bn_frozen_act_bwd: view strides smaller than the view");
    YXH_CHECK_ARG(((uintptr_t)y->ptr % esz(dt)) == 0 && ((uintptr_t)dout->ptr & 3u) == 0 &&
                      ((uintptr_t)dx % esz(dt)) == 0 && ((uintptr_t)stats & 3u) == 0,
                  "bn_frozen_act_bwd: pointers not aligned to their element");
    const long long M = (long long)B * y->h * y->w;
    YXH_CHECK_ARG(M < (1LL << 31), "too many pixels");
    const int epc = 16 / esz(dt);
    const long long total = M * ((C + epc - 1) / epc);
    YXH_CHECK_ARG((total + 255) / 256 < (1LL << 31), "bn_frozen_act_bwd: grid too large");
    dim3 grid((unsigned)((total + 255) / 256));
#define YXH_BNZ(T) \
    hipLaunchKernelGGL(bn_frozen_act_bwd_k<T>, grid, dim3(256), 0, st, tview(y, C), tview(dout, C), stats, act, (int)M, (T*)dx)
    if (dt == YXH_BF16) YXH_BNZ(bf16);
    else if (dt == YXH_F16) YXH_BNZ(f16);
    else YXH_BNZ(float);
#undef YXH_BNZ
    YXH_CHECK_LAUNCH("bn_frozen_act_bwd");
    return YXH_OK;
}

int channel_sum_launch(int dt, int B, const yxh_src* x, float* out, void* ws, size_t ws_bytes, hipStream_t st) {
    if (int rc = check_view(x, dt, "channel_sum x")) return rc;
    YXH_CHECK_ARG(out, "channel_sum: null out");
    FinArgs f{};
    f.out0 = out;
    return run_reduce(RED_SUM, dt, B, x, nullptr, nullptr, 0, ws, ws_bytes, f, st);
}

}  // namespace yxh
