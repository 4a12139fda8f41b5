// The rest of YoloxModule's backward pass on gfx950 (MI355X) besides BatchNorm (train_bn.hip) and
// the weight gradients (wgrad*.hip).  The data-gradient convolutions run on the forward conv
// kernels with transposed/flipped weights, which the packers here produce.
//
//  pack_dgrad      : one conv's data-gradient weights (yxh_pack_dgrad_weight).
//  pack_batch      : every repack of a training step in one launch.
//  spp_bwd         : max_pool2d(5/9/13, s1) backward (first max in row-major scan, as
//                    torch) + the identity branch of SPPBottleneck's concat.
//  upsample_bwd    : nn.Upsample(nearest x2) backward (2x2 sums), accumulated.
#include "train_common.hpp"

namespace yxh {

// dgrad weights: w [cout][cin][kh][kw] fp32 -> [c_count][kh][kw][cout_pad] of T, taps
// flipped (ky -> kh-1-ky), input channels [c_begin, c_begin + c_count).
template <typename T>
__global__ __launch_bounds__(256) void pack_dgrad(const float* w, int cout, int cin, int kh, int kw, int c_begin,
                                                  int c_count, int cout_pad, T* out) {
    const long long total = (long long)c_count * kh * kw * cout_pad;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int n = (int)(idx % cout_pad);
    const int t = (int)((idx / cout_pad) % (kh * kw));
    const int c = (int)(idx / ((long long)cout_pad * kh * kw));
    const int ky = t / kw, kx = t - ky * kw;
    float v = 0.0f;
    if (n < cout) v = w[(((long long)n * cin + c_begin + c) * kh + (kh - 1 - ky)) * kw + (kw - 1 - kx)];
    out[idx] = from_f32<T>(v);
}

// Every repack of a training step in one launch: block b belongs to the last job whose
// block0 <= b (binary search over the job table, which stays in L2); element order and
// values as fold_bn_pack without BN (kind FWD) and pack_dgrad (kind DGRAD).
template <typename T>
__global__ __launch_bounds__(256) void pack_batch(const yxh_pack_job* jobs, int njobs) {
    const int b = blockIdx.x;
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const yxh_pack_job& j = jobs[lo];
    const long long idx = (long long)(b - j.block0) * 256 + threadIdx.x;
    const int taps = j.kh * j.kw;
    if (j.kind == YXH_PACK_FWD) {
        const long long total = (long long)j.cout * taps * j.pad;
        if (idx >= total) return;
        const int c = (int)(idx % j.pad);
        const int t = (int)((idx / j.pad) % taps);
        const int n = (int)(idx / ((long long)j.pad * taps));
        const int ky = t / j.kw, kx = t - ky * j.kw;
        const float v = c < j.cin ? j.w[(((long long)n * j.cin + c) * j.kh + ky) * j.kw + kx] : 0.0f;
        ((T*)j.out)[idx] = from_f32<T>(v);
        if (t == 0 && c == 0 && j.bias_out) j.bias_out[n] = j.cb ? j.cb[n] : 0.0f;
    } else {
        const long long total = (long long)j.c_count * taps * j.pad;
        if (idx >= total) return;
        const int n = (int)(idx % j.pad);
        const int t = (int)((idx / j.pad) % taps);
        const int c = (int)(idx / ((long long)j.pad * taps));
        const int ky = t / j.kw, kx = t - ky * j.kw;
        float v = 0.0f;
        if (n < j.cout) v = j.w[(((long long)n * j.cin + j.c_begin + c) * j.kh + (j.kh - 1 - ky)) * j.kw + (j.kw - 1 - kx)];
        ((T*)j.out)[idx] = from_f32<T>(v);
    }
}

// ------------------------------------------------------------------ SPP / upsample backward
// Block = (CPB channels, image), 1024 threads: the plane lives in LDS.  Per pool radius r (2, 4, 6):
// horizontal pass -> first max column hcol of each row window; vertical pass -> first max row brow
// among those = torch's argmax (first maximum in row-major scan, -inf padding): output (oy, ox)
// routes its gradient to pixel (brow, hcol[brow][ox]).  Every input pixel then GATHERS those
// gradients separably (fixed order, no atomics: deterministic): G1[y][ox] = the outputs of column
// ox whose argmax row is y (2r + 1 candidates), then pixel (y, x) sums the G1[y][ox] whose row-window
// max sits in column x (2r + 1 more) -- 2 (2r + 1) LDS reads per pixel instead of (2r + 1)^2.
// dx = dcat[:, :c] + the three gathers.  (The round-4 form gathered over the whole square window
// with one wave per SIMD: 3.4 ms of the configs[4] step's main stream for yolox_x's 40x40x640 SPP.)
template <typename T, int CPB>
__global__ __launch_bounds__(1024) void spp_bwd(TView cat, int H, int W, int c, const float* dcat, float* dx,
                                                int B) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int HW = H * W, n = HW * CPB;
    unsigned short* brow = (unsigned short*)sm;  // [3][n] argmax row of output q
    unsigned short* hcol = brow + 3 * n;         // [3][n] first max column of row y's window around x
    float* pl = (float*)(hcol + 3 * n);          // plane, then the staged output gradients of pool k
    float* hv = pl + n;                          // row-window max, then G1
    float* acc = hv + n;                         // the input gradient being gathered
    const int c0 = blockIdx.x * CPB, b = blockIdx.y, nt = blockDim.x;
    const T* xb = (const T*)cat.ptr + (long long)b * cat.bs;
    const float* db = dcat + (long long)b * HW * 4 * c;
    for (int q = threadIdx.x; q < n; q += nt) {
        const int pix = q / CPB, j = q - pix * CPB;
        const bool in = c0 + j < c;
        pl[q] = in ? to_f32(xb[(long long)pix * cat.cs + c0 + j]) : 0.0f;
        acc[q] = in ? db[(long long)pix * 4 * c + c0 + j] : 0.0f;
    }
    __syncthreads();
    for (int k = 0; k < 3; ++k) {
        const int r = 2 + 2 * k;
        for (int q = threadIdx.x; q < n; q += nt) {
            const int pix = q / CPB, j = q - pix * CPB;
            const int y = pix / W, x = pix - y * W;
            float best = 0.0f;
            int bc = -1;
            for (int xx = max(0, x - r); xx <= min(W - 1, x + r); ++xx) {
                const float v = pl[(y * W + xx) * CPB + j];
                if (bc < 0 || v > best) {
                    best = v;
                    bc = xx;
                }
            }
            hv[q] = best;
            hcol[k * n + q] = (unsigned short)bc;
        }
        __syncthreads();
        for (int q = threadIdx.x; q < n; q += nt) {
            const int pix = q / CPB, j = q - pix * CPB;
            const int y = pix / W, x = pix - y * W;
            float best = 0.0f;
            int br = -1;
            for (int yy = max(0, y - r); yy <= min(H - 1, y + r); ++yy) {
                const float v = hv[(yy * W + x) * CPB + j];
                if (br < 0 || v > best) {
                    best = v;
                    br = yy;
                }
            }
            brow[k * n + q] = (unsigned short)br;
        }
        __syncthreads();
    }
    // the plane is dead: per pool, stage its output gradients, gather by columns, then by rows
    for (int k = 0; k < 3; ++k) {
        const int r = 2 + 2 * k;
        const unsigned short* bk = brow + k * n;
        const unsigned short* hk = hcol + k * n;
        for (int q = threadIdx.x; q < n; q += nt) {
            const int pix = q / CPB, j = q - pix * CPB;
            pl[q] = c0 + j < c ? db[(long long)pix * 4 * c + (k + 1) * c + c0 + j] : 0.0f;
        }
        __syncthreads();
        for (int q = threadIdx.x; q < n; q += nt) {  // G1[y][ox]
            const int pix = q / CPB, j = q - pix * CPB;
            const int y = pix / W, ox = pix - y * W;
            float g = 0.0f;
            for (int oy = max(0, y - r); oy <= min(H - 1, y + r); ++oy) {
                const int o = (oy * W + ox) * CPB + j;
                if (bk[o] == y) g += pl[o];
            }
            hv[q] = g;
        }
        __syncthreads();
        for (int q = threadIdx.x; q < n; q += nt) {
            const int pix = q / CPB, j = q - pix * CPB;
            const int y = pix / W, x = pix - y * W;
            float g = 0.0f;
            for (int ox = max(0, x - r); ox <= min(W - 1, x + r); ++ox) {
                const int o = (y * W + ox) * CPB + j;
                if (hk[o] == x) g += hv[o];
            }
            acc[q] += g;
        }
        __syncthreads();
    }
    for (int q = threadIdx.x; q < n; q += nt) {
        const int pix = q / CPB, j = q - pix * CPB;
        if (c0 + j < c) dx[((long long)b * HW + pix) * c + c0 + j] = acc[q];
    }
}

__global__ __launch_bounds__(256) void upsample_bwd(const float* g, int B, int h, int w, int C, float* dst) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nc4 = C / 4;
    if (idx >= (long long)B * h * w * nc4) return;
    const int c = (int)(idx % nc4) * 4;
    const long long m = idx / nc4;
    const int b = (int)(m / ((long long)h * w)), pix = (int)(m - (long long)b * h * w);
    const int y = pix / w, x = pix - y * w;
    const float* gb = g + (long long)b * 4 * h * w * C;
    float4 s = *(float4*)(dst + m * C + c);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const float4 u = *(const float4*)(gb + ((long long)(2 * y + dy) * 2 * w + 2 * x + dx) * C + c);
            s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
        }
    *(float4*)(dst + m * C + c) = s;
}

// ================================================================== host
int pack_dgrad_launch(const float* w, int cout, int cin, int kh, int kw, int c_begin, int c_count, int cout_pad, int dt,
                      void* out, hipStream_t st) {
    YXH_CHECK_ARG(w && out && a16(out), "pack_dgrad: null / unaligned");
    YXH_CHECK_ARG(cout > 0 && cin > 0 && kh > 0 && kw > 0 && c_begin >= 0 && c_count > 0 && c_begin + c_count <= cin &&
                      cout_pad >= cout,
                  "pack_dgrad geometry");
    const long long total = (long long)c_count * kh * kw * cout_pad;
    dim3 grid((unsigned)((total + 255) / 256));
    if (dt == YXH_BF16) hipLaunchKernelGGL(pack_dgrad<bf16>, grid, dim3(256), 0, st, w, cout, cin, kh, kw, c_begin, c_count, cout_pad, (bf16*)out);
    else if (dt == YXH_F16) hipLaunchKernelGGL(pack_dgrad<f16>, grid, dim3(256), 0, st, w, cout, cin, kh, kw, c_begin, c_count, cout_pad, (f16*)out);
    else if (dt == YXH_F32) hipLaunchKernelGGL(pack_dgrad<float>, grid, dim3(256), 0, st, w, cout, cin, kh, kw, c_begin, c_count, cout_pad, (float*)out);
    else {
        set_error("pack_dgrad dtype %d", dt);
        return YXH_EINVAL;
    }
    YXH_CHECK_LAUNCH("pack_dgrad");
    return YXH_OK;
}

int pack_batch_launch(const yxh_pack_job* jobs, int njobs, int total_blocks, int dt, hipStream_t st) {
    YXH_CHECK_ARG(jobs && njobs > 0 && total_blocks > 0, "pack_batch: empty job table");
    if (dt == YXH_BF16) hipLaunchKernelGGL(pack_batch<bf16>, dim3(total_blocks), dim3(256), 0, st, jobs, njobs);
    else if (dt == YXH_F16) hipLaunchKernelGGL(pack_batch<f16>, dim3(total_blocks), dim3(256), 0, st, jobs, njobs);
    else if (dt == YXH_F32) hipLaunchKernelGGL(pack_batch<float>, dim3(total_blocks), dim3(256), 0, st, jobs, njobs);
    else {
        set_error("pack_batch dtype %d", dt);
        return YXH_EINVAL;
    }
    YXH_CHECK_LAUNCH("pack_batch");
    return YXH_OK;
}

int spp_bwd_launch(int dt, int B, const yxh_src* cat, int c, const float* dcat, float* dx, hipStream_t st) {
    YXH_CHECK_ARG(cat && cat->ptr && dcat && dx && B > 0 && c > 0 && cat->cstride >= 4 * c, "spp_bwd arguments");
    const int HW = cat->h * cat->w;
    // LDS per channel and pixel: brow + hcol u16 [3] each, plane / row max / gradient f32
    constexpr size_t kPer = 6 + 6 + 12;
    const int cpb = (size_t)HW * 4 * kPer <= 160 * 1024 ? 4 : (size_t)HW * 2 * kPer <= 160 * 1024 ? 2 : 1;
    const size_t lds = (size_t)HW * cpb * kPer;
    YXH_CHECK_ARG(lds <= 160 * 1024 && HW < 65536, "spp_bwd plane %dx%d too large for LDS", cat->h, cat->w);
    dim3 grid((c + cpb - 1) / cpb, B);
    TView v = tview(cat, c);
#define YXH_SPPB(T, P)                                                                                     \
    do {                                                                                                   \
        (void)hipFuncSetAttribute((const void*)spp_bwd<T, P>, hipFuncAttributeMaxDynamicSharedMemorySize,  \
                                  (int)lds);                                                               \
        hipLaunchKernelGGL((spp_bwd<T, P>), grid, dim3(1024), lds, st, v, cat->h, cat->w, c, dcat, dx, B); \
    } while (0)
#define YXH_SPPB_T(T)                 \
    do {                              \
        if (cpb == 4) YXH_SPPB(T, 4); \
        else if (cpb == 2) YXH_SPPB(T, 2); \
        else YXH_SPPB(T, 1);          \
    } while (0)
    if (dt == YXH_BF16) YXH_SPPB_T(bf16);
    else if (dt == YXH_F16) YXH_SPPB_T(f16);
    else YXH_SPPB_T(float);
#undef YXH_SPPB_T
#undef YXH_SPPB
    YXH_CHECK_LAUNCH("spp_bwd");
    return YXH_OK;
}

int upsample_bwd_launch(const float* g, int B, int h, int w, int C, float* dst, hipStream_t st) {
    YXH_CHECK_ARG(g && dst && a16(g) && a16(dst) && B > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0,
                  "upsample_bwd arguments");
    const long long total = (long long)B * h * w * (C / 4);
    hipLaunchKernelGGL(upsample_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g, B, h, w, C, dst);
    YXH_CHECK_LAUNCH("upsample_bwd");
    return YXH_OK;
}

}  // namespace yxh
