// RGB stem conv on gfx950: the first layer of Darknet-53 (reference darknet.py:31, a
// BaseConv 3x3 stride 1 pad 1 straight from the 3-channel image, BN folded, LeakyReLU).
//
// K = 3 x 3 taps x 3 channels = 27, padded to 32 with k = (ky*3 + kx)*3 + c: for the 16-bit
// types exactly one 16x16x32 MFMA per 16 pixels x 16 output channels (fp32: eight 16x16x4).
// In an NHWC image row the 9 values (kx, c) of one kernel row are contiguous, so the operand
// of a pixel is three 9-element runs of an LDS copy of the tile's input rows.
//
//  * rgb_stem_conv: block = 256 threads = 4 waves = a 4 x 64 tile of output pixels of one
//    image (wave = output row), all output channels (<= 64).  The 6 x 66 input pixels the
//    tile needs are staged once in LDS, already converted, zero outside the image; the weights
//    live in registers; the output tile goes back through LDS and leaves as 16-byte chunks of
//    whole pixel rows (the kernel is store-bound: 64 B written per pixel at 32 bf16 channels
//    against 3-12 B read).
//  * rgb_pack: the image as NHWC with 16 channels (3 used, 13 zero) for the generic conv
//    (yxh_focus_pack without the space-to-depth): the fallback path.
//  * rgb_stem_pack: weight [cout][3][3][3] with BN -> [round16(cout)][32].
#include "conv_common.hpp"

namespace yxh {

constexpr int kRgbTY = 4, kRgbTX = 64;
constexpr int kRgbRows = kRgbTY + 2;              // output rows + halo
constexpr int kRgbRowElems = (kRgbTX + 2) * 3;    // 198: pixel x0 - 1 + i at element 3i
constexpr int kRgbZero = kRgbRows * kRgbRowElems; // a zero element behind the rows (k >= 27)
constexpr int kRgbInElems = kRgbZero + 8;
constexpr int kRgbK = 32;

struct RgbParams {
    const void* img;
    int layout, B, H, W, cout, act;
    const void* w;  // [cout_pad][32]
    const float* bias;
    void* dst;
    int dst_cs;
    long long dst_bs;
};

template <typename TI>
__device__ __forceinline__ float rgb_px(const RgbParams& p, int b, int y, int x, int c) {
    const TI* img = (const TI*)p.img;
    if (p.layout == YXH_NCHW) return to_f32(img[(((long long)b * 3 + c) * p.H + y) * p.W + x]);
    return to_f32(img[(((long long)b * p.H + y) * p.W + x) * 3 + c]);
}

template <typename T, typename TI, int FR>
__global__ __launch_bounds__(256) void rgb_stem_conv(RgbParams p) {
    constexpr int EPC = Chunk<T>::N;
    constexpr int SLABS = kRgbK / (4 * EPC);  // 64-byte K slabs: 1 (bf16/f16), 2 (f32)
    constexpr int IN_BYTES = (kRgbInElems * (int)sizeof(T) + 15) / 16 * 16;
    constexpr int OUT_ROW = FR * 16 * sizeof(T) + 16;
    constexpr int OUT_BYTES = kRgbTY * kRgbTX * OUT_ROW;
    constexpr int SMEM = IN_BYTES > OUT_BYTES ? IN_BYTES : OUT_BYTES;
    __shared__ __attribute__((aligned(16))) char smem[SMEM];
    T* in = (T*)smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fq = lane >> 4;
    const int b = blockIdx.z;
    const int oy0 = blockIdx.y * kRgbTY, ox0 = blockIdx.x * kRgbTX;

    // weights and bias into registers first: their latency overlaps the staging
    const T* wt = (const T*)p.w;
    uint4 wreg[SLABS][FR];
#pragma unroll
    for (int s = 0; s < SLABS; ++s)
#pragma unroll
        for (int i = 0; i < FR; ++i)
            wreg[s][i] = *(const uint4*)(wt + (i * 16 + frow) * kRgbK + s * 4 * EPC + fq * EPC);
    float bias[FR][4];
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) bias[i][r] = p.bias[i * 16 + fq * 4 + r];  // [cout_pad], zeros past cout

    // stage rows oy0 - 1 .. oy0 + 4, pixels ox0 - 1 .. ox0 + 64 as T, zero outside the image
    for (int q = tid; q < kRgbInElems; q += 256) {
        const int r = q / kRgbRowElems, e = q - r * kRgbRowElems;
        const int px = e / 3, c = e - px * 3;
        const int y = oy0 - 1 + r, x = ox0 - 1 + px;
        float v = 0.0f;
        if (r < kRgbRows && y >= 0 && y < p.H && x >= 0 && x < p.W) v = rgb_px<TI>(p, b, y, x, c);
        in[q] = from_f32<T>(v);
    }
    __syncthreads();

    // this lane's K elements: k = (ky*3 + kx)*3 + c lives at row ky, element 3*ox + (k - 9*ky)
    int koff[SLABS][EPC];
#pragma unroll
    for (int s = 0; s < SLABS; ++s)
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const int k = s * 4 * EPC + fq * EPC + e;
            const int ky = k / 9;
            koff[s][e] = k < 27 ? (wave + ky) * kRgbRowElems + (k - 9 * ky) : -1;
        }

    f32x4 acc[FR][4];
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < SLABS; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int oxl = j * 16 + frow;
            T t[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) t[e] = in[koff[s][e] < 0 ? kRgbZero : koff[s][e] + 3 * oxl];
            uint4 bf;
            __builtin_memcpy(&bf, t, 16);
#pragma unroll
            for (int i = 0; i < FR; ++i) Mma<T>::run(acc[i][j], wreg[s][i], bf);
        }
    }
    __syncthreads();  // input tile dead; reuse LDS for the output tile
    // epilogue: bias + act in registers, tile [4*64 px][FR*16 ch] through LDS
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pl = wave * kRgbTX + j * 16 + frow;
#pragma unroll
        for (int i = 0; i < FR; ++i) {
            const int n = i * 16 + fq * 4;
            T t[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                t[r] = from_f32<T>(apply_act<sizeof(T) == 4>(acc[i][j][r] + bias[i][r], p.act));
            char* d = smem + pl * OUT_ROW + n * sizeof(T);
            if constexpr (sizeof(T) == 2) {
                uint2 u;
                __builtin_memcpy(&u, t, 8);
                *(uint2*)d = u;
            } else {
                uint4 u;
                __builtin_memcpy(&u, t, 16);
                *(uint4*)d = u;
            }
        }
    }
    __syncthreads();
    const int cpo = p.cout * (int)sizeof(T) / 16;  // chunks per output pixel (cout % 16 == 0)
    for (int q = tid; q < kRgbTY * kRgbTX * cpo; q += 256) {
        const int px = q / cpo, c = q - px * cpo;
        const int oy = oy0 + px / kRgbTX, ox = ox0 + (px % kRgbTX);
        if (oy >= p.H || ox >= p.W) continue;
        const uint4 u = *(const uint4*)(smem + px * OUT_ROW + c * 16);
        *(uint4*)((char*)p.dst + (b * p.dst_bs + ((long long)oy * p.W + ox) * p.dst_cs) * (long long)sizeof(T) +
                  c * 16) = u;
    }
}

// ---------------------------------------------------------------- rgb pack
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void rgb_pack(const TI* img, int layout, int B, int H, int W, TO* dst) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * H * W) return;
    const int x = (int)(idx % W);
    const int y = (int)((idx / W) % H);
    const int b = (int)(idx / ((long long)W * H));
    TO out[16];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = layout == YXH_NCHW ? to_f32(img[(((long long)b * 3 + c) * H + y) * W + x])
                                           : to_f32(img[idx * 3 + c]);
        out[c] = from_f32<TO>(v);
    }
#pragma unroll
    for (int k = 3; k < 16; ++k) out[k] = from_f32<TO>(0.0f);
    uint4* d = (uint4*)(dst + idx * 16);
#pragma unroll
    for (int k = 0; k < (int)(16 * sizeof(TO) / 16); ++k) {
        uint4 u;
        __builtin_memcpy(&u, (const char*)out + 16 * k, 16);
        d[k] = u;
    }
}

// Pack the RGB stem BaseConv (weight [cout][3][3][3] = [n][c][ky][kx], with BN) to [cout_pad][32].
template <typename T>
__global__ void rgb_stem_pack(const float* w, const float* g, const float* beta, const float* mean,
                              const float* var, float eps, int cout, int cout_pad, T* wo, float* bo) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= cout_pad * kRgbK) return;
    const int k = idx % kRgbK, n = idx / kRgbK;
    float v = 0.0f;
    if (n < cout && k < 27) {
        const int tap = k / 3, c = k - tap * 3;  // tap = ky*3 + kx
        const float scale = g ? g[n] / sqrtf(var[n] + eps) : 1.0f;
        v = w[(n * 3 + c) * 9 + tap] * scale;
    }
    wo[idx] = from_f32<T>(v);
    if (idx < cout_pad) {
        const float scale = g && idx < cout ? g[idx] / sqrtf(var[idx] + eps) : 1.0f;
        bo[idx] = idx < cout && g ? beta[idx] - mean[idx] * scale : 0.0f;
    }
}

template <typename T, typename TI>
static int rgb_launch_ti(const RgbParams& p, hipStream_t st) {
    dim3 grid((p.W + kRgbTX - 1) / kRgbTX, (p.H + kRgbTY - 1) / kRgbTY, p.B);
    switch (p.cout / 16) {
        case 1: hipLaunchKernelGGL((rgb_stem_conv<T, TI, 1>), grid, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL((rgb_stem_conv<T, TI, 2>), grid, dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL((rgb_stem_conv<T, TI, 3>), grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL((rgb_stem_conv<T, TI, 4>), grid, dim3(256), 0, st, p); break;
    }
    YXH_CHECK_LAUNCH("rgb_stem_conv launch");
    return YXH_OK;
}

template <typename T>
static int rgb_launch_t(const RgbParams& p, int idt, hipStream_t st) {
    switch (idt) {
        case YXH_F32: return rgb_launch_ti<T, float>(p, st);
        case YXH_U8: return rgb_launch_ti<T, uint8_t>(p, st);
        case YXH_BF16: return rgb_launch_ti<T, bf16>(p, st);
        default: return rgb_launch_ti<T, f16>(p, st);
    }
}

int rgb_stem_launch(const yxh_stem_desc* d, hipStream_t st) {
    YXH_CHECK_ARG(d && d->img && d->weight && d->bias && d->dst, "rgb stem: null pointer");
    YXH_CHECK_ARG(d->batch > 0 && d->h >= 1 && d->w >= 1, "rgb stem: image %d x %dx%d", d->batch, d->h, d->w);
    YXH_CHECK_ARG(d->layout == YXH_NCHW || d->layout == YXH_NHWC, "rgb stem: layout %d", d->layout);
    YXH_CHECK_ARG(d->img_dtype == YXH_F32 || d->img_dtype == YXH_U8 || d->img_dtype == YXH_BF16 ||
                      d->img_dtype == YXH_F16,
                  "rgb stem: image dtype %d", d->img_dtype);
    YXH_CHECK_ARG(d->dtype == YXH_F32 || d->dtype == YXH_BF16 || d->dtype == YXH_F16, "rgb stem: compute dtype %d",
                  d->dtype);
    YXH_CHECK_ARG(d->act == YXH_ACT_NONE || d->act == YXH_ACT_SILU || d->act == YXH_ACT_RELU ||
                      d->act == YXH_ACT_LRELU,
                  "rgb stem: activation %d", d->act);
    YXH_CHECK_ARG(d->cout > 0, "rgb stem: cout %d", d->cout);
    if (d->layout == YXH_NCHW && d->img_dtype != YXH_F32) {
        set_error("rgb stem: NCHW images are float32 (dtype %d)", d->img_dtype);
        return YXH_EUNSUPPORTED;
    }
    if (d->cout % 16 || d->cout > 64) {
        set_error("rgb stem: cout %d is not a multiple of 16 up to 64", d->cout);
        return YXH_EUNSUPPORTED;
    }
    if ((d->h + kRgbTY - 1) / kRgbTY > 65535 || d->batch > 65535) {
        set_error("rgb stem: grid of %d images x %d rows", d->batch, d->h);
        return YXH_EUNSUPPORTED;
    }
    const int es = d->dtype == YXH_F32 ? 4 : 2;
    YXH_CHECK_ARG(d->dst_cstride >= d->cout && d->dst_bstride >= (long long)d->h * d->w * d->dst_cstride,
                  "rgb stem: dst strides %d / %lld", d->dst_cstride, (long long)d->dst_bstride);
    YXH_CHECK_ARG(((uintptr_t)d->dst % 16) == 0 && ((uintptr_t)d->weight % 16) == 0 &&
                      (d->dst_cstride * es) % 16 == 0 && (d->dst_bstride * es) % 16 == 0,
                  "rgb stem: dst / weight alignment");
    RgbParams p;
    p.img = d->img;
    p.layout = d->layout;
    p.B = d->batch;
    p.H = d->h;
    p.W = d->w;
    p.cout = d->cout;
    p.act = d->act;
    p.w = d->weight;
    p.bias = d->bias;
    p.dst = d->dst;
    p.dst_cs = d->dst_cstride;
    p.dst_bs = d->dst_bstride;
    if (d->dtype == YXH_BF16) return rgb_launch_t<bf16>(p, d->img_dtype, st);
    if (d->dtype == YXH_F16) return rgb_launch_t<f16>(p, d->img_dtype, st);
    return rgb_launch_t<float>(p, d->img_dtype, st);
}

int rgb_pack_launch(const void* img, int layout, int idt, int B, int H, int W, void* dst, int odt, hipStream_t st) {
    YXH_CHECK_ARG(img && dst, "rgb pack: null pointer");
    YXH_CHECK_ARG(B > 0 && H >= 1 && W >= 1, "rgb pack: image size %dx%d", H, W);
    YXH_CHECK_ARG(layout == YXH_NCHW || layout == YXH_NHWC, "rgb pack: layout %d", layout);
    YXH_CHECK_ARG(((uintptr_t)dst % 16) == 0, "rgb pack: dst not aligned");
    const long long total = (long long)B * H * W;
    YXH_CHECK_ARG((total + 255) / 256 < (1LL << 31), "rgb pack: too many pixels");
    dim3 grid((unsigned)((total + 255) / 256));
#define YXH_RGBP(TI, TO) \
    hipLaunchKernelGGL((rgb_pack<TI, TO>), grid, dim3(256), 0, st, (const TI*)img, layout, B, H, W, (TO*)dst)
#define YXH_RGBP_OUT(TI)                          \
    if (odt == YXH_BF16) YXH_RGBP(TI, bf16);      \
    else if (odt == YXH_F16) YXH_RGBP(TI, f16);   \
    else if (odt == YXH_F32) YXH_RGBP(TI, float); \
    else { set_error("rgb pack: dst dtype %d", odt); return YXH_EINVAL; }
    if (idt == YXH_F32) { YXH_RGBP_OUT(float) }
    else if (idt == YXH_U8) { YXH_RGBP_OUT(uint8_t) }
    else if (idt == YXH_BF16) { YXH_RGBP_OUT(bf16) }
    else if (idt == YXH_F16) { YXH_RGBP_OUT(f16) }
    else { set_error("rgb pack: img dtype %d", idt); return YXH_EINVAL; }
#undef YXH_RGBP_OUT
#undef YXH_RGBP
    YXH_CHECK_LAUNCH("rgb_pack launch");
    return YXH_OK;
}

int rgb_stem_pack_launch(const float* w, const float* g, const float* beta, const float* mean, const float* var,
                         float eps, int cout, int dt, void* wo, float* bo, hipStream_t st) {
    YXH_CHECK_ARG(w && wo && bo && cout > 0 && cout <= 64, "rgb stem pack: null pointer or cout %d", cout);
    YXH_CHECK_ARG(!g || (beta && mean && var), "rgb stem pack: partial BN parameters");
    const int cout_pad = (cout + 15) / 16 * 16;
    dim3 grid((cout_pad * kRgbK + 255) / 256);
    if (dt == YXH_BF16)
        hipLaunchKernelGGL(rgb_stem_pack<bf16>, grid, dim3(256), 0, st, w, g, beta, mean, var, eps, cout, cout_pad,
                           (bf16*)wo, bo);
    else if (dt == YXH_F16)
        hipLaunchKernelGGL(rgb_stem_pack<f16>, grid, dim3(256), 0, st, w, g, beta, mean, var, eps, cout, cout_pad,
                           (f16*)wo, bo);
    else if (dt == YXH_F32)
        hipLaunchKernelGGL(rgb_stem_pack<float>, grid, dim3(256), 0, st, w, g, beta, mean, var, eps, cout, cout_pad,
                           (float*)wo, bo);
    else {
        set_error("rgb stem pack: dtype %d", dt);
        return YXH_EINVAL;
    }
    YXH_CHECK_LAUNCH("rgb stem pack");
    return YXH_OK;
}

}  // namespace yxh
