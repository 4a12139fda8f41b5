// The arithmetic of the JPEG render stage, stated once for the host restatement (jpeg_host.cpp)
// and the device kernels (jpeg.hip): geometry of the component planes, libjpeg's "islow" 8x8
// IDCT, the "fancy" chroma upsampling and the YCbCr -> RGB conversion, all in 32-bit integers.
// Everything is computed in uint32_t (two's-complement wrap-around is defined there) and
// reinterpreted as int32_t only for the arithmetic right shifts, so absurd coefficients from a
// damaged file give the same bytes on both sides instead of undefined behaviour.
#pragma once

#include <stdint.h>

#include "yoloxhip.h"

#if defined(__HIP__)  // spelled as attributes: jpeg_host.cpp includes no HIP header
#define YXH_JPEG_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define YXH_JPEG_HD inline
#endif

namespace yxh {
namespace jpeg {

typedef uint32_t u32;

constexpr int kMaxSide = 65535;            // SOF's 16-bit sizes
constexpr long long kMaxPixels = 1ll << 30;  // pixel indices stay in int32

// Where the planes and the coefficients of one image lie.  Component 0 is luma (or the only
// component); block rows are padded to whole MCUs, the cropped sizes are what upsampling reads.
struct Geom {
    int ncomp;
    int bw[3], bh[3];         // blocks per row / block rows, padded to whole MCUs
    int cw[3], ch[3];         // cropped plane size: ceil(W * h / hmax) x ceil(H * v / vmax)
    long long blk0[4];        // first block of each component in the image's coefficients; [3] = total
    long long plane[4];       // byte offset of each component plane in the image's workspace; [3] = total
};

YXH_JPEG_HD bool geom(int H, int W, int ncomp, int sampling, Geom& g) {
    if (H < 1 || W < 1 || H > kMaxSide || W > kMaxSide || (long long)H * W > kMaxPixels) return false;
    if (sampling < YXH_JPEG_GRAY || sampling > YXH_JPEG_420) return false;
    if (ncomp != (sampling == YXH_JPEG_GRAY ? 1 : 3)) return false;
    const int hmax = sampling >= YXH_JPEG_422 ? 2 : 1, vmax = sampling == YXH_JPEG_420 ? 2 : 1;
    const int mx = (W + 8 * hmax - 1) / (8 * hmax), my = (H + 8 * vmax - 1) / (8 * vmax);
    g.ncomp = ncomp;
    g.blk0[0] = 0;
    g.plane[0] = 0;
    for (int c = 0; c < 3; ++c) {
        const bool on = c < ncomp;
        g.bw[c] = !on ? 0 : c == 0 ? mx * hmax : mx;
        g.bh[c] = !on ? 0 : c == 0 ? my * vmax : my;
        g.cw[c] = !on ? 0 : c == 0 ? W : (W + hmax - 1) / hmax;
        g.ch[c] = !on ? 0 : c == 0 ? H : (H + vmax - 1) / vmax;
        const long long n = (long long)g.bw[c] * g.bh[c];
        g.blk0[c + 1] = g.blk0[c] + n;
        g.plane[c + 1] = g.plane[c] + n * 64;
    }
    return true;
}

// One 1-D pass of the islow IDCT (13-bit constants) over eight dequantised inputs; the outputs
// are not yet descaled.
YXH_JPEG_HD void idct8(const u32 x[8], u32 o[8]) {
    u32 z1 = (x[2] + x[6]) * 4433u;
    const u32 t2 = z1 - x[6] * 15137u;
    const u32 t3 = z1 + x[2] * 6270u;
    const u32 t0 = (x[0] + x[4]) << 13;
    const u32 t1 = (x[0] - x[4]) << 13;
    const u32 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u32 a = x[7], b = x[5], c = x[3], d = x[1];
    z1 = a + d;
    u32 z2 = b + c, z3 = a + c, z4 = b + d;
    const u32 z5 = (z3 + z4) * 9633u;
    a *= 2446u;
    b *= 16819u;
    c *= 25172u;
    d *= 12299u;
    z1 *= (u32)-7373;
    z2 *= (u32)-20995;
    z3 = z3 * (u32)-16069 + z5;
    z4 = z4 * (u32)-3196 + z5;
    a += z1 + z3;
    b += z2 + z4;
    c += z2 + z3;
    d += z1 + z4;
    o[0] = t10 + d;
    o[7] = t10 - d;
    o[1] = t11 + c;
    o[6] = t11 - c;
    o[2] = t12 + b;
    o[5] = t12 - b;
    o[3] = t13 + a;
    o[4] = t13 - a;
}

YXH_JPEG_HD u32 pass1_descale(u32 v) { return (u32)((int32_t)(v + 1024u) >> 11); }

YXH_JPEG_HD int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

YXH_JPEG_HD int pass2_sample(u32 v) { return clamp255(((int32_t)(v + 131072u) >> 18) + 128); }

YXH_JPEG_HD u32 dequant(int16_t c, uint16_t q) { return (u32)(int32_t)c * (u32)q; }

// A whole block, scalar: 64 coefficients in natural order -> 8 rows of 8 samples at `out`.
YXH_JPEG_HD void idct_block(const int16_t* coef, const uint16_t* q, uint8_t* out, long long stride) {
    u32 ws[64], x[8], o[8];
    for (int c = 0; c < 8; ++c) {
        for (int k = 0; k < 8; ++k) x[k] = dequant(coef[k * 8 + c], q[k * 8 + c]);
        idct8(x, o);
        for (int k = 0; k < 8; ++k) ws[k * 8 + c] = pass1_descale(o[k]);
    }
    for (int r = 0; r < 8; ++r) {
        idct8(ws + r * 8, o);
        for (int k = 0; k < 8; ++k) out[r * stride + k] = (uint8_t)pass2_sample(o[k]);
    }
}

// The upsampled chroma sample of output pixel (x, y) from the cropped plane `p` (row stride
// `stride`, cw x ch samples); samples past an edge replicate the edge sample, which gives
// libjpeg's plain copies at the first and last column.
YXH_JPEG_HD int chroma_at(const uint8_t* p, long long stride, int cw, int ch, int sampling, int x, int y) {
    if (sampling == YXH_JPEG_444) return p[y * stride + x];
    const int i = x >> 1;
    const int in = (x & 1) ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
    if (sampling == YXH_JPEG_422) {
        const uint8_t* r = p + y * stride;
        return (3 * r[i] + r[in] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int j = y >> 1;
    const int jn = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
    const uint8_t* r0 = p + j * stride;
    const uint8_t* r1 = p + jn * stride;
    const int s = 3 * r0[i] + r1[i], sn = 3 * r0[in] + r1[in];
    return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

// Output pixel (x, y) of one image whose planes start at `ws`.
YXH_JPEG_HD void pixel_rgb(const uint8_t* ws, const Geom& g, int sampling, int x, int y, int rgb[3]) {
    const int Y = ws[g.plane[0] + (long long)y * (g.bw[0] * 8) + x];
    if (g.ncomp == 1) {
        rgb[0] = rgb[1] = rgb[2] = Y;
        return;
    }
    const long long cs = (long long)g.bw[1] * 8;
    const int cb = chroma_at(ws + g.plane[1], cs, g.cw[1], g.ch[1], sampling, x, y) - 128;
    const int cr = chroma_at(ws + g.plane[2], cs, g.cw[2], g.ch[2], sampling, x, y) - 128;
    rgb[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
    rgb[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

// What the render stage accepts of a descriptor's caller-set fields.
YXH_JPEG_HD bool offsets_ok(const yxh_jpeg_image& im) {
    return im.coef_offset >= 0 && (im.coef_offset & 15) == 0 && im.ws_offset >= 0 && (im.ws_offset & 15) == 0 &&
           im.dst_offset >= 0;
}

}  // namespace jpeg
}  // namespace yxh
