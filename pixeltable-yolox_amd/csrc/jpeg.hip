// Device half of the JPEG decoder (yxh_jpeg_render_batch): from the host's entropy-decoded int16
// coefficients to packed uint8 RGB, for a ragged batch in one call of two launches on one stream.
// The arithmetic is csrc/jpeg_math.hpp, shared with the host restatement (jpeg_host.cpp), so the
// bytes are the same by construction.
//
//   jpeg_idct    dequantise + islow IDCT of every block of every component into the image's
//                component planes in the caller's workspace (uint8, rows of blocks_w * 8).  A
//                256-thread workgroup takes 32 consecutive blocks: each lane loads one 16-byte
//                coefficient row (1 KiB contiguous per wave), the block sits in LDS as 8 x 9
//                dwords, lane (block, c) runs the column pass, lane (block, r) the row pass and
//                stores its 8 samples as one 8-byte word.
//   jpeg_colour  fancy chroma upsampling + YCbCr -> RGB.  The chroma halo across block and MCU
//                borders is why the planes exist: this pass reads neighbours freely.  An image is
//                a flat run of H * W pixels; a workgroup takes 1024 consecutive pixels, 4 per lane
//                (12 bytes = 3 dwords into LDS), and the 3072 bytes leave as aligned dword stores
//                whatever dst_offset's alignment is: LDS dwords are re-cut by the byte phase of the
//                destination, and only the first and last, partial dwords go out by bytes.  No byte
//                outside [dst_offset, dst_offset + H*W*3) is written.
//
// blockIdx.y is the image and the blocks of a grid row stride over its work, so one grid serves
// every size in the batch (the sizes are device data: the host entry never reads them).
#include "jpeg_math.hpp"
#include "yxh_common.hpp"

namespace yxh {

namespace J = jpeg;

constexpr int kJpegThreads = 256;
constexpr int kIdctBlocks = kJpegThreads / 8;   // 8x8 blocks per workgroup pass
constexpr int kColourPixels = kJpegThreads * 4;  // pixels per workgroup pass

struct JpegImage {  // what a workgroup needs of its descriptor, in LDS
    J::Geom g;
    long long coef, ws, dst;  // offsets; coef < 0: skip the image
    int sampling, height, width;
};

__device__ void jpeg_load_image(const yxh_jpeg_image& im, JpegImage& s) {
    const bool ok = J::offsets_ok(im) && J::geom(im.height, im.width, im.components, im.sampling, s.g);
    s.coef = ok ? im.coef_offset : -1;
    s.ws = im.ws_offset;
    s.dst = im.dst_offset;
    s.sampling = im.sampling;
    s.height = im.height;
    s.width = im.width;
}

__global__ __launch_bounds__(kJpegThreads) void jpeg_idct(const int16_t* coef, const yxh_jpeg_image* images,
                                                          uint8_t* workspace) {
    __shared__ JpegImage si;
    __shared__ uint16_t sq[3][64];
    __shared__ uint32_t tile[kIdctBlocks][8][9];
    const int tid = threadIdx.x;
    const yxh_jpeg_image* im = images + blockIdx.y;
    if (tid == 0) jpeg_load_image(*im, si);
    if (tid < 192) sq[tid >> 6][tid & 63] = im->quant[tid >> 6][tid & 63];
    __syncthreads();
    if (si.coef < 0) return;
    const J::Geom& g = si.g;
    const long long total = g.blk0[3];
    const int16_t* cf = coef + si.coef / 2;
    uint8_t* ws = workspace + si.ws;
    const int lb = tid >> 3, r = tid & 7;
    for (long long base = (long long)blockIdx.x * kIdctBlocks; base < total;
         base += (long long)gridDim.x * kIdctBlocks) {
        const long long blk = base + lb;
        const bool active = blk < total;
        const int c = blk >= g.blk0[2] ? 2 : blk >= g.blk0[1] ? 1 : 0;
        if (active) {
            const uint4 v = *(const uint4*)(cf + blk * 64 + r * 8);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint16_t* q = sq[c] + r * 8;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                tile[lb][r][2 * k] = J::dequant((int16_t)(w[k] & 0xffff), q[2 * k]);
                tile[lb][r][2 * k + 1] = J::dequant((int16_t)(w[k] >> 16), q[2 * k + 1]);
            }
        }
        __syncthreads();
        J::u32 x[8], o[8];
        if (active) {  // pass 1 down column r
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = tile[lb][k][r];
            J::idct8(x, o);
#pragma unroll
            for (int k = 0; k < 8; ++k) tile[lb][k][r] = J::pass1_descale(o[k]);
        }
        __syncthreads();
        if (active) {  // pass 2 along row r
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = tile[lb][r][k];
            J::idct8(x, o);
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lo |= (uint32_t)J::pass2_sample(o[k]) << (8 * k);
                hi |= (uint32_t)J::pass2_sample(o[k + 4]) << (8 * k);
            }
            const long long in = blk - g.blk0[c];
            const int by = (int)(in / g.bw[c]), bx = (int)(in - (long long)by * g.bw[c]);
            const long long stride = (long long)g.bw[c] * 8;
            // plane offsets and strides are multiples of 64 / 8 and ws is 16-aligned: 8-byte aligned
            *(uint2*)(ws + g.plane[c] + ((long long)by * 8 + r) * stride + bx * 8) = make_uint2(lo, hi);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kJpegThreads) void jpeg_colour(const yxh_jpeg_image* images, const uint8_t* workspace,
                                                            uint8_t* dst) {
    __shared__ JpegImage si;
    __shared__ uint32_t sw[kColourPixels * 3 / 4 + 2];  // [0] and the last stay zero: the re-cut's neighbours
    const int tid = threadIdx.x;
    if (tid == 0) {
        jpeg_load_image(images[blockIdx.y], si);
        sw[0] = 0;
        sw[kColourPixels * 3 / 4 + 1] = 0;
    }
    __syncthreads();
    if (si.coef < 0) return;
    const J::Geom& g = si.g;
    const int W = si.width, sampling = si.sampling;
    const int npix = si.height * W;  // <= 2^30 (geom)
    const uint8_t* ws = workspace + si.ws;
    uint8_t* out = dst + si.dst;
    for (long long p0 = (long long)blockIdx.x * kColourPixels; p0 < npix; p0 += (long long)gridDim.x * kColourPixels) {
        const int n = (int)min((long long)kColourPixels, npix - p0);
        {
            const int p = (int)p0 + tid * 4;
            int y = p / W, x = p - y * W;
            uint8_t t[12];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int rgb[3] = {0, 0, 0};
                if (tid * 4 + j < n) J::pixel_rgb(ws, g, sampling, x, y, rgb);
                t[3 * j] = (uint8_t)rgb[0];
                t[3 * j + 1] = (uint8_t)rgb[1];
                t[3 * j + 2] = (uint8_t)rgb[2];
                if (++x == W) {
                    x = 0;
                    ++y;
                }
            }
            uint32_t w[3];
            __builtin_memcpy(w, t, 12);
            sw[1 + tid * 3] = w[0];
            sw[2 + tid * 3] = w[1];
            sw[3 + tid * 3] = w[2];
        }
        __syncthreads();
        // stream byte i of this pass (0 <= i < nbytes) lives in LDS dword 1 + i / 4 and goes to a + i
        uint8_t* a = out + p0 * 3;
        const int nbytes = n * 3;
        const int mis = (int)((uintptr_t)a & 3);
        const int nwords = (mis + nbytes + 3) >> 2;  // aligned destination dwords touched
        for (int k = tid; k < nwords; k += kJpegThreads) {
            // destination dword k covers stream bytes 4k - mis .. 4k - mis + 3
            const uint64_t pair = ((uint64_t)sw[1 + k] << 32) | sw[k];
            const uint32_t v = (uint32_t)(pair >> (32 - 8 * mis));
            const int first = 4 * k - mis;
            uint8_t* d = a + first;
            if (first >= 0 && first + 4 <= nbytes) {
                *(uint32_t*)d = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (first + i >= 0 && first + i < nbytes) d[i] = (uint8_t)(v >> (8 * i));
            }
        }
        __syncthreads();
    }
}

int jpeg_render_launch(const int16_t* coef, const yxh_jpeg_image* images, int B, uint8_t* workspace, uint8_t* dst,
                       hipStream_t st) {
    YXH_CHECK_ARG(coef && images && workspace && dst, "jpeg_render: null pointer");
    YXH_CHECK_ARG(B > 0 && B <= 65535, "jpeg_render batch %d", B);
    YXH_CHECK_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)workspace & 15) == 0,
                  "jpeg_render: coef and workspace must be 16-byte aligned");
    // about 2048 workgroups in flight whatever the batch: 8 waves on each of the 256 CUs
    const int per_image = B >= 128 ? 16 : B >= 8 ? 2048 / B : 256;
    hipLaunchKernelGGL(jpeg_idct, dim3(per_image, B), dim3(kJpegThreads), 0, st, coef, images, workspace);
    YXH_CHECK_LAUNCH("jpeg_idct");
    hipLaunchKernelGGL(jpeg_colour, dim3(per_image, B), dim3(kJpegThreads), 0, st, images, workspace, dst);
    YXH_CHECK_LAUNCH("jpeg_colour");
    return YXH_OK;
}

}  // namespace yxh
