// Serving-side result packing: the detections yxh_postprocess* left per image ([B, A, 7] rows and
// [B] counts) compacted into one run of 32-byte records the host fetches with a single copy
// (yolox_amd/serve.py).  Each record is what YoloxProcessor.postprocess (reference processor.py:39-54)
// builds per detection on the CPU: the box divided by the letterbox ratio -- an IEEE fp32 divide, as
// torch's CPU kernel does for `boxes / ratio` -- and the two confidences and the label untouched.
#include "yxh_common.hpp"

namespace yxh {

// rows of one image a block moves; 7 floats each, staged through LDS so that the global reads are
// aligned 16-byte chunks although a det row is 28 bytes and an image's first row sits at any
// 4-byte phase (A * 7 floats per image)
constexpr int kPackRows = 256;
constexpr int kPackThreads = 256;

// grid (ceil(A / kPackRows), B): block (t, b) packs rows [t * kPackRows, ...) of image b.  Every block
// sums the counts in front of its image itself (B is a serving batch, tens of images): no scan launch.
// det_floats = B * A * 7, the end of `det`: aligned chunks never reach past it.
__global__ __launch_bounds__(kPackThreads) void detections_pack(
    const float* __restrict__ det, const int* __restrict__ counts, int B, int A, int n_valid,
    const float* __restrict__ ratios, float* __restrict__ rows_out, int capacity_rows,
    int* __restrict__ offsets_out, long long det_floats) {
    __shared__ __attribute__((aligned(16))) float tile[kPackRows * 7 + 4];
    __shared__ int wave_sum[kPackThreads / kWave];
    const int b = blockIdx.y, tid = threadIdx.x;
    // counts clamped to [0, A] (what yxh_postprocess* writes); images >= n_valid hold nothing
    int part = 0;
    for (int i = tid; i < b; i += kPackThreads)
        if (i < n_valid) part += min(max(counts[i], 0), A);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, kWave);
    if ((tid & (kWave - 1)) == 0) wave_sum[tid / kWave] = part;
    __syncthreads();
    int first = 0;
#pragma unroll
    for (int w = 0; w < kPackThreads / kWave; ++w) first += wave_sum[w];
    const int count = b < n_valid ? min(max(counts[b], 0), A) : 0;
    if (blockIdx.x == 0 && tid == 0) {
        offsets_out[b] = first;
        if (b == B - 1) offsets_out[B] = first + count;
    }
    const int r0 = blockIdx.x * kPackRows;
    if (r0 >= count) return;  // block-uniform
    const int nrows = min(kPackRows, count - r0);
    // floats [f0, f1) of det hold the block's rows; read from the aligned chunk at or below f0
    const long long f0 = ((long long)b * A + r0) * 7, f1 = f0 + (long long)nrows * 7;
    const long long a0 = f0 & ~3LL;
    for (long long i = a0 + 4LL * tid; i < f1; i += 4LL * kPackThreads) {
        f32x4 v;
        if (i + 4 <= det_floats) {
            v = *reinterpret_cast<const f32x4*>(det + i);
        } else {  // the last, partial chunk of the whole array
            v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i + j < det_floats) v[j] = det[i + j];
        }
        *reinterpret_cast<f32x4*>(tile + (i - a0)) = v;
    }
    __syncthreads();
    const float ratio = ratios[b];
    const int phase = (int)(f0 - a0);
    for (int r = tid; r < nrows; r += kPackThreads) {
        const long long o = (long long)first + r0 + r;
        if (o >= capacity_rows) continue;  // counted in offsets_out, written nowhere
        const float* s = tile + phase + r * 7;
        const f32x4 box = {s[0] / ratio, s[1] / ratio, s[2] / ratio, s[3] / ratio};
        const f32x4 rest = {s[4], s[5], __int_as_float((int)s[6]), __int_as_float(b)};
        f32x4* d = reinterpret_cast<f32x4*>(rows_out + o * 8);
        d[0] = box;
        d[1] = rest;
    }
}

int detections_pack_launch(const float* det, const int* counts, int B, int A, int n_valid, const float* ratios,
                           void* rows_out, int capacity_rows, int* offsets_out, hipStream_t st) {
    YXH_CHECK_ARG(det && counts && ratios && rows_out && offsets_out, "yxh_detections_pack: null pointer");
    YXH_CHECK_ARG(B > 0 && A > 0, "yxh_detections_pack: batch %d anchors %d", B, A);
    YXH_CHECK_ARG((long long)B * A <= 0x7fffffffLL / 8, "yxh_detections_pack: batch %d x anchors %d rows", B, A);
    YXH_CHECK_ARG(B <= 65535, "yxh_detections_pack: batch %d above the grid limit 65535", B);
    YXH_CHECK_ARG(n_valid >= 0 && n_valid <= B, "yxh_detections_pack: n_valid %d outside [0, %d]", n_valid, B);
    YXH_CHECK_ARG(capacity_rows >= 0, "yxh_detections_pack: negative capacity_rows %d", capacity_rows);
    YXH_CHECK_ARG(((uintptr_t)det & 15) == 0 && ((uintptr_t)rows_out & 15) == 0,
                  "yxh_detections_pack: det and rows_out must be 16-byte aligned");
    hipLaunchKernelGGL(detections_pack, dim3((A + kPackRows - 1) / kPackRows, B), dim3(kPackThreads), 0, st, det,
                       counts, B, A, n_valid, ratios, (float*)rows_out, capacity_rows, offsets_out,
                       (long long)B * A * 7);
    YXH_CHECK_LAUNCH("detections_pack");
    return YXH_OK;
}

}  // namespace yxh
