// Standalone IouLoss (reference yolox/models/losses.py:7-51) on gfx950: forward with
// reduction none / sum / mean and the gradient w.r.t. pred and (optionally) target.
// The per-pair math is iou_loss.hpp, the same functions the SimOTA loss kernels call.
//
//   iou_loss_fwd    : thread per box pair, 256-thread blocks; each row is one 16-byte load.
//                     none: out[i].  sum / mean: block tree in LDS -> partial[block].
//   iou_loss_reduce : one block walks the partials in a fixed order, tree in LDS, one store.
//                     Partials and trees are fp64 and the result is rounded to fp32 once, so
//                     sum / mean are deterministic and equal the fp64 sum of the fp32 losses
//                     to fp32 rounding.  Mean divides the rounded sum by (float)n.
//   iou_loss_bwd    : thread per box pair; g_pred / g_target rows are one 16-byte store each.
#pragma clang fp contract(off)  // round like torch's separate ops

#include "iou_loss.hpp"
#include "yxh_common.hpp"

namespace yxh {

constexpr int kIouThreads = 256;

__device__ __forceinline__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kIouThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

template <int TYPE, bool REDUCE>
__global__ __launch_bounds__(kIouThreads) void iou_loss_fwd(const float4* pred, const float4* target, long long n,
                                                             float* out, double* partial) {
    __shared__ double red[kIouThreads];
    const long long i = (long long)blockIdx.x * kIouThreads + threadIdx.x;
    float loss = 0.0f;
    if (i < n) {
        const float4 p4 = pred[i], t4 = target[i];
        const float p[4] = {p4.x, p4.y, p4.z, p4.w}, t[4] = {t4.x, t4.y, t4.z, t4.w};
        loss = iou_loss_pair<TYPE>(p, t);
        if (!REDUCE) out[i] = loss;
    }
    if (REDUCE) {
        const double s = block_sum((double)loss, red);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kIouThreads) void iou_loss_reduce(const double* partial, long long nparts, long long n,
                                                                int mean, float* out) {
    __shared__ double red[kIouThreads];
    double acc = 0.0;
    for (long long j = threadIdx.x; j < nparts; j += kIouThreads) acc += partial[j];
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) {
        const float r = (float)s;
        out[0] = mean ? r / (float)n : r;
    }
}

template <int TYPE, bool WANT_T>
__global__ __launch_bounds__(kIouThreads) void iou_loss_bwd(const float4* pred, const float4* target, long long n,
                                                             const float* grad_out, int per_row, int mean,
                                                             float4* g_pred, float4* g_target) {
    const long long i = (long long)blockIdx.x * kIouThreads + threadIdx.x;
    if (i >= n) return;
    float go = per_row ? grad_out[i] : grad_out[0];
    if (mean) go = go / (float)n;
    const float4 p4 = pred[i], t4 = target[i];
    const float p[4] = {p4.x, p4.y, p4.z, p4.w}, t[4] = {t4.x, t4.y, t4.z, t4.w};
    float gp[4], gt[4];
    iou_loss_pair_bwd<TYPE, WANT_T>(p, t, go, gp, gt);
    g_pred[i] = make_float4(gp[0], gp[1], gp[2], gp[3]);
    if (WANT_T) g_target[i] = make_float4(gt[0], gt[1], gt[2], gt[3]);
}

// ------------------------------------------------------------------ host
static bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

static int check_common(const char* who, long long n, int type, int reduction) {
    YXH_CHECK_ARG(type == YXH_IOU_LOSS_IOU || type == YXH_IOU_LOSS_GIOU, "%s: loss_type %d", who, type);
    YXH_CHECK_ARG(reduction == YXH_REDUCE_NONE || reduction == YXH_REDUCE_SUM || reduction == YXH_REDUCE_MEAN,
                  "%s: reduction %d", who, reduction);
    YXH_CHECK_ARG(n >= 0 && n < (1LL << 31) * kIouThreads, "%s: n=%lld", who, n);
    return YXH_OK;
}

size_t iou_loss_workspace(long long n) {
    if (n <= 0) return 0;
    return sizeof(double) * (size_t)((n + kIouThreads - 1) / kIouThreads);
}

int iou_loss_launch(const float* pred, const float* target, long long n, int type, int reduction, float* out, void* ws,
                    size_t ws_bytes, hipStream_t st) {
    if (int rc = check_common("iou_loss", n, type, reduction)) return rc;
    if (n == 0) return YXH_OK;
    YXH_CHECK_ARG(pred && target && out, "iou_loss: null pointer");
    YXH_CHECK_ARG(aligned16(pred) && aligned16(target), "iou_loss: pred and target must be 16-byte aligned");
    const long long nblk = (n + kIouThreads - 1) / kIouThreads;
    const dim3 grid((unsigned)nblk), block(kIouThreads);
    const float4* p = (const float4*)pred;
    const float4* t = (const float4*)target;
    if (reduction == YXH_REDUCE_NONE) {
        if (type == YXH_IOU_LOSS_GIOU)
            hipLaunchKernelGGL((iou_loss_fwd<YXH_IOU_LOSS_GIOU, false>), grid, block, 0, st, p, t, n, out, nullptr);
        else
            hipLaunchKernelGGL((iou_loss_fwd<YXH_IOU_LOSS_IOU, false>), grid, block, 0, st, p, t, n, out, nullptr);
        YXH_CHECK_LAUNCH("iou_loss_fwd");
        return YXH_OK;
    }
    YXH_CHECK_ARG(ws && ((uintptr_t)ws % 8) == 0 && ws_bytes >= iou_loss_workspace(n),
                  "iou_loss: workspace too small or not 8-byte aligned");
    double* partial = (double*)ws;
    if (type == YXH_IOU_LOSS_GIOU)
        hipLaunchKernelGGL((iou_loss_fwd<YXH_IOU_LOSS_GIOU, true>), grid, block, 0, st, p, t, n, nullptr, partial);
    else
        hipLaunchKernelGGL((iou_loss_fwd<YXH_IOU_LOSS_IOU, true>), grid, block, 0, st, p, t, n, nullptr, partial);
    YXH_CHECK_LAUNCH("iou_loss_fwd");
    hipLaunchKernelGGL(iou_loss_reduce, dim3(1), block, 0, st, partial, nblk, n, reduction == YXH_REDUCE_MEAN ? 1 : 0,
                       out);
    YXH_CHECK_LAUNCH("iou_loss_reduce");
    return YXH_OK;
}

int iou_loss_bwd_launch(const float* pred, const float* target, long long n, int type, int reduction,
                        const float* grad_out, float* g_pred, float* g_target, hipStream_t st) {
    if (int rc = check_common("iou_loss_bwd", n, type, reduction)) return rc;
    if (n == 0) return YXH_OK;
    YXH_CHECK_ARG(pred && target && grad_out && g_pred, "iou_loss_bwd: null pointer");
    YXH_CHECK_ARG(aligned16(pred) && aligned16(target) && aligned16(g_pred) && aligned16(g_target),
                  "iou_loss_bwd: pred, target, g_pred and g_target must be 16-byte aligned");
    const dim3 grid((unsigned)((n + kIouThreads - 1) / kIouThreads)), block(kIouThreads);
    const int per_row = reduction == YXH_REDUCE_NONE ? 1 : 0, mean = reduction == YXH_REDUCE_MEAN ? 1 : 0;
#define YXH_IB(K, W)                                                                                             \
    hipLaunchKernelGGL((iou_loss_bwd<K, W>), grid, block, 0, st, (const float4*)pred, (const float4*)target, n, \
                       grad_out, per_row, mean, (float4*)g_pred, (float4*)g_target)
    if (type == YXH_IOU_LOSS_GIOU) {
        if (g_target) YXH_IB(YXH_IOU_LOSS_GIOU, true);
        else YXH_IB(YXH_IOU_LOSS_GIOU, false);
    } else {
        if (g_target) YXH_IB(YXH_IOU_LOSS_IOU, true);
        else YXH_IB(YXH_IOU_LOSS_IOU, false);
    }
#undef YXH_IB
    YXH_CHECK_LAUNCH("iou_loss_bwd");
    return YXH_OK;
}

}  // namespace yxh
