// What the training-side units share (train_bn.hip, train_bwd.hip, wgrad.hip): the strided NHWC
// view and its 16-byte chunk loads / stores, the activation derivative, and the host-side view checks.
#pragma once

#include "conv_common.hpp"

namespace yxh {

// A strided NHWC view (yxh_src): pixel m = b*HW + pix -> b*bs + pix*cs elements.
struct TView {
    const void* ptr;
    int C, cs, HW;
    long long bs;
};

__device__ __forceinline__ long long vofs(const TView& v, int m) {
    if (v.bs == (long long)v.HW * v.cs) return (long long)m * v.cs;  // images back to back: no (b, pix) split
    const int b = m / v.HW, pix = m - b * v.HW;
    return (long long)b * v.bs + (long long)pix * v.cs;
}

template <typename T, int N>
__device__ __forceinline__ void load_f(const T* p, float (&o)[N]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int q = 0; q < N; q += 4) {
            const float4 u = *(const float4*)(p + q);
            o[q] = u.x; o[q + 1] = u.y; o[q + 2] = u.z; o[q + 3] = u.w;
        }
    } else {
        static_assert(N % 8 == 0, "16-bit chunks");
#pragma unroll
        for (int q = 0; q < N; q += 8) {
            const uint4 u = *(const uint4*)(p + q);
            T t[8];
            __builtin_memcpy(t, &u, 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[q + e] = to_f32(t[e]);
        }
    }
}

template <typename T, int N>
__device__ __forceinline__ void store_f(T* p, const float (&o)[N]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int q = 0; q < N; q += 4) *(float4*)(p + q) = make_float4(o[q], o[q + 1], o[q + 2], o[q + 3]);
    } else {
#pragma unroll
        for (int q = 0; q < N; q += 8) {
            T t[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) t[e] = from_f32<T>(o[q + e]);
            uint4 u;
            __builtin_memcpy(&u, t, 16);
            *(uint4*)(p + q) = u;
        }
    }
}

// d act(z) / dz
template <bool PRECISE>
__device__ __forceinline__ float act_grad(float z, int act) {
    switch (act) {
        case YXH_ACT_SILU: {
            const float s = PRECISE ? 1.0f / (1.0f + expf(-z)) : __builtin_amdgcn_rcpf(1.0f + __expf(-z));
            return s * (1.0f + z * (1.0f - s));
        }
        case YXH_ACT_RELU: return z > 0.0f ? 1.0f : 0.0f;
        case YXH_ACT_LRELU: return z > 0.0f ? 1.0f : 0.1f;
        default: return 1.0f;
    }
}

// ------------------------------------------------------------------ host
inline int esz(int dt) { return dt == YXH_F32 ? 4 : 2; }

inline TView tview(const yxh_src* s, int C) {
    TView v;
    v.ptr = s ? s->ptr : nullptr;
    v.C = C;
    v.cs = s ? s->cstride : 0;
    v.HW = s ? s->h * s->w : 1;
    v.bs = s ? s->bstride : 0;
    return v;
}

inline bool a16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline int check_view(const yxh_src* s, int dt, const char* what) {
    YXH_CHECK_ARG(s && s->ptr, "%s: null view", what);
    const int epc = 16 / esz(dt);
    YXH_CHECK_ARG(a16(s->ptr) && s->channels > 0 && s->channels % epc == 0 && s->cstride % epc == 0 &&
                      s->bstride % epc == 0 && s->h > 0 && s->w > 0,
                  "%s: view not 16-byte aligned / chunked (channels %d, cstride %d)", what, s->channels, s->cstride);
    return YXH_OK;
}

}  // namespace yxh
