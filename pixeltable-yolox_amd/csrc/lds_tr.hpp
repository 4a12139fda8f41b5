// gfx950's transposed LDS read (ds_read_b64_tr_b16), shared by the 16-bit weight-gradient
// families that read their MFMA operands pixel(K)-major out of a pixel-major LDS image
// (wgrad_glds.hip, wgrad9t_h.hip).
#pragma once

#include "conv_common.hpp"

namespace yxh {

typedef short wg_i16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint2 lds_read_tr16(const char* ptr) {
    const auto q = (__attribute__((address_space(3))) wg_i16x4*)(const_cast<char*>(ptr));
    return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16(q));
}

}  // namespace yxh
