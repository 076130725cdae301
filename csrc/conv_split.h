// The split-f16 product the convolution kernels share (conv3x3.hip, conv_taps.hip): every fp32 value t, scaled by a power of
// two so that the largest of its group lands in [2^14, 2^15), is hi = f16(t), lo = f16(t - hi); a dot product is
// hi·lo + lo·hi + hi·hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation (the dropped lo·lo is below 2^-22 of |x||w|).
#pragma once

#include "common.h"

#include <cfloat>

namespace tmx {

constexpr int kCvLd = 72;  // halves per LDS row: 32 hi | 32 lo | 8 pad (the 16 lanes of a ds_read_b128 group hit distinct bank quads)
constexpr int kCvThreads = 256, kCvK = 32;
typedef short cv_frag8 __attribute__((ext_vector_type(8)));
typedef short cv_frag4 __attribute__((ext_vector_type(4)));
typedef float cv_acc4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ cv_acc4 cv_mma(cv_frag8 a, cv_frag8 b, cv_acc4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(reinterpret_cast<__attribute__((ext_vector_type(8))) _Float16&>(a),
                                                reinterpret_cast<__attribute__((ext_vector_type(8))) _Float16&>(b), c, 0, 0, 0);
}

// shift that puts a finite positive maximum in [2^14, 2^15); 0 for zero, inf and NaN
__device__ __forceinline__ int cv_shift(float mx) {
  int e = 0;
  if (!(mx > 0.f && mx <= FLT_MAX)) return 0;
  frexpf(mx, &e);
  return 15 - e;
}

__device__ __forceinline__ void cv_split(float v, int s, short& hi, short& lo) {
  const float t = ldexpf(v, s);
  const __half h = __float2half_rn(t);
  const __half l = __float2half_rn(t - __half2float(h));
  hi = static_cast<short>(bits16<__half>(h));
  lo = static_cast<short>(bits16<__half>(l));
}

}  // namespace tmx
