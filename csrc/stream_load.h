// 16 bytes of fp32 / bf16 / fp16 elements per lane for the streaming kernels (csrc/spectral.hip, csrc/neighbour_diff.hip): the
// vector width, the up-cast of one 16-byte register quad, and the generic / vector load pair.
#pragma once

#include "device_common.h"

namespace tmx {

template <typename T> struct SpecVec { static constexpr int n = 16 / sizeof(T); };

template <typename T> __device__ __forceinline__ void spec_unpack(const uint4& r, float (&o)[SpecVec<T>::n]);
template <> __device__ __forceinline__ void spec_unpack<float>(const uint4& r, float (&o)[4]) {
  o[0] = __uint_as_float(r.x), o[1] = __uint_as_float(r.y), o[2] = __uint_as_float(r.z), o[3] = __uint_as_float(r.w);
}
template <> __device__ __forceinline__ void spec_unpack<__hip_bfloat16>(const uint4& r, float (&o)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // bf16 -> fp32 is a 16-bit shift (what __bfloat162float does)
    o[2 * i] = __uint_as_float(w[i] << 16);
    o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
template <> __device__ __forceinline__ void spec_unpack<__half>(const uint4& r, float (&o)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = __half2float(__ushort_as_half(static_cast<unsigned short>(w[i] & 0xffffu)));
    o[2 * i + 1] = __half2float(__ushort_as_half(static_cast<unsigned short>(w[i] >> 16)));
  }
}

// V consecutive elements in flight.  VEC: one 16-byte load (src 16-byte aligned, all V in range).  Generic: scalar loads of
// the first ``valid`` elements, the others read as 0.
template <typename T, bool VEC> struct SpecLoad;
template <typename T> struct SpecLoad<T, true> {
  uint4 r;
  __device__ __forceinline__ void load(const T* __restrict__ src, int) { r = *reinterpret_cast<const uint4*>(src); }
  __device__ __forceinline__ void get(float (&o)[SpecVec<T>::n], int) const { spec_unpack<T>(r, o); }
};
template <typename T> struct SpecLoad<T, false> {
  T e[SpecVec<T>::n];
  __device__ __forceinline__ void load(const T* __restrict__ src, int valid) {
#pragma unroll
    for (int j = 0; j < SpecVec<T>::n; ++j) {
      if (j < valid) e[j] = src[j];
    }
  }
  __device__ __forceinline__ void get(float (&o)[SpecVec<T>::n], int valid) const {
#pragma unroll
    for (int j = 0; j < SpecVec<T>::n; ++j) o[j] = j < valid ? to_f32<T>(e[j]) : 0.f;
  }
};

}  // namespace tmx
