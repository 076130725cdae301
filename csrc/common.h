// Shared device/host helpers for the torchmetrics_forked_amd native library (gfx950 / CDNA4 only).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <cstdint>
#include <type_traits>

#include "device_common.h"

namespace tmx {

inline hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

#define TMX_CHECK_HIP(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e), " at ", #expr); \
  } while (0)

#define TMX_LAUNCH_CHECK() TMX_CHECK_HIP(hipGetLastError())

// The y and z axes of a grid hold at most this many workgroups: an op whose planes sit on z launches that many per call.
constexpr int64_t kMaxGridPlanes = 65535;

// Calls f(std::integral_constant<int, KS>{}) for the odd window sizes the window kernels are instantiated for.
template <typename F>
void dispatch_odd_window(int64_t ks, const char* name, F&& f) {
  switch (ks) {
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    case 9: f(std::integral_constant<int, 9>{}); break;
    case 11: f(std::integral_constant<int, 11>{}); break;
    case 13: f(std::integral_constant<int, 13>{}); break;
    case 15: f(std::integral_constant<int, 15>{}); break;
    default: TORCH_CHECK(false, name, ": unsupported window size ", ks);
  }
}

// Calls f(std::integral_constant<int, WS>{}) for the box-window sizes 2 .. 16, even and odd (csrc/box_window.hip).
template <typename F>
void dispatch_box_window(int64_t ws, const char* name, F&& f) {
  switch (ws) {
#define TMX_BOX_WINDOW_CASE(n) case n: f(std::integral_constant<int, n>{}); break;
    TMX_BOX_WINDOW_CASE(2) TMX_BOX_WINDOW_CASE(3) TMX_BOX_WINDOW_CASE(4) TMX_BOX_WINDOW_CASE(5) TMX_BOX_WINDOW_CASE(6)
    TMX_BOX_WINDOW_CASE(7) TMX_BOX_WINDOW_CASE(8) TMX_BOX_WINDOW_CASE(9) TMX_BOX_WINDOW_CASE(10) TMX_BOX_WINDOW_CASE(11)
    TMX_BOX_WINDOW_CASE(12) TMX_BOX_WINDOW_CASE(13) TMX_BOX_WINDOW_CASE(14) TMX_BOX_WINDOW_CASE(15) TMX_BOX_WINDOW_CASE(16)
#undef TMX_BOX_WINDOW_CASE
    default: TORCH_CHECK(false, name, ": unsupported window size ", ws);
  }
}

// Calls f(T{}) for the element type of an fp32 / bf16 / fp16 tensor (no fp64 instantiation, unlike TMX_DISPATCH_FLOAT).
template <typename F>
void dispatch_float3(at::ScalarType dtype, const char* name, F&& f) {
  switch (dtype) {
    case at::kFloat: f(float{}); break;
    case at::kBFloat16: f(__hip_bfloat16{}); break;
    case at::kHalf: f(__half{}); break;
    default: TORCH_CHECK(false, name, ": unsupported dtype ", dtype);
  }
}

}  // namespace tmx



// Dispatch over the float dtypes the framework accepts for score tensors.
#define TMX_DISPATCH_FLOAT(dtype, NAME, ...)                                       \
  [&] {                                                                            \
    switch (dtype) {                                                               \
      case at::kFloat: { using scalar_t = float; return __VA_ARGS__(); }           \
      case at::kDouble: { using scalar_t = double; return __VA_ARGS__(); }         \
      case at::kBFloat16: { using scalar_t = __hip_bfloat16; return __VA_ARGS__(); } \
      case at::kHalf: { using scalar_t = __half; return __VA_ARGS__(); }           \
      default: TORCH_CHECK(false, NAME, ": unsupported dtype ", dtype);            \
    }                                                                              \
  }()

#define TMX_DISPATCH_HALF(dtype, NAME, ...)                                        \
  [&] {                                                                            \
    switch (dtype) {                                                               \
      case at::kBFloat16: { using scalar_t = __hip_bfloat16; return __VA_ARGS__(); } \
      case at::kHalf: { using scalar_t = __half; return __VA_ARGS__(); }           \
      default: TORCH_CHECK(false, NAME, ": expected a 16-bit float tensor, got ", dtype); \
    }                                                                              \
  }()
