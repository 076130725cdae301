// Fused separable-window universal image quality index (UQI) for gfx950: per plane pair, the sum of the UQI of every valid
// window.  Serves universal_image_quality_index (pair n = plane n of preds and of target) and the spectral distortion index
// D-lambda (pair n = two bands of one image, decoded in the kernel: no gathered copies, no index tensor).
//
// The reference reflect-pads both images, stacks (a, b, a², b², a·b) into a 5·B-image batch, runs a grouped conv2d and crops
// the padded border.  With a square window the crop keeps exactly the windows that lie fully inside the image, so the padding
// is never needed (as in SSIM, csrc/image.hip).  Per window, with the five moments m0..m4 = E[a], E[b], E[aa], E[bb], E[ab]:
//   upper = 2 (m4 − m0 m1),  lower = (m2 − m0²) + (m3 − m1²) + eps,  uqi = (2 m0 m1) · upper / ((m0² + m1²) · lower)
// in fp32 with an IEEE division; the per-window values are added in fp64 and the map is never written.
//
// The row march of ssim_valid_kernel on the packed moments of window_moments.h: one workgroup = 256 output columns and a
// strip of kUqiRows output rows of one pair.  Per input row the workgroup stages the row segment (256 + KS − 1 columns) in
// LDS as interleaved (a, b) pairs (double buffered, converted to fp32 on load: any element alignment), every thread takes
// the horizontal taps of its column (moments5_taps) into a register ring of the last KS rows, addressed with compile-time
// slots, and the vertical pass runs in registers (moments5_ring).  One fp64 partial per workgroup (block_sum_store), no atomics.
//
// Grid: x = pair (up to 2^31 − 1 in one launch), y = column blocks, z = row strips.
// Two kernels with the same arithmetic in the same order (bit-equal sums): uqi_pair_kernel (any dtype and alignment, one row
// staged per barrier) and uqi_pair_v2_kernel (fp32, W % 4 == 0, 16-B aligned planes: KS rows per barrier, 16-B loads).
#include "common.h"
#include "window_moments.h"

#include <cstdlib>
#include <vector>

namespace tmx {

constexpr int kUqiThreads = 256;  // output columns per workgroup
constexpr int kUqiRows = 64;      // output rows per strip

__device__ __forceinline__ float uqi_window(const Moments5& m, float eps) {
  const float mu_aa = m.m01.x * m.m01.x, mu_bb = m.m01.y * m.m01.y, mu_ab = m.m01.x * m.m01.y;
  const float upper = 2.f * (m.m4 - mu_ab);
  const float lower = (m.m23.x - mu_aa) + (m.m23.y - mu_bb) + eps;
  return (2.f * mu_ab) * upper / ((mu_aa + mu_bb) * lower);
}

// Where the two planes of this workgroup's pair (blockIdx.x) live, and the pair's partial slot.
// BAND = false: pair n = (a plane n, b plane n), slot n.
// BAND = true:  a == b == x [B, L, H, W]; pair n -> image n / npairs, band pair k = n % npairs of the strict upper triangle
//               in row-major order (torch.triu_indices(L, L, 1)), slot k B + image: the result is [npairs, B].
template <bool BAND>
__device__ __forceinline__ void uqi_pair_planes(int L, int npairs, int64_t& plane_a, int64_t& plane_b, int64_t& slot) {
  const int64_t n = blockIdx.x;
  plane_a = plane_b = slot = n;
  if constexpr (BAND) {
    const int64_t image = n / npairs;
    int k = static_cast<int>(n % npairs);
    // row i of the strict upper triangle holds the L − 1 − i pairs (i, i + 1) .. (i, L − 1): at most L uniform steps
    int i = 0, row_len = L - 1;
    while (k >= row_len) {
      k -= row_len;
      ++i;
      --row_len;
    }
    const int j = i + 1 + k;
    plane_a = image * L + i;
    plane_b = image * L + j;
    slot = (n % npairs) * (gridDim.x / npairs) + image;
  }
}

template <typename T, int KS, bool BAND>
__global__ __launch_bounds__(kUqiThreads) void uqi_pair_kernel(const T* __restrict__ a, const T* __restrict__ b, int H, int W, int L,
                                                               int npairs, const float* __restrict__ wx, const float* __restrict__ wy,
                                                               float eps, double* __restrict__ partial) {
  constexpr int kSeg = kUqiThreads + KS - 1;
  __shared__ f2 s_ab[2][kSeg];

  const int Hv = H - KS + 1, Wv = W - KS + 1;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.y * kUqiThreads;
  const int y0 = blockIdx.z * kUqiRows;
  const int64_t plane_size = static_cast<int64_t>(H) * W;
  int64_t plane_a, plane_b, slot;
  uqi_pair_planes<BAND>(L, npairs, plane_a, plane_b, slot);
  const T* A = a + plane_a * plane_size;
  const T* Bp = b + plane_b * plane_size;

  float wxr[KS], wyr[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    wxr[k] = wx[k];
    wyr[k] = wy[k];
    // uniform values: left to itself the compiler keeps them (and their splatted pairs) in SGPRs and spills SGPRs from
    // KS 11 on (6 / 19 / 40 at KS 11 / 13 / 15); pinned to VGPRs no instantiation spills
    asm volatile("" : "+v"(wxr[k]));
    asm volatile("" : "+v"(wyr[k]));
  }

  // ring of horizontal window sums of the last KS input rows: (E[a], E[b]), (E[aa], E[bb]) packed, E[ab] scalar
  f2 rm[KS], rq[KS];
  float rx[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    rm[k] = f2{0.f, 0.f};
    rq[k] = f2{0.f, 0.f};
    rx[k] = 0.f;
  }

  const int out_rows = min(kUqiRows, Hv - y0);
  const int in_rows = out_rows + KS - 1;  // input rows y0 .. y0 + in_rows − 1 <= H − 1
  const bool col_ok = (x0 + tid) < Wv;
  double acc = 0.0;

  auto stage = [&](int r, int buf) {
    const int64_t row = static_cast<int64_t>(y0 + r) * W;
    for (int i = tid; i < kSeg; i += kUqiThreads) {
      const int x = x0 + i;
      const bool ok = x < W;
      s_ab[buf][i] = ok ? f2{to_f32<T>(A[row + x]), to_f32<T>(Bp[row + x])} : f2{0.f, 0.f};
    }
  };

  if (in_rows > 0) stage(0, 0);
  __syncthreads();

  for (int base = 0; base < in_rows; base += KS) {
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int r = base + j;
      if (r < in_rows) {  // uniform across the workgroup
        const int buf = r & 1;
        if (r + 1 < in_rows) stage(r + 1, buf ^ 1);
        const Moments5 h = moments5_taps(&s_ab[buf][tid], std::integral_constant<int, KS>{}, [&](int k) { return wxr[k]; });
        rm[j] = h.m01;
        rq[j] = h.m23;
        rx[j] = h.m4;
        if (r >= KS - 1 && col_ok) {
          const Moments5 m = moments5_ring(rm, rq, rx, j, [&](int k) { return wyr[k]; });
          acc += static_cast<double>(uqi_window(m, eps));
        }
        __syncthreads();  // staged row r + 1 visible; buffer of row r free for row r + 2
      }
    }
  }

  double v[1] = {acc};
  double* const out[1] = {partial};
  block_sum_store<1, kUqiThreads>(v, out, [&] { return (slot * gridDim.z + blockIdx.z) * gridDim.y + blockIdx.y; });
}

// ------------------------------------------------------------------------------------------------------------
// fp32, W % 4 == 0, 16-B aligned planes: the same windows, the same arithmetic in the same order (results are bit-equal to
// uqi_pair_kernel's), restructured as ssim_v2_kernel is: KS input rows staged per barrier instead of one, prefetched into
// registers with 16-B loads while the previous group is computed.
template <int KS, bool BAND>
__global__ __launch_bounds__(kUqiThreads) void uqi_pair_v2_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                                  int L, int npairs, const float* __restrict__ wx,
                                                                  const float* __restrict__ wy, float eps, double* __restrict__ partial) {
  constexpr int kSeg4 = (kUqiThreads + KS - 1 + 3) / 4;  // float4 columns per staged row segment
  constexpr int kSegF = kSeg4 * 4;
  constexpr int kItems = KS * kSeg4;                     // (row, column quad) items per group
  constexpr int kPer = (kItems + kUqiThreads - 1) / kUqiThreads;
  __shared__ f2 s_ab[2][KS][kSegF];

  const int Hv = H - KS + 1, Wv = W - KS + 1;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.y * kUqiThreads;
  const int y0 = blockIdx.z * kUqiRows;
  const int64_t plane_size = static_cast<int64_t>(H) * W;
  int64_t plane_a, plane_b, slot;
  uqi_pair_planes<BAND>(L, npairs, plane_a, plane_b, slot);
  const float* A = a + plane_a * plane_size;
  const float* Bp = b + plane_b * plane_size;

  float wxr[KS], wyr[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    wxr[k] = wx[k];
    wyr[k] = wy[k];
    asm volatile("" : "+v"(wxr[k]));  // (as in uqi_pair_kernel: no SGPR spills)
    asm volatile("" : "+v"(wyr[k]));
  }
  const int out_rows = min(kUqiRows, Hv - y0);
  const int in_rows = out_rows + KS - 1;  // input rows y0 .. y0 + in_rows − 1 <= H − 1
  const bool col_ok = (x0 + tid) < Wv;

  float4 pre_a[kPer], pre_b[kPer];
  auto fetch = [&](int g) {  // group g = input rows y0 + g KS .. + KS − 1 into registers
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int e = tid + i * kUqiThreads;
      const int r = e / kSeg4, q = e % kSeg4;
      const int y = y0 + g * KS + r, x = x0 + 4 * q;
      const bool ok = e < kItems && g * KS + r < in_rows && x < W;  // W % 4 == 0: a quad is all in or all out
      const int64_t o = static_cast<int64_t>(y) * W + x;
      pre_a[i] = ok ? *reinterpret_cast<const float4*>(A + o) : make_float4(0.f, 0.f, 0.f, 0.f);
      pre_b[i] = ok ? *reinterpret_cast<const float4*>(Bp + o) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int e = tid + i * kUqiThreads;
      if (e < kItems) {
        const int r = e / kSeg4, q = e % kSeg4;
        f2* d = &s_ab[buf][r][4 * q];
        d[0] = f2{pre_a[i].x, pre_b[i].x};
        d[1] = f2{pre_a[i].y, pre_b[i].y};
        d[2] = f2{pre_a[i].z, pre_b[i].z};
        d[3] = f2{pre_a[i].w, pre_b[i].w};
      }
    }
  };

  f2 rm[KS], rq[KS];
  float rx[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    rm[k] = f2{0.f, 0.f};
    rq[k] = f2{0.f, 0.f};
    rx[k] = 0.f;
  }
  double acc = 0.0;
  const int groups = (in_rows + KS - 1) / KS;
  if (groups > 0) {
    fetch(0);
    store(0);
  }
  __syncthreads();
  for (int g = 0; g < groups; ++g) {
    const int buf = g & 1;
    if (g + 1 < groups) fetch(g + 1);  // in flight during this group's arithmetic
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int r = g * KS + j;
      if (r < in_rows) {  // uniform across the workgroup
        const Moments5 h = moments5_taps(&s_ab[buf][j][tid], std::integral_constant<int, KS>{}, [&](int k) { return wxr[k]; });
        rm[j] = h.m01;
        rq[j] = h.m23;
        rx[j] = h.m4;
        if (r >= KS - 1 && col_ok) {
          const Moments5 m = moments5_ring(rm, rq, rx, j, [&](int k) { return wyr[k]; });
          acc += static_cast<double>(uqi_window(m, eps));
        }
      }
    }
    if (g + 1 < groups) {
      store(buf ^ 1);  // the other buffer was last read in group g − 1, before the previous barrier
      __syncthreads();
    }
  }

  double v[1] = {acc};
  double* const out[1] = {partial};
  block_sum_store<1, kUqiThreads>(v, out, [&] { return (slot * gridDim.z + blockIdx.z) * gridDim.y + blockIdx.y; });
}

// (output rows per strip, output columns per workgroup): what the tests need to place their strip and column-block edges
std::vector<int64_t> uqi_tile() { return {kUqiRows, kUqiThreads}; }

namespace {

struct UqiWindows {
  at::Tensor wy, wx;
  int64_t KS;
};

UqiWindows uqi_windows(const at::Tensor& ref, const at::Tensor& wy_in, const at::Tensor& wx_in, const char* name) {
  TORCH_CHECK(wy_in.is_cuda() && wx_in.is_cuda() && wy_in.device() == ref.device() && wx_in.device() == ref.device(), name,
              ": the windows must be on the inputs' device");
  const int64_t KS = wy_in.numel();
  TORCH_CHECK(wx_in.numel() == KS, name, ": window size mismatch");
  TORCH_CHECK(KS % 2 == 1 && KS >= 3 && KS <= 15, name, ": unsupported window size ", KS);
  return {wy_in.to(at::kFloat).contiguous(), wx_in.to(at::kFloat).contiguous(), KS};
}

// ``pairs`` plane pairs of H x W; returns fp64 [pairs] in the kernel's slot order
template <bool BAND>
at::Tensor uqi_run(const at::Tensor& a, const at::Tensor& b, int64_t pairs, int64_t H, int64_t W, int64_t L, int64_t npairs,
                   const UqiWindows& win, double eps, const char* name) {
  const int64_t KS = win.KS;
  TORCH_CHECK(H >= KS && W >= KS, name, ": plane smaller than the window");
  TORCH_CHECK(H * W <= INT32_MAX, name, ": plane too large");
  const int64_t Hv = H - KS + 1, Wv = W - KS + 1;
  const int64_t col_blocks = (Wv + kUqiThreads - 1) / kUqiThreads, strips = (Hv + kUqiRows - 1) / kUqiRows;
  TORCH_CHECK(pairs <= INT32_MAX && col_blocks <= 65535 && strips <= 65535, name, ": too many workgroups for one launch");
  auto partial = at::empty({pairs, strips * col_blocks}, a.options().dtype(at::kDouble));
  const dim3 grid(static_cast<unsigned>(pairs), static_cast<unsigned>(col_blocks), static_cast<unsigned>(strips));
  static const bool v2_off = std::getenv("TMX_UQI_V1") != nullptr;  // A/B knob (tools/uqi_bench.py)
  const bool v2 = !v2_off && a.scalar_type() == at::kFloat && W % 4 == 0 && (reinterpret_cast<uintptr_t>(a.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(b.data_ptr()) & 15) == 0;
  if (v2) {
    dispatch_odd_window(KS, name, [&](auto ks) {
      hipLaunchKernelGGL((uqi_pair_v2_kernel<decltype(ks)::value, BAND>), grid, dim3(kUqiThreads), 0, stream(), a.data_ptr<float>(),
                         b.data_ptr<float>(), static_cast<int>(H), static_cast<int>(W), static_cast<int>(L), static_cast<int>(npairs),
                         win.wx.data_ptr<float>(), win.wy.data_ptr<float>(), static_cast<float>(eps), partial.data_ptr<double>());
    });
  } else {
    dispatch_float3(a.scalar_type(), name, [&](auto tag) {
      using T = decltype(tag);
      dispatch_odd_window(KS, name, [&](auto ks) {
        hipLaunchKernelGGL((uqi_pair_kernel<T, decltype(ks)::value, BAND>), grid, dim3(kUqiThreads), 0, stream(),
                           reinterpret_cast<const T*>(a.data_ptr()), reinterpret_cast<const T*>(b.data_ptr()), static_cast<int>(H),
                           static_cast<int>(W), static_cast<int>(L), static_cast<int>(npairs), win.wx.data_ptr<float>(),
                           win.wy.data_ptr<float>(), static_cast<float>(eps), partial.data_ptr<double>());
      });
    });
  }
  TMX_LAUNCH_CHECK();
  return partial.size(1) == 1 ? partial.view({pairs}) : partial.sum(1);
}

}  // namespace

// preds / target [P, H, W] planes, fp32 / bf16 / fp16; wy / wx fp32 [KS] windows of the H / W axis, KS odd in 3 .. 15.
// Returns fp64 [P]: per plane the sum of the UQI over all valid windows.
at::Tensor uqi_sums(const at::Tensor& preds_in, const at::Tensor& target_in, const at::Tensor& wy_in, const at::Tensor& wx_in, double eps) {
  TORCH_CHECK(preds_in.is_cuda() && target_in.is_cuda(), "uqi_sums: expected GPU tensors");
  TORCH_CHECK(preds_in.device() == target_in.device(), "uqi_sums: preds and target on different devices");
  TORCH_CHECK(preds_in.dim() == 3 && preds_in.sizes() == target_in.sizes(), "uqi_sums: expected matching [P, H, W]");
  TORCH_CHECK(preds_in.scalar_type() == target_in.scalar_type(), "uqi_sums: dtype mismatch");
  const auto dtype = preds_in.scalar_type();
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16 || dtype == at::kHalf, "uqi_sums: unsupported dtype ", dtype);
  const auto win = uqi_windows(preds_in, wy_in, wx_in, "uqi_sums");
  const at::DeviceGuard guard(preds_in.device());
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  const int64_t P = p.size(0), H = p.size(1), W = p.size(2);
  if (P == 0) return at::zeros({0}, p.options().dtype(at::kDouble));
  return uqi_run<false>(p, t, P, H, W, 0, 1, win, eps, "uqi_sums");
}

// x [B, L, H, W]; returns fp64 [L (L − 1) / 2, B]: for every band pair (i < j), in torch.triu_indices(L, L, 1) order, and
// every image the sum of the UQI between bands i and j over all valid windows.  The bands are read in place.
at::Tensor uqi_band_pair_sums(const at::Tensor& x_in, const at::Tensor& wy_in, const at::Tensor& wx_in, double eps) {
  TORCH_CHECK(x_in.is_cuda(), "uqi_band_pair_sums: expected a GPU tensor");
  TORCH_CHECK(x_in.dim() == 4, "uqi_band_pair_sums: expected [B, L, H, W]");
  const auto dtype = x_in.scalar_type();
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16 || dtype == at::kHalf, "uqi_band_pair_sums: unsupported dtype ", dtype);
  const auto win = uqi_windows(x_in, wy_in, wx_in, "uqi_band_pair_sums");
  const at::DeviceGuard guard(x_in.device());
  auto x = x_in.contiguous();
  const int64_t B = x.size(0), L = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(L <= 65536, "uqi_band_pair_sums: too many bands");
  const int64_t npairs = L * (L - 1) / 2;
  if (npairs == 0 || B == 0) return at::zeros({npairs, B}, x.options().dtype(at::kDouble));
  TORCH_CHECK(npairs <= INT32_MAX / B, "uqi_band_pair_sums: too many band pairs for one launch");
  return uqi_run<true>(x, x, B * npairs, H, W, L, npairs, win, eps, "uqi_band_pair_sums").view({npairs, B});
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("uqi_sums(Tensor preds, Tensor target, Tensor wy, Tensor wx, float eps) -> Tensor");
  m.def("uqi_band_pair_sums(Tensor x, Tensor wy, Tensor wx, float eps) -> Tensor");
  m.def("uqi_tile() -> int[]", &tmx::uqi_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("uqi_sums", &tmx::uqi_sums);
  m.impl("uqi_band_pair_sums", &tmx::uqi_band_pair_sums);
}
