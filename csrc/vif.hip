// Fused pixel-domain visual information fidelity (VIF-p) for gfx950: tmx::vif_sums.
//
// The composition (functional/image/vif.py: _vif_planes) runs, per scale s = 0 .. 3 with window N = 17, 9, 5, 3, five dense
// N x N convolutions for the window moments of (p, t), about twenty pointwise launches on full maps and, from scale 1 on,
// two more full-resolution convolutions of which [::2, ::2] keeps a quarter.  The window is exactly outer(w, w) of a 1-D
// Gaussian, so here every filter is a row pass and a column pass (2N taps instead of N²), and no map reaches HBM:
//
//   vif_scale_kernel<T, N>: a 256-thread workgroup owns a kVifTH x kVifTW footprint of valid windows of one plane.  It
//     stages the (footprint + N − 1)² tile of (p, t) in LDS as float2, filters p, t, p², t², p·t along W into an LDS
//     intermediate and along H into registers (four output pixels per thread), evaluates the per-pixel VIF terms in fp32
//     in the composition's order, accumulates them in fp64 and writes ONE (num, den) partial pair;
//   vif_decim_kernel<T, N>: writes the next level's fp32 (p, t) planes, computing only the outputs [::2, ::2] keeps
//     (level size ceil((H − N + 1) / 2)); a 16 x 16 output footprint per workgroup;
//   vif_fold_kernel: one wave per (scale, num | den, plane) adds that plane's partials in a fixed order.
// No float atomics anywhere: two calls are bit-equal.  Seven filter launches and one fold per call.
//
// The 1-D windows are fixed by the scale: the host computes them once in fp64 and passes them by value (kernel
// arguments, read as scalars); there is no window tensor and no launch to make one.
//
// Footprint (exported by tmx::vif_tile): 32 x 32 outputs.  At N = 17 the staged tile is 48 x 48 (2.25x the outputs; a
// 16 x 16 footprint would restage 4x) and the W pass runs over 1.5 tile rows per output row.  LDS at N = 17: 18 KiB tile
// + 30 KiB row moments = 48 KiB, three workgroups per CU.
#include "common.h"
#include "window_moments.h"

#include <cmath>
#include <vector>

namespace tmx {

constexpr int kVifThreads = 256;
constexpr int kVifTH = 32, kVifTW = 32;                     // output footprint of the scale kernel
constexpr int kVifPer = kVifTH * kVifTW / kVifThreads;      // 4 output pixels per thread
constexpr int kVifRowStep = kVifThreads / kVifTW;           // a thread's outputs are kVifRowStep rows apart
constexpr int kVifDT = 16;                                  // the decimating kernel's footprint is kVifDT x kVifDT
constexpr int kVifScales = 4;
constexpr int kVifWin[kVifScales] = {17, 9, 5, 3};
static_assert(kVifTH * kVifTW % kVifThreads == 0 && kVifThreads % kVifTW == 0, "whole rows of outputs per pass");
static_assert(kVifDT * kVifDT == kVifThreads, "one decimated output per thread");

template <int N>
struct VifWindow {
  float w[N];
};

// One (num, den) term of one window, fp32, in the order of _vif_planes.  Comparisons (not fmaxf) so that a NaN moment
// stays NaN, as torch.clamp / torch.where keep it.
__device__ __forceinline__ void vif_pixel(float mu_p, float mu_t, float e_pp, float e_tt, float e_pt, float sigma_n_sq,
                                          float& num, float& den) {
  constexpr float eps = 1e-10f;
  float s_tt = e_tt - mu_t * mu_t;
  float s_pp = e_pp - mu_p * mu_p;
  s_tt = s_tt < 0.f ? 0.f : s_tt;
  s_pp = s_pp < 0.f ? 0.f : s_pp;
  const float s_tp = e_pt - mu_t * mu_p;
  float g = s_tp / (s_tt + eps);
  float s_v = s_pp - g * s_tp;
  if (s_tt < eps) {  // mask 1
    g = 0.f;
    s_v = s_pp;
    s_tt = 0.f;
  }
  if (s_pp < eps) {  // mask 2
    g = 0.f;
    s_v = 0.f;
  }
  if (g < 0.f) {  // mask 3
    s_v = s_pp;
    g = 0.f;
  }
  s_v = s_v < eps ? eps : s_v;
  num = log10f(1.f + g * g * s_tt / (s_v + sigma_n_sq));
  den = log10f(1.f + s_tt / sigma_n_sq);
}

// grid.x = (plane * tiles_h + tile_y) * tiles_w + tile_x; partials at part[0 | 1][that index]
template <typename T, int N>
__global__ __launch_bounds__(kVifThreads) void vif_scale_kernel(const T* __restrict__ preds, const T* __restrict__ target, int H, int W,
                                                                int tiles_h, int tiles_w, VifWindow<N> win, float sigma_n_sq,
                                                                double* __restrict__ part_num, double* __restrict__ part_den) {
  constexpr int kRows = kVifTH + N - 1, kSeg = kVifTW + N - 1;
  constexpr int kStage = kRows * kSeg, kRowItems = kRows * kVifTW;
  __shared__ f2 s_pt[kStage];
  __shared__ f2 s_m01[kRowItems];  // (mu_p, mu_t) after the W pass
  __shared__ f2 s_m23[kRowItems];  // (E[pp], E[tt])
  __shared__ float s_m4[kRowItems];  // E[pt]

  const int tid = threadIdx.x;
  unsigned b = blockIdx.x;
  const int x0 = static_cast<int>(b % tiles_w) * kVifTW;
  b /= tiles_w;
  const int y0 = static_cast<int>(b % tiles_h) * kVifTH;
  const int64_t plane = b / tiles_h;
  const int Hv = H - N + 1, Wv = W - N + 1;
  const T* P = preds + plane * H * W;
  const T* Tt = target + plane * H * W;

  // tile of (p, t); pixels outside the plane are zero-filled: they only reach windows that are masked below
  for (int e = tid; e < kStage; e += kVifThreads) {
    const int r = e / kSeg, c = e - r * kSeg;
    const int y = y0 + r, x = x0 + c;
    f2 v = f2{0.f, 0.f};
    if (y < H && x < W) {
      const int64_t o = static_cast<int64_t>(y) * W + x;
      v = f2{to_f32<T>(P[o]), to_f32<T>(Tt[o])};
    }
    s_pt[e] = v;
  }
  __syncthreads();

  // W pass: (tile row, output column) items
  for (int e = tid; e < kRowItems; e += kVifThreads) {
    const Moments5 h = moments5_taps(s_pt + (e / kVifTW) * kSeg + (e % kVifTW), std::integral_constant<int, N>{}, [&](int k) { return win.w[k]; });
    s_m01[e] = h.m01;
    s_m23[e] = h.m23;
    s_m4[e] = h.m4;
  }
  __syncthreads();

  // H pass and the per-pixel terms: outputs (ty + i * kVifRowStep, tx)
  const int tx = tid % kVifTW, ty = tid / kVifTW;
  double acc_num = 0.0, acc_den = 0.0;
#pragma unroll
  for (int i = 0; i < kVifPer; ++i) {
    const int oy = ty + i * kVifRowStep;
    Moments5 v;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int idx = (oy + k) * kVifTW + tx;
      v.add(win.w[k], s_m01[idx], s_m23[idx], s_m4[idx]);
    }
    if (y0 + oy < Hv && x0 + tx < Wv) {
      float num, den;
      vif_pixel(v.m01.x, v.m01.y, v.m23.x, v.m23.y, v.m4, sigma_n_sq, num, den);
      acc_num += static_cast<double>(num);
      acc_den += static_cast<double>(den);
    }
  }

  double acc[2] = {acc_num, acc_den};
  block_sum_store<2, kVifThreads>(acc, {part_num, part_den}, [&] { return blockIdx.x; });
}

// out[y][x] = sum_ij w[i] w[j] in[2y + i][2x + j] for y < Ho = ceil((H − N + 1) / 2), x < Wo: the level the composition
// gets from conv2d(., outer(w, w))[::2, ::2].  grid.x as above with kVifDT x kVifDT output tiles.
template <typename T, int N>
__global__ __launch_bounds__(kVifThreads) void vif_decim_kernel(const T* __restrict__ preds, const T* __restrict__ target, int H, int W,
                                                                int Ho, int Wo, int tiles_h, int tiles_w, VifWindow<N> win,
                                                                float* __restrict__ out_p, float* __restrict__ out_t) {
  constexpr int kRows = 2 * (kVifDT - 1) + N, kSeg = kRows;  // input rows 2y .. 2y + N − 1 of kVifDT outputs
  constexpr int kStage = kRows * kSeg, kRowItems = kRows * kVifDT;
  __shared__ f2 s_pt[kStage];
  __shared__ f2 s_mid[kRowItems];

  const int tid = threadIdx.x;
  unsigned b = blockIdx.x;
  const int x0 = static_cast<int>(b % tiles_w) * kVifDT;
  b /= tiles_w;
  const int y0 = static_cast<int>(b % tiles_h) * kVifDT;
  const int64_t plane = b / tiles_h;
  const T* P = preds + plane * H * W;
  const T* Tt = target + plane * H * W;

  for (int e = tid; e < kStage; e += kVifThreads) {
    const int r = e / kSeg, c = e - r * kSeg;
    const int y = 2 * y0 + r, x = 2 * x0 + c;
    f2 v = f2{0.f, 0.f};
    if (y < H && x < W) {
      const int64_t o = static_cast<int64_t>(y) * W + x;
      v = f2{to_f32<T>(P[o]), to_f32<T>(Tt[o])};
    }
    s_pt[e] = v;
  }
  __syncthreads();
  for (int e = tid; e < kRowItems; e += kVifThreads) {
    const f2* src = s_pt + (e / kVifDT) * kSeg + 2 * (e % kVifDT);
    f2 h = f2{0.f, 0.f};
#pragma unroll
    for (int k = 0; k < N; ++k) h = __builtin_elementwise_fma(f2{win.w[k], win.w[k]}, src[k], h);
    s_mid[e] = h;
  }
  __syncthreads();
  const int tx = tid % kVifDT, ty = tid / kVifDT;
  const int oy = y0 + ty, ox = x0 + tx;
  if (oy < Ho && ox < Wo) {
    f2 v = f2{0.f, 0.f};
#pragma unroll
    for (int k = 0; k < N; ++k) v = __builtin_elementwise_fma(f2{win.w[k], win.w[k]}, s_mid[(2 * ty + k) * kVifDT + tx], v);
    const int64_t o = (plane * Ho + oy) * Wo + ox;
    out_p[o] = v.x;
    out_t[o] = v.y;
  }
}

struct VifFoldArgs {
  int64_t offset[kVifScales];  // start of the scale's [2, P, tiles] partials
  int tiles[kVifScales];
};

// grid.x = (scale * 2 + k) * P + plane, one wave each: lane l adds tiles l, l + 64, ... in order, then the wave folds
__global__ __launch_bounds__(kWave) void vif_fold_kernel(const double* __restrict__ part, VifFoldArgs args, int P, double* __restrict__ out) {
  const int plane = blockIdx.x % P;
  const int sk = blockIdx.x / P;
  const int s = sk >> 1, k = sk & 1;
  const int tiles = args.tiles[s];
  const double* src = part + args.offset[s] + (static_cast<int64_t>(k) * P + plane) * tiles;
  double acc = 0.0;
  for (int i = threadIdx.x; i < tiles; i += kWave) acc += src[i];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// e_i = exp(−(i − (N − 1) / 2)² / (2 (N / 5)²)), w = e / sum(e): the 2-D kernel of _vif_planes is outer(w, w)
template <int N>
VifWindow<N> vif_window() {
  double e[N], sum = 0.0;
  const double sigma = N / 5.0;
  for (int i = 0; i < N; ++i) {
    const double d = i - (N - 1) / 2.0;
    e[i] = std::exp(-d * d / (2.0 * sigma * sigma));
    sum += e[i];
  }
  VifWindow<N> win;
  for (int i = 0; i < N; ++i) win.w[i] = static_cast<float>(e[i] / sum);
  return win;
}

template <typename T, int N>
void launch_vif_scale(const T* p, const T* t, int64_t P, int64_t H, int64_t W, float sigma_n_sq, double* part, int64_t tiles_h,
                      int64_t tiles_w) {
  static const VifWindow<N> win = vif_window<N>();
  const int64_t groups = P * tiles_h * tiles_w;
  hipLaunchKernelGGL((vif_scale_kernel<T, N>), dim3(static_cast<unsigned>(groups)), dim3(kVifThreads), 0, stream(), p, t, static_cast<int>(H),
                     static_cast<int>(W), static_cast<int>(tiles_h), static_cast<int>(tiles_w), win, sigma_n_sq, part, part + groups);
}

template <typename T, int N>
void launch_vif_decim(const T* p, const T* t, int64_t P, int64_t H, int64_t W, int64_t Ho, int64_t Wo, float* out_p, float* out_t) {
  static const VifWindow<N> win = vif_window<N>();
  const int64_t tiles_h = (Ho + kVifDT - 1) / kVifDT, tiles_w = (Wo + kVifDT - 1) / kVifDT;
  hipLaunchKernelGGL((vif_decim_kernel<T, N>), dim3(static_cast<unsigned>(P * tiles_h * tiles_w)), dim3(kVifThreads), 0, stream(), p, t,
                     static_cast<int>(H), static_cast<int>(W), static_cast<int>(Ho), static_cast<int>(Wo), static_cast<int>(tiles_h),
                     static_cast<int>(tiles_w), win, out_p, out_t);
}

// (rows, columns) of the scale kernel's output footprint: what the tests need to place their tile edges
std::vector<int64_t> vif_tile() { return {kVifTH, kVifTW}; }

template <typename T>
void vif_run(const at::Tensor& p, const at::Tensor& t, float sigma_n_sq, const int64_t* h, const int64_t* w, const int64_t* tiles_h,
             const int64_t* tiles_w, const int64_t* offset, double* part, float* levels) {
  const int64_t P = p.size(0);
  const T* p0 = reinterpret_cast<const T*>(p.data_ptr());
  const T* t0 = reinterpret_cast<const T*>(t.data_ptr());
  // level s >= 1: p planes then t planes, fp32
  float* lp[kVifScales] = {nullptr};
  float* lt[kVifScales] = {nullptr};
  float* cur = levels;
  for (int s = 1; s < kVifScales; ++s) {
    lp[s] = cur;
    lt[s] = cur + P * h[s] * w[s];
    cur += 2 * P * h[s] * w[s];
  }
  launch_vif_scale<T, 17>(p0, t0, P, h[0], w[0], sigma_n_sq, part + offset[0], tiles_h[0], tiles_w[0]);
  launch_vif_decim<T, 9>(p0, t0, P, h[0], w[0], h[1], w[1], lp[1], lt[1]);
  launch_vif_scale<float, 9>(lp[1], lt[1], P, h[1], w[1], sigma_n_sq, part + offset[1], tiles_h[1], tiles_w[1]);
  launch_vif_decim<float, 5>(lp[1], lt[1], P, h[1], w[1], h[2], w[2], lp[2], lt[2]);
  launch_vif_scale<float, 5>(lp[2], lt[2], P, h[2], w[2], sigma_n_sq, part + offset[2], tiles_h[2], tiles_w[2]);
  launch_vif_decim<float, 3>(lp[2], lt[2], P, h[2], w[2], h[3], w[3], lp[3], lt[3]);
  launch_vif_scale<float, 3>(lp[3], lt[3], P, h[3], w[3], sigma_n_sq, part + offset[3], tiles_h[3], tiles_w[3]);
}

// preds / target [P, H, W] planes (P = B*C), fp32 / bf16 / fp16, H, W >= 41.  Returns fp64 [4, 2, P]: per scale and plane
// the sums over all valid windows of log10(1 + g² st² / (sv² + sn²)) and of log10(1 + st² / sn²).
at::Tensor vif_sums(const at::Tensor& preds_in, const at::Tensor& target_in, double sigma_n_sq) {
  TORCH_CHECK(preds_in.is_cuda() && target_in.is_cuda(), "vif_sums: expected GPU tensors");
  TORCH_CHECK(preds_in.device() == target_in.device(), "vif_sums: preds and target on different devices");
  TORCH_CHECK(preds_in.dim() == 3 && preds_in.sizes() == target_in.sizes(), "vif_sums: expected matching [P, H, W]");
  TORCH_CHECK(preds_in.scalar_type() == target_in.scalar_type(), "vif_sums: dtype mismatch");
  const auto dtype = preds_in.scalar_type();
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16 || dtype == at::kHalf, "vif_sums: unsupported dtype ", dtype);
  TORCH_CHECK(sigma_n_sq > 0, "vif_sums: sigma_n_sq must be positive");
  const int64_t P = preds_in.size(0), H = preds_in.size(1), W = preds_in.size(2);
  TORCH_CHECK(H >= 41 && W >= 41, "vif_sums: planes smaller than 41 x 41");
  TORCH_CHECK(H * W <= INT32_MAX, "vif_sums: plane too large");
  const at::DeviceGuard guard(preds_in.device());
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  auto opts = p.options().dtype(at::kDouble);
  if (P == 0) return at::zeros({kVifScales, 2, 0}, opts);

  int64_t h[kVifScales], w[kVifScales], tiles_h[kVifScales], tiles_w[kVifScales], offset[kVifScales];
  int64_t n_part = 0, n_level = 0;
  VifFoldArgs fold;
  for (int s = 0; s < kVifScales; ++s) {
    const int64_t n = kVifWin[s];
    h[s] = s == 0 ? H : (h[s - 1] - n + 2) / 2;  // ceil((h − n + 1) / 2)
    w[s] = s == 0 ? W : (w[s - 1] - n + 2) / 2;
    tiles_h[s] = (h[s] - n + 1 + kVifTH - 1) / kVifTH;
    tiles_w[s] = (w[s] - n + 1 + kVifTW - 1) / kVifTW;
    offset[s] = n_part;
    fold.offset[s] = n_part;
    fold.tiles[s] = static_cast<int>(tiles_h[s] * tiles_w[s]);
    n_part += 2 * P * tiles_h[s] * tiles_w[s];
    if (s > 0) n_level += 2 * P * h[s] * w[s];
  }
  // all workgroups of a launch sit in grid.x; the decimating kernel of level 1 has the most (16 x 16 outputs each)
  const int64_t max_groups = P * ((h[1] + kVifDT - 1) / kVifDT) * ((w[1] + kVifDT - 1) / kVifDT);
  TORCH_CHECK(max_groups <= INT32_MAX && P * tiles_h[0] * tiles_w[0] <= INT32_MAX && P * 2 * kVifScales <= INT32_MAX,
              "vif_sums: too many workgroups for one launch");
  auto partial = at::empty({n_part}, opts);
  auto levels = at::empty({n_level}, p.options().dtype(at::kFloat));
  auto out = at::empty({kVifScales, 2, P}, opts);
  const float sn = static_cast<float>(sigma_n_sq);
  double* part = partial.data_ptr<double>();
  float* lv = levels.data_ptr<float>();
  dispatch_float3(dtype, "vif_sums", [&](auto tag) { vif_run<decltype(tag)>(p, t, sn, h, w, tiles_h, tiles_w, offset, part, lv); });
  hipLaunchKernelGGL(vif_fold_kernel, dim3(static_cast<unsigned>(2 * kVifScales * P)), dim3(kWave), 0, stream(), part, fold,
                     static_cast<int>(P), out.data_ptr<double>());
  TMX_LAUNCH_CHECK();
  return out;
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("vif_sums(Tensor preds, Tensor target, float sigma_n_sq) -> Tensor");
  m.def("vif_tile() -> int[]", &tmx::vif_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) { m.impl("vif_sums", &tmx::vif_sums); }
