// Streaming kernels for gfx950 behind peak_signal_noise_ratio_with_blocked_effect, total_variation and image_gradients: the
// difference of a pixel with its right and its lower neighbour over [B, C, H, W] planes (fp32 / bf16 / fp16, read in place, once), no
// LDS staging, no full-size temporary.
//
// One tile walk (nd_walk) for the three kernel families.  The grid is flat on x over (plane, row strip, column block), the
// index decoded in int64.  A workgroup of kNdThreads = 256 threads takes kNdRows = 32 rows by CW = 64 · V columns of one plane (V = 16
// bytes of the element type: 4 fp32, 8 bf16 / fp16; CW = 256 or 512); wave w of the four takes the kNdWaveRows = 8 rows
// 8w .. 8w + 7 of the strip, lane l the V columns V·l .. of the column block.  A thread loads its V columns of its eight rows and of
// the one halo row below them, all nine loads in flight, and walks down with the previous row in registers:
//   vertical pair   (i, i + 1) of a column: row i + 1 − row i, both in registers; it belongs to the thread that owns row i (the halo row
//                   is read for it and owns nothing), so the last row of the plane owns no pair;
//   horizontal pair (j, j + 1) of a row: inside the vector from registers; across the vector's right edge the next lane's first
//                   element, by a cross-lane move, and for the last lane of a wave one scalar load.  It belongs to the thread that
//                   owns column j, so the last column owns no pair.
// Every pair is counted exactly once.  The difference is one fp32 subtraction of the up-cast inputs (what the composition
// computes and what image_gradients stores); its square or absolute value is widened and added to per-thread fp64 sums, which
// block_sum_store adds to one fp64 partial per workgroup and quantity; a fold kernel adds the partials in a fixed order.  No
// atomics: two runs are bit-equal.
//
// PSNR-B.  block_size is a run-time integer >= 1.  A thread's columns do not change on the way down: the boundary flags
// (j + 1) % block_size == 0 of its V horizontal pairs are a bit mask formed once per thread (one modulo, then a counter), the flag
// of a row pair is uniform per wave (one modulo per thread, then a counter): no division in the per-element path.  psnrb_kernel
// also reads target once for Σ(p − t)² and its minimum and maximum (fminf / fmaxf and a NaN count: a NaN gives NaN for both, as
// torch.min / torch.max do).
//
// Every kernel has a generic instantiation (scalar loads and stores, any W, any alignment) and a vector one (16-byte loads and
// stores: planes 16-byte aligned and W a multiple of V).  Both assign the same elements to the same thread and run the same
// arithmetic in the same order: their results are bit-equal.
#include "common.h"
#include "stream_load.h"
#include "window_moments.h"

#include <cmath>
#include <cstdlib>
#include <limits>
#include <tuple>
#include <vector>

namespace tmx {

constexpr int kNdThreads = 256;
constexpr int kNdWaves = kNdThreads / kWave;
constexpr int kNdWaveRows = 8;                    // rows a wave walks down; one more is read as its halo
constexpr int kNdRows = kNdWaves * kNdWaveRows;   // rows per strip (workgroup)
constexpr int kNdCols = kWave * 4;                // fp32 columns per workgroup (16-bit: twice as many)

// Where a thread stands: fixed for the whole walk.
struct NdPos {
  int64_t plane, row0, col0;  // first row of the wave, first column of the thread
  int nrows;                  // rows of the wave inside the plane: 0 .. kNdWaveRows (uniform per wave)
  int valid;                  // columns of the thread inside the plane: 0 .. V (vector kernels: 0 or V)
  int hpairs;                 // horizontal pairs the thread owns: columns j with j < W − 1
};

template <int V>
__device__ __forceinline__ NdPos nd_pos(int64_t H, int64_t W, int64_t strips, int64_t cblocks) {
  const int64_t wg = blockIdx.x;
  const int64_t cb = wg % cblocks, rest = wg / cblocks;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  NdPos p;
  p.plane = rest / strips;
  p.row0 = (rest % strips) * kNdRows + wave * kNdWaveRows;
  p.col0 = (cb * kWave + lane) * V;
  p.nrows = p.row0 < H ? static_cast<int>(min(static_cast<int64_t>(kNdWaveRows), H - p.row0)) : 0;
  p.valid = p.col0 < W ? static_cast<int>(min(static_cast<int64_t>(V), W - p.col0)) : 0;
  p.hpairs = p.col0 < W - 1 ? static_cast<int>(min(static_cast<int64_t>(V), W - 1 - p.col0)) : 0;
  return p;
}

// Walks the thread's rows of ``plane`` [H, W]: f(r, cur, right, nxt, has_next) per row row0 + r with cur the V columns of the row,
// right the element after them (meaningful where the thread owns V pairs), nxt the row below (has_next: uniform per wave).
template <typename T, bool VEC, typename F>
__device__ __forceinline__ void nd_walk(const T* __restrict__ plane, int64_t H, int64_t W, const NdPos& pos, F&& f) {
  constexpr int V = SpecVec<T>::n;
  const int lane = threadIdx.x & (kWave - 1);
  const bool edge = lane == kWave - 1 && pos.col0 + V < W;  // the next column is another workgroup's: one scalar load per row
  const T* at = plane + pos.row0 * W + pos.col0;

  SpecLoad<T, VEC> ld[kNdWaveRows + 1];
  T beyond[kNdWaveRows];
#pragma unroll
  for (int r = 0; r <= kNdWaveRows; ++r) {
    if (pos.row0 + r < H && pos.valid > 0) ld[r].load(at + r * W, pos.valid);  // r == nrows: the halo row, where the plane has one
  }
#pragma unroll
  for (int r = 0; r < kNdWaveRows; ++r) {
    if (r < pos.nrows && edge) beyond[r] = at[r * W + V];
  }

  float cur[V], nxt[V];
#pragma unroll
  for (int k = 0; k < V; ++k) cur[k] = nxt[k] = 0.f;
  if (pos.nrows > 0 && pos.valid > 0) ld[0].get(cur, pos.valid);
#pragma unroll
  for (int r = 0; r < kNdWaveRows; ++r) {
    if (r < pos.nrows) {
      const bool has_next = pos.row0 + r + 1 < H;
      if (has_next && pos.valid > 0) ld[r + 1].get(nxt, pos.valid);
      float right = __shfl_down(cur[0], 1, kWave);
      if (edge) right = to_f32<T>(beyond[r]);
      f(r, cur, right, nxt, has_next);
#pragma unroll
      for (int k = 0; k < V; ++k) cur[k] = nxt[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------------- total variation
template <typename T, bool VEC>
__device__ __forceinline__ void tv_body(const T* __restrict__ img, int64_t H, int64_t W, int64_t strips, int64_t cblocks,
                                        double* __restrict__ partial) {
  constexpr int V = SpecVec<T>::n;
  const NdPos pos = nd_pos<V>(H, W, strips, cblocks);
  double acc = 0.0;
  nd_walk<T, VEC>(img + pos.plane * H * W, H, W, pos, [&](int, const float (&cur)[V], float right, const float (&nxt)[V], bool has_next) {
    if (has_next) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (k < pos.valid) acc += static_cast<double>(fabsf(nxt[k] - cur[k]));
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float r = k + 1 < V ? cur[k + 1 < V ? k + 1 : k] : right;
      if (k < pos.hpairs) acc += static_cast<double>(fabsf(r - cur[k]));
    }
  });
  double v[1] = {acc};
  double* const out[1] = {partial};
  block_sum_store<1, kNdThreads>(v, out, [&] { return static_cast<int64_t>(blockIdx.x); });
}

template <typename T>
__global__ __launch_bounds__(kNdThreads) void tv_generic_kernel(const T* __restrict__ img, int64_t H, int64_t W, int64_t strips, int64_t cblocks,
                                                               double* __restrict__ partial) {
  tv_body<T, false>(img, H, W, strips, cblocks, partial);
}

template <typename T>
__global__ __launch_bounds__(kNdThreads) void tv_vec_kernel(const T* __restrict__ img, int64_t H, int64_t W, int64_t strips, int64_t cblocks,
                                                           double* __restrict__ partial) {
  tv_body<T, true>(img, H, W, strips, cblocks, partial);
}

// out[r] = the sum of part[r][0 .. n): one wave per row; lane l adds entries l, l + 64, ... in order, then the lanes are added
// by the fixed tree of block_sum_store.
__global__ __launch_bounds__(kWave) void tv_fold_kernel(const double* __restrict__ part, int64_t n, double* __restrict__ out) {
  const double* row = part + static_cast<int64_t>(blockIdx.x) * n;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kWave) acc += row[i];
  double v[1] = {acc};
  double* const o[1] = {out};
  block_sum_store<1, kWave>(v, o, [&] { return static_cast<int64_t>(blockIdx.x); });
}

// ------------------------------------------------------------------------------------------------------------ PSNR-B
constexpr int kPsnrbSums = 4;  // Σ(p − t)², D_B, D_BC, NaN pixels of target; then min and max of target

// The workgroup's minimum and maximum (NaN-free by construction) to lo[index] / hi[index]: wave shuffles, one LDS slot per wave.
template <int kThreads>
__device__ __forceinline__ void block_minmax_store(float mn, float mx, double* __restrict__ lo, double* __restrict__ hi, int64_t index) {
  __shared__ float red[2][kThreads / kWave];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, off, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
  }
  const int tid = threadIdx.x;
  if ((tid & (kWave - 1)) == 0) red[0][tid / kWave] = mn, red[1][tid / kWave] = mx;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kThreads / kWave; ++w) mn = fminf(mn, red[0][w]), mx = fmaxf(mx, red[1][w]);
    lo[index] = static_cast<double>(mn);
    hi[index] = static_cast<double>(mx);
  }
}

// part: [6][workgroups] = the kPsnrbSums sums, then min and max.
template <typename T, bool VEC>
__device__ __forceinline__ void psnrb_body(const T* __restrict__ preds, const T* __restrict__ target, int64_t H, int64_t W, int64_t strips,
                                           int64_t cblocks, int bs, double* __restrict__ part) {
  constexpr int V = SpecVec<T>::n;
  const NdPos pos = nd_pos<V>(H, W, strips, cblocks);
  const int64_t groups = gridDim.x;

  // bit k: the pair (col0 + k, col0 + k + 1) crosses a block boundary.  One modulo per thread, here.
  unsigned hflags = 0;
  int m = static_cast<int>((pos.col0 + 1) % bs);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    hflags |= (m == 0 ? 1u : 0u) << k;
    m = m + 1 == bs ? 0 : m + 1;
  }
  int rm = static_cast<int>((pos.row0 + 1) % bs);  // (row + 1) % bs of the row the walk stands on: uniform per wave

  // target rows: no halo.  Issued before the walk so that they are in flight with the walk's loads.
  SpecLoad<T, VEC> lt[kNdWaveRows];
  const T* tat = target + pos.plane * H * W + pos.row0 * W + pos.col0;
#pragma unroll
  for (int r = 0; r < kNdWaveRows; ++r) {
    if (r < pos.nrows && pos.valid > 0) lt[r].load(tat + r * W, pos.valid);
  }

  double sse = 0.0, hb = 0.0, hbc = 0.0, vb = 0.0, vbc = 0.0, nans = 0.0;
  float mn = std::numeric_limits<float>::infinity(), mx = -std::numeric_limits<float>::infinity();
  nd_walk<T, VEC>(preds + pos.plane * H * W, H, W, pos, [&](int r, const float (&cur)[V], float right, const float (&nxt)[V], bool has_next) {
    if (pos.valid > 0) {
      float tv[V];
      lt[r].get(tv, pos.valid);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (k < pos.valid) {
          const double d = static_cast<double>(cur[k] - tv[k]);
          sse = fma(d, d, sse);
          mn = fminf(mn, tv[k]);
          mx = fmaxf(mx, tv[k]);
          nans += tv[k] != tv[k] ? 1.0 : 0.0;
        }
      }
    }
    if (has_next) {
      double row = 0.0;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (k < pos.valid) {
          const double d = static_cast<double>(nxt[k] - cur[k]);
          row = fma(d, d, row);
        }
      }
      if (rm == 0) vb += row; else vbc += row;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float rt = k + 1 < V ? cur[k + 1 < V ? k + 1 : k] : right;
      if (k < pos.hpairs) {
        const float d = rt - cur[k];
        const bool b = (hflags >> k) & 1u;
        const double on = static_cast<double>(b ? d : 0.f), off = static_cast<double>(b ? 0.f : d);
        hb = fma(on, on, hb);
        hbc = fma(off, off, hbc);
      }
    }
    rm = rm + 1 == bs ? 0 : rm + 1;
  });

  double v[kPsnrbSums] = {sse, hb + vb, hbc + vbc, nans};
  double* const out[kPsnrbSums] = {part, part + groups, part + 2 * groups, part + 3 * groups};
  block_sum_store<kPsnrbSums, kNdThreads>(v, out, [&] { return static_cast<int64_t>(blockIdx.x); });
  block_minmax_store<kNdThreads>(mn, mx, part + 4 * groups, part + 5 * groups, blockIdx.x);
}

template <typename T>
__global__ __launch_bounds__(kNdThreads) void psnrb_generic_kernel(const T* __restrict__ preds, const T* __restrict__ target, int64_t H, int64_t W,
                                                                  int64_t strips, int64_t cblocks, int bs, double* __restrict__ part) {
  psnrb_body<T, false>(preds, target, H, W, strips, cblocks, bs, part);
}

template <typename T>
__global__ __launch_bounds__(kNdThreads) void psnrb_vec_kernel(const T* __restrict__ preds, const T* __restrict__ target, int64_t H, int64_t W,
                                                              int64_t strips, int64_t cblocks, int bs, double* __restrict__ part) {
  psnrb_body<T, true>(preds, target, H, W, strips, cblocks, bs, part);
}

// One workgroup: thread t adds the partials t, t + 256, ... of each sum in order; the threads by the fixed tree of block_sum_store.
// out[5] = Σ(p − t)², D_B, D_BC, min target, max target; a NaN pixel in target makes the last two NaN.
__global__ __launch_bounds__(kNdThreads) void psnrb_fold_kernel(const double* __restrict__ part, int64_t n, double* __restrict__ out) {
  double v[kPsnrbSums];
#pragma unroll
  for (int q = 0; q < kPsnrbSums; ++q) v[q] = 0.0;
  float mn = std::numeric_limits<float>::infinity(), mx = -std::numeric_limits<float>::infinity();
  for (int64_t i = threadIdx.x; i < n; i += kNdThreads) {
#pragma unroll
    for (int q = 0; q < kPsnrbSums; ++q) v[q] += part[q * n + i];
    mn = fminf(mn, static_cast<float>(part[4 * n + i]));  // fp32 values, widened by the streaming kernel: exact
    mx = fmaxf(mx, static_cast<float>(part[5 * n + i]));
  }
  __shared__ double nan_count[1];
  double* const o[kPsnrbSums] = {out, out + 1, out + 2, nan_count};
  block_sum_store<kPsnrbSums, kNdThreads>(v, o, [&] { return static_cast<int64_t>(0); });
  block_minmax_store<kNdThreads>(mn, mx, out + 3, out + 4, 0);
  if (threadIdx.x == 0 && nan_count[0] > 0.0) out[3] = out[4] = std::numeric_limits<double>::quiet_NaN();  // (thread 0 wrote all three)
}

// --------------------------------------------------------------------------------------------------- image gradients
template <typename T> __device__ __forceinline__ T nd_round(float v);
template <> __device__ __forceinline__ float nd_round<float>(float v) { return v; }
template <> __device__ __forceinline__ __hip_bfloat16 nd_round<__hip_bfloat16>(float v) {
  const uint16_t bits = v != v ? uint16_t{0x7fc0} : round_bits16<__hip_bfloat16>(v);  // one NaN pattern, as the CPU's rounding gives
  return *reinterpret_cast<const __hip_bfloat16*>(&bits);
}
template <> __device__ __forceinline__ __half nd_round<__half>(float v) { return __float2half_rn(v); }

template <typename T, bool VEC>
__device__ __forceinline__ void nd_store(T* __restrict__ dst, const float (&v)[SpecVec<T>::n], int valid) {
  constexpr int V = SpecVec<T>::n;
  if constexpr (VEC) {  // W a multiple of V and the output a fresh allocation: 16-byte aligned
    T e[V];
#pragma unroll
    for (int k = 0; k < V; ++k) e[k] = nd_round<T>(v[k]);
    *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(e);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (k < valid) dst[k] = nd_round<T>(v[k]);
    }
  }
}

// dy[i][j] = x[i + 1][j] − x[i][j], dx[i][j] = x[i][j + 1] − x[i][j]; the last row of dy and the last column of dx are stored as zeros.
template <typename T, bool VEC>
__device__ __forceinline__ void gradients_body(const T* __restrict__ img, int64_t H, int64_t W, int64_t strips, int64_t cblocks, T* __restrict__ dy,
                                               T* __restrict__ dx) {
  constexpr int V = SpecVec<T>::n;
  const NdPos pos = nd_pos<V>(H, W, strips, cblocks);
  const int64_t base = pos.plane * H * W + pos.row0 * W + pos.col0;
  nd_walk<T, VEC>(img + pos.plane * H * W, H, W, pos, [&](int r, const float (&cur)[V], float right, const float (&nxt)[V], bool has_next) {
    if (pos.valid > 0) {
      float gy[V], gx[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float rt = k + 1 < V ? cur[k + 1 < V ? k + 1 : k] : right;
        gy[k] = has_next ? nxt[k] - cur[k] : 0.f;
        gx[k] = k < pos.hpairs ? rt - cur[k] : 0.f;
      }
      nd_store<T, VEC>(dy + base + r * W, gy, pos.valid);
      nd_store<T, VEC>(dx + base + r * W, gx, pos.valid);
    }
  });
}

template <typename T>
__global__ __launch_bounds__(kNdThreads) void gradients_generic_kernel(const T* __restrict__ img, int64_t H, int64_t W, int64_t strips,
                                                                      int64_t cblocks, T* __restrict__ dy, T* __restrict__ dx) {
  gradients_body<T, false>(img, H, W, strips, cblocks, dy, dx);
}

template <typename T>
__global__ __launch_bounds__(kNdThreads) void gradients_vec_kernel(const T* __restrict__ img, int64_t H, int64_t W, int64_t strips, int64_t cblocks,
                                                                  T* __restrict__ dy, T* __restrict__ dx) {
  gradients_body<T, true>(img, H, W, strips, cblocks, dy, dx);
}

// ------------------------------------------------------------------------------------------------------------- host
namespace {

struct NdInputs {
  at::Tensor x;
  int64_t B, C, H, W, strips, cblocks, groups;
  bool vec;
};

// TMX_GRADIENT_GENERIC: the A/B knob of the 16-byte-load kernels, read once per process
bool nd_vec_off() {
  static const bool off = std::getenv("TMX_GRADIENT_GENERIC") != nullptr;
  return off;
}

void nd_check(const at::Tensor& x, const char* name) {
  TORCH_CHECK(x.is_cuda(), name, ": expected GPU tensors");
  TORCH_CHECK(x.dim() == 4, name, ": expected [B, C, H, W]");
  const auto dtype = x.scalar_type();
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16 || dtype == at::kHalf, name, ": unsupported dtype ", dtype);
  TORCH_CHECK(x.numel() > 0, name, ": empty input");
}

NdInputs nd_inputs(const at::Tensor& x_in, const char* name) {
  nd_check(x_in, name);
  NdInputs in;
  in.x = x_in.contiguous();
  in.B = in.x.size(0), in.C = in.x.size(1), in.H = in.x.size(2), in.W = in.x.size(3);
  const int64_t V = 16 / static_cast<int64_t>(in.x.element_size());
  in.strips = (in.H + kNdRows - 1) / kNdRows;
  in.cblocks = (in.W + kWave * V - 1) / (kWave * V);
  TORCH_CHECK(in.B * in.C <= INT32_MAX / (in.strips * in.cblocks), name, ": too many workgroups for one launch");
  in.groups = in.B * in.C * in.strips * in.cblocks;
  in.vec = !nd_vec_off() && in.W % V == 0 && (reinterpret_cast<uintptr_t>(in.x.data_ptr()) & 15) == 0;
  return in;
}

}  // namespace

// fp64 [B]: per image Σ|x[i + 1][j] − x[i][j]| + Σ|x[i][j + 1] − x[i][j]| over C, H, W of img [B, C, H, W].
at::Tensor tv_sums(const at::Tensor& img) {
  const char* name = "tv_sums";
  const at::DeviceGuard guard(img.device());
  const auto in = nd_inputs(img, name);
  const int64_t per_image = in.groups / in.B;
  auto partial = at::empty({in.B, per_image}, in.x.options().dtype(at::kDouble));
  dispatch_float3(in.x.scalar_type(), name, [&](auto tag) {
    using T = decltype(tag);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(in.groups)), dim3(kNdThreads), 0, stream(), reinterpret_cast<const T*>(in.x.data_ptr()),
                         in.H, in.W, in.strips, in.cblocks, partial.data_ptr<double>());
    };
    in.vec ? launch(tv_vec_kernel<T>) : launch(tv_generic_kernel<T>);
  });
  TMX_LAUNCH_CHECK();
  if (per_image == 1) return partial.view({in.B});
  auto sums = at::empty({in.B}, partial.options());
  hipLaunchKernelGGL(tv_fold_kernel, dim3(static_cast<unsigned>(in.B)), dim3(kWave), 0, stream(), partial.data_ptr<double>(), per_image,
                     sums.data_ptr<double>());
  TMX_LAUNCH_CHECK();
  return sums;
}

// fp64 [5]: Σ(p − t)², D_B, D_BC, min target, max target over preds / target [B, 1, H, W].  D_B: the squared differences of preds over
// the horizontal pairs (j, j + 1) with (j + 1) % block_size == 0 and the vertical pairs (i, i + 1) with (i + 1) % block_size == 0; D_BC:
// over every other pair.
at::Tensor psnrb_sums(const at::Tensor& preds, const at::Tensor& target, int64_t block_size) {
  const char* name = "psnrb_sums";
  TORCH_CHECK(preds.is_cuda() && target.is_cuda(), name, ": expected GPU tensors");
  TORCH_CHECK(preds.device() == target.device(), name, ": preds and target on different devices");
  TORCH_CHECK(preds.dim() == 4 && preds.sizes() == target.sizes(), name, ": expected matching [B, 1, H, W]");
  TORCH_CHECK(preds.scalar_type() == target.scalar_type(), name, ": dtype mismatch");
  TORCH_CHECK(preds.size(1) == 1, name, ": expected one channel");
  TORCH_CHECK(block_size >= 1 && block_size <= INT32_MAX, name, ": block_size must be a positive 32-bit integer");
  const at::DeviceGuard guard(preds.device());
  auto in = nd_inputs(preds, name);
  auto t = target.contiguous();
  in.vec = in.vec && (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
  auto part = at::empty({kPsnrbSums + 2, in.groups}, in.x.options().dtype(at::kDouble));
  dispatch_float3(in.x.scalar_type(), name, [&](auto tag) {
    using T = decltype(tag);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(in.groups)), dim3(kNdThreads), 0, stream(), reinterpret_cast<const T*>(in.x.data_ptr()),
                         reinterpret_cast<const T*>(t.data_ptr()), in.H, in.W, in.strips, in.cblocks, static_cast<int>(block_size),
                         part.data_ptr<double>());
    };
    in.vec ? launch(psnrb_vec_kernel<T>) : launch(psnrb_generic_kernel<T>);
  });
  TMX_LAUNCH_CHECK();
  auto out = at::empty({5}, part.options());
  hipLaunchKernelGGL(psnrb_fold_kernel, dim3(1), dim3(kNdThreads), 0, stream(), part.data_ptr<double>(), in.groups, out.data_ptr<double>());
  TMX_LAUNCH_CHECK();
  return out;
}

// (dy, dx) in the dtype and shape of img [B, C, H, W]: the difference with the lower and with the right neighbour, zeros in the
// last row of dy and the last column of dx (stored by the same kernel).
std::tuple<at::Tensor, at::Tensor> image_gradients(const at::Tensor& img) {
  const char* name = "image_gradients";
  const at::DeviceGuard guard(img.device());
  const auto in = nd_inputs(img, name);
  auto dy = at::empty(in.x.sizes(), in.x.options());
  auto dx = at::empty(in.x.sizes(), in.x.options());
  const bool vec = in.vec && (reinterpret_cast<uintptr_t>(dy.data_ptr()) & 15) == 0 && (reinterpret_cast<uintptr_t>(dx.data_ptr()) & 15) == 0;
  dispatch_float3(in.x.scalar_type(), name, [&](auto tag) {
    using T = decltype(tag);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(in.groups)), dim3(kNdThreads), 0, stream(), reinterpret_cast<const T*>(in.x.data_ptr()),
                         in.H, in.W, in.strips, in.cblocks, reinterpret_cast<T*>(dy.data_ptr()), reinterpret_cast<T*>(dx.data_ptr()));
    };
    vec ? launch(gradients_vec_kernel<T>) : launch(gradients_generic_kernel<T>);
  });
  TMX_LAUNCH_CHECK();
  return {dy, dx};
}

// (fp32 columns per workgroup (16-bit inputs: twice as many), rows per strip): what the tests need to place their edge shapes
std::vector<int64_t> gradient_tile() { return {kNdCols, kNdRows}; }

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("psnrb_sums(Tensor preds, Tensor target, int block_size) -> Tensor");
  m.def("tv_sums(Tensor img) -> Tensor");
  m.def("image_gradients(Tensor img) -> (Tensor, Tensor)");
  m.def("gradient_tile() -> int[]", &tmx::gradient_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("psnrb_sums", &tmx::psnrb_sums);
  m.impl("tv_sums", &tmx::tv_sums);
  m.impl("image_gradients", &tmx::image_gradients);
}
