// Fused box-window kernel for gfx950 behind root_mean_squared_error_using_sliding_window and
// relative_average_spectral_error: the batch sum of the per-image sliding-window RMSE map, its cropped sum per channel and,
// for RASE, the batch sum of the window mean of the target, from [B, C, H, W] inputs read in place.
//
// The reference pads both axes by SciPy's edge-including symmetric reflection (front WS / 2, back (WS − 1) / 2), runs a dense
// WS x WS box convolution over (t − p)² (and over t for RASE), takes the square root, sums over the batch and crops
// round(WS / 2) pixels (Python's banker's rounding) for the scalar.  Here, per image b, channel c and pixel (y, x), in fp32:
//   S  = sum of (t − p)² over rows y − WS/2 .. y + (WS − 1)/2 and the same columns, indices reflected (−k -> k − 1,
//        H − 1 + k -> H − k; H, W > 2 crop >= WS makes one reflection enough),
//   r  = sqrt(S · (1 / WS²)),  m = (sum of t over the window · (1 / WS²)) · (1 / WS²)   (the second scale is the reference's),
//   rmse_map[c, y, x] = Σ_b r,  target_mean[c, y, x] = Σ_b m,  crop_sums[c] = Σ_b Σ_{crop <= y < H − crop, crop <= x < W − crop} r in fp64.
// The window sum is separable and direct (no running add / subtract window: that cancels on smooth data): a WS-tap row sum
// from LDS, a WS-slot register ring down the columns, slots addressed at compile time (the row march of uqi_pair_kernel).
//
// One workgroup = kBoxCols output columns and a strip of kBoxRows output rows of one channel, for the images of one batch
// chunk.  Per input row it stages the row segment (kBoxCols + WS − 1 columns, reflected) in LDS, double buffered and fetched
// two rows ahead into registers, as d² (a dword per column) or, with the target mean, as (d², t) pairs (8 bytes per column:
// one ds_read_b64 per tap, consecutive lanes on consecutive bank pairs, conflict free per 32-lane half).  The per-pixel batch sums live in LDS, one column per
// thread (no barrier, no conflict), and are written once at the end; the first image of a chunk stores, the others add, in
// image order.  Small C·H·W with a large batch would leave too few workgroups, so the batch is split into chunks on the
// grid (box_batch_chunks: a function of the shape alone); each chunk writes its partial maps and box_fold_kernel adds them
// in chunk order.  No atomics anywhere: two runs are bit-equal.
//
// Grid: x = chunk · C + channel, y = column blocks, z = row strips.
#include "common.h"
#include "window_moments.h"

#include <algorithm>
#include <cstdlib>
#include <tuple>
#include <vector>

namespace tmx {

constexpr int kBoxCols = 128;  // output columns per workgroup = threads
constexpr int kBoxRows = 32;   // output rows per strip
constexpr int kBoxTargetGroups = 2048;  // batch chunks are added until the grid has about this many workgroups

// edge-including reflection of an index in [−n, 2 n): −k -> k − 1, n − 1 + k -> n − k
__device__ __forceinline__ int box_reflect(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

template <bool TM> struct BoxStage { using type = float; };
template <> struct BoxStage<true> { using type = f2; };

template <typename T, int WS, bool TM>
__global__ __launch_bounds__(kBoxCols) void box_rmse_kernel(const T* __restrict__ preds, const T* __restrict__ target, int C, int H, int W,
                                                            int B, int per_chunk, int crop, float* __restrict__ rmse_part,
                                                            float* __restrict__ mean_part, double* __restrict__ crop_part) {
  constexpr int kSeg = kBoxCols + WS - 1;
  constexpr int kFront = WS / 2, kBack = (WS - 1) / 2;
  constexpr float kInv = 1.f / static_cast<float>(WS * WS);
  using Staged = typename BoxStage<TM>::type;
  __shared__ Staged s_row[2][kSeg];
  __shared__ float s_rmse[kBoxRows][kBoxCols];
  __shared__ float s_mean[TM ? kBoxRows : 1][kBoxCols];

  const int tid = threadIdx.x;
  const int c = blockIdx.x % C, chunk = blockIdx.x / C;
  const int x0 = blockIdx.y * kBoxCols;
  const int y0 = blockIdx.z * kBoxRows;
  const int64_t plane_size = static_cast<int64_t>(H) * W;
  const int b0 = chunk * per_chunk, b1 = min(B, b0 + per_chunk);

  const int out_rows = min(kBoxRows, H - y0);
  const int in_rows = out_rows + WS - 1;  // padded rows y0 − kFront .. y0 + out_rows − 1 + kBack <= H − 1 + kBack
  const int x = x0 + tid;
  const bool col_ok = x < W;
  const bool col_in_crop = x >= crop && x < W - crop;

  float rd[WS], rt[TM ? WS : 1];
#pragma unroll
  for (int k = 0; k < WS; ++k) rd[k] = 0.f;
#pragma unroll
  for (int k = 0; k < (TM ? WS : 1); ++k) rt[k] = 0.f;
  double acc = 0.0;

  // Row pipeline over the flat sequence q of (image, padded row) of this chunk: the raw elements of row q + 2 are in flight into
  // registers while row q is summed from LDS and row q + 1 is converted and stored to the other buffer, one barrier per row.
  constexpr int kPer = (kSeg + kBoxCols - 1) / kBoxCols;  // staged columns per thread
  T pre_p[kPer], pre_t[kPer];
  bool pre_ok[kPer];
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int s = tid + i * kBoxCols;
    pre_ok[i] = s < kSeg && x0 - kFront + s < W + kBack;  // beyond the padded row: columns no kept output reads
  }
  int fb = b0, fr = 0;  // the next (image, row) to fetch
  auto fetch = [&] {
    const int64_t row = (static_cast<int64_t>(fb) * C + c) * plane_size + static_cast<int64_t>(box_reflect(y0 - kFront + fr, H)) * W;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      if (pre_ok[i]) {
        const int64_t o = row + box_reflect(x0 - kFront + tid + i * kBoxCols, W);
        pre_p[i] = preds[o];
        pre_t[i] = target[o];
      }
    }
    if (++fr == in_rows) {
      fr = 0;
      ++fb;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int s = tid + i * kBoxCols;
      if (s < kSeg) {
        float d2 = 0.f, tv = 0.f;
        if (pre_ok[i]) {
          tv = to_f32<T>(pre_t[i]);
          const float d = tv - to_f32<T>(pre_p[i]);
          d2 = d * d;
        }
        if constexpr (TM) {
          s_row[buf][s] = f2{d2, tv};
        } else {
          s_row[buf][s] = d2;
        }
      }
    }
  };

  const int total = (b1 - b0) * in_rows;  // >= 2: every chunk holds an image and WS >= 2
  int q = 0;
  fetch();
  store(0);
  fetch();
  __syncthreads();

  for (int b = b0; b < b1; ++b) {
    const bool first = b == b0;
    for (int base = 0; base < in_rows; base += WS) {
#pragma unroll
      for (int j = 0; j < WS; ++j) {
        const int r = base + j;
        if (r < in_rows) {  // uniform across the workgroup
          const int buf = q & 1;
          if (q + 1 < total) store(buf ^ 1);  // last read in row q − 1, before the previous barrier
          if (q + 2 < total) fetch();
          const Staged* src = &s_row[buf][tid];
          if constexpr (TM) {
            f2 h = src[0];
#pragma unroll
            for (int k = 1; k < WS; ++k) h += src[k];
            rd[j] = h.x;
            rt[j] = h.y;
          } else {
            float h = src[0];
#pragma unroll
            for (int k = 1; k < WS; ++k) h += src[k];
            rd[j] = h;
          }
          if (r >= WS - 1) {
            const int o = r - (WS - 1);  // output row y0 + o
            float sd = rd[(j + 1) % WS];  // oldest first
#pragma unroll
            for (int k = 1; k < WS; ++k) sd += rd[(j + 1 + k) % WS];
            const float v = sqrtf(sd * kInv);
            s_rmse[o][tid] = first ? v : s_rmse[o][tid] + v;
            if constexpr (TM) {
              float st = rt[(j + 1) % WS];
#pragma unroll
              for (int k = 1; k < WS; ++k) st += rt[(j + 1 + k) % WS];
              const float m = (st * kInv) * kInv;
              s_mean[o][tid] = first ? m : s_mean[o][tid] + m;
            }
            const int y = y0 + o;
            if (col_in_crop && y >= crop && y < H - crop) acc += static_cast<double>(v);
          }
          __syncthreads();  // staged row q + 1 visible; buffer of row q free for row q + 2
          ++q;
        }
      }
    }
  }

  if (col_ok) {  // each thread reads back only what it wrote
    const int64_t plane = (static_cast<int64_t>(chunk) * C + c) * plane_size;
    for (int o = 0; o < out_rows; ++o) {
      const int64_t at = plane + static_cast<int64_t>(y0 + o) * W + x;
      rmse_part[at] = s_rmse[o][tid];
      if constexpr (TM) mean_part[at] = s_mean[o][tid];
    }
  }

  double v[1] = {acc};
  double* const out[1] = {crop_part};
  block_sum_store<1, kBoxCols>(v, out, [&] {
    return ((static_cast<int64_t>(c) * (gridDim.x / C) + chunk) * gridDim.z + blockIdx.z) * gridDim.y + blockIdx.y;
  });
}

// out[i] = part[0][i] + part[1][i] + ... in chunk order
__global__ __launch_bounds__(256) void box_fold_kernel(const float* __restrict__ part, int64_t n, int chunks, float* __restrict__ out) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float s = part[i];
    for (int k = 1; k < chunks; ++k) s += part[k * n + i];
    out[i] = s;
  }
}

// RASE from the accumulated maps, in fp64: per cropped pixel 100 / mean_c(target_sum / n) · sqrt(mean_c((rmse_map / n)²)); one fp64
// partial sum per workgroup.
template <typename T>
__global__ __launch_bounds__(256) void rase_fold_kernel(const T* __restrict__ rmse_map, const T* __restrict__ target_sum,
                                                        const double* __restrict__ total_images, int C, int H, int W, int crop,
                                                        double* __restrict__ partial) {
  const int Hc = H - 2 * crop, Wc = W - 2 * crop;
  const int64_t count = static_cast<int64_t>(Hc) * Wc, plane_size = static_cast<int64_t>(H) * W;
  const double n = total_images[0];
  double acc = 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t at = (i / Wc + crop) * W + (i % Wc + crop);
    double mean = 0.0, sq = 0.0;
    for (int c = 0; c < C; ++c) {
      const double r = static_cast<double>(to_f32<T>(rmse_map[c * plane_size + at])) / n;
      mean += static_cast<double>(to_f32<T>(target_sum[c * plane_size + at])) / n;
      sq += r * r;
    }
    acc += 100.0 / (mean / C) * sqrt(sq / C);
  }
  double v[1] = {acc};
  double* const out[1] = {partial};
  block_sum_store<1, 256>(v, out, [&] { return static_cast<int64_t>(blockIdx.x); });
}

// (output rows per strip, output columns per workgroup): what the tests need to place their strip and column-block edges
std::vector<int64_t> box_tile() { return {kBoxRows, kBoxCols}; }

// How many batch chunks box_rmse_maps puts on the grid for a [B, C, H, W] call: a function of the shape alone.  Chunk k holds
// images k · ceil(B / chunks) .. of the batch; every chunk is non-empty.
int64_t box_batch_chunks(int64_t B, int64_t C, int64_t H, int64_t W) {
  TORCH_CHECK(B >= 1 && C >= 1 && H >= 1 && W >= 1, "box_batch_chunks: expected a non-empty shape");
  const int64_t groups = C * ((H + kBoxRows - 1) / kBoxRows) * ((W + kBoxCols - 1) / kBoxCols);
  // TMX_BOX_TARGET_GROUPS: the A/B knob of the chunk rule (README), read once per process
  static const int64_t target = [] {
    const char* e = std::getenv("TMX_BOX_TARGET_GROUPS");
    const int64_t v = e ? std::atoll(e) : 0;
    return v > 0 ? v : kBoxTargetGroups;
  }();
  const int64_t want = std::min<int64_t>(B, std::max<int64_t>(1, target / groups));
  const int64_t per_chunk = (B + want - 1) / want;
  return (B + per_chunk - 1) / per_chunk;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> box_rmse_maps(const at::Tensor& preds_in, const at::Tensor& target_in, int64_t window_size,
                                                             int64_t crop, bool with_target_mean) {
  const char* name = "box_rmse_maps";
  TORCH_CHECK(preds_in.is_cuda() && target_in.is_cuda(), name, ": expected GPU tensors");
  TORCH_CHECK(preds_in.device() == target_in.device(), name, ": preds and target on different devices");
  TORCH_CHECK(preds_in.dim() == 4 && preds_in.sizes() == target_in.sizes(), name, ": expected matching [B, C, H, W]");
  TORCH_CHECK(preds_in.scalar_type() == target_in.scalar_type(), name, ": dtype mismatch");
  const auto dtype = preds_in.scalar_type();
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16 || dtype == at::kHalf, name, ": unsupported dtype ", dtype);
  TORCH_CHECK(window_size >= 2 && window_size <= 16, name, ": unsupported window size ", window_size);
  const int64_t B = preds_in.size(0), C = preds_in.size(1), H = preds_in.size(2), W = preds_in.size(3);
  TORCH_CHECK(B >= 1 && C >= 1, name, ": empty input");
  // crop is the caller's round(window_size / 2); with it above window_size / 2 one reflection per side is enough
  TORCH_CHECK(crop >= window_size / 2 && H > 2 * crop && W > 2 * crop, name, ": the plane must be larger than twice the crop");
  TORCH_CHECK(H * W <= INT32_MAX, name, ": plane too large");
  const at::DeviceGuard guard(preds_in.device());
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();

  const int64_t chunks = box_batch_chunks(B, C, H, W);
  const int64_t per_chunk = (B + chunks - 1) / chunks;
  const int64_t col_blocks = (W + kBoxCols - 1) / kBoxCols, strips = (H + kBoxRows - 1) / kBoxRows;
  TORCH_CHECK(C * chunks <= INT32_MAX && col_blocks <= 65535 && strips <= 65535, name, ": too many workgroups for one launch");
  const auto f32 = p.options().dtype(at::kFloat);
  // with one chunk the kernel writes the results themselves
  auto rmse_part = at::empty({chunks, C, H, W}, f32);
  auto mean_part = with_target_mean ? at::empty({chunks, C, H, W}, f32) : at::empty({0}, f32);
  auto crop_part = at::empty({C, chunks * strips * col_blocks}, p.options().dtype(at::kDouble));
  const dim3 grid(static_cast<unsigned>(C * chunks), static_cast<unsigned>(col_blocks), static_cast<unsigned>(strips));
  dispatch_float3(dtype, name, [&](auto tag) {
    using T = decltype(tag);
    dispatch_box_window(window_size, name, [&](auto ws) {
      auto launch = [&](auto tm) {
        hipLaunchKernelGGL((box_rmse_kernel<T, decltype(ws)::value, decltype(tm)::value>), grid, dim3(kBoxCols), 0, stream(),
                           reinterpret_cast<const T*>(p.data_ptr()), reinterpret_cast<const T*>(t.data_ptr()), static_cast<int>(C),
                           static_cast<int>(H), static_cast<int>(W), static_cast<int>(B), static_cast<int>(per_chunk),
                           static_cast<int>(crop), rmse_part.data_ptr<float>(), mean_part.data_ptr<float>(), crop_part.data_ptr<double>());
      };
      if (with_target_mean) {
        launch(std::true_type{});
      } else {
        launch(std::false_type{});
      }
    });
  });
  TMX_LAUNCH_CHECK();

  auto fold = [&](const at::Tensor& part) {
    if (chunks == 1) return part.view({C, H, W});
    auto out = at::empty({C, H, W}, f32);
    const int64_t n = C * H * W;
    hipLaunchKernelGGL(box_fold_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream(), part.data_ptr<float>(), n, static_cast<int>(chunks),
                       out.data_ptr<float>());
    TMX_LAUNCH_CHECK();
    return out;
  };
  auto rmse_map = fold(rmse_part);
  auto target_mean = with_target_mean ? fold(mean_part) : mean_part;
  auto crop_sums = crop_part.size(1) == 1 ? crop_part.view({C}) : crop_part.sum(1);
  return {rmse_map, crop_sums, target_mean};
}

at::Tensor rase_fold(const at::Tensor& rmse_map_in, const at::Tensor& target_sum_in, const at::Tensor& total_images, int64_t crop) {
  const char* name = "rase_fold";
  TORCH_CHECK(rmse_map_in.is_cuda() && target_sum_in.is_cuda() && total_images.is_cuda(), name, ": expected GPU tensors");
  TORCH_CHECK(rmse_map_in.device() == target_sum_in.device() && rmse_map_in.device() == total_images.device(), name,
              ": tensors on different devices");
  TORCH_CHECK(rmse_map_in.dim() == 3 && rmse_map_in.sizes() == target_sum_in.sizes(), name, ": expected matching [C, H, W] maps");
  TORCH_CHECK(rmse_map_in.scalar_type() == target_sum_in.scalar_type(), name, ": dtype mismatch");
  TORCH_CHECK(total_images.numel() == 1, name, ": total_images must hold one value");
  const int64_t C = rmse_map_in.size(0), H = rmse_map_in.size(1), W = rmse_map_in.size(2);
  TORCH_CHECK(C >= 1 && C <= INT32_MAX, name, ": unsupported channel count");
  TORCH_CHECK(crop >= 1 && H > 2 * crop && W > 2 * crop, name, ": the plane must be larger than twice the crop");
  TORCH_CHECK(H * W <= INT32_MAX, name, ": plane too large");
  const at::DeviceGuard guard(rmse_map_in.device());
  auto rmse_map = rmse_map_in.contiguous();
  auto target_sum = target_sum_in.contiguous();
  auto n = total_images.reshape({1}).to(at::kDouble);  // a device cast: no host read
  const int64_t count = (H - 2 * crop) * (W - 2 * crop);
  const int blocks = grid_for(count, 256, 1024);
  auto partial = at::empty({blocks}, rmse_map.options().dtype(at::kDouble));
  dispatch_float3(rmse_map.scalar_type(), name, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(rase_fold_kernel<T>, dim3(blocks), dim3(256), 0, stream(), reinterpret_cast<const T*>(rmse_map.data_ptr()),
                       reinterpret_cast<const T*>(target_sum.data_ptr()), n.data_ptr<double>(), static_cast<int>(C), static_cast<int>(H),
                       static_cast<int>(W), static_cast<int>(crop), partial.data_ptr<double>());
  });
  TMX_LAUNCH_CHECK();
  return partial.sum() / static_cast<double>(count);
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("box_rmse_maps(Tensor preds, Tensor target, int window_size, int crop, bool with_target_mean) -> (Tensor, Tensor, Tensor)");
  m.def("rase_fold(Tensor rmse_map, Tensor target_sum, Tensor total_images, int crop) -> Tensor");
  m.def("box_tile() -> int[]", &tmx::box_tile);
  m.def("box_batch_chunks(int B, int C, int H, int W) -> int", &tmx::box_batch_chunks);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("box_rmse_maps", &tmx::box_rmse_maps);
  m.impl("rase_fold", &tmx::rase_fold);
}
