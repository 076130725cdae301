// Streaming kernels for gfx950 behind spectral_angle_mapper and error_relative_global_dimensionless_synthesis: one read of
// preds / target [B, C, H, W] (fp32 / bf16 / fp16, read in place), no LDS staging, no full-size temporary.
//
// SAM.  A thread owns V consecutive pixels of one image (V = 16 bytes of the element type: 4 fp32, 8 bf16 / fp16) and walks
// the C band planes at stride H·W, kSamBands bands' loads in flight, keeping <p,t>, <p,p> and <t,t> of every pixel in
// registers: fp64 fused multiply-adds of the exact fp32 products, in band order (a sequential fp32 sum over 200 bands is
// past the value rule of tests/test_spectral_gpu.py; the kernel is memory bound and the fp64 work is a few per cent of the
// vector rate).  Per pixel (sam_angle):
//   cos = <p,t> / sqrt(<p,p> · <t,t>) in fp64,  clamped to [−1, 1] by comparisons (NaN passes),  angle = acosf((float)cos).
// Bit-identical non-zero p and t give the same fp64 value x three times; x / sqrt(x · x) is within two fp64 ulp of 1 and
// rounds to 1.0f, the angle is exactly 0 (the fp32 norm product of the composition gives up to 7e-4 there).  A zero vector
// gives 0 / 0 = NaN.  sam_map stores the angle; sam_sums adds the same fp32 value, widened, to a per-thread fp64 sum in pixel order and
// writes one fp64 partial per workgroup (block_sum_store); with more than one workgroup per image spectral_fold_kernel adds
// an image's partials in a fixed order.  No atomics: two runs are bit-equal.
//
// ERGAS.  ergas_plane_kernel runs on a flat (plane, chunk) grid: a workgroup reads one chunk of one [H·W] plane of preds and
// target, 16 bytes per lane and kErgasUnroll vectors in flight, sums (p − t)² and t over the V elements of a vector in fp32
// and adds the two vector sums to per-thread fp64 sums (no long fp32 running sum), and writes two fp64 partials.
// ergas_fold_kernel adds each plane's partials in chunk order and forms 100 · ratio · sqrt(mean_c((SSE / HW) / mean_t²)) per
// image in fp64.  A plane is split into chunks until the grid has about kSpecTargetGroups workgroups (ergas_chunks: a
// function of the shape alone).
//
// Every kernel has a generic instantiation (scalar loads, any H·W, any alignment) and a vector one (16-byte loads: base
// pointers 16-byte aligned and H·W a multiple of V).  Both assign the same elements to the same thread and run the same
// arithmetic in the same order: their results are bit-equal.
//
// Grids are flat on x (image or plane index decoded in the kernel), so B and B·C are not limited to 65 535.
#include "common.h"
#include "stream_load.h"
#include "window_moments.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace tmx {

constexpr int kSpecThreads = 256;
constexpr int kSamBands = 4;             // bands whose loads are in flight together
constexpr int kSamPixels = kSpecThreads * 4;  // fp32 pixels per workgroup (16-bit: twice as many)
constexpr int kErgasUnroll = 4;          // vectors per thread in flight (per input)
constexpr int64_t kErgasChunkMin = 4096;  // no chunk is made smaller than this many elements
constexpr int64_t kErgasAlign = kSpecThreads * 8;  // chunk lengths are multiples of this: chunk starts keep the 16-byte alignment
constexpr int64_t kSpecTargetGroups = 2048;  // planes are split into chunks until the grid has about this many workgroups

// -------------------------------------------------------------------------------------------------------------- SAM
// The one place the angle is formed: sam_map stores this value and sam_sums adds it.
__device__ __forceinline__ float sam_angle(double dot, double pp, double tt) {
  double c = dot / sqrt(pp * tt);
  c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);  // comparisons, not fmin / fmax: NaN stays NaN
  return acosf(static_cast<float>(c));
}

// Workgroup w of the flat grid: image w / groups_per_image, pixels (w % groups_per_image) · kSpecThreads · V ..
template <typename T, bool VEC, bool MAP>
__device__ __forceinline__ void sam_body(const T* __restrict__ preds, const T* __restrict__ target, int C, int64_t HW, int64_t groups_per_image,
                                         float* __restrict__ map, double* __restrict__ partial) {
  constexpr int V = SpecVec<T>::n;
  const int64_t wg = blockIdx.x;
  const int64_t b = wg / groups_per_image;
  const int64_t pix0 = ((wg % groups_per_image) * kSpecThreads + threadIdx.x) * V;
  const int valid = pix0 < HW ? static_cast<int>(min(static_cast<int64_t>(V), HW - pix0)) : 0;  // VEC: 0 or V

  double dot[V], pp[V], tt[V];
#pragma unroll
  for (int j = 0; j < V; ++j) dot[j] = pp[j] = tt[j] = 0.0;

  if (valid > 0) {
    const T* p = preds + b * C * HW + pix0;
    const T* t = target + b * C * HW + pix0;
    auto add = [&](const SpecLoad<T, VEC>& lp, const SpecLoad<T, VEC>& lt) {
      float pv[V], tv[V];
      lp.get(pv, valid);
      lt.get(tv, valid);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double pj = pv[j], tj = tv[j];
        dot[j] = fma(pj, tj, dot[j]);
        pp[j] = fma(pj, pj, pp[j]);
        tt[j] = fma(tj, tj, tt[j]);
      }
    };
    int c = 0;
    for (; c + kSamBands <= C; c += kSamBands) {
      SpecLoad<T, VEC> lp[kSamBands], lt[kSamBands];
#pragma unroll
      for (int u = 0; u < kSamBands; ++u) {
        lp[u].load(p + (c + u) * HW, valid);
        lt[u].load(t + (c + u) * HW, valid);
      }
#pragma unroll
      for (int u = 0; u < kSamBands; ++u) add(lp[u], lt[u]);
    }
    for (; c < C; ++c) {
      SpecLoad<T, VEC> lp, lt;
      lp.load(p + c * HW, valid);
      lt.load(t + c * HW, valid);
      add(lp, lt);
    }
  }

  if constexpr (MAP) {
    if (valid > 0) {
      float* o = map + b * HW + pix0;
      if constexpr (VEC) {  // b · HW + pix0 is a multiple of V and the map is a fresh allocation: 16-byte aligned
#pragma unroll
        for (int j = 0; j < V; j += 4) {
          *reinterpret_cast<float4*>(o + j) = make_float4(sam_angle(dot[j], pp[j], tt[j]), sam_angle(dot[j + 1], pp[j + 1], tt[j + 1]),
                                                          sam_angle(dot[j + 2], pp[j + 2], tt[j + 2]), sam_angle(dot[j + 3], pp[j + 3], tt[j + 3]));
        }
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if (j < valid) o[j] = sam_angle(dot[j], pp[j], tt[j]);
        }
      }
    }
  } else {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (j < valid) acc += static_cast<double>(sam_angle(dot[j], pp[j], tt[j]));
    }
    double v[1] = {acc};
    double* const out[1] = {partial};
    block_sum_store<1, kSpecThreads>(v, out, [&] { return wg; });
  }
}

template <typename T, bool MAP>
__global__ __launch_bounds__(kSpecThreads) void sam_generic_kernel(const T* __restrict__ preds, const T* __restrict__ target, int C, int64_t HW,
                                                                   int64_t groups_per_image, float* __restrict__ map,
                                                                   double* __restrict__ partial) {
  sam_body<T, false, MAP>(preds, target, C, HW, groups_per_image, map, partial);
}

template <typename T, bool MAP>
__global__ __launch_bounds__(kSpecThreads) void sam_vec_kernel(const T* __restrict__ preds, const T* __restrict__ target, int C, int64_t HW,
                                                               int64_t groups_per_image, float* __restrict__ map, double* __restrict__ partial) {
  sam_body<T, true, MAP>(preds, target, C, HW, groups_per_image, map, partial);
}

// out[r] = the sum of part[r][0 .. n): one wave per row; lane l adds entries l, l + 64, ... in order, then the lanes are added
// by the fixed tree of block_sum_store.
__global__ __launch_bounds__(kWave) void spectral_fold_kernel(const double* __restrict__ part, int64_t n, double* __restrict__ out) {
  const double* row = part + static_cast<int64_t>(blockIdx.x) * n;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kWave) acc += row[i];
  double v[1] = {acc};
  double* const o[1] = {out};
  block_sum_store<1, kWave>(v, o, [&] { return static_cast<int64_t>(blockIdx.x); });
}

// ------------------------------------------------------------------------------------------------------------ ERGAS
// Workgroup w of the flat grid: plane w / chunks, elements (w % chunks) · per_chunk .. of it.  A thread takes the vectors
// tid, tid + 256, ... of the chunk.
template <typename T, bool VEC>
__device__ __forceinline__ void ergas_body(const T* __restrict__ preds, const T* __restrict__ target, int64_t HW, int64_t per_chunk, int64_t chunks,
                                           double* __restrict__ part_sse, double* __restrict__ part_t) {
  constexpr int V = SpecVec<T>::n;
  constexpr int64_t kTile = static_cast<int64_t>(kSpecThreads) * V * kErgasUnroll;
  const int64_t wg = blockIdx.x;
  const int64_t plane = wg / chunks;
  const int64_t e0 = (wg % chunks) * per_chunk, e1 = min(HW, e0 + per_chunk);
  const T* p = preds + plane * HW;
  const T* t = target + plane * HW;

  double sse = 0.0, st = 0.0;
  for (int64_t base = e0; base < e1; base += kTile) {
    SpecLoad<T, VEC> lp[kErgasUnroll], lt[kErgasUnroll];
    int valid[kErgasUnroll];
#pragma unroll
    for (int u = 0; u < kErgasUnroll; ++u) {
      const int64_t at = base + (static_cast<int64_t>(u) * kSpecThreads + threadIdx.x) * V;
      valid[u] = at < e1 ? static_cast<int>(min(static_cast<int64_t>(V), e1 - at)) : 0;  // VEC: 0 or V
      if (valid[u] > 0) {
        lp[u].load(p + at, valid[u]);
        lt[u].load(t + at, valid[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kErgasUnroll; ++u) {
      if (valid[u] > 0) {
        float pv[V], tv[V];
        lp[u].get(pv, valid[u]);
        lt[u].get(tv, valid[u]);
        float s2 = 0.f, s1 = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float d = pv[j] - tv[j];
          s2 = fmaf(d, d, s2);
          s1 += tv[j];
        }
        sse += static_cast<double>(s2);
        st += static_cast<double>(s1);
      }
    }
  }
  double v[2] = {sse, st};
  double* const out[2] = {part_sse, part_t};
  block_sum_store<2, kSpecThreads>(v, out, [&] { return wg; });
}

template <typename T>
__global__ __launch_bounds__(kSpecThreads) void ergas_plane_generic_kernel(const T* __restrict__ preds, const T* __restrict__ target, int64_t HW,
                                                                           int64_t per_chunk, int64_t chunks, double* __restrict__ part_sse,
                                                                           double* __restrict__ part_t) {
  ergas_body<T, false>(preds, target, HW, per_chunk, chunks, part_sse, part_t);
}

template <typename T>
__global__ __launch_bounds__(kSpecThreads) void ergas_plane_vec_kernel(const T* __restrict__ preds, const T* __restrict__ target, int64_t HW,
                                                                       int64_t per_chunk, int64_t chunks, double* __restrict__ part_sse,
                                                                       double* __restrict__ part_t) {
  ergas_body<T, true>(preds, target, HW, per_chunk, chunks, part_sse, part_t);
}

// One wave per image: lane l takes the bands l, l + 64, ...; per band the chunk partials are added in chunk order, the bands'
// terms of a lane in band order, the lanes by the fixed tree of wave_sum.  All in fp64.
__global__ __launch_bounds__(kWave) void ergas_fold_kernel(const double* __restrict__ part_sse, const double* __restrict__ part_t, int C,
                                                          int64_t chunks, double HW, double ratio, double* __restrict__ scores) {
  const int64_t b = blockIdx.x;
  double acc = 0.0;
  for (int c = threadIdx.x; c < C; c += kWave) {
    const int64_t at = (b * C + c) * chunks;
    double sse = part_sse[at], st = part_t[at];
    for (int64_t k = 1; k < chunks; ++k) {
      sse += part_sse[at + k];
      st += part_t[at + k];
    }
    const double mean_t = st / HW;
    acc += (sse / HW) / (mean_t * mean_t);  // a zero mean gives x / 0 = inf or 0 / 0 = NaN, as the composition does
  }
  acc = wave_sum(acc);
  if (threadIdx.x == 0) scores[b] = 100.0 * ratio * sqrt(acc / static_cast<double>(C));
}

// ------------------------------------------------------------------------------------------------------------- host
namespace {

struct SpectralInputs {
  at::Tensor p, t;
  int64_t B, C, HW;
  bool vec;
};

// TMX_SPECTRAL_GENERIC: the A/B knob of the 16-byte-load kernels (tools/spectral_bench.py), read once per process
bool spectral_vec_off() {
  static const bool off = std::getenv("TMX_SPECTRAL_GENERIC") != nullptr;
  return off;
}

SpectralInputs spectral_inputs(const at::Tensor& preds_in, const at::Tensor& target_in, int64_t min_bands, const char* name) {
  TORCH_CHECK(preds_in.is_cuda() && target_in.is_cuda(), name, ": expected GPU tensors");
  TORCH_CHECK(preds_in.device() == target_in.device(), name, ": preds and target on different devices");
  TORCH_CHECK(preds_in.dim() == 4 && preds_in.sizes() == target_in.sizes(), name, ": expected matching [B, C, H, W]");
  TORCH_CHECK(preds_in.scalar_type() == target_in.scalar_type(), name, ": dtype mismatch");
  const auto dtype = preds_in.scalar_type();
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16 || dtype == at::kHalf, name, ": unsupported dtype ", dtype);
  const int64_t B = preds_in.size(0), C = preds_in.size(1), HW = preds_in.size(2) * preds_in.size(3);
  TORCH_CHECK(B >= 1 && HW >= 1, name, ": empty input");
  TORCH_CHECK(C >= min_bands && C <= INT32_MAX, name, ": expected at least ", min_bands, " bands");
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  const int64_t V = 16 / static_cast<int64_t>(p.element_size());
  const bool vec = !spectral_vec_off() && HW % V == 0 && (reinterpret_cast<uintptr_t>(p.data_ptr()) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
  return {p, t, B, C, HW, vec};
}

at::Tensor sam_run(const at::Tensor& preds_in, const at::Tensor& target_in, bool want_map, const char* name) {
  const at::DeviceGuard guard(preds_in.device());
  const auto in = spectral_inputs(preds_in, target_in, 2, name);
  const int64_t V = 16 / static_cast<int64_t>(in.p.element_size());
  const int64_t per_group = kSpecThreads * V;
  const int64_t groups_per_image = (in.HW + per_group - 1) / per_group;
  TORCH_CHECK(in.B * groups_per_image <= INT32_MAX, name, ": too many workgroups for one launch");
  const dim3 grid(static_cast<unsigned>(in.B * groups_per_image));
  at::Tensor map, partial;
  if (want_map) {
    map = at::empty({in.B, preds_in.size(2), preds_in.size(3)}, in.p.options().dtype(at::kFloat));
  } else {
    partial = at::empty({in.B, groups_per_image}, in.p.options().dtype(at::kDouble));
  }
  float* map_ptr = want_map ? map.data_ptr<float>() : nullptr;
  double* part_ptr = want_map ? nullptr : partial.data_ptr<double>();
  dispatch_float3(in.p.scalar_type(), name, [&](auto tag) {
    using T = decltype(tag);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kSpecThreads), 0, stream(), reinterpret_cast<const T*>(in.p.data_ptr()),
                         reinterpret_cast<const T*>(in.t.data_ptr()), static_cast<int>(in.C), in.HW, groups_per_image, map_ptr, part_ptr);
    };
    if (in.vec) {
      want_map ? launch(sam_vec_kernel<T, true>) : launch(sam_vec_kernel<T, false>);
    } else {
      want_map ? launch(sam_generic_kernel<T, true>) : launch(sam_generic_kernel<T, false>);
    }
  });
  TMX_LAUNCH_CHECK();
  if (want_map) return map;
  if (groups_per_image == 1) return partial.view({in.B});
  auto sums = at::empty({in.B}, partial.options());
  hipLaunchKernelGGL(spectral_fold_kernel, dim3(static_cast<unsigned>(in.B)), dim3(kWave), 0, stream(), partial.data_ptr<double>(),
                     groups_per_image, sums.data_ptr<double>());
  TMX_LAUNCH_CHECK();
  return sums;
}

// elements per chunk of an ERGAS plane: a multiple of kErgasAlign
int64_t ergas_per_chunk(int64_t planes, int64_t HW) {
  const int64_t want = std::max<int64_t>(1, (kSpecTargetGroups + planes - 1) / planes);
  const int64_t most = std::max<int64_t>(1, HW / kErgasChunkMin);
  const int64_t n = std::min(want, most);
  const int64_t per = (HW + n - 1) / n;
  return (per + kErgasAlign - 1) / kErgasAlign * kErgasAlign;
}

}  // namespace

// fp32 [B, H, W]: per pixel the angle between the band vectors of preds and target [B, C, H, W], C >= 2.
at::Tensor sam_map(const at::Tensor& preds, const at::Tensor& target) { return sam_run(preds, target, true, "sam_map"); }

// fp64 [B]: per image the sum of the same per-pixel angles; no map is written.
at::Tensor sam_sums(const at::Tensor& preds, const at::Tensor& target) { return sam_run(preds, target, false, "sam_sums"); }

// How many chunks ergas_scores splits every plane of a [B, C, H, W] call into: a function of the shape alone.  Chunk k holds
// the elements k · per_chunk .. of the plane with per_chunk = ceil(ceil(HW / n) / 2048) · 2048; every chunk is non-empty and
// only the last one may be short.
int64_t ergas_chunks(int64_t B, int64_t C, int64_t H, int64_t W) {
  TORCH_CHECK(B >= 1 && C >= 1 && H >= 1 && W >= 1, "ergas_chunks: expected a non-empty shape");
  const int64_t per = ergas_per_chunk(B * C, H * W);
  return (H * W + per - 1) / per;
}

// (fp32 pixels per workgroup of the SAM kernels (16-bit inputs: twice as many), least elements per ERGAS chunk): what the
// tests need to place their edge shapes
std::vector<int64_t> spectral_tile() { return {kSamPixels, kErgasChunkMin}; }

// fp64 [B]: 100 · ratio · sqrt(mean_c((SSE_bc / HW) / mean_t_bc²)) of preds / target [B, C, H, W].
at::Tensor ergas_scores(const at::Tensor& preds_in, const at::Tensor& target_in, double ratio) {
  const char* name = "ergas_scores";
  const at::DeviceGuard guard(preds_in.device());
  const auto in = spectral_inputs(preds_in, target_in, 1, name);
  const int64_t planes = in.B * in.C;
  const int64_t per_chunk = ergas_per_chunk(planes, in.HW);
  const int64_t chunks = (in.HW + per_chunk - 1) / per_chunk;
  TORCH_CHECK(planes * chunks <= INT32_MAX, name, ": too many workgroups for one launch");
  auto part = at::empty({2, planes * chunks}, in.p.options().dtype(at::kDouble));
  double* part_sse = part.data_ptr<double>();
  double* part_t = part_sse + planes * chunks;
  const dim3 grid(static_cast<unsigned>(planes * chunks));
  dispatch_float3(in.p.scalar_type(), name, [&](auto tag) {
    using T = decltype(tag);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kSpecThreads), 0, stream(), reinterpret_cast<const T*>(in.p.data_ptr()),
                         reinterpret_cast<const T*>(in.t.data_ptr()), in.HW, per_chunk, chunks, part_sse, part_t);
    };
    in.vec ? launch(ergas_plane_vec_kernel<T>) : launch(ergas_plane_generic_kernel<T>);
  });
  TMX_LAUNCH_CHECK();
  auto scores = at::empty({in.B}, part.options());
  hipLaunchKernelGGL(ergas_fold_kernel, dim3(static_cast<unsigned>(in.B)), dim3(kWave), 0, stream(), part_sse, part_t, static_cast<int>(in.C),
                     chunks, static_cast<double>(in.HW), ratio, scores.data_ptr<double>());
  TMX_LAUNCH_CHECK();
  return scores;
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("sam_map(Tensor preds, Tensor target) -> Tensor");
  m.def("sam_sums(Tensor preds, Tensor target) -> Tensor");
  m.def("ergas_scores(Tensor preds, Tensor target, float ratio) -> Tensor");
  m.def("ergas_chunks(int B, int C, int H, int W) -> int", &tmx::ergas_chunks);
  m.def("spectral_tile() -> int[]", &tmx::spectral_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("sam_map", &tmx::sam_map);
  m.impl("sam_sums", &tmx::sam_sums);
  m.impl("ergas_scores", &tmx::ergas_scores);
}
