// Streaming kernels for gfx950 behind signal_noise_ratio, scale_invariant_signal_distortion_ratio (and the SI-SNR calls built
// on it), source_aggregated_signal_distortion_ratio and the pair matrix of permutation_invariant_training: preds / target
// [G, S, T] (fp32 / bf16 / fp16, read in place), no full-size temporary, no expanded [G·S², T] copy.
//
// The ratio of a pair (p, t) keeps the residual form of the composition, in fp64:
//   p~ = p − mean(p), t~ = t − mean(t) (zero_mean),  α = (Σ p~ t~ + eps) / (Σ t~² + eps) (scale invariant; else α = 1),
//   ratio = 10 log10((α² Σ t~² + eps) / (Σ (α t~ − p~)² + eps)).
// The one-pass raw-moment form Σp² − (Σpt)² / Σt² cancels: it is 2.7e-4 dB off at p = 0.5 t and negative at p = nextafter(t).
// Because α is the least-squares scale, the residual sum is insensitive to α's rounding.
//
// Passes (each followed by signal_fold_kernel, which adds the chunk partials in a fixed order and leaves the next pass's
// scalars on the device: the host reads nothing between passes, and there are no atomics, so two runs are bit-equal):
//   M (zero_mean)        Σp and Σt of every signal in fp64 -> fp64 means; later passes centre in fp64 on load;
//   A (scale_invariant)  per pair Σ p~ t~ and per target Σ t~²: fp64 fused multiply-adds of the up-cast samples, the same
//                        instruction for both, so p == t gives α = 1 exactly; pairing 2 sums over S before dividing;
//   B                    per pair Σ (α t~ − p~)²;  for SNR (α = 1) Σ t~² is accumulated here and pass A does not run.
// SNR without zero_mean is one read of the inputs, SI-SDR two, zero_mean adds one.
//
// Grid: flat on x over (group, pair tile, chunk), decoded in the kernel, so neither G nor G·tiles is limited to 65 535.
// E is the compile-time tile extent.  E = 1: the pair (p_s, t_s) of one signal index (pairings 0 and 2, and S == 1: diagonal
// pairs share no loads, so a wider tile buys nothing).  E = 2 / 4 (pairing 1): E preds x E targets of a group; a workgroup loads
// its <= 2 E signals' chunk once and updates <= E² + E fp64 sums per thread; S > 4 is covered by more tiles, signals past S
// read as 0 and their sums are never looked at.  A thread takes the vectors tid, tid + 256, ... of its chunk in order whatever
// E and the unroll are, so the diagonal of pairing 1 has the bits of pairing 0 under equal chunking.
// Every workgroup writes its sums to part[n][workgroup] (block_sum_store): always in bounds, no remainder case.
//
// Every kernel has a generic instantiation (scalar loads, any T, any alignment) and a vector one (16-byte loads: signal bases
// 16-byte aligned and T a multiple of V).  Both assign the same samples to the same thread in the same order: bit-equal.
#include "common.h"
#include "window_moments.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace tmx {

constexpr int kSigThreads = 256;
constexpr int kSigTile = 4;                          // largest pair tile: 4 preds x 4 targets
constexpr int64_t kSigAlign = kSigThreads * 8;       // chunk lengths are multiples of this: chunk starts keep the 16-byte alignment
constexpr int64_t kSigChunkMin = 2 * kSigAlign;      // the host's own chunking splits a signal into at most T / this many chunks
constexpr int64_t kSigTargetGroups = 2048;           // signals are split into chunks until the grid has about this many workgroups

enum SigPass { kSigMean = 0, kSigA = 1, kSigB = 2, kSigSnr = 3 };

template <typename T> struct SigVec { static constexpr int n = 16 / sizeof(T); };

template <typename T> __device__ __forceinline__ void sig_unpack(const uint4& r, float (&o)[SigVec<T>::n]);
template <> __device__ __forceinline__ void sig_unpack<float>(const uint4& r, float (&o)[4]) {
  o[0] = __uint_as_float(r.x), o[1] = __uint_as_float(r.y), o[2] = __uint_as_float(r.z), o[3] = __uint_as_float(r.w);
}
template <> __device__ __forceinline__ void sig_unpack<__hip_bfloat16>(const uint4& r, float (&o)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // bf16 -> fp32 is a 16-bit shift
    o[2 * i] = __uint_as_float(w[i] << 16);
    o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
template <> __device__ __forceinline__ void sig_unpack<__half>(const uint4& r, float (&o)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = __half2float(__ushort_as_half(static_cast<unsigned short>(w[i] & 0xffffu)));
    o[2 * i + 1] = __half2float(__ushort_as_half(static_cast<unsigned short>(w[i] >> 16)));
  }
}

// V consecutive samples in flight.  VEC: one 16-byte load (src 16-byte aligned, all V in range).  Generic: scalar loads of the
// first ``valid`` samples; the others read as 0 and the callers skip them.  zero(): a signal past S.
template <typename T, bool VEC> struct SigLoad;
template <typename T> struct SigLoad<T, true> {
  uint4 r;
  __device__ __forceinline__ void zero() { r = make_uint4(0u, 0u, 0u, 0u); }
  __device__ __forceinline__ void load(const T* __restrict__ src, int) { r = *reinterpret_cast<const uint4*>(src); }
  __device__ __forceinline__ void get(float (&o)[SigVec<T>::n], int) const { sig_unpack<T>(r, o); }
};
template <typename T> struct SigLoad<T, false> {
  float e[SigVec<T>::n];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int j = 0; j < SigVec<T>::n; ++j) e[j] = 0.f;
  }
  __device__ __forceinline__ void load(const T* __restrict__ src, int valid) {
#pragma unroll
    for (int j = 0; j < SigVec<T>::n; ++j) e[j] = j < valid ? to_f32<T>(src[j]) : 0.f;
  }
  __device__ __forceinline__ void get(float (&o)[SigVec<T>::n], int) const {
#pragma unroll
    for (int j = 0; j < SigVec<T>::n; ++j) o[j] = e[j];
  }
};

template <int E, int PASS> struct SigSums {  // fp64 sums a workgroup writes
  static constexpr int n = PASS == kSigMean ? 2 : (PASS == kSigB ? E * E : E * E + E);
};

template <int N> struct SigRows { double* at[N]; };  // row n of the partials: where sum n of every workgroup goes

// What the pair passes read.  mean: [2][nsig] (preds' means, then target's) or null; alpha: per output or null.
struct SigArgs {
  int64_t S, T, tiles, per_chunk, chunks, nsig, nwg;
  int pairing;
  const double* mean;
  const double* alpha;
  double* part;
};

template <typename T, bool VEC, int E, int PASS>
__device__ __forceinline__ void signal_body(const T* __restrict__ preds, const T* __restrict__ target, const SigArgs& a) {
  constexpr int V = SigVec<T>::n;
  constexpr int U = E == 1 ? 4 : (E == 2 ? 2 : 1);  // vectors per signal in flight: 8 loads per thread for every E
  constexpr int N = SigSums<E, PASS>::n;
  constexpr int64_t kStep = static_cast<int64_t>(kSigThreads) * V * U;
  const int64_t wg = blockIdx.x;
  const int64_t chunk = wg % a.chunks, tile = wg / a.chunks;
  int64_t g, p0, t0;
  if constexpr (E == 1) {
    g = tile / a.S, p0 = t0 = tile % a.S;
  } else {
    const int64_t per_group = a.tiles * a.tiles, r = tile % per_group;
    g = tile / per_group, t0 = (r / a.tiles) * E, p0 = (r % a.tiles) * E;
  }
  const int np = static_cast<int>(min(static_cast<int64_t>(E), a.S - p0));
  const int nt = static_cast<int>(min(static_cast<int64_t>(E), a.S - t0));
  const T* p = preds + (g * a.S + p0) * a.T;
  const T* t = target + (g * a.S + t0) * a.T;

  double mp[E], mt[E], al[E * E];
#pragma unroll
  for (int i = 0; i < E; ++i) {
    mp[i] = (PASS != kSigMean && a.mean != nullptr && i < np) ? a.mean[g * a.S + p0 + i] : 0.0;
    mt[i] = (PASS != kSigMean && a.mean != nullptr && i < nt) ? a.mean[a.nsig + g * a.S + t0 + i] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < E; ++i) {
#pragma unroll
    for (int j = 0; j < E; ++j) {
      if (PASS == kSigB && i < np && j < nt) {
        al[i * E + j] = a.alpha[E == 1 ? (a.pairing == 2 ? g : tile) : (g * a.S + t0 + j) * a.S + p0 + i];
      } else {
        al[i * E + j] = 1.0;
      }
    }
  }

  double acc[N];
#pragma unroll
  for (int n = 0; n < N; ++n) acc[n] = 0.0;

  const int64_t e0 = chunk * a.per_chunk, e1 = min(a.T, e0 + a.per_chunk);
  for (int64_t base = e0; base < e1; base += kStep) {
    SigLoad<T, VEC> lp[U][E], lt[U][E];
    int valid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t at = base + (static_cast<int64_t>(u) * kSigThreads + threadIdx.x) * V;
      valid[u] = at < e1 ? static_cast<int>(min(static_cast<int64_t>(V), e1 - at)) : 0;  // VEC: 0 or V
      if (valid[u] > 0) {
#pragma unroll
        for (int i = 0; i < E; ++i) {
          if (i < np) lp[u][i].load(p + i * a.T + at, valid[u]); else lp[u][i].zero();
          if (i < nt) lt[u][i].load(t + i * a.T + at, valid[u]); else lt[u][i].zero();
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (valid[u] > 0) {
        float pv[E][V], tv[E][V];
#pragma unroll
        for (int i = 0; i < E; ++i) {
          lp[u][i].get(pv[i], valid[u]);
          lt[u][i].get(tv[i], valid[u]);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if (VEC || j < valid[u]) {
            double pd[E], td[E];
#pragma unroll
            for (int i = 0; i < E; ++i) {
              pd[i] = static_cast<double>(pv[i][j]) - mp[i];
              td[i] = static_cast<double>(tv[i][j]) - mt[i];
            }
            if constexpr (PASS == kSigMean) {
              acc[0] += pd[0];
              acc[1] += td[0];
            } else {
#pragma unroll
              for (int i = 0; i < E; ++i) {
#pragma unroll
                for (int k = 0; k < E; ++k) {
                  if constexpr (PASS == kSigA) {
                    acc[i * E + k] = fma(pd[i], td[k], acc[i * E + k]);
                  } else {
                    const double r = PASS == kSigB ? fma(al[i * E + k], td[k], -pd[i]) : td[k] - pd[i];
                    acc[i * E + k] = fma(r, r, acc[i * E + k]);
                  }
                }
              }
              if constexpr (PASS != kSigB) {
#pragma unroll
                for (int k = 0; k < E; ++k) acc[E * E + k] = fma(td[k], td[k], acc[E * E + k]);
              }
            }
          }
        }
      }
    }
  }

  SigRows<N> rows;
#pragma unroll
  for (int n = 0; n < N; ++n) rows.at[n] = a.part + n * a.nwg;
  const SigRows<N> out = rows;
  block_sum_store<N, kSigThreads>(acc, out.at, [&] { return wg; });
}

template <typename T, int E, int PASS>
__global__ __launch_bounds__(kSigThreads) void signal_pairs_generic_kernel(const T* __restrict__ preds, const T* __restrict__ target, SigArgs a) {
  signal_body<T, false, E, PASS>(preds, target, a);
}

template <typename T, int E, int PASS>
__global__ __launch_bounds__(kSigThreads) void signal_pairs_vec_kernel(const T* __restrict__ preds, const T* __restrict__ target, SigArgs a) {
  signal_body<T, true, E, PASS>(preds, target, a);
}

// One wave per output: lane l adds the entries l, l + 64, ... of the output's partials in order, the lanes are added by the
// fixed tree of wave_sum.  Output o is signal o (STAGE 0), or entry o of the result in its own layout: pairing 0 [G, S],
// pairing 1 [G, S(target), S(preds)], pairing 2 [G] (all S signals' partials of a group, which are contiguous).
//   STAGE 0: mean[o], mean[nsig + o] = Σp / T, Σt / T            (partials of pass M)
//   STAGE 1: alpha[o] = (Σ p~t~ + eps) / (Σ t~² + eps), tt[o] = Σ t~²   (pass A)
//   STAGE 2: out[o] = 10 log10((num + eps) / (noise + eps)); num = alpha[o]² tt[o], or Σ t~² of pass B's partials (snr)
struct SigFold {
  const double* part;
  int64_t nwg, S, tiles, chunks, nsig;
  int E, pairing;
  bool snr;
  double eps, T;
  double* mean;
  double* alpha;
  double* tt;
  double* out;
};

template <int STAGE>
__global__ __launch_bounds__(kWave) void signal_fold_kernel(SigFold f) {
  const int64_t o = blockIdx.x;
  int64_t wg0 = o * f.chunks, count = f.chunks;
  int n_first = 0, n_second = 1;
  if (STAGE != 0) {
    if (f.E > 1) {
      const int64_t i = o % f.S, j = (o / f.S) % f.S, g = o / (f.S * f.S);
      wg0 = ((g * f.tiles + j / f.E) * f.tiles + i / f.E) * f.chunks;
      n_first = static_cast<int>(i % f.E) * f.E + static_cast<int>(j % f.E);
      n_second = f.E * f.E + static_cast<int>(j % f.E);
    } else if (f.pairing == 2) {
      wg0 = o * f.S * f.chunks, count = f.S * f.chunks;
    }
  }
  const bool second = STAGE != 2 || f.snr;
  const double* first = f.part + n_first * f.nwg + wg0;
  const double* other = f.part + n_second * f.nwg + wg0;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t k = threadIdx.x; k < count; k += kWave) {
    s0 += first[k];
    if (second) s1 += other[k];
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if (threadIdx.x != 0) return;
  if (STAGE == 0) {
    f.mean[o] = s0 / f.T;
    f.mean[f.nsig + o] = s1 / f.T;
  } else if (STAGE == 1) {
    f.alpha[o] = (s0 + f.eps) / (s1 + f.eps);
    f.tt[o] = s1;
  } else {
    const double num = f.snr ? s1 : f.alpha[o] * f.alpha[o] * f.tt[o];
    f.out[o] = 10.0 * log10((num + f.eps) / (s0 + f.eps));
  }
}

// ------------------------------------------------------------------------------------------------------------- host
namespace {

// samples per chunk of a signal when ``rows`` (group, tile) rows share the grid: a multiple of kSigAlign.  TMX_SIGNAL_CHUNK
// (read per call, rounded up to the alignment) overrides it: it lets a test place chunk edges inside a short signal.
int64_t signal_per_chunk(int64_t rows, int64_t T) {
  if (const char* env = std::getenv("TMX_SIGNAL_CHUNK")) {
    const long long v = std::atoll(env);
    if (v > 0) return (std::min<int64_t>(v, int64_t{1} << 40) + kSigAlign - 1) / kSigAlign * kSigAlign;
  }
  const int64_t want = std::max<int64_t>(1, (kSigTargetGroups + rows - 1) / rows);
  const int64_t most = std::max<int64_t>(1, T / kSigChunkMin);
  const int64_t n = std::min(want, most);
  const int64_t per = (T + n - 1) / n;
  return (per + kSigAlign - 1) / kSigAlign * kSigAlign;
}

struct SigGeometry {
  int E;
  int64_t tiles, rows;  // tiles per axis of a group (E == 1: S), (group, tile) rows on the grid
};

SigGeometry signal_geometry(int64_t G, int64_t S, int64_t pairing) {
  if (pairing != 1 || S == 1) return {1, S, G * S};
  const int E = S <= 2 ? 2 : kSigTile;
  const int64_t tiles = (S + E - 1) / E;
  return {E, tiles, G * tiles * tiles};
}

template <typename T, int E, int PASS>
void signal_launch(bool vec, int64_t nwg, const at::Tensor& p, const at::Tensor& t, const SigArgs& a) {
  auto kernel = vec ? signal_pairs_vec_kernel<T, E, PASS> : signal_pairs_generic_kernel<T, E, PASS>;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(nwg)), dim3(kSigThreads), 0, stream(), reinterpret_cast<const T*>(p.data_ptr()),
                     reinterpret_cast<const T*>(t.data_ptr()), a);
  TMX_LAUNCH_CHECK();
}

template <typename T, int PASS>
void signal_launch_tile(int E, bool vec, int64_t nwg, const at::Tensor& p, const at::Tensor& t, const SigArgs& a) {
  switch (E) {
    case 1: signal_launch<T, 1, PASS>(vec, nwg, p, t, a); break;
    case 2: signal_launch<T, 2, PASS>(vec, nwg, p, t, a); break;
    default: signal_launch<T, kSigTile, PASS>(vec, nwg, p, t, a); break;
  }
}

template <int STAGE>
void signal_fold(int64_t outputs, const SigFold& f) {
  hipLaunchKernelGGL(signal_fold_kernel<STAGE>, dim3(static_cast<unsigned>(outputs)), dim3(kWave), 0, stream(), f);
  TMX_LAUNCH_CHECK();
}

}  // namespace

// (threads per workgroup, fp32 samples per 16-byte load (16-bit inputs: twice as many), largest pair-tile extent, chunk
// alignment in samples: the least TMX_SIGNAL_CHUNK): what the tests need to place their edge shapes
std::vector<int64_t> signal_tile() { return {kSigThreads, 4, kSigTile, kSigAlign}; }

// How many chunks the pair passes of signal_pair_ratios split every signal of a [G, S, T] call into: a function of the shape
// and the pairing alone (and of TMX_SIGNAL_CHUNK where a test sets it).  Only the last chunk may be short.
int64_t signal_chunks(int64_t G, int64_t S, int64_t T, int64_t pairing) {
  TORCH_CHECK(G >= 1 && S >= 1 && T >= 1 && pairing >= 0 && pairing <= 2, "signal_chunks: expected a non-empty shape and a pairing in 0 .. 2");
  const int64_t per = signal_per_chunk(signal_geometry(G, S, pairing).rows, T);
  return (T + per - 1) / per;
}

// fp64 ratios in dB of preds / target [G, S, T].  pairing 0: [G, S], the pairs (p_s, t_s); 1: [G, S, S] with
// out[g, j, i] = ratio(preds[g, i], target[g, j]); 2: [G], one α and one ratio over the S diagonal pairs of a group.
at::Tensor signal_pair_ratios(const at::Tensor& preds_in, const at::Tensor& target_in, bool scale_invariant, bool zero_mean, int64_t pairing,
                              double eps) {
  const char* name = "signal_pair_ratios";
  TORCH_CHECK(preds_in.is_cuda() && target_in.is_cuda(), name, ": expected GPU tensors");
  TORCH_CHECK(preds_in.device() == target_in.device(), name, ": preds and target on different devices");
  TORCH_CHECK(preds_in.dim() == 3 && preds_in.sizes() == target_in.sizes(), name, ": expected matching [G, S, T]");
  TORCH_CHECK(preds_in.scalar_type() == target_in.scalar_type(), name, ": dtype mismatch");
  const auto dtype = preds_in.scalar_type();
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16 || dtype == at::kHalf, name, ": unsupported dtype ", dtype);
  TORCH_CHECK(preds_in.numel() > 0, name, ": empty input");
  TORCH_CHECK(pairing >= 0 && pairing <= 2, name, ": pairing must be 0, 1 or 2");
  const at::DeviceGuard guard(preds_in.device());
  const int64_t G = preds_in.size(0), S = preds_in.size(1), T = preds_in.size(2);
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  const int64_t V = 16 / static_cast<int64_t>(p.element_size());
  const bool vec = T % V == 0 && (reinterpret_cast<uintptr_t>(p.data_ptr()) & 15) == 0 && (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;

  const SigGeometry geo = signal_geometry(G, S, pairing);
  const int64_t nsig = G * S;
  const int64_t outputs = pairing == 0 ? nsig : (pairing == 1 ? nsig * S : G);
  const int64_t per_chunk = signal_per_chunk(geo.rows, T), chunks = (T + per_chunk - 1) / per_chunk;
  const int64_t mean_per_chunk = signal_per_chunk(nsig, T), mean_chunks = (T + mean_per_chunk - 1) / mean_per_chunk;
  const int64_t nwg = geo.rows * chunks, mean_nwg = nsig * mean_chunks;
  TORCH_CHECK(nwg <= INT32_MAX && mean_nwg <= INT32_MAX && outputs <= INT32_MAX, name, ": too many workgroups for one launch");

  const auto f64 = p.options().dtype(at::kDouble);
  const int64_t sums = geo.E * geo.E + geo.E;  // the most any pass writes (E == 1: 2, as pass M)
  auto part = at::empty({std::max(sums * nwg, zero_mean ? 2 * mean_nwg : int64_t{0})}, f64);
  auto scalars = at::empty({2 * nsig + 2 * outputs}, f64);
  double* mean = scalars.data_ptr<double>();
  double* alpha = mean + 2 * nsig;
  double* tt = alpha + outputs;
  at::Tensor out = pairing == 0 ? at::empty({G, S}, f64) : (pairing == 1 ? at::empty({G, S, S}, f64) : at::empty({G}, f64));

  SigArgs a{S, T, geo.tiles, per_chunk, chunks, nsig, nwg, static_cast<int>(pairing), zero_mean ? mean : nullptr, alpha, part.data_ptr<double>()};
  SigFold f{part.data_ptr<double>(), nwg, S, geo.tiles, chunks, nsig, geo.E, static_cast<int>(pairing), !scale_invariant, eps,
            static_cast<double>(T), mean, alpha, tt, out.data_ptr<double>()};

  dispatch_float3(dtype, name, [&](auto tag) {
    using T_ = decltype(tag);
    if (zero_mean) {
      SigArgs am = a;
      am.tiles = S, am.per_chunk = mean_per_chunk, am.chunks = mean_chunks, am.nwg = mean_nwg, am.mean = nullptr;
      SigFold fm = f;
      fm.nwg = mean_nwg, fm.chunks = mean_chunks, fm.E = 1;
      signal_launch<T_, 1, kSigMean>(vec, mean_nwg, p, t, am);
      signal_fold<0>(nsig, fm);
    }
    if (scale_invariant) {
      signal_launch_tile<T_, kSigA>(geo.E, vec, nwg, p, t, a);
      signal_fold<1>(outputs, f);
      signal_launch_tile<T_, kSigB>(geo.E, vec, nwg, p, t, a);
    } else {
      signal_launch_tile<T_, kSigSnr>(geo.E, vec, nwg, p, t, a);
    }
    signal_fold<2>(outputs, f);
  });
  return out;
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("signal_pair_ratios(Tensor preds, Tensor target, bool scale_invariant, bool zero_mean, int pairing, float eps) -> Tensor");
  m.def("signal_chunks(int G, int S, int T, int pairing) -> int", &tmx::signal_chunks);
  m.def("signal_tile() -> int[]", &tmx::signal_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) { m.impl("signal_pair_ratios", &tmx::signal_pair_ratios); }
