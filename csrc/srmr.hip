// SRMR (speech-to-reverberation modulation energy ratio, the chain functional/audio/srmr.py states) for gfx950: every signal of a
// [B, T] batch in the same launches, fp64 arithmetic on the up-cast samples, nothing read to the host, no atomics: every sum runs in
// an order that depends on the signal's own sizes only, so two runs are bit-equal and a signal alone has the bits it has in a batch.
//
// Both recursions are serial in time; what the kernels remove is everything around them.
//   srmr_gammatone_kernel  one thread per (signal, channel), one wave per (signal, 64 channels): the four direct-form-I biquads of the
//                          gammatone cascade, skewed by one sample each so that an iteration holds four independent recursions
//                          (stage s works on sample i − s), each stage clamped to [-1, 1] before it feeds the next, the division by the
//                          gain fused.  The wave's channels read the same sample: a block of 64 up-cast samples sits in LDS (the next
//                          block's load is in flight while this one is filtered), and every thread stages its 64 outputs in LDS so that
//                          rows leave as 512-byte runs.  The tail [T, nfft) is written as zeros for the Hilbert FFT.
//   srmr_energies_kernel   one thread per (signal, channel, modulation filter), 64 / M channels per wave: |z| of the analytic signal
//                          (complex128, read in place with 16-byte loads, hypot once per channel and sample) goes through LDS, the
//                          biquad runs without a clamp, and (y[n] w[n − f w_inc])² is added to the at most four frames that hold sample
//                          n: four accumulators in registers, rotated every w_inc samples, a frame written once when it leaves.  The
//                          window (zero-filled to 4 w_inc) sits in LDS when it fits beside the staging buffer, else it is read through
//                          the cache.  Neither the [B, N, M, T] filter output nor any frame tensor exists.
//   srmr_scores_kernel     one workgroup per signal: optional 30 dB normalisation, frame means, the cumulative energy percentage from the
//                          lowest channel upwards, k90, k* = kstar[k90] and the ratio; NaN where there is no k90.
#include "common.h"

#include <vector>

namespace tmx {

constexpr int kSrmrBlock = 64;                  // time steps per staged block, and threads per workgroup of the two filter kernels
constexpr int kSrmrLd = kSrmrBlock + 1;         // LDS stride of a thread's row of staged values: rows start on different banks
constexpr int kSrmrSkew = 3;                    // stage 3 is that many samples behind stage 0
constexpr int kSrmrSlots = 4;                   // frames that can hold one sample: w_length <= 4 w_inc
constexpr int kSrmrScoreThreads = 256;
constexpr int64_t kSrmrWindowLds = 48 * 1024;   // the zero-filled window goes to LDS up to this many bytes
constexpr int64_t kSrmrScoreLds = 60 * 1024;

template <typename S> __device__ __forceinline__ double srmr_ld(const S* __restrict__ p, int64_t i) {
  if constexpr (std::is_same<S, double>::value) return p[i];
  else return static_cast<double>(to_f32<S>(p[i]));
}

__device__ __forceinline__ double srmr_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// torch.clamp(v, -1, 1): a NaN stays
__device__ __forceinline__ double srmr_clamp(double v) { return v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v); }

// One direct-form-I biquad step in iir_kernel's order: the b terms added in tap order, then the a terms subtracted in tap order.
struct SrmrBiquad {
  double b0, b1, b2, a1, a2, x1, x2, y1, y2;
  __device__ __forceinline__ double step(double x) {
    double acc = b0 * x;
    acc = fma(b1, x1, acc);
    acc = fma(b2, x2, acc);
    acc = fma(-a1, y1, acc);
    acc = fma(-a2, y2, acc);
    x2 = x1, x1 = x;
    y2 = y1, y1 = acc;
    return acc;
  }
};

// ------------------------------------------------------------------------------------------------------------ gammatone
// out[b][n][0 .. nfft).  Grid: flat over (b, 64-channel chunk).
template <typename S>
__global__ __launch_bounds__(kSrmrBlock) void srmr_gammatone_kernel(const S* __restrict__ x, int64_t stride, const double* __restrict__ coefs, int64_t N,
                                                                    int64_t T, int64_t nfft, int64_t chunks, double* __restrict__ out) {
  __shared__ double xs[kSrmrBlock];
  __shared__ double ys[kSrmrBlock * kSrmrLd];
  __shared__ double gs[kSrmrBlock];
  const int lane = threadIdx.x;
  const int64_t id = blockIdx.x, b = id / chunks, n0 = (id % chunks) * kSrmrBlock;
  const int64_t rows = min(static_cast<int64_t>(kSrmrBlock), N - n0);
  const bool live = lane < rows;
  const S* src = x + b * stride;
  double* dst = out + (b * N + n0) * nfft;

  // a thread past the last channel filters with channel n0's table and writes nothing
  const double* c = coefs + (n0 + (live ? lane : 0)) * 10;
  const double a0 = c[6];
  SrmrBiquad st[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) st[s] = {c[0] / a0, c[1 + s] / a0, c[5] / a0, c[7] / a0, c[8] / a0, 0.0, 0.0, 0.0, 0.0};
  gs[lane] = c[9];  // the division by the gain waits for the write-out, where a lane divides one value per row and block
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;  // clamped outputs of stages 0 .. 2 of the previous iteration

  // iteration i: stage s filters sample i − s; the samples before 0 and from T on are zeros and leave every state as it is
  const int64_t steps = T + kSrmrSkew;
  double next = lane < T ? srmr_ld<S>(src, lane) : 0.0;
  for (int64_t i0 = 0; i0 < steps; i0 += kSrmrBlock) {
    __syncthreads();  // the previous block's rows have been written out
    xs[lane] = next;
    __syncthreads();
    const int64_t ahead = i0 + kSrmrBlock + lane;
    next = ahead < T ? srmr_ld<S>(src, ahead) : 0.0;
    const int len = static_cast<int>(min(static_cast<int64_t>(kSrmrBlock), steps - i0));
    for (int k = 0; k < len; ++k) {
      const double y3 = st[3].step(f2);
      const double y2 = st[2].step(f1);
      const double y1 = st[1].step(f0);
      const double y0 = st[0].step(xs[k]);
      f2 = srmr_clamp(y2), f1 = srmr_clamp(y1), f0 = srmr_clamp(y0);
      ys[lane * kSrmrLd + k] = srmr_clamp(y3);
    }
    __syncthreads();
    // slot k of this block is sample i0 + k − 3
    const int64_t j = i0 + lane - kSrmrSkew;
    if (lane < len && j >= 0 && j < T)
      for (int r = 0; r < rows; ++r) dst[r * nfft + j] = ys[r * kSrmrLd + lane] / gs[r];
  }
  for (int r = 0; r < rows; ++r)
    for (int64_t j = T + lane; j < nfft; j += kSrmrBlock) dst[r * nfft + j] = 0.0;
}

// ------------------------------------------------------------------------------------------------- modulation energies
// energy[b][n][m][f].  Grid: flat over (b, group of cpb = 64 / M channels); thread (c, m) = (tid / M, tid % M).
// Dynamic LDS: cpb rows of the envelope block, then (WLDS) the window zero-filled to 4 w_inc.
template <bool WLDS>
__global__ __launch_bounds__(kSrmrBlock) void srmr_energies_kernel(const double2* __restrict__ z, int64_t row_stride, int64_t N, int M, int cpb, int64_t groups,
                                                                   const double* __restrict__ mod, const double* __restrict__ window, int64_t w_length,
                                                                   int64_t w_inc, int64_t F, double* __restrict__ energy) {
  extern __shared__ double smem[];
  double* env = smem;
  double* wl = smem + cpb * kSrmrLd;
  const int tid = threadIdx.x, c = tid / M, m = tid % M;
  const int64_t id = blockIdx.x, b = id / groups, n0 = (id % groups) * cpb;
  const int rows = static_cast<int>(min(static_cast<int64_t>(cpb), N - n0));
  const bool live = c < rows;
  const int64_t wpad = kSrmrSlots * w_inc;
  if constexpr (WLDS) {
    for (int64_t i = tid; i < wpad; i += kSrmrBlock) wl[i] = i < w_length ? window[i] : 0.0;
  }
  auto win = [&](int64_t i) -> double {
    if constexpr (WLDS) return wl[i];
    else return i < w_length ? window[i] : 0.0;
  };

  const double* q = mod + m * 6;
  const double a0 = q[3];
  SrmrBiquad st = {q[0] / a0, q[1] / a0, q[2] / a0, q[4] / a0, q[5] / a0, 0.0, 0.0, 0.0, 0.0};
  const double2* src = z + (b * N + n0) * row_stride;
  double* dst = energy + (((b * N + n0 + (live ? c : 0)) * M) + m) * F;
  const int er = live ? c : 0;  // an idle thread filters row 0 and writes nothing

  const int64_t n_end = (F - 1) * w_inc + w_length;  // the last sample of the last frame, <= T
  double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;      // frames g, g − 1, g − 2, g − 3 of the w_inc-segment g the loop is in
  int64_t g = 0, r = 0;                                // n = g w_inc + r
  for (int64_t t0 = 0; t0 < n_end; t0 += kSrmrBlock) {
    const int len = static_cast<int>(min(static_cast<int64_t>(kSrmrBlock), n_end - t0));
    __syncthreads();  // the previous block has been consumed (and, the first time, the window is complete)
    for (int row = 0; row < rows; ++row) {
      if (tid < len) {
        const double2 v = src[row * row_stride + t0 + tid];
        env[row * kSrmrLd + tid] = hypot(v.x, v.y);
      }
    }
    __syncthreads();
    for (int k = 0; k < len; ++k) {
      const double y = st.step(env[er * kSrmrLd + k]);
      const double v0 = y * win(r), v1 = y * win(r + w_inc), v2 = y * win(r + 2 * w_inc), v3 = y * win(r + 3 * w_inc);
      e0 = fma(v0, v0, e0);
      e1 = fma(v1, v1, e1);
      e2 = fma(v2, v2, e2);
      e3 = fma(v3, v3, e3);
      if (++r == w_inc) {  // segment g ends: frame g − 3 has passed its last sample
        const int64_t f = g - (kSrmrSlots - 1);
        if (live && f >= 0 && f < F) dst[f] = e3;
        e3 = e2, e2 = e1, e1 = e0, e0 = 0.0;
        r = 0, ++g;
      }
    }
  }
  if (r != 0) {  // close the partial segment the same way
    const int64_t f = g - (kSrmrSlots - 1);
    if (live && f >= 0 && f < F) dst[f] = e3;
    e3 = e2, e2 = e1, e1 = e0;
    ++g;
  }
  // e1, e2, e3 hold frames g − 1, g − 2, g − 3
  if (live) {
    if (g - 1 >= 0 && g - 1 < F) dst[g - 1] = e1;
    if (g - 2 >= 0 && g - 2 < F) dst[g - 2] = e2;
    if (g - 3 >= 0 && g - 3 < F) dst[g - 3] = e3;
  }
}

// --------------------------------------------------------------------------------------------------------------- scores
// Dynamic LDS: avg[N][M], row[N], den[N].  One workgroup per signal.
__global__ __launch_bounds__(kSrmrScoreThreads) void srmr_scores_kernel(const double* __restrict__ energy, const int* __restrict__ kstar, int64_t N, int M,
                                                                        int64_t F, bool norm, double* __restrict__ scores) {
  extern __shared__ double smem[];
  __shared__ double wpeak[kSrmrScoreThreads / kWave];
  __shared__ int ks;
  double* avg = smem;
  double* row = smem + N * M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x, MF = static_cast<int64_t>(M) * F;
  const double* e = energy + b * N * MF;

  double peak = 0.0, floor_ = 0.0;
  if (norm) {  // peak: the largest channel mean over filters and frames
    double p = -INFINITY;
    for (int64_t i = tid; i < MF; i += kSrmrScoreThreads) {
      double s = 0.0;
      for (int64_t n = 0; n < N; ++n) s += e[n * MF + i];
      const double mean = s / static_cast<double>(N);
      p = mean > p ? mean : p;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(p, off, kWave);
      p = o > p ? o : p;
    }
    if (lane == 0) wpeak[wave] = p;
    __syncthreads();
    peak = wpeak[0];
    for (int w = 1; w < kSrmrScoreThreads / kWave; ++w) peak = wpeak[w] > peak ? wpeak[w] : peak;
    floor_ = peak * 1e-3;
  }
  for (int64_t i = tid; i < N * M; i += kSrmrScoreThreads) {  // frame mean of every (channel, filter), frames in order
    const double* p = e + i * F;
    double s = 0.0;
    for (int64_t f = 0; f < F; ++f) {
      double v = p[f];
      if (norm) {
        v = v < floor_ ? floor_ : v;
        v = v > peak ? peak : v;
      }
      s += v;
    }
    avg[i] = s / static_cast<double>(F);
  }
  __syncthreads();
  for (int64_t n = tid; n < N; n += kSrmrScoreThreads) {
    double s = 0.0;
    for (int k = 0; k < M; ++k) s += avg[n * M + k];
    row[n] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int64_t n = 0; n < N; ++n) total += row[n];
    // channel N − 1 is the lowest in frequency: k90 counts from there
    double cum = 0.0;
    int64_t k90 = -1;
    for (int64_t i = 0; i < N; ++i) {
      cum += row[N - 1 - i] * 100.0 / total;
      if (cum > 90.0) {
        k90 = i;
        break;
      }
    }
    const int k = k90 >= 0 ? kstar[k90] : 0;
    ks = (k >= 4 && k <= M) ? k : 0;
  }
  __syncthreads();
  const int k = ks;
  if (k == 0) {
    if (tid == 0) scores[b] = srmr_nan();
    return;
  }
  // per channel: the first four filters, and filters 4 .. k* − 1 (thread 0 read row[] before it wrote ks, so row[] is free again)
  double* num = row;
  double* den = row + N;
  for (int64_t n = tid; n < N; n += kSrmrScoreThreads) {
    double s = 0.0, d = 0.0;
    for (int i = 0; i < 4; ++i) s += avg[n * M + i];
    for (int i = 4; i < k; ++i) d += avg[n * M + i];
    num[n] = s;
    den[n] = d;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0, d = 0.0;
    for (int64_t n = 0; n < N; ++n) {
      s += num[n];
      d += den[n];
    }
    scores[b] = s / d;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
namespace {

unsigned srmr_grid(int64_t n, const char* name) {
  TORCH_CHECK(n >= 1 && n <= INT32_MAX, name, ": too many workgroups for one launch");
  return static_cast<unsigned>(n);
}

}  // namespace

// preds [B, T] (fp32 / fp64 / bf16 / fp16, unit stride along T, any row stride), coefs [N, 10] fp64 -> [B, N, nfft] fp64, zeros from T on
at::Tensor srmr_gammatone(const at::Tensor& preds, const at::Tensor& coefs, int64_t nfft) {
  const char* name = "srmr_gammatone";
  TORCH_CHECK(preds.is_cuda() && coefs.is_cuda() && preds.device() == coefs.device(), name, ": expected GPU tensors on one device");
  TORCH_CHECK(preds.dim() == 2 && preds.size(0) >= 1 && preds.size(1) >= 1, name, ": expected non-empty [B, T]");
  TORCH_CHECK(coefs.dim() == 2 && coefs.size(1) == 10 && coefs.size(0) >= 1 && coefs.scalar_type() == at::kDouble && coefs.is_contiguous(), name,
              ": expected a contiguous fp64 [N, 10] table");
  const int64_t B = preds.size(0), T = preds.size(1), N = coefs.size(0);
  TORCH_CHECK(nfft >= T, name, ": nfft below the signal length");
  const at::DeviceGuard guard(preds.device());
  auto p = (preds.stride(1) == 1 && preds.stride(0) >= 0) ? preds : preds.contiguous();
  auto out = at::empty({B, N, nfft}, p.options().dtype(at::kDouble));
  const int64_t chunks = (N + kSrmrBlock - 1) / kSrmrBlock;
  TMX_DISPATCH_FLOAT(p.scalar_type(), name, [&] {
    hipLaunchKernelGGL(srmr_gammatone_kernel<scalar_t>, dim3(srmr_grid(B * chunks, name)), dim3(kSrmrBlock), 0, stream(),
                       reinterpret_cast<const scalar_t*>(p.data_ptr()), p.stride(0), coefs.data_ptr<double>(), N, T, nfft, chunks, out.data_ptr<double>());
  });
  TMX_LAUNCH_CHECK();
  return out;
}

// analytic [B, N, nfft] complex128 (unit stride along time, rows nfft apart or more), mod [M, 2, 3], window [w_length] fp64
// -> [B, N, M, F] fp64, F = 1 + (T − w_length) / w_inc
at::Tensor srmr_energies(const at::Tensor& analytic, int64_t T, const at::Tensor& mod, const at::Tensor& window, int64_t w_inc) {
  const char* name = "srmr_energies";
  TORCH_CHECK(analytic.is_cuda() && mod.is_cuda() && window.is_cuda() && analytic.device() == mod.device() && analytic.device() == window.device(), name,
              ": expected GPU tensors on one device");
  TORCH_CHECK(analytic.dim() == 3 && analytic.scalar_type() == at::kComplexDouble && analytic.size(0) >= 1 && analytic.size(1) >= 1, name,
              ": expected a non-empty complex128 [B, N, nfft]");
  TORCH_CHECK(mod.dim() == 3 && mod.size(1) == 2 && mod.size(2) == 3 && mod.scalar_type() == at::kDouble && mod.is_contiguous(), name,
              ": expected a contiguous fp64 [M, 2, 3] table");
  TORCH_CHECK(window.dim() == 1 && window.scalar_type() == at::kDouble && window.is_contiguous(), name, ": expected a contiguous fp64 window");
  const int64_t B = analytic.size(0), N = analytic.size(1), M = mod.size(0), w_length = window.numel();
  TORCH_CHECK(M >= 1 && M <= kSrmrBlock, name, ": 1 <= M <= ", kSrmrBlock);
  TORCH_CHECK(w_inc >= 1 && w_length >= 1 && w_length <= kSrmrSlots * w_inc, name, ": expected 1 <= w_length <= 4 w_inc");
  TORCH_CHECK(T >= w_length && T <= analytic.size(2), name, ": expected w_length <= T <= nfft");
  const at::DeviceGuard guard(analytic.device());
  const bool in_place = analytic.stride(2) == 1 && analytic.stride(1) >= analytic.size(2) && analytic.stride(0) == N * analytic.stride(1);
  auto z = in_place ? analytic : analytic.contiguous();
  const int64_t F = 1 + (T - w_length) / w_inc;
  auto out = at::empty({B, N, M, F}, z.options().dtype(at::kDouble));
  const int cpb = kSrmrBlock / static_cast<int>(M);
  const int64_t groups = (N + cpb - 1) / cpb;
  const int64_t wbytes = kSrmrSlots * w_inc * static_cast<int64_t>(sizeof(double));
  const bool wlds = wbytes <= kSrmrWindowLds;
  const size_t shmem = static_cast<size_t>(cpb) * kSrmrLd * sizeof(double) + (wlds ? static_cast<size_t>(wbytes) : 0);
  auto kernel = wlds ? srmr_energies_kernel<true> : srmr_energies_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(srmr_grid(B * groups, name)), dim3(kSrmrBlock), shmem, stream(), reinterpret_cast<const double2*>(z.data_ptr()), z.stride(1), N,
                     static_cast<int>(M), cpb, groups, mod.data_ptr<double>(), window.data_ptr<double>(), w_length, w_inc, F, out.data_ptr<double>());
  TMX_LAUNCH_CHECK();
  return out;
}

// energy [B, N, M, F] fp64, kstar [N] int32 (indexed by k90, counted from the lowest channel) -> scores [B] fp64
at::Tensor srmr_scores(const at::Tensor& energy, const at::Tensor& kstar, bool norm) {
  const char* name = "srmr_scores";
  TORCH_CHECK(energy.is_cuda() && kstar.is_cuda() && energy.device() == kstar.device(), name, ": expected GPU tensors on one device");
  TORCH_CHECK(energy.dim() == 4 && energy.scalar_type() == at::kDouble && energy.numel() >= 1, name, ": expected a non-empty fp64 [B, N, M, F]");
  const int64_t B = energy.size(0), N = energy.size(1), M = energy.size(2), F = energy.size(3);
  TORCH_CHECK(kstar.dim() == 1 && kstar.size(0) == N && kstar.scalar_type() == at::kInt && kstar.is_contiguous(), name, ": expected a contiguous int32 [N] table");
  TORCH_CHECK(M >= 4 && M <= kSrmrBlock, name, ": 4 <= M <= ", kSrmrBlock);
  const int64_t lds = (N * M + 2 * N) * static_cast<int64_t>(sizeof(double));
  TORCH_CHECK(lds <= kSrmrScoreLds, name, ": too many channels for one workgroup's LDS");
  const at::DeviceGuard guard(energy.device());
  auto e = energy.contiguous();
  auto out = at::empty({B}, e.options());
  hipLaunchKernelGGL(srmr_scores_kernel, dim3(srmr_grid(B, name)), dim3(kSrmrScoreThreads), static_cast<size_t>(lds), stream(), e.data_ptr<double>(),
                     kstar.data_ptr<int>(), N, static_cast<int>(M), F, norm, out.data_ptr<double>());
  TMX_LAUNCH_CHECK();
  return out;
}

// (time steps per staged block = threads per workgroup of the filter kernels, frames that can hold one sample, bytes up to which the
// zero-filled window is kept in LDS)
std::vector<int64_t> srmr_tile() { return {kSrmrBlock, kSrmrSlots, kSrmrWindowLds}; }

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("srmr_gammatone(Tensor preds, Tensor coefs, int nfft) -> Tensor");
  m.def("srmr_energies(Tensor analytic, int T, Tensor mod, Tensor window, int w_inc) -> Tensor");
  m.def("srmr_scores(Tensor energy, Tensor kstar, bool norm) -> Tensor");
  m.def("srmr_tile() -> int[]", &tmx::srmr_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("srmr_gammatone", &tmx::srmr_gammatone);
  m.impl("srmr_energies", &tmx::srmr_energies);
  m.impl("srmr_scores", &tmx::srmr_scores);
}
