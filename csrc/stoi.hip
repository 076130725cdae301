// STOI / ESTOI (pystoi's algorithm, as functional/audio/stoi.py states it) for gfx950: every signal of a [B, T] batch in the same
// launches, fp64 arithmetic on the up-cast samples (fp32 / fp64 / bf16 / fp16 read in place), nothing read to the host between
// the stages, no atomics: every sum is folded in a fixed order that depends on the signal's own sizes only, so two runs are
// bit-equal and a signal alone has the bits it has inside a batch.
//
// Stages (x is the clean signal ``target``, y is ``preds``):
//   stoi_resample_kernel  (fs != 10 kHz) y[j] = Σ_m x[m] h'[j·down − m·up]: one thread per output walks the ceil(len(h') / up)
//                         taps of its phase; h' (padded, up-scaled, built by the host once per rate and device) is read through
//                         the cache, as at 22.05 / 44.1 kHz its 250 KiB do not fit in LDS.  Both signals in one launch.
//   stoi_energy_kernel    one wave per 256-sample Hann frame of x (hop 128): e = 20 log10(‖w·frame‖ + EPS).
//   stoi_keep_kernel      one workgroup per signal: max e (a NaN wins, as torch.max), keep = (max − 40 − e) < 0, and an in-order
//                         compaction (ballot prefix per 256-frame strip): K[b] and the source frame of every kept slot.
//   stoi_bands_kernel     one workgroup per (signal, x or y, 16 STFT frames): the 17·128 compacted samples the tile covers are
//                         rebuilt in LDS from the source frames k_{j−1}, k_j, k_{j+1} through the kept list (the compacted signal
//                         never exists in HBM), windowed again on the way into v_mfma_f64_16x16x4_f64: [16, 256] frames times
//                         [256, 2·224] twiddles from a 512-entry table indexed by (k·n) mod 512, bins 7 .. 230 of the 512-point
//                         zero-padded transform (only 7 .. 218 are used).  |X|² goes through LDS, one thread per (band, frame) adds
//                         its contiguous bins in order: sqrt -> bands[sig][b][band][j].
//   stoi_segments_kernel  one wave per 30-frame segment (32 segments per workgroup): STOI's clipped, normalised row correlation or
//                         ESTOI's row-then-column normalisation in LDS; one partial per workgroup.
//   stoi_final_kernel     partials of a signal added in order, J < 30 -> 1e-5, frames[b] = J[b].
#include "common.h"

#include <cmath>
#include <tuple>
#include <vector>

namespace tmx {

constexpr int kStoiThreads = 256;
constexpr int kStoiFrame = 256, kStoiHop = 128, kStoiBands = 15, kStoiSeg = 30;
constexpr int kStoiBin0 = 7;
constexpr int kStoiTileFrames = 16;                    // STFT frames per workgroup of the band kernel (one MFMA tile of rows)
constexpr int kStoiColTiles = 14;                      // 16-bin column tiles: bins 7 .. 230 cover the bands' 7 .. 218
constexpr int kStoiSegBlock = 32;                      // segments per workgroup of the segment kernel
constexpr int kStoiSpan = kStoiTileFrames + 1;         // 128-sample pieces of compacted signal under a tile of frames
constexpr int kStoiPiece = kStoiHop + 4;               // LDS stride of a piece: the 16 frames of a fragment read hit other banks
constexpr int kStoiPw = 240;                           // LDS stride of a frame's |X|² row
constexpr int kStoiTables = kStoiFrame + 512 + 512;    // Hann window, cos and sin of 2 pi i / 512
constexpr double kStoiEps = 2.220446049250313e-16;

__constant__ int kStoiEdge[kStoiBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

template <typename S> __device__ __forceinline__ double stoi_ld(const S* __restrict__ p, int64_t i) {
  if constexpr (std::is_same<S, double>::value) return p[i];
  else return static_cast<double>(to_f32<S>(p[i]));
}

__device__ __forceinline__ double stoi_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// torch.minimum / torch.max: a NaN operand wins
__device__ __forceinline__ double stoi_min(double a, double b) { return (a != a || b != b) ? stoi_nan() : (a < b ? a : b); }
__device__ __forceinline__ double stoi_max(double a, double b) { return (a != a || b != b) ? stoi_nan() : (a > b ? a : b); }

// ---------------------------------------------------------------------------------------------------------- resampler
// out[sig][b][j], sig 0 = x, 1 = y.  Grid: flat over (sig, b, 256-output strip).
template <typename S>
__global__ __launch_bounds__(kStoiThreads) void stoi_resample_kernel(const S* __restrict__ x, const S* __restrict__ y, const double* __restrict__ h,
                                                                     double* __restrict__ out, int64_t B, int64_t n_in, int64_t n_out, int64_t strips,
                                                                     int64_t up, int64_t down, int64_t pre_remove, int64_t len_h) {
  const int64_t id = blockIdx.x, strip = id % strips, rest = id / strips, b = rest % B, sig = rest / B;
  const int64_t j = strip * kStoiThreads + threadIdx.x;
  if (j >= n_out) return;
  const S* src = (sig ? y : x) + b * n_in;
  const int64_t pos = (j + pre_remove) * down, m0 = pos / up, phase = pos - m0 * up;
  // tap t reads h'[phase + t·up] and x[m0 − t]: the taps with the filter index below len_h and 0 <= m0 − t < n_in, in order
  const int64_t t_hi = min((len_h - phase + up - 1) / up, m0 + 1), t_lo = max(int64_t{0}, m0 - n_in + 1);
  const double* hp = h + phase + t_lo * up;
  const S* sp = src + (m0 - t_lo);
  double acc = 0.0;
#pragma unroll 4
  for (int64_t t = t_lo; t < t_hi; ++t, hp += up, --sp) acc = fma(*hp, stoi_ld<S>(sp, 0), acc);
  out[(sig * B + b) * n_out + j] = acc;
}

// ------------------------------------------------------------------------------------------------------ frame energies
// e[b][f] of the clean signal.  Grid: flat over (b, 4-frame block); a wave per frame, lane l takes samples l, l + 64, ...
template <typename S>
__global__ __launch_bounds__(kStoiThreads) void stoi_energy_kernel(const S* __restrict__ x, int64_t stride, int64_t F, int64_t fblocks,
                                                                   const double* __restrict__ tab, double* __restrict__ e) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t id = blockIdx.x, b = id / fblocks, f = (id % fblocks) * (kStoiThreads / kWave) + wave;
  if (f >= F) return;
  const S* src = x + b * stride + f * kStoiHop;
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < kStoiFrame / kWave; ++i) {
    const int q = lane + kWave * i;
    const double v = tab[q] * stoi_ld<S>(src, q);
    acc = fma(v, v, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) e[b * F + f] = 20.0 * log10(sqrt(acc) + kStoiEps);
}

// ------------------------------------------------------------------------------------------------------ kept-frame list
// One workgroup per signal.  kept[b][i] = source frame of kept slot i (i < K[b]), in order.
__global__ __launch_bounds__(kStoiThreads) void stoi_keep_kernel(const double* __restrict__ e, int64_t F, int* __restrict__ kept, int* __restrict__ K) {
  __shared__ double wmax[kStoiThreads / kWave];
  __shared__ int wcount[kStoiThreads / kWave];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const double* eb = e + b * F;
  double m = -INFINITY;
  for (int64_t f = tid; f < F; f += kStoiThreads) m = stoi_max(m, eb[f]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = stoi_max(m, __shfl_xor(m, off, kWave));
  if (lane == 0) wmax[wave] = m;
  __syncthreads();
  m = stoi_max(stoi_max(wmax[0], wmax[1]), stoi_max(wmax[2], wmax[3]));
  int running = 0;
  for (int64_t base = 0; base < F; base += kStoiThreads) {
    const int64_t f = base + tid;
    const bool keep = f < F && (m - 40.0 - eb[f]) < 0.0;
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();  // the previous strip's counts have been read
    if (lane == 0) wcount[wave] = __popcll(mask);
    __syncthreads();
    int off = running;
    for (int w = 0; w < wave; ++w) off += wcount[w];
    if (keep) kept[b * F + off + before] = static_cast<int>(f);
    running += wcount[0] + wcount[1] + wcount[2] + wcount[3];
  }
  if (tid == 0) K[b] = running;
}

// -------------------------------------------------------------------------------- overlap-add + STFT + third-octave bands
// bands[sig][b][band][j] for the 16 STFT frames j0 .. j0 + 15 of one signal.  Grid: flat over (sig, b, tile).
template <typename S>
__global__ __launch_bounds__(kStoiThreads) void stoi_bands_kernel(const S* __restrict__ x, const S* __restrict__ y, int64_t stride, const int* __restrict__ kept,
                                                                  const int* __restrict__ K, int64_t F, const double* __restrict__ tab,
                                                                  double* __restrict__ bands, int64_t B, int64_t Jmax, int64_t tiles) {
  typedef double V4 __attribute__((ext_vector_type(4)));
  __shared__ double c[kStoiSpan * kStoiPiece];
  __shared__ double w[kStoiFrame];
  __shared__ double tc[512], ts[512];
  __shared__ double pw[kStoiTileFrames * kStoiPw];
  __shared__ int slot[kStoiSpan + 1];  // source frames of the kept slots j0 − 1 .. j0 + 16, −1 where there is none

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t id = blockIdx.x, tile = id % tiles, rest = id / tiles, b = rest % B, sig = rest / B;
  const int64_t Kb = K[b], J = Kb > 0 ? Kb - 1 : 0, j0 = tile * kStoiTileFrames;
  if (j0 >= J) return;
  const S* src = (sig ? y : x) + b * stride;

  for (int i = tid; i < kStoiFrame; i += kStoiThreads) w[i] = tab[i];
  for (int i = tid; i < 512; i += kStoiThreads) {
    tc[i] = tab[kStoiFrame + i];
    ts[i] = tab[kStoiFrame + 512 + i];
  }
  if (tid < kStoiSpan + 1) {
    const int64_t i = j0 - 1 + tid;
    slot[tid] = (i >= 0 && i < Kb) ? kept[b * F + i] : -1;
  }
  __syncthreads();
  // compacted sample 128 (j0 + piece) + r: the first half of kept slot j0 + piece plus the second half of slot j0 + piece − 1
  for (int n = tid; n < kStoiSpan * kStoiHop; n += kStoiThreads) {
    const int piece = n >> 7, r = n & (kStoiHop - 1);
    const int cur = slot[piece + 1], prev = slot[piece];
    double v = 0.0;
    if (prev >= 0) v = w[kStoiHop + r] * stoi_ld<S>(src, static_cast<int64_t>(prev) * kStoiHop + kStoiHop + r);
    if (cur >= 0) v += w[r] * stoi_ld<S>(src, static_cast<int64_t>(cur) * kStoiHop + r);
    c[piece * kStoiPiece + r] = v;
  }
  __syncthreads();

  const int fk = lane >> 4, fr = lane & 15;  // A: frame fr, sample 4 s + fk;  B: sample 4 s + fk, bin fr of the column tile
  for (int ct = wave; ct < kStoiColTiles; ct += kStoiThreads / kWave) {
    const int bin = kStoiBin0 + ct * 16 + fr;
    V4 re = {0.0, 0.0, 0.0, 0.0}, im = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < kStoiFrame / 4; ++s) {
      const int q = 4 * s + fk, n = kStoiHop * fr + q;
      const double a = w[q] * c[(n >> 7) * kStoiPiece + (n & (kStoiHop - 1))];
      const int ti = (bin * q) & 511;
      re = __builtin_amdgcn_mfma_f64_16x16x4f64(a, tc[ti], re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f64_16x16x4f64(a, ts[ti], im, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) pw[(fk + 4 * r) * kStoiPw + ct * 16 + fr] = re[r] * re[r] + im[r] * im[r];  // f64 C/D map: row fk + 4 r
  }
  __syncthreads();

  if (tid < kStoiBands * kStoiTileFrames) {
    const int band = tid / kStoiTileFrames, f = tid % kStoiTileFrames;
    const int64_t j = j0 + f;
    if (j < J) {
      double s = 0.0;
      for (int k = kStoiEdge[band]; k < kStoiEdge[band + 1]; ++k) s += pw[f * kStoiPw + k - kStoiBin0];
      bands[((sig * B + b) * kStoiBands + band) * Jmax + j] = sqrt(s);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ segments
// part[b][sb]: the sum over the 32 segments sb·32 .. of signal b.  Wave w takes segments sb·32 + 4 i + w, i = 0 .. 7.
template <bool EXT>
__global__ __launch_bounds__(kStoiThreads) void stoi_segments_kernel(const double* __restrict__ bands, const int* __restrict__ K, int64_t B, int64_t Jmax,
                                                                     int64_t sblocks, double clip1, double* __restrict__ part) {
  constexpr int kLd = kStoiSeg + 1, kWaves = kStoiThreads / kWave;
  __shared__ double sx[kWaves][kStoiBands * kLd], sy[kWaves][kStoiBands * kLd];
  __shared__ double wsum[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t id = blockIdx.x, sb = id % sblocks, b = id / sblocks;
  const int64_t Kb = K[b], J = Kb > 0 ? Kb - 1 : 0, nseg = J - (kStoiSeg - 1);
  if (sb * kStoiSegBlock >= nseg) return;
  const double* xb = bands + b * kStoiBands * Jmax;
  const double* yb = bands + (B + b) * kStoiBands * Jmax;
  double* px = sx[wave];
  double* py = sy[wave];
  double mine = 0.0;
  for (int it = 0; it < kStoiSegBlock / kWaves; ++it) {
    const int64_t s = sb * kStoiSegBlock + it * kWaves + wave;
    const bool active = s < nseg;
    if (active) {
      for (int i = lane; i < kStoiBands * kStoiSeg; i += kWave) {
        const int band = i / kStoiSeg, n = i % kStoiSeg;
        px[band * kLd + n] = xb[band * Jmax + s + n];
        py[band * kLd + n] = yb[band * Jmax + s + n];
      }
    }
    __syncthreads();
    if constexpr (EXT) {
      if (active && lane < 2 * kStoiBands) {  // rows: centre, then divide by the norm
        double* row = (lane < kStoiBands ? px : py) + (lane % kStoiBands) * kLd;
        double sum = 0.0, sq = 0.0;
        for (int n = 0; n < kStoiSeg; ++n) sum += row[n];
        const double mean = sum / kStoiSeg;
        for (int n = 0; n < kStoiSeg; ++n) {
          const double v = row[n] - mean;
          row[n] = v;
          sq = fma(v, v, sq);
        }
        const double norm = sqrt(sq);
        for (int n = 0; n < kStoiSeg; ++n) row[n] = row[n] / norm;
      }
      __syncthreads();
      if (active && (lane & 31) < kStoiSeg) {  // columns
        double* col = (lane < 32 ? px : py) + (lane & 31);
        double sum = 0.0, sq = 0.0;
        for (int k = 0; k < kStoiBands; ++k) sum += col[k * kLd];
        const double mean = sum / kStoiBands;
        for (int k = 0; k < kStoiBands; ++k) {
          const double v = col[k * kLd] - mean;
          col[k * kLd] = v;
          sq = fma(v, v, sq);
        }
        const double norm = sqrt(sq);
        for (int k = 0; k < kStoiBands; ++k) col[k * kLd] = col[k * kLd] / norm;
      }
      __syncthreads();
      if (active) {
        double v = 0.0;
        if (lane < kStoiSeg)
          for (int k = 0; k < kStoiBands; ++k) v += px[k * kLd + lane] * py[k * kLd + lane] / kStoiSeg;
        mine += wave_sum(v);
      }
    } else {
      if (active) {
        double v = 0.0;
        if (lane < kStoiBands) {
          const double* xr = px + lane * kLd;
          double* yr = py + lane * kLd;
          double xx = 0.0, yy = 0.0;
          for (int n = 0; n < kStoiSeg; ++n) {
            xx = fma(xr[n], xr[n], xx);
            yy = fma(yr[n], yr[n], yy);
          }
          const double scale = sqrt(xx) / (sqrt(yy) + kStoiEps);
          double sum_x = 0.0, sum_y = 0.0;
          for (int n = 0; n < kStoiSeg; ++n) {
            const double yp = stoi_min(yr[n] * scale, xr[n] * clip1);
            yr[n] = yp;
            sum_y += yp;
            sum_x += xr[n];
          }
          const double mx = sum_x / kStoiSeg, my = sum_y / kStoiSeg;
          double nx = 0.0, ny = 0.0;
          for (int n = 0; n < kStoiSeg; ++n) {
            const double a = xr[n] - mx, c = yr[n] - my;
            nx = fma(a, a, nx);
            ny = fma(c, c, ny);
          }
          nx = sqrt(nx) + kStoiEps, ny = sqrt(ny) + kStoiEps;
          for (int n = 0; n < kStoiSeg; ++n) v += ((yr[n] - my) / ny) * ((xr[n] - mx) / nx);
        }
        mine += wave_sum(v);
      }
    }
    __syncthreads();
  }
  if (lane == 0) wsum[wave] = mine;
  __syncthreads();
  if (tid == 0) part[b * sblocks + sb] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(kStoiThreads) void stoi_final_kernel(const double* __restrict__ part, const int* __restrict__ K, int64_t B, int64_t sblocks,
                                                                  bool extended, double* __restrict__ scores, int* __restrict__ frames) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kStoiThreads + threadIdx.x;
  if (b >= B) return;
  const int64_t Kb = K[b], J = Kb > 0 ? Kb - 1 : 0;
  frames[b] = static_cast<int>(J);
  if (J < kStoiSeg) {
    scores[b] = 1e-5;
    return;
  }
  const int64_t nseg = J - (kStoiSeg - 1), nb = (nseg + kStoiSegBlock - 1) / kStoiSegBlock;
  double s = 0.0;
  for (int64_t i = 0; i < nb; ++i) s += part[b * sblocks + i];
  scores[b] = extended ? s / static_cast<double>(nseg) : s / static_cast<double>(nseg * kStoiBands);
}

// ---------------------------------------------------------------------------------------------------------------- host
namespace {

template <typename F>
void stoi_dispatch(at::ScalarType dtype, const char* name, F&& f) {
  switch (dtype) {
    case at::kFloat: f(float{}); break;
    case at::kDouble: f(double{}); break;
    case at::kBFloat16: f(__hip_bfloat16{}); break;
    case at::kHalf: f(__half{}); break;
    default: TORCH_CHECK(false, name, ": unsupported dtype ", dtype);
  }
}

unsigned stoi_grid(int64_t n, const char* name) {
  TORCH_CHECK(n >= 1 && n <= INT32_MAX, name, ": too many workgroups for one launch");
  return static_cast<unsigned>(n);
}

struct StoiOut {
  at::Tensor scores, frames, bands;
};

StoiOut stoi_run(const char* name, const at::Tensor& preds_in, const at::Tensor& target_in, const at::Tensor& tables, const at::Tensor& filt, int64_t up,
                 int64_t down, int64_t pre_remove, bool extended, bool want_scores) {
  TORCH_CHECK(preds_in.is_cuda() && target_in.is_cuda() && tables.is_cuda(), name, ": expected GPU tensors");
  TORCH_CHECK(preds_in.device() == target_in.device() && tables.device() == preds_in.device(), name, ": tensors on different devices");
  TORCH_CHECK(preds_in.dim() == 2 && preds_in.sizes() == target_in.sizes(), name, ": expected matching [B, T]");
  TORCH_CHECK(preds_in.scalar_type() == target_in.scalar_type(), name, ": dtype mismatch");
  TORCH_CHECK(preds_in.size(0) >= 1 && preds_in.size(1) >= 1, name, ": empty input");
  TORCH_CHECK(tables.scalar_type() == at::kDouble && tables.is_contiguous() && tables.numel() == kStoiTables, name, ": expected ", kStoiTables,
              " fp64 table entries");
  TORCH_CHECK(up >= 1 && down >= 1 && pre_remove >= 0, name, ": bad resampling ratio");
  const bool resample = up != down;
  if (resample) {
    TORCH_CHECK(filt.is_cuda() && filt.device() == preds_in.device() && filt.scalar_type() == at::kDouble && filt.is_contiguous() && filt.numel() >= 1,
                name, ": expected a contiguous fp64 filter on the signals' device");
  }
  const at::DeviceGuard guard(preds_in.device());
  const auto dtype = preds_in.scalar_type();
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  const int64_t B = p.size(0), T = p.size(1);
  TORCH_CHECK(T <= (int64_t{1} << 40) / std::max<int64_t>(up, down), name, ": signal too long");
  const auto f64 = p.options().dtype(at::kDouble);
  const auto i32 = p.options().dtype(at::kInt);
  const double* tab = tables.data_ptr<double>();

  // stage 1: x = resampled[0], y = resampled[1] (fp64), or the inputs themselves at 10 kHz
  int64_t L = T;
  at::Tensor resampled;
  if (resample) {
    L = T * up / down + ((T * up) % down != 0);
    TORCH_CHECK(L >= 1, name, ": signal too short to resample");
    resampled = at::empty({2, B, L}, f64);
    const int64_t strips = (L + kStoiThreads - 1) / kStoiThreads;
    stoi_dispatch(dtype, name, [&](auto tag) {
      using S = decltype(tag);
      hipLaunchKernelGGL(stoi_resample_kernel<S>, dim3(stoi_grid(2 * B * strips, name)), dim3(kStoiThreads), 0, stream(),
                         reinterpret_cast<const S*>(t.data_ptr()), reinterpret_cast<const S*>(p.data_ptr()), filt.data_ptr<double>(),
                         resampled.data_ptr<double>(), B, T, L, strips, up, down, pre_remove, filt.numel());
    });
    TMX_LAUNCH_CHECK();
  }
  const int64_t F = L >= kStoiFrame ? (L - kStoiFrame) / kStoiHop + 1 : 0;  // source frames
  const int64_t Jmax = F > 0 ? F - 1 : 0;                                    // most STFT frames a signal can have
  TORCH_CHECK(F <= INT32_MAX, name, ": too many frames");

  auto K = at::zeros({B}, i32);
  at::Tensor bands = want_scores ? at::empty({2, B, kStoiBands, Jmax}, f64) : at::zeros({2, B, kStoiBands, Jmax}, f64);
  // every stage after the resampler reads x / y through one element type: fp64 when resampled
  auto with_signals = [&](auto&& f) {
    if (resample) f(static_cast<const double*>(resampled.data_ptr<double>()), static_cast<const double*>(resampled.data_ptr<double>()) + B * L);
    else stoi_dispatch(dtype, name, [&](auto tag) {
      using S = decltype(tag);
      f(reinterpret_cast<const S*>(t.data_ptr()), reinterpret_cast<const S*>(p.data_ptr()));
    });
  };

  if (F > 0) {
    auto e = at::empty({B, F}, f64);
    auto kept = at::empty({B, F}, i32);
    const int64_t fblocks = (F + kStoiThreads / kWave - 1) / (kStoiThreads / kWave);
    with_signals([&](auto* xs, auto* ys) {
      using S = std::remove_cv_t<std::remove_pointer_t<decltype(xs)>>;
      (void)ys;
      hipLaunchKernelGGL(stoi_energy_kernel<S>, dim3(stoi_grid(B * fblocks, name)), dim3(kStoiThreads), 0, stream(), xs, L, F, fblocks, tab,
                         e.data_ptr<double>());
    });
    TMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(stoi_keep_kernel, dim3(stoi_grid(B, name)), dim3(kStoiThreads), 0, stream(), e.data_ptr<double>(), F, kept.data_ptr<int>(),
                       K.data_ptr<int>());
    TMX_LAUNCH_CHECK();
    if (Jmax > 0) {
      const int64_t tiles = (Jmax + kStoiTileFrames - 1) / kStoiTileFrames;
      with_signals([&](auto* xs, auto* ys) {
        using S = std::remove_cv_t<std::remove_pointer_t<decltype(xs)>>;
        hipLaunchKernelGGL(stoi_bands_kernel<S>, dim3(stoi_grid(2 * B * tiles, name)), dim3(kStoiThreads), 0, stream(), xs, ys, L, kept.data_ptr<int>(),
                           K.data_ptr<int>(), F, tab, bands.data_ptr<double>(), B, Jmax, tiles);
      });
      TMX_LAUNCH_CHECK();
    }
  }

  StoiOut out;
  out.bands = bands;
  out.frames = at::empty({B}, i32);
  out.scores = at::empty({B}, f64);
  const int64_t maxseg = Jmax - (kStoiSeg - 1);
  const int64_t sblocks = maxseg > 0 ? (maxseg + kStoiSegBlock - 1) / kStoiSegBlock : 1;
  auto part = at::empty({B, sblocks}, f64);
  if (want_scores && maxseg > 0) {
    const double clip1 = 1.0 + std::pow(10.0, 15.0 / 20.0);
    auto kernel = extended ? stoi_segments_kernel<true> : stoi_segments_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(stoi_grid(B * sblocks, name)), dim3(kStoiThreads), 0, stream(), bands.data_ptr<double>(), K.data_ptr<int>(), B, Jmax,
                       sblocks, clip1, part.data_ptr<double>());
    TMX_LAUNCH_CHECK();
  }
  // without scores (stoi_bands) only frames is meaningful: the partials are in bounds but nobody wrote them
  hipLaunchKernelGGL(stoi_final_kernel, dim3(stoi_grid((B + kStoiThreads - 1) / kStoiThreads, name)), dim3(kStoiThreads), 0, stream(),
                     part.data_ptr<double>(), K.data_ptr<int>(), B, sblocks, extended, out.scores.data_ptr<double>(), out.frames.data_ptr<int>());
  TMX_LAUNCH_CHECK();
  return out;
}

}  // namespace

// (STFT frames per workgroup of the band kernel, segments per workgroup of the segment kernel, outputs per workgroup of the
// resampler, frames per strip of the kept-frame scan, frames per workgroup of the energy kernel)
std::vector<int64_t> stoi_tile() { return {kStoiTileFrames, kStoiSegBlock, kStoiThreads, kStoiThreads, kStoiThreads / kWave}; }

// scores fp64 [B] and frames int32 [B] (STFT frames J[b]) of preds / target [B, T].  tables: Hann window (256), cos and sin of
// 2 pi i / 512 (512 each), fp64.  filt: the padded, up-scaled polyphase filter (ignored when up == down); up / down reduced.
std::tuple<at::Tensor, at::Tensor> stoi_scores(const at::Tensor& preds, const at::Tensor& target, const at::Tensor& tables, const at::Tensor& filt, int64_t up,
                                               int64_t down, int64_t pre_remove, bool extended) {
  auto out = stoi_run("stoi_scores", preds, target, tables, filt, up, down, pre_remove, extended, true);
  return {out.scores, out.frames};
}

// the third-octave envelopes of stage 3: x_tob, y_tob fp64 [B, 15, Jmax] (zero past J[b]) and frames int32 [B]
std::tuple<at::Tensor, at::Tensor, at::Tensor> stoi_bands(const at::Tensor& preds, const at::Tensor& target, const at::Tensor& tables, const at::Tensor& filt,
                                                          int64_t up, int64_t down, int64_t pre_remove) {
  auto out = stoi_run("stoi_bands", preds, target, tables, filt, up, down, pre_remove, false, false);
  return {out.bands[0], out.bands[1], out.frames};
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("stoi_scores(Tensor preds, Tensor target, Tensor tables, Tensor filt, int up, int down, int pre_remove, bool extended) -> (Tensor, Tensor)");
  m.def("stoi_bands(Tensor preds, Tensor target, Tensor tables, Tensor filt, int up, int down, int pre_remove) -> (Tensor, Tensor, Tensor)");
  m.def("stoi_tile() -> int[]", &tmx::stoi_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("stoi_scores", &tmx::stoi_scores);
  m.impl("stoi_bands", &tmx::stoi_bands);
}
