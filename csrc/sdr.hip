// signal_distortion_ratio (the chain functional/audio/sdr.py states) for gfx950: preds / target [G, S, T] (fp32 / bf16 / fp16, read in
// place), fp64 arithmetic on the up-cast samples, no FFT, no full-size temporary, nothing read to the host, no atomics.
//
// Only the first L = filter_length lags of the correlations are used, so they are summed directly:
//   r[k] = Σ_n t~[n] t~[n + k],  c[k] = Σ_n t~[n] p~[n + k]  (k < L),  pp = Σ p~²,   t~ = t − mean(t), p~ = p − mean(p) when zero_mean
// (irfft(conj(T) P)[k] of the composition: the target is the unshifted factor).  A product of two fp32 values is exact in fp64.
// The composition's normalisation is linear and is applied to the sums: s_t = 1 / max(sqrt(r[0]), 1e-6), s_p = 1 / max(sqrt(pp), 1e-6),
// r <- r s_t², b = c s_t s_p, r[0] += load_diag.
//
// Passes:
//   M (zero_mean)  sdr_mean_kernel: fp64 chunk sums of every signal, sdr_mean_fold_kernel adds them in chunk order and divides by T.
//   C              sdr_corr_kernel, the hot path.  A "series" q of target j is the target itself (q = 0: autocorrelation) or a pred
//                  (q >= 1: cross-correlation); PAIR_DIAGONAL has Q = 2 series per target, PAIR_ALL Q = S + 1, so a target's
//                  autocorrelation is summed once whatever S is.  Grid: flat over (g, j, q, lag tile, chunk).  A workgroup stages 2048
//                  centred samples of the target and 2048 + 64 of the series (the halo of the lag tile; zeros past T) in LDS as fp64,
//                  in a [8][264] layout (sample m at row m % 8, column m / 8; 264 = 8 mod 32, so both the staging stores and the
//                  reads below are free of bank conflicts).  Wave w owns lags 16 w .. 16 w + 15 of the 64-lag tile; a lane takes 8
//                  consecutive samples t~[n .. n + 8) and the window x~[n + k .. n + k + 23) into registers and issues 128 v_fma_f64 on
//                  31 LDS reads.  The 16 accumulators of a lane are added over the wave by a fixed butterfly and written to
//                  part[g][j][q][chunk][lag]; slot L of a row holds Σ x~² of the chunk (lag tile 0, wave 0).
//                  sdr_corr_mfma_kernel is the same pass on v_mfma_f64_16x16x4_f64 in tiles of 256 lags (see there); it is taken for
//                  T >= 16384 when the filter fills 3/4 of its tiles (sdr_use_mfma), the measured winner there.
//   fold           sdr_fold_kernel adds the chunk partials in chunk order (skipped when there is one chunk).
//   S              sdr_solve_kernel: one workgroup per target and batch of NR <= 8 right-hand sides: scaling, load_diag, the Levinson
//                  recursion with r, the Durbin vector y and x in LDS (x[k] takes b[k]'s place when step k is done), coh = Σ b x and
//                  10 log10(coh / (1 − coh)).  The two dot products of a step (and the NR of the right-hand sides) read the state
//                  the step starts from, so they share one reduction: two barriers per step, none that waits on another wave when
//                  L <= 512 (one wave, 2 or 8 elements per lane; 256 threads above that).  A step issues all its LDS loads before
//                  the first use and reduces inside the wave with DPP row operations and one lane read, not with LDS shuffles.
//                  The Durbin vector depends on r only: in PAIR_ALL one recursion serves the S (up to 8, or what LDS holds) preds
//                  of a target.  Always L − 1 steps: a zero or NaN system ends with NaN.
// Every sum runs in an order that depends on the shape alone (sdr_chunks): two runs are bit-equal, and an entry of the pair matrix
// has the bits of the diagonal call on that pair when both chunk alike.
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

namespace tmx {

constexpr int kSdrThreads = 256;
constexpr int kSdrJ = 8;                                          // consecutive samples a lane holds
constexpr int kSdrR = 16;                                         // adjacent lags a lane holds
constexpr int kSdrWin = kSdrJ + kSdrR - 1;                        // the window of the series a lane holds
constexpr int kSdrLagTile = (kSdrThreads / kWave) * kSdrR;        // 64 lags per workgroup
constexpr int kSdrBlock = kWave * kSdrJ;                          // 512 samples per wave step
constexpr int kSdrStage = kSdrThreads * kSdrJ;                    // 2048 samples staged at a time
constexpr int kSdrCols = (kSdrStage + kSdrLagTile) / kSdrJ;       // 264 columns of the [8][264] LDS layout
constexpr int kSdrLoads = (kSdrStage + kSdrLagTile + kSdrThreads - 1) / kSdrThreads;  // staging loads per thread
constexpr int kSdrSeriesTile = 1;                                 // series of a target per workgroup of sdr_corr_kernel: 2 measured slower
constexpr int64_t kSdrMfmaMinT = 16384;                           // the matrix-core form of pass C takes signals from this length on ...
constexpr int kSdrMfmaUse = 3;                                    // ... whose filter fills 3/4 or more of its 256-lag tiles
constexpr int64_t kSdrTargetGroups = 2048;                       // signals are split into chunks until the grid has about this many workgroups
constexpr int kSdrPer = 8;                                        // elements per thread the solve kernel covers
constexpr int kSdrPerShort = 2;                                   // ... for filters up to 128 taps
constexpr int kSdrMaxL = kSdrThreads * kSdrPer;                   // 2048: the filter_length cap (3 L fp64 = 48 KB of LDS)
constexpr int kSdrWaveL = kWave * kSdrPer;                        // 512: up to here the solve runs in one wave
constexpr int kSdrMaxRhs = 8;
constexpr int64_t kSdrSolveLds = 60 * 1024;

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "csrc/sdr.hip: the row_bcast DPP controls of sdr_wave_sum_rows and the fp64 MFMA exist on GFX9 (CDNA) targets only"
#endif

static_assert(kSdrR % kSdrJ == 0 && kSdrCols % 32 == 8, "the LDS layout of sdr_corr_kernel");

template <typename S> __device__ __forceinline__ double sdr_ld(const S* __restrict__ p, int64_t i) { return static_cast<double>(to_f32<S>(p[i])); }

__device__ __forceinline__ double sdr_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// ------------------------------------------------------------------------------------------------------------------ pass M
// part[sig][chunk], sig = 0 .. 2 nsig − 1 (preds, then target)
template <typename S>
__global__ __launch_bounds__(kSdrThreads) void sdr_mean_kernel(const S* __restrict__ preds, const S* __restrict__ target, int64_t nsig, int64_t T,
                                                               int64_t per, int64_t chunks, double* __restrict__ part) {
  __shared__ double red[kSdrThreads / kWave];
  const int64_t id = blockIdx.x, chunk = id % chunks, sig = id / chunks;
  const S* src = sig < nsig ? preds + sig * T : target + (sig - nsig) * T;
  const int64_t c0 = chunk * per, c1 = min(T, c0 + per);
  double s = 0.0;
  for (int64_t n = c0 + threadIdx.x; n < c1; n += kSdrThreads) s += sdr_ld<S>(src, n);
  s = sdr_wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[id] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kSdrThreads) void sdr_mean_fold_kernel(const double* __restrict__ part, int64_t nsig2, int64_t chunks, double T,
                                                                    double* __restrict__ mean) {
  const int64_t sig = static_cast<int64_t>(blockIdx.x) * kSdrThreads + threadIdx.x;
  if (sig >= nsig2) return;
  double s = 0.0;
  for (int64_t c = 0; c < chunks; ++c) s += part[sig * chunks + c];
  mean[sig] = s / T;
}

// ------------------------------------------------------------------------------------------------------------------ pass C
struct SdrCorr {
  int64_t S, T, Q, L, q_tiles, lag_tiles, per, chunks, nsig;
  int pairing;
  const double* mean;  // [2][nsig] (preds, then target) or null
  double* part;        // [G S Q][chunks][L + 1]
};

// E series of one target per workgroup: the target's chunk is staged once for all of them.  A series computes the same sums in
// the same order whatever E is.  E = 2 holds 240 VGPRs and 50 688 bytes of LDS against 148 and 33 792 (two waves per SIMD, not three)
// and measured 8 to 26 % slower at L = 512 (README), so only E = kSdrSeriesTile = 1 is instantiated.
template <typename S, int E>
__global__ __launch_bounds__(kSdrThreads) void sdr_corr_kernel(const S* __restrict__ preds, const S* __restrict__ target, SdrCorr a) {
  __shared__ double ts[kSdrJ * kSdrCols];
  __shared__ double xs[E][kSdrJ * kSdrCols];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t id = blockIdx.x;
  const int64_t chunk = id % a.chunks;
  id /= a.chunks;
  const int64_t k0 = (id % a.lag_tiles) * kSdrLagTile;
  id /= a.lag_tiles;
  const int64_t q0 = (id % a.q_tiles) * E, sig_t = id / a.q_tiles;  // sig_t = g S + j
  const S* tp = target + sig_t * a.T;
  const double mt = a.mean != nullptr ? a.mean[a.nsig + sig_t] : 0.0;
  const S* xp[E];
  double mx[E];
  bool on[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {  // a series past the last reads the target again and writes nothing
    const int64_t q = q0 + e;
    on[e] = q < a.Q;
    const bool pred = on[e] && q > 0;
    const int64_t sig_p = a.pairing == 1 ? (sig_t / a.S) * a.S + (pred ? q - 1 : 0) : sig_t;
    xp[e] = pred ? preds + sig_p * a.T : tp;
    mx[e] = a.mean != nullptr ? (pred ? a.mean[sig_p] : mt) : 0.0;
  }
  const int64_t c0 = chunk * a.per, c1 = min(a.T, c0 + a.per);
  // this wave's window starts at x~[n]: it also sums x~² over the chunk (for the target's own series that repeats r[0]; it keeps
  // every slot of a row defined for the fold)
  const bool norm = k0 == 0 && wave == 0;

  double acc[E][kSdrR], pp[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    pp[e] = 0.0;
#pragma unroll
    for (int j = 0; j < kSdrR; ++j) acc[e][j] = 0.0;
  }

  for (int64_t s0 = c0; s0 < c1; s0 += kSdrStage) {
    double tv[kSdrLoads], xv[E][kSdrLoads];
#pragma unroll
    for (int u = 0; u < kSdrLoads; ++u) {
      const int m = tid + u * kSdrThreads;
      const int64_t n = s0 + m, nx = n + k0;
      tv[u] = (m < kSdrStage && n < c1) ? sdr_ld<S>(tp, n) - mt : 0.0;
#pragma unroll
      for (int e = 0; e < E; ++e) xv[e][u] = (m < kSdrStage + kSdrLagTile && nx < a.T) ? sdr_ld<S>(xp[e], nx) - mx[e] : 0.0;
    }
    __syncthreads();  // the previous stage has been consumed
#pragma unroll
    for (int u = 0; u < kSdrLoads; ++u) {
      const int m = tid + u * kSdrThreads;
      if (m < kSdrStage + kSdrLagTile) {
        const int at = (m & (kSdrJ - 1)) * kSdrCols + (m >> 3);
        ts[at] = tv[u];  // columns 256 .. 263 of ts are zeros nobody reads
#pragma unroll
        for (int e = 0; e < E; ++e) xs[e][at] = xv[e][u];
      }
    }
    __syncthreads();
    const int blocks = static_cast<int>(min(static_cast<int64_t>(kSdrStage / kSdrBlock), (c1 - s0 + kSdrBlock - 1) / kSdrBlock));
    for (int blk = 0; blk < blocks; ++blk) {
      const int col = blk * kWave + lane;
      double t8[kSdrJ];
#pragma unroll
      for (int i = 0; i < kSdrJ; ++i) t8[i] = ts[i * kSdrCols + col];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        double xw[kSdrWin];
#pragma unroll
        for (int i = 0; i < kSdrWin; ++i) xw[i] = xs[e][(i & (kSdrJ - 1)) * kSdrCols + col + (kSdrR / kSdrJ) * wave + (i >> 3)];
#pragma unroll
        for (int i = 0; i < kSdrJ; ++i) {
#pragma unroll
          for (int j = 0; j < kSdrR; ++j) acc[e][j] = fma(t8[i], xw[i + j], acc[e][j]);
        }
        if (norm) {
          const int64_t n = s0 + static_cast<int64_t>(col) * kSdrJ;
#pragma unroll
          for (int i = 0; i < kSdrJ; ++i) pp[e] = fma(n + i < c1 ? xw[i] : 0.0, xw[i], pp[e]);
        }
      }
    }
  }

#pragma unroll
  for (int e = 0; e < E; ++e) {
    double* dst = a.part + ((sig_t * a.Q + (on[e] ? q0 + e : q0)) * a.chunks + chunk) * (a.L + 1);
#pragma unroll
    for (int j = 0; j < kSdrR; ++j) {
      const double s = sdr_wave_sum(acc[e][j]);
      const int64_t k = k0 + wave * kSdrR + j;
      if (lane == 0 && on[e] && k < a.L) dst[k] = s;
    }
    if (norm) {
      const double s = sdr_wave_sum(pp[e]);
      if (lane == 0 && on[e]) dst[a.L] = s;
    }
  }
}

// The matrix-core form of pass C: one series of one target, a tile of 256 lags, a chunk.  With m = n + v,
//   D[u][v] = Σ_m x~[m + k0 + 16 u] t~[m − v]  is the sum of lag k0 + 16 u + v,
// a product A[u][m] B[m][v] that v_mfma_f64_16x16x4_f64 takes four values of m at a time: lane l = (i = l & 15, kk = l >> 4) hands it
// A = x~[m0 + kk + k0 + 16 i] and B = t~[m0 + kk − i] and holds D[(l >> 4) + 4 reg][l & 15].  A stage of 2048 values of m sits in LDS:
// t~ with a back halo of 15 samples (zeros outside the chunk), x~ with a forward halo of 240, one pad value after every 16 so that the
// 16 rows of A, 128 bytes apart, fall on different banks.  A wave takes a quarter of the stage into two accumulators (even and odd
// steps); the four waves' tiles are added through LDS in wave order.  Σ x~² (slot L) is summed while x~ is staged, lag tile 0 only.
typedef double sdr_d4 __attribute__((ext_vector_type(4)));
constexpr int kSdrMfmaLags = 256;
constexpr int kSdrMfmaBack = 15;
constexpr int kSdrMfmaT = kSdrStage + kSdrMfmaBack;          // staged target values
constexpr int kSdrMfmaX = kSdrStage + kSdrMfmaLags - 16;     // staged series values: m + 16 u up to 2047 + 240
constexpr int kSdrMfmaSteps = kSdrStage / (kSdrThreads / kWave) / 4;  // 128 instructions per wave and stage

__device__ __forceinline__ int sdr_mfma_pad(int j) { return j + (j >> 4); }

template <typename S>
__global__ __launch_bounds__(kSdrThreads) void sdr_corr_mfma_kernel(const S* __restrict__ preds, const S* __restrict__ target, SdrCorr a) {
  __shared__ double tl[kSdrMfmaT + 1];
  __shared__ double xl[kSdrMfmaX + kSdrMfmaX / 16 + 2];
  static_assert(kSdrMfmaX + kSdrMfmaX / 16 + 2 >= 4 * kSdrMfmaLags && kSdrMfmaT >= kSdrThreads / kWave, "the reductions reuse the staging buffers");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t id = blockIdx.x;
  const int64_t chunk = id % a.chunks;
  id /= a.chunks;
  const int64_t k0 = (id % a.lag_tiles) * kSdrMfmaLags;
  id /= a.lag_tiles;
  const int64_t q = id % a.Q, sig_t = id / a.Q;
  const int64_t sig_p = a.pairing == 1 ? (sig_t / a.S) * a.S + (q > 0 ? q - 1 : 0) : sig_t;
  const S* tp = target + sig_t * a.T;
  const S* xp = q == 0 ? tp : preds + sig_p * a.T;
  const double mt = a.mean != nullptr ? a.mean[a.nsig + sig_t] : 0.0;
  const double mx = a.mean != nullptr ? (q == 0 ? mt : a.mean[sig_p]) : 0.0;
  const int64_t c0 = chunk * a.per, c1 = min(a.T, c0 + a.per);
  const bool norm = k0 == 0;

  sdr_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  double pp = 0.0;
  const int i = lane & 15, kk = lane >> 4;
  const int ja = (kSdrStage / 4) * wave + kk + 16 * i;             // this lane's A value of step 0, before padding
  const int jb = (kSdrStage / 4) * wave + kk - i + kSdrMfmaBack;   // and its B value

  for (int64_t s0 = c0; s0 < c1 + kSdrMfmaBack; s0 += kSdrStage) {
    __syncthreads();  // the previous stage has been consumed
    for (int j = tid; j < kSdrMfmaT; j += kSdrThreads) {
      const int64_t n = s0 - kSdrMfmaBack + j;
      tl[j] = (n >= c0 && n < c1) ? sdr_ld<S>(tp, n) - mt : 0.0;
    }
    for (int j = tid; j < kSdrMfmaX; j += kSdrThreads) {
      const int64_t n = s0 + j, nx = n + k0;
      const double v = nx < a.T ? sdr_ld<S>(xp, nx) - mx : 0.0;
      xl[sdr_mfma_pad(j)] = v;
      if (norm && j < kSdrStage && n < c1) pp = fma(v, v, pp);
    }
    __syncthreads();
    if (s0 + (kSdrStage / 4) * wave < c1 + kSdrMfmaBack) {  // (wave-uniform) a quarter past the chunk holds zeros only
#pragma unroll 8
      for (int s = 0; s < kSdrMfmaSteps; s += 2) {
        const double a0 = xl[sdr_mfma_pad(ja + 4 * s)], b0 = tl[jb + 4 * s];
        const double a1 = xl[sdr_mfma_pad(ja + 4 * s + 4)], b1 = tl[jb + 4 * s + 4];
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
      }
    }
  }

  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) xl[wave * kSdrMfmaLags + 16 * (kk + 4 * r) + i] = acc0[r] + acc1[r];
  pp = sdr_wave_sum(pp);
  if (lane == 0) tl[wave] = pp;
  __syncthreads();
  double* dst = a.part + ((sig_t * a.Q + q) * a.chunks + chunk) * (a.L + 1);
  const double s = ((xl[tid] + xl[kSdrMfmaLags + tid]) + xl[2 * kSdrMfmaLags + tid]) + xl[3 * kSdrMfmaLags + tid];
  if (k0 + tid < a.L) dst[k0 + tid] = s;
  if (norm && tid == 0) dst[a.L] = ((tl[0] + tl[1]) + tl[2]) + tl[3];
}

// rc[row][slot] = Σ_chunk part[row][chunk][slot], chunks in order
__global__ __launch_bounds__(kSdrThreads) void sdr_fold_kernel(const double* __restrict__ part, int64_t rows, int64_t chunks, int64_t slots,
                                                               double* __restrict__ rc) {
  const int64_t o = static_cast<int64_t>(blockIdx.x) * kSdrThreads + threadIdx.x;
  if (o >= rows * slots) return;
  const int64_t row = o / slots, slot = o % slots;
  double s = 0.0;
  for (int64_t c = 0; c < chunks; ++c) s += part[(row * chunks + c) * slots + slot];
  rc[o] = s;
}

// ------------------------------------------------------------------------------------------------------------------ pass S
struct SdrSolve {
  int64_t S, Q, L, batches, npred;
  int pairing;
  bool has_diag;
  double load_diag;
  const double* rc;  // [G S Q][L + 1]
  double* out;       // PAIR_DIAGONAL [G S], PAIR_ALL [G S(target) S(preds)]
};

// one step of a reduction inside a row of 16 lanes: the value of the lane the DPP control names (every lane has a source)
template <int CTRL>
__device__ __forceinline__ double sdr_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// as sdr_dpp for a control that writes the rows of ROWS only: the other rows read 0
template <int CTRL, int ROWS>
__device__ __forceinline__ double sdr_dpp_rows(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xf, false);
  return __hiloint2double(hi, lo);
}

// The sum over the wave, the same bits in every lane, without an LDS round trip per step (the recursion waits on it 511 times):
// lane ^ 1, lane ^ 2, the mirrored half row and the mirrored row bring every lane the sum of its row of 16 (a + b == b + a, so the
// lanes of a row agree); row_bcast:15 adds row 0 to row 1 and row 2 to row 3, row_bcast:31 adds rows 0 + 1 to row 3, and lane 63's
// (r3 + r2) + (r1 + r0) is read into a scalar: two SGPRs per value, where reading the four row sums took eight.  Every lane must be active.
__device__ __forceinline__ double sdr_wave_sum_rows(double v) {
  v += sdr_dpp<0xB1>(v);              // quad_perm [1, 0, 3, 2]
  v += sdr_dpp<0x4E>(v);              // quad_perm [2, 3, 0, 1]
  v += sdr_dpp<0x141>(v);             // row_half_mirror
  v += sdr_dpp<0x140>(v);             // row_mirror
  v += sdr_dpp_rows<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v += sdr_dpp_rows<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  double total = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
  asm volatile("" : "+v"(total));  // lives on in vector registers: nine uniform sums held as scalars made the 8-right-hand-side forms spill SGPRs
  return total;
}

// the sums of v[0 .. N) over the workgroup, the same bits in every thread; ends with every thread past a barrier
template <int NT, int N>
__device__ __forceinline__ void sdr_block_sum(double (&v)[N], double* red) {
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = sdr_wave_sum_rows(v[n]);
  if constexpr (NT > kWave) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();  // red is free again
    if (lane == 0) {
#pragma unroll
      for (int n = 0; n < N; ++n) red[wave * N + n] = v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) {
      double s = red[n];
#pragma unroll
      for (int w = 1; w < NT / kWave; ++w) s += red[w * N + n];
      v[n] = s;
    }
  } else {
    __syncthreads();
  }
}

// Dynamic LDS: r[L] (off-diagonals over the diagonal), y[L], x[NR][L] (holds b over the diagonal until the step that solves it).
// A thread covers PER elements of a dot product: L <= NT PER.
template <int NT, int NR, int PER>
__global__ __launch_bounds__(NT) void sdr_solve_kernel(SdrSolve a) {
  extern __shared__ double smem[];
  __shared__ double red[(NT / kWave) * (NR + 1)];
  const int64_t L = a.L;
  double* r = smem;
  double* y = r + L;
  double* x = y + L;
  const int tid = threadIdx.x;
  const int64_t batch = static_cast<int64_t>(blockIdx.x) % a.batches, sig_t = static_cast<int64_t>(blockIdx.x) / a.batches;
  const int64_t i0 = batch * NR;
  const int nr = static_cast<int>(min(static_cast<int64_t>(NR), a.npred - i0));
  const int64_t slots = L + 1;
  const double* rrow = a.rc + sig_t * a.Q * slots;
  const double st = 1.0 / fmax(sqrt(rrow[0]), 1e-6);
  const double r0 = rrow[0] * st * st + (a.has_diag ? a.load_diag : 0.0);
  // row of right-hand side e (one past the last repeats the batch's first and is not written) and its scale s_t s_p; both are
  // worked out where they are used, before and after the recursion, so that the loop carries neither
  // (fmax returns 1e-6 for a NaN sum where torch.clamp keeps the NaN: the NaN still arrives, through the sums r[0] or c[0] it came from)
  auto rhs_row = [&](int e) { return a.rc + (sig_t * a.Q + 1 + i0 + (e < nr ? e : 0)) * slots; };
  auto rhs_scale = [&](const double* row) { return st * (1.0 / fmax(sqrt(row[L]), 1e-6)); };
  for (int64_t i = tid; i < L; i += NT) {
    r[i] = rrow[i] * st * st / r0;
    y[i] = 0.0;
  }
#pragma unroll 1
  for (int e = 0; e < NR; ++e) {
    const double* crow = rhs_row(e);
    const double bs = rhs_scale(crow);
    for (int64_t i = tid; i < L; i += NT) x[e * L + i] = crow[i] * bs / r0;
  }
  __syncthreads();
  double beta = 1.0;
  double alpha = L > 1 ? -r[1] : 0.0;
  __syncthreads();
  if (tid == 0 && L > 1) y[0] = alpha;
  __syncthreads();
  // 0-based Levinson recursion on the unit-diagonal system: step k extends the solutions from order k to k + 1
  for (int64_t k = 1; k < L; ++k) {
    beta = (1.0 - alpha * alpha) * beta;
    double v[NR + 1];  // Σ_{i<k} r[i+1] x_e[k-1-i] for every right-hand side, then Σ_{i<k} r[i+1] y[k-1-i]
    double bk[NR];
#pragma unroll
    for (int n = 0; n <= NR; ++n) v[n] = 0.0;
#pragma unroll
    for (int e = 0; e < NR; ++e) bk[e] = x[e * L + k];
    // every load of the step is issued before the first use (an element past k reads element 0's operands and adds nothing)
    double rv[PER], yv[PER], xv[PER][NR];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int64_t i = tid + u * NT, ii = i < k ? i : 0;
      rv[u] = r[ii + 1];
      yv[u] = y[k - 1 - ii];
#pragma unroll
      for (int e = 0; e < NR; ++e) xv[u][e] = x[e * L + k - 1 - ii];
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const bool live = tid + u * NT < k;
#pragma unroll
      for (int e = 0; e < NR; ++e) v[e] = live ? fma(rv[u], xv[u][e], v[e]) : v[e];
      v[NR] = live ? fma(rv[u], yv[u], v[NR]) : v[NR];
    }
    sdr_block_sum<NT, NR + 1>(v, red);
    const bool more = k < L - 1;
    const double an = more ? (-r[k + 1] - v[NR]) / beta : 0.0;
    double mu[NR];
#pragma unroll
    for (int e = 0; e < NR; ++e) mu[e] = (bk[e] - v[e]) / beta;
    // (every thread read the state before the barriers of the sum)  the pair (i, k-1-i) belongs to one thread: x takes the old y, y its mirrored old self
    // (the middle element is its own mirror: both stores of a pair then write the same value to the same place)
    constexpr int HALF = (PER + 1) / 2;
    double yi[HALF], yj[HALF], xi[HALF][NR], xj[HALF][NR];
#pragma unroll
    for (int u = 0; u < HALF; ++u) {
      const int64_t i = tid + u * NT, ii = i < (k + 1) / 2 ? i : 0, j = k - 1 - ii;
      yi[u] = y[ii], yj[u] = y[j];
#pragma unroll
      for (int e = 0; e < NR; ++e) xi[u][e] = x[e * L + ii], xj[u][e] = x[e * L + j];
    }
#pragma unroll
    for (int u = 0; u < HALF; ++u) {
      const int64_t i = tid + u * NT, j = k - 1 - i;
      if (i < (k + 1) / 2) {
#pragma unroll
        for (int e = 0; e < NR; ++e) {
          x[e * L + i] = fma(mu[e], yj[u], xi[u][e]);
          x[e * L + j] = fma(mu[e], yi[u], xj[u][e]);
        }
        if (more) {
          y[i] = fma(an, yj[u], yi[u]);
          y[j] = fma(an, yi[u], yj[u]);
        }
      }
    }
    if (tid == 0) {
#pragma unroll
      for (int e = 0; e < NR; ++e) x[e * L + k] = mu[e];
      if (more) y[k] = an;
    }
    alpha = an;
    __syncthreads();
  }
  double coh[NR];
#pragma unroll
  for (int e = 0; e < NR; ++e) {
    const double* crow = rhs_row(e);
    const double bs = rhs_scale(crow);
    double c = 0.0;
    for (int64_t i = tid; i < L; i += NT) c = fma(crow[i] * bs, x[e * L + i], c);
    coh[e] = c;
  }
  sdr_block_sum<NT, NR>(coh, red);
  if (tid == 0) {
#pragma unroll
    for (int e = 0; e < NR; ++e) {
      if (e < nr) {
        const double val = 10.0 * log10(coh[e] / (1.0 - coh[e]));
        if (a.pairing == 1) a.out[sig_t * a.S + i0 + e] = val;
        else a.out[sig_t] = val;
      }
    }
  }
}

// --------------------------------------------------------------------------------------------------------------------- host
namespace {

struct SdrGeometry {
  int64_t Q, lag_tiles, rows, per, chunks;  // rows: (g, j, q, lag tile) workgroup rows of the grid
};

// TMX_SDR_CHUNK (samples per chunk, read per call) overrides the chunk length: it lets a test place chunk edges inside a short signal.
SdrGeometry sdr_geometry(int64_t G, int64_t S, int64_t T, int64_t L, int64_t pairing) {
  SdrGeometry geo;
  geo.Q = pairing == 1 ? S + 1 : 2;
  geo.lag_tiles = (L + kSdrLagTile - 1) / kSdrLagTile;
  geo.rows = G * S * geo.Q * geo.lag_tiles;
  geo.per = 0;
  if (const char* env = std::getenv("TMX_SDR_CHUNK")) {
    const long long v = std::atoll(env);
    if (v > 0) geo.per = std::min<int64_t>(v, int64_t{1} << 40);
  }
  if (geo.per == 0) {
    const int64_t want = std::max<int64_t>(1, (kSdrTargetGroups + geo.rows - 1) / geo.rows);
    const int64_t most = std::max<int64_t>(1, T / kSdrStage);
    const int64_t n = std::min(want, most);
    geo.per = ((T + n - 1) / n + kSdrStage - 1) / kSdrStage * kSdrStage;
  }
  geo.chunks = (T + geo.per - 1) / geo.per;
  return geo;
}

void sdr_check(const at::Tensor& preds, const at::Tensor& target, int64_t L, int64_t pairing, const char* name) {
  TORCH_CHECK(preds.is_cuda() && target.is_cuda(), name, ": expected GPU tensors");
  TORCH_CHECK(preds.device() == target.device(), name, ": preds and target on different devices");
  TORCH_CHECK(preds.dim() == 3 && preds.sizes() == target.sizes(), name, ": expected matching [G, S, T]");
  TORCH_CHECK(preds.scalar_type() == target.scalar_type(), name, ": dtype mismatch");
  const auto dtype = preds.scalar_type();
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16 || dtype == at::kHalf, name, ": unsupported dtype ", dtype);
  TORCH_CHECK(preds.numel() > 0, name, ": empty input");
  TORCH_CHECK(L >= 1 && L <= kSdrMaxL, name, ": filter_length must be in [1, ", kSdrMaxL, "]");
  TORCH_CHECK(pairing == 0 || pairing == 1, name, ": pairing must be 0 (diagonal) or 1 (all pairs)");
}

// The form of pass C, from the filter and the signal length alone (what a diagonal call and a pair-matrix call on the same signals
// share, so both take the same form): the matrix-core kernel measured 0.64 to 0.69 of the VALU kernel's time where its 256-lag tiles
// are full and the signals long, and more than it at L = 64 (a quarter of a tile) and at T = 8000 (too few workgroups).
bool sdr_use_mfma(int64_t L, int64_t T) {
  const int64_t tiles = (L + kSdrMfmaLags - 1) / kSdrMfmaLags;
  return T >= kSdrMfmaMinT && 4 * L >= kSdrMfmaUse * tiles * kSdrMfmaLags;
}

unsigned sdr_grid(int64_t n, const char* name) {
  TORCH_CHECK(n >= 1 && n <= INT32_MAX, name, ": too many workgroups for one launch");
  return static_cast<unsigned>(n);
}

// the folded lag sums rc [G S Q][L + 1]: row (g, j, q), slots 0 .. L − 1 the lags and slot L = Σ x~² of the series
at::Tensor sdr_lag_sums(const at::Tensor& preds_in, const at::Tensor& target_in, int64_t L, bool zero_mean, int64_t pairing, const SdrGeometry& geo,
                        const char* name) {
  const int64_t G = preds_in.size(0), S = preds_in.size(1), T = preds_in.size(2), nsig = G * S;
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  const auto f64 = p.options().dtype(at::kDouble);
  const int64_t rows = nsig * geo.Q, slots = L + 1;
  const int64_t q_tiles = (geo.Q + kSdrSeriesTile - 1) / kSdrSeriesTile;
  const unsigned nwg = sdr_grid(nsig * q_tiles * geo.lag_tiles * geo.chunks, name);
  sdr_grid(rows * slots, name);
  // slot L of a row is written by lag tile 0 only and every lag below L by exactly one wave: nothing to clear
  auto rc = at::empty({rows, slots}, f64);
  at::Tensor part = geo.chunks == 1 ? rc : at::empty({rows * geo.chunks, slots}, f64);
  at::Tensor mean;
  if (zero_mean) {
    const int64_t want = std::max<int64_t>(1, (kSdrTargetGroups + 2 * nsig - 1) / (2 * nsig));
    const int64_t n = std::min(want, std::max<int64_t>(1, T / (2 * kSdrStage)));
    const int64_t mper = (T + n - 1) / n, mchunks = (T + mper - 1) / mper;
    mean = at::empty({2 * nsig}, f64);
    auto mpart = at::empty({2 * nsig * mchunks}, f64);
    const unsigned mgrid = sdr_grid(2 * nsig * mchunks, name);
    dispatch_float3(p.scalar_type(), name, [&](auto tag) {
      using T_ = decltype(tag);
      hipLaunchKernelGGL(sdr_mean_kernel<T_>, dim3(mgrid), dim3(kSdrThreads), 0, stream(), reinterpret_cast<const T_*>(p.data_ptr()),
                         reinterpret_cast<const T_*>(t.data_ptr()), nsig, T, mper, mchunks, mpart.data_ptr<double>());
    });
    TMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdr_mean_fold_kernel, dim3(sdr_grid((2 * nsig + kSdrThreads - 1) / kSdrThreads, name)), dim3(kSdrThreads), 0, stream(),
                       mpart.data_ptr<double>(), 2 * nsig, mchunks, static_cast<double>(T), mean.data_ptr<double>());
    TMX_LAUNCH_CHECK();
  }
  SdrCorr a{S, T, geo.Q, L, q_tiles, geo.lag_tiles, geo.per, geo.chunks, nsig, static_cast<int>(pairing),
            zero_mean ? mean.data_ptr<double>() : nullptr, part.data_ptr<double>()};
  // TMX_SDR_CORR_FORM (valu or mfma, read per call) forces a form: the A/B switch of tools/sdr_bench.py and of the tests
  bool mfma = sdr_use_mfma(L, T);
  if (const char* env = std::getenv("TMX_SDR_CORR_FORM")) mfma = std::string(env) == "mfma" ? true : (std::string(env) == "valu" ? false : mfma);
  if (mfma) {
    a.q_tiles = geo.Q;
    a.lag_tiles = (L + kSdrMfmaLags - 1) / kSdrMfmaLags;
    const unsigned mgrid = sdr_grid(nsig * geo.Q * a.lag_tiles * geo.chunks, name);
    dispatch_float3(p.scalar_type(), name, [&](auto tag) {
      using T_ = decltype(tag);
      hipLaunchKernelGGL(sdr_corr_mfma_kernel<T_>, dim3(mgrid), dim3(kSdrThreads), 0, stream(), reinterpret_cast<const T_*>(p.data_ptr()),
                         reinterpret_cast<const T_*>(t.data_ptr()), a);
    });
  } else {
    dispatch_float3(p.scalar_type(), name, [&](auto tag) {
      using T_ = decltype(tag);
      hipLaunchKernelGGL((sdr_corr_kernel<T_, kSdrSeriesTile>), dim3(nwg), dim3(kSdrThreads), 0, stream(), reinterpret_cast<const T_*>(p.data_ptr()),
                         reinterpret_cast<const T_*>(t.data_ptr()), a);
    });
  }
  TMX_LAUNCH_CHECK();
  if (geo.chunks > 1) {
    hipLaunchKernelGGL(sdr_fold_kernel, dim3(sdr_grid((rows * slots + kSdrThreads - 1) / kSdrThreads, name)), dim3(kSdrThreads), 0, stream(),
                       part.data_ptr<double>(), rows, geo.chunks, slots, rc.data_ptr<double>());
    TMX_LAUNCH_CHECK();
  }
  return rc;
}

template <int NT, int NR, int PER>
void sdr_solve_launch(unsigned grid, size_t shmem, const SdrSolve& a) {
  hipLaunchKernelGGL((sdr_solve_kernel<NT, NR, PER>), dim3(grid), dim3(NT), shmem, stream(), a);
  TMX_LAUNCH_CHECK();
}

template <int NT, int PER>
void sdr_solve_rhs(int nr, unsigned grid, size_t shmem, const SdrSolve& a) {
  switch (nr) {
    case 1: sdr_solve_launch<NT, 1, PER>(grid, shmem, a); break;
    case 2: sdr_solve_launch<NT, 2, PER>(grid, shmem, a); break;
    case 4: sdr_solve_launch<NT, 4, PER>(grid, shmem, a); break;
    default: sdr_solve_launch<NT, kSdrMaxRhs, PER>(grid, shmem, a); break;
  }
}

}  // namespace

// (lags per workgroup of pass C, adjacent lags per lane, samples staged at a time, the filter_length cap, the longest filter the solve
// runs in one wave, right-hand sides one recursion serves at most, lags per workgroup of the matrix-core form of pass C, the signal
// length from which it is used): what the tests size their shapes by
std::vector<int64_t> sdr_tile() { return {kSdrLagTile, kSdrR, kSdrStage, kSdrMaxL, kSdrWaveL, kSdrMaxRhs, kSdrMfmaLags, kSdrMfmaMinT}; }

// How many chunks pass C splits every signal of a [G, S, T] call into: a function of the shape, the filter length and the pairing alone
// (and of TMX_SDR_CHUNK where a test sets it).  Only the last chunk may be short.
int64_t sdr_chunks(int64_t G, int64_t S, int64_t T, int64_t L, int64_t pairing) {
  TORCH_CHECK(G >= 1 && S >= 1 && T >= 1 && L >= 1 && L <= kSdrMaxL && (pairing == 0 || pairing == 1),
              "sdr_chunks: expected a non-empty shape, 1 <= filter_length <= ", kSdrMaxL, " and a pairing in 0 .. 1");
  return sdr_geometry(G, S, T, L, pairing).chunks;
}

// The folded raw lag sums before any scaling: r [G, S, L], c [G, S, L] (pairing 0) or [G, S(target), S(preds), L] (pairing 1), pp [G, S].
std::tuple<at::Tensor, at::Tensor, at::Tensor> sdr_correlations(const at::Tensor& preds, const at::Tensor& target, int64_t L, bool zero_mean,
                                                                int64_t pairing) {
  const char* name = "sdr_correlations";
  sdr_check(preds, target, L, pairing, name);
  const at::DeviceGuard guard(preds.device());
  const int64_t G = preds.size(0), S = preds.size(1), T = preds.size(2);
  const SdrGeometry geo = sdr_geometry(G, S, T, L, pairing);
  auto rc = sdr_lag_sums(preds, target, L, zero_mean, pairing, geo, name).view({G, S, geo.Q, L + 1});
  auto r = rc.select(2, 0).narrow(2, 0, L).contiguous();
  if (pairing == 1) return {r, rc.narrow(2, 1, S).narrow(3, 0, L).contiguous(), rc.select(1, 0).narrow(1, 1, S).select(2, L).contiguous()};
  return {r, rc.select(2, 1).narrow(2, 0, L).contiguous(), rc.select(2, 1).select(2, L).contiguous()};
}

// fp64 SDR in dB of preds / target [G, S, T].  pairing 0: [G, S], the pairs (p_s, t_s); 1: [G, S, S] with
// out[g, j, i] = SDR(preds[g, i], target[g, j]).
at::Tensor sdr_scores(const at::Tensor& preds, const at::Tensor& target, int64_t L, bool zero_mean, c10::optional<double> load_diag, int64_t pairing) {
  const char* name = "sdr_scores";
  sdr_check(preds, target, L, pairing, name);
  const at::DeviceGuard guard(preds.device());
  const int64_t G = preds.size(0), S = preds.size(1), T = preds.size(2);
  const SdrGeometry geo = sdr_geometry(G, S, T, L, pairing);
  auto rc = sdr_lag_sums(preds, target, L, zero_mean, pairing, geo, name);
  const auto f64 = rc.options();
  at::Tensor out = pairing == 1 ? at::empty({G, S, S}, f64) : at::empty({G, S}, f64);
  const int64_t npred = pairing == 1 ? S : 1;
  int nr = 1;  // right-hand sides per recursion: the largest of 1, 2, 4, 8 that the preds of a target and LDS ask for
  while (nr < kSdrMaxRhs && nr < npred && (2 + 2 * nr) * L * static_cast<int64_t>(sizeof(double)) <= kSdrSolveLds) nr *= 2;
  const int64_t batches = (npred + nr - 1) / nr;
  const size_t shmem = static_cast<size_t>((2 + nr) * L) * sizeof(double);
  SdrSolve a{S, geo.Q, L, batches, npred, static_cast<int>(pairing), load_diag.has_value(), load_diag.value_or(0.0), rc.data_ptr<double>(),
             out.data_ptr<double>()};
  const unsigned grid = sdr_grid(G * S * batches, name);
  if (L <= kWave * kSdrPerShort) sdr_solve_rhs<kWave, kSdrPerShort>(nr, grid, shmem, a);
  else if (L <= kSdrWaveL) sdr_solve_rhs<kWave, kSdrPer>(nr, grid, shmem, a);
  else sdr_solve_rhs<kSdrThreads, kSdrPer>(nr, grid, shmem, a);
  return out;
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("sdr_scores(Tensor preds, Tensor target, int filter_length, bool zero_mean, float? load_diag, int pairing) -> Tensor");
  m.def("sdr_correlations(Tensor preds, Tensor target, int filter_length, bool zero_mean, int pairing) -> (Tensor, Tensor, Tensor)");
  m.def("sdr_chunks(int G, int S, int T, int filter_length, int pairing) -> int", &tmx::sdr_chunks);
  m.def("sdr_tile() -> int[]", &tmx::sdr_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("sdr_scores", &tmx::sdr_scores);
  m.impl("sdr_correlations", &tmx::sdr_correlations);
}
