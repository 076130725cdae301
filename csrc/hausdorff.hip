// Hausdorff distance between the boundaries of two segmentation masks for gfx950, per (sample, class) plane of H x W pixels:
//   E(M)       the pixels of M that are not interior (interior: the pixel and its four neighbours are in M; outside the plane is not in M),
//   h(A -> B)  max over a in E(A) of min over b in E(B) of d(a, b)   (max over nothing 0, min over nothing +inf),
// d euclidean, chessboard or taxicab on pixel offsets, optionally scaled by a spacing (sy, sx).  The result is h(preds -> target), or
// the larger of the two directions.
//
// The form is the separable exact one, not all pairs.  All three distances increase in |dy| for a fixed dx, so the nearest edge pixel
// of B to (y, x) is min over x' of f(|x - x'|, G_B[y, x']) with G_B[y, x'] the row distance from y to the nearest edge pixel of B in
// column x': an integer whatever the metric or spacing, 0 on an edge pixel, kHdNoEdge for a column without one.
//
// hausdorff_columns_kernel  (kernel 1) edges and column distances of both masks of a plane.  A workgroup takes kHdCols columns of one
//     plane, one lane per column, and splits the rows into kHdStrips strips, one wave each.  Membership is computed here (label == class
//     for the index form: every kept class reads the same label map, nothing is expanded).  A row's membership is a wave ballot, so the
//     edge test is 64-bit bit logic on ballots: left / right neighbours are the ballot shifted by one with the two halo columns (read
//     by lanes 0 .. 3) shifted in, up / down neighbours the ballots of the rows before and after, kept in registers; rows are
//     loaded kHdBatch at a time, every load of a wave 64 consecutive elements of a row.  The down sweep writes the strip-local distance
//     to the nearest edge above; each strip leaves its first and last edge distance per column in LDS, and because the column distance
//     is a min-plus scan those carries combine exactly.  The up sweep re-reads the strip bottom-up (an own value of 0 marks an edge
//     pixel), applies both carries and writes G as 16-bit integers.
// hausdorff_rows_kernel     (kernel 2) a workgroup takes kHdRows rows of a plane, one wave each.  The wave stages G_preds[y, :] and
//     G_target[y, :] in LDS and compacts the columns with G == 0 (the source pixels of the row) by ballot and prefix count, so lanes
//     are dense in sources; a row without a source pixel is done.  Each source scans outwards from its own column on both sides,
//     from best = f(0, G_B[y, x]), and stops when the dx term alone reaches best: exact, since f(dx, g) >= f(dx, 0) in all three
//     metrics.  A row of B without any edge column (B is empty) answers +inf without a scan.  Wave maximum, workgroup maximum, then
//     one atomicMax per workgroup and direction into the plane's word.  Without spacing the word is the integer squared distance
//     (euclidean) or the integer distance; with spacing it is the bit pattern of a non-negative float (the squared distance for
//     euclidean), which orders as an unsigned integer.  Both directions run in the same launch unless directed.
// hausdorff_finish_kernel   (kernel 3) words to fp32: all-ones word / +inf to inf, sqrt in fp64 then one rounding to fp32, the maximum of
//     the two directions.  A plane whose source mask is empty never touches its word: it stays 0.
//
// Arithmetic.  Without spacing everything up to the final sqrt is integer and exact: H, W <= 32767 keeps dy² + dx² below 2^31.  With
// spacing the scaled offsets, their squares and the sum are fp32, rounded once each, and the prune compares the rounded values
// (rounding is monotone, so the rounded candidate is never below the rounded dx term).  Integer maxima and integer atomics only:
// two runs are bit-equal.
//
// Cost bound.  Kernel 1 reads the masks once and writes, reads and writes 2 bytes per pixel and mask.  Kernel 2 is bounded by
// H · W · W LDS reads per plane and direction: the worst case is a full outline against a single far pixel, where every source
// scans its whole row before the dx term reaches best.  Masks whose boundaries are near each other stop after a few steps.
//
// Limits.  W <= kHdMaxW (the LDS rows of kernel 2), H <= kHdMaxH.  The scratch is 2 · planes · H · W 16-bit integers; planes are
// launched in chunks under TMX_HAUSDORFF_SCRATCH_MB (read per call, default 256) with offset pointers, and grids are flat on x, so
// plane counts beyond a 16-bit grid axis work.
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <limits>
#include <vector>

namespace tmx {

constexpr int kHdCols = kWave;     // columns of a workgroup of kernel 1: one lane each
constexpr int kHdStrips = 8;       // row strips of a column block: one wave each
constexpr int kHdBatch = 4;        // rows in flight per lane (their ballots live in SGPRs: 8 rows spilled them)
constexpr int kHdRows = 4;         // rows of a workgroup of kernel 2: one wave each
constexpr int kHdMaxW = 2048;      // kHdRows · 4 rows of 16-bit entries: 64 KiB of LDS
constexpr int kHdMaxH = 32767;
constexpr uint32_t kHdNoEdge = 0xFFFFu;  // G of a column without an edge pixel
constexpr int kHdFar = 1 << 20;          // "no edge" in the sweeps' int arithmetic: above every real distance, far from overflow
constexpr uint32_t kHdInfWord = 0xFFFFFFFFu;

enum HdMetric { kHdEuclidean = 0, kHdChessboard = 1, kHdTaxicab = 2 };

struct HdArgs {
  int64_t plane0, kept, c0, C;  // first plane of this chunk; planes are (sample, kept class), classes c0 .. C - 1
  int H, W, colblocks, directed;
  float sy, sx;
};

template <typename T, bool ONEHOT> __device__ __forceinline__ bool hd_member(T v, int c) {
  if (ONEHOT) return v != T(0);
  return static_cast<uint64_t>(static_cast<int64_t>(v)) == static_cast<uint64_t>(c);  // uint8 zero-extends, the signed types sign-extend
}

// ------------------------------------------------------------------------------------------- kernel 1: edges, column distances
template <typename TP, typename TT, bool ONEHOT>
__global__ __launch_bounds__(kHdCols* kHdStrips) void hausdorff_columns_kernel(const TP* __restrict__ preds, const TT* __restrict__ target,
                                                                                uint16_t* __restrict__ G, HdArgs a) {
  __shared__ int s_first[kHdStrips][2][kHdCols];  // per strip and mask: distance from the strip's first row down to its first edge pixel
  __shared__ int s_last[kHdStrips][2][kHdCols];   // ... and from its last row up to its last edge pixel (kHdFar: none)
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t local = static_cast<int64_t>(blockIdx.x) / a.colblocks;
  const int cb = static_cast<int>(static_cast<int64_t>(blockIdx.x) % a.colblocks);
  const int64_t plane = a.plane0 + local, b = plane / a.kept;
  const int c = static_cast<int>(a.c0 + plane % a.kept);
  const int64_t hw = static_cast<int64_t>(a.H) * a.W;
  const int64_t src = ONEHOT ? (b * a.C + c) * hw : b * hw;
  const TP* __restrict__ p = preds + src;
  const TT* __restrict__ t = target + src;
  uint16_t* __restrict__ gp = G + local * 2 * hw;
  uint16_t* __restrict__ gt = gp + hw;

  const int x = cb * kHdCols + lane;
  const bool in = x < a.W;
  // lanes 0 and 1 also read the column left / right of the block in preds, lanes 2 and 3 in target
  const int hx = (lane & 1) == 0 ? cb * kHdCols - 1 : cb * kHdCols + kHdCols;
  const bool halo = lane < 4 && hx >= 0 && hx < a.W, halo_p = halo && lane < 2, halo_t = halo && lane >= 2;
  const int rows = (a.H + kHdStrips - 1) / kHdStrips;
  const int y0 = min(a.H, wave * rows), y1 = min(a.H, y0 + rows);  // this wave's strip; empty when H is small

  int dp = kHdFar, dt = kHdFar, fp = kHdFar, ft = kHdFar;
  if (y0 < y1) {
    // rows y0 - 1 .. y1 stream through (previous, current, next) ballots; row n - 1 is finished when row n arrives
    uint64_t prev_p = 0, prev_t = 0, cur_p = 0, cur_t = 0, hz_p = 0, hz_t = 0;
    for (int n0 = y0 - 1; n0 <= y1; n0 += kHdBatch) {
      TP vp[kHdBatch], wp[kHdBatch];
      TT vt[kHdBatch], wt[kHdBatch];
#pragma unroll
      for (int j = 0; j < kHdBatch; ++j) {
        const int n = n0 + j;
        const bool row = n >= 0 && n < a.H && n <= y1;
        const int64_t at = static_cast<int64_t>(n) * a.W;
        vp[j] = row && in ? p[at + x] : TP(0);
        vt[j] = row && in ? t[at + x] : TT(0);
        wp[j] = row && halo_p ? p[at + hx] : TP(0);
        wt[j] = row && halo_t ? t[at + hx] : TT(0);
      }
#pragma unroll
      for (int j = 0; j < kHdBatch; ++j) {
        const int n = n0 + j;
        if (n <= y1) {
          const bool row = n >= 0 && n < a.H;
          const uint64_t next_p = __ballot(row && in && hd_member<TP, ONEHOT>(vp[j], c));
          const uint64_t next_t = __ballot(row && in && hd_member<TT, ONEHOT>(vt[j], c));
          // bit 0 / 1: left / right halo of preds, bit 2 / 3: of target
          const uint64_t side = __ballot(row && ((halo_p && hd_member<TP, ONEHOT>(wp[j], c)) || (halo_t && hd_member<TT, ONEHOT>(wt[j], c))));
          if (n - 1 >= y0) {
            const int y = n - 1;
            const uint64_t edge_p = cur_p & ~(hz_p & prev_p & next_p), edge_t = cur_t & ~(hz_t & prev_t & next_t);
            const bool ep = (edge_p >> lane) & 1, et = (edge_t >> lane) & 1;
            dp = ep ? 0 : min(dp + 1, kHdFar);
            dt = et ? 0 : min(dt + 1, kHdFar);
            if (ep && fp == kHdFar) fp = y - y0;
            if (et && ft == kHdFar) ft = y - y0;
            if (in) {
              const int64_t at = static_cast<int64_t>(y) * a.W + x;
              gp[at] = static_cast<uint16_t>(min(dp, static_cast<int>(kHdNoEdge)));
              gt[at] = static_cast<uint16_t>(min(dt, static_cast<int>(kHdNoEdge)));
            }
          }
          prev_p = cur_p, prev_t = cur_t, cur_p = next_p, cur_t = next_t;
          // members whose left and right neighbours are members
          hz_p = cur_p & ((cur_p << 1) | (side & 1)) & ((cur_p >> 1) | (((side >> 1) & 1) << 63));
          hz_t = cur_t & ((cur_t << 1) | ((side >> 2) & 1)) & ((cur_t >> 1) | (((side >> 3) & 1) << 63));
        }
      }
    }
  }
  s_last[wave][0][lane] = dp, s_last[wave][1][lane] = dt;
  s_first[wave][0][lane] = fp, s_first[wave][1][lane] = ft;
  __syncthreads();
  if (y0 >= y1) return;

  // carries: the distance from row y0 - 1 to the nearest edge above, and from row y1 to the nearest edge below
  int above_p = kHdFar, above_t = kHdFar, below_p = kHdFar, below_t = kHdFar;
#pragma unroll
  for (int v = 0; v < kHdStrips; ++v) {
    const int v0 = min(a.H, v * rows), v1 = min(a.H, v0 + rows);
    if (v < wave) {
      above_p = min(above_p, s_last[v][0][lane] + (y0 - v1));
      above_t = min(above_t, s_last[v][1][lane] + (y0 - v1));
    } else if (v > wave) {
      below_p = min(below_p, s_first[v][0][lane] + (v0 - y1));
      below_t = min(below_t, s_first[v][1][lane] + (v0 - y1));
    }
  }
  int up = min(below_p, kHdFar), ut = min(below_t, kHdFar);
  above_p = min(above_p, kHdFar), above_t = min(above_t, kHdFar);
  for (int yb = y1 - 1; yb >= y0; yb -= kHdBatch) {
    uint32_t rp[kHdBatch], rt[kHdBatch];
#pragma unroll
    for (int j = 0; j < kHdBatch; ++j) {
      const int y = yb - j;
      const bool row = y >= y0 && in;
      const int64_t at = static_cast<int64_t>(y) * a.W + x;
      rp[j] = row ? gp[at] : kHdNoEdge;
      rt[j] = row ? gt[at] : kHdNoEdge;
    }
#pragma unroll
    for (int j = 0; j < kHdBatch; ++j) {
      const int y = yb - j;
      if (y >= y0) {
        const int lp = rp[j] == kHdNoEdge ? kHdFar : static_cast<int>(rp[j]), lt = rt[j] == kHdNoEdge ? kHdFar : static_cast<int>(rt[j]);
        up = lp == 0 ? 0 : min(up + 1, kHdFar);
        ut = lt == 0 ? 0 : min(ut + 1, kHdFar);
        const int g_p = min(min(lp, above_p + (y - y0) + 1), up), g_t = min(min(lt, above_t + (y - y0) + 1), ut);
        if (in) {
          const int64_t at = static_cast<int64_t>(y) * a.W + x;
          gp[at] = static_cast<uint16_t>(min(g_p, static_cast<int>(kHdNoEdge)));
          gt[at] = static_cast<uint16_t>(min(g_t, static_cast<int>(kHdNoEdge)));
        }
      }
    }
  }
}

// --------------------------------------------------------------------------------------------- kernel 2: row envelope, maximum
// best over the row of B for the source pixel in column x.  Integer form: the squared distance (euclidean) or the distance.
template <int METRIC>
__device__ __forceinline__ uint32_t hd_scan_int(const uint16_t* __restrict__ gb, int x, int W) {
  const uint32_t g0 = gb[x];
  uint32_t best = g0 == kHdNoEdge ? kHdInfWord : (METRIC == kHdEuclidean ? g0 * g0 : g0);
  for (int dx = 1;; ++dx) {
    const uint32_t fx = METRIC == kHdEuclidean ? static_cast<uint32_t>(dx) * dx : static_cast<uint32_t>(dx);
    const int xl = x - dx, xr = x + dx;
    if (fx >= best || (xl < 0 && xr >= W)) break;
    if (xl >= 0) {
      const uint32_t g = gb[xl];
      if (g != kHdNoEdge) best = min(best, METRIC == kHdEuclidean ? fx + g * g : (METRIC == kHdChessboard ? max(fx, g) : fx + g));
    }
    if (xr < W) {
      const uint32_t g = gb[xr];
      if (g != kHdNoEdge) best = min(best, METRIC == kHdEuclidean ? fx + g * g : (METRIC == kHdChessboard ? max(fx, g) : fx + g));
    }
  }
  return best;
}

// fp32 form: scaled offsets, the squared distance for euclidean.  +inf when B has no edge pixel.
template <int METRIC> __device__ __forceinline__ float hd_combine(float fx, float fxx, uint32_t g, float sy) {
  const float fy = sy * static_cast<float>(g);
  return METRIC == kHdEuclidean ? fxx + fy * fy : (METRIC == kHdChessboard ? fmaxf(fx, fy) : fx + fy);
}

template <int METRIC>
__device__ __forceinline__ uint32_t hd_scan_f32(const uint16_t* __restrict__ gb, int x, int W, float sy, float sx) {
  const uint32_t g0 = gb[x];
  float best = g0 == kHdNoEdge ? std::numeric_limits<float>::infinity() : hd_combine<METRIC>(0.f, 0.f, g0, sy);
  for (int dx = 1;; ++dx) {
    const float fx = sx * static_cast<float>(dx), fxx = fx * fx;
    const int xl = x - dx, xr = x + dx;
    if ((METRIC == kHdEuclidean ? fxx : fx) >= best || (xl < 0 && xr >= W)) break;
    if (xl >= 0) {
      const uint32_t g = gb[xl];
      if (g != kHdNoEdge) best = fminf(best, hd_combine<METRIC>(fx, fxx, g, sy));
    }
    if (xr < W) {
      const uint32_t g = gb[xr];
      if (g != kHdNoEdge) best = fminf(best, hd_combine<METRIC>(fx, fxx, g, sy));
    }
  }
  return __float_as_uint(best);
}

__device__ __forceinline__ uint32_t hd_wave_max(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), off, kWave)));
  return v;
}

template <int METRIC, bool SPACED>
__global__ __launch_bounds__(kHdRows* kWave) void hausdorff_rows_kernel(const uint16_t* __restrict__ G, uint32_t* __restrict__ words, HdArgs a) {
  extern __shared__ uint16_t hd_lds[];  // per wave: G_preds row, G_target row, source columns of preds, source columns of target
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int W = a.W;
  const int64_t groups = (a.H + kHdRows - 1) / kHdRows;
  const int64_t local = static_cast<int64_t>(blockIdx.x) / groups;
  const int y = static_cast<int>(static_cast<int64_t>(blockIdx.x) % groups) * kHdRows + wave;
  const bool row = y < a.H;  // wave-uniform
  uint16_t* gs[2] = {hd_lds + static_cast<size_t>(wave) * 4 * W, hd_lds + (static_cast<size_t>(wave) * 4 + 1) * W};
  uint16_t* list[2] = {hd_lds + (static_cast<size_t>(wave) * 4 + 2) * W, hd_lds + (static_cast<size_t>(wave) * 4 + 3) * W};

  int count[2] = {0, 0};
  bool any[2] = {false, false};  // the mask has an edge pixel in some column: it is not empty
  if (row) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint16_t* __restrict__ src = G + ((local * 2 + s) * a.H + y) * W;
      for (int x0 = 0; x0 < W; x0 += kWave) {
        const int x = x0 + lane;
        const uint32_t g = x < W ? src[x] : kHdNoEdge;
        if (x < W) gs[s][x] = static_cast<uint16_t>(g);
        const uint64_t sources = __ballot(g == 0u);
        any[s] = any[s] || __ballot(g != kHdNoEdge) != 0;
        if (g == 0u) list[s][count[s] + __popcll(sources & ((uint64_t{1} << lane) - 1))] = static_cast<uint16_t>(x);
        count[s] += __popcll(sources);
      }
    }
  }
  __syncthreads();

  const int dirs = a.directed ? 1 : 2;  // direction 0: preds -> target, 1: target -> preds
  uint32_t most[2] = {0u, 0u};
  if (row) {
    for (int d = 0; d < dirs; ++d) {
      if (count[d] == 0) continue;  // no source pixel in this row
      if (!any[1 - d]) {
        most[d] = SPACED ? __float_as_uint(std::numeric_limits<float>::infinity()) : kHdInfWord;
        continue;
      }
      const uint16_t* __restrict__ gb = gs[1 - d];
      for (int i = lane; i < count[d]; i += kWave) {
        const int x = list[d][i];
        most[d] = max(most[d], SPACED ? hd_scan_f32<METRIC>(gb, x, W, a.sy, a.sx) : hd_scan_int<METRIC>(gb, x, W));
      }
    }
  }
  most[0] = hd_wave_max(most[0]);
  most[1] = hd_wave_max(most[1]);
  __syncthreads();  // every wave is done with its rows: the start of the LDS takes the waves' maxima
  uint32_t* part = reinterpret_cast<uint32_t*>(hd_lds);
  if (lane == 0) part[wave * 2] = most[0], part[wave * 2 + 1] = most[1];
  __syncthreads();
  if (threadIdx.x < dirs) {
    uint32_t m = 0u;
#pragma unroll
    for (int w = 0; w < kHdRows; ++w) m = max(m, part[w * 2 + threadIdx.x]);
    if (m != 0u) atomicMax(words + (a.plane0 + local) * 2 + threadIdx.x, m);
  }
}

// -------------------------------------------------------------------------------------------------- kernel 3: words to results
__global__ __launch_bounds__(256) void hausdorff_finish_kernel(const uint32_t* __restrict__ words, float* __restrict__ out, int64_t planes, int metric,
                                                               bool spaced, bool directed) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= planes) return;
  float r = 0.f;
  for (int d = 0; d < (directed ? 1 : 2); ++d) {
    const uint32_t w = words[i * 2 + d];
    float v;
    if (spaced) {
      const float f = __uint_as_float(w);
      v = metric == kHdEuclidean ? static_cast<float>(sqrt(static_cast<double>(f))) : f;
    } else if (w == kHdInfWord) {
      v = std::numeric_limits<float>::infinity();
    } else {
      v = metric == kHdEuclidean ? static_cast<float>(sqrt(static_cast<double>(w))) : static_cast<float>(w);
    }
    r = fmaxf(r, v);
  }
  out[i] = r;
}

// ------------------------------------------------------------------------------------------------------------------------ host
namespace {

template <typename F>
void hd_dispatch_label(at::ScalarType dtype, const char* name, F&& f) {
  switch (dtype) {
    case at::kByte: f(uint8_t{}); break;
    case at::kShort: f(int16_t{}); break;
    case at::kInt: f(int32_t{}); break;
    case at::kLong: f(int64_t{}); break;
    default: TORCH_CHECK(false, name, ": unsupported label dtype ", dtype);
  }
}

template <typename F>
void hd_dispatch_mask(at::ScalarType dtype, const char* name, F&& f) {
  switch (dtype) {
    case at::kBool:  // one byte, nonzero = member: the uint8 instantiation
    case at::kByte: f(uint8_t{}); break;
    case at::kInt: f(int32_t{}); break;
    case at::kLong: f(int64_t{}); break;
    default: TORCH_CHECK(false, name, ": unsupported mask dtype ", dtype);
  }
}

template <bool ONEHOT, typename F>
void hd_dispatch(at::ScalarType dtype, const char* name, F&& f) {
  if constexpr (ONEHOT) hd_dispatch_mask(dtype, name, std::forward<F>(f));
  else hd_dispatch_label(dtype, name, std::forward<F>(f));
}

// scratch cap of the column distances in bytes (TMX_HAUSDORFF_SCRATCH_MB, read per call: a test forces several chunks with it)
int64_t hd_scratch_bytes() {
  const char* e = std::getenv("TMX_HAUSDORFF_SCRATCH_MB");
  const long v = e ? std::atol(e) : 0;
  return static_cast<int64_t>(v > 0 ? std::min(v, 16384L) : 256) << 20;
}

template <int METRIC>
void hd_launch_rows(bool spaced, int64_t grid, size_t lds, const uint16_t* G, uint32_t* words, const HdArgs& a) {
  if (spaced) hipLaunchKernelGGL((hausdorff_rows_kernel<METRIC, true>), dim3(static_cast<unsigned>(grid)), dim3(kHdRows * kWave), lds, stream(), G, words, a);
  else hipLaunchKernelGGL((hausdorff_rows_kernel<METRIC, false>), dim3(static_cast<unsigned>(grid)), dim3(kHdRows * kWave), lds, stream(), G, words, a);
  TMX_LAUNCH_CHECK();
}

template <bool ONEHOT>
at::Tensor hausdorff_impl(const char* name, const at::Tensor& preds_in, const at::Tensor& target_in, int64_t num_classes, bool include_background,
                          int64_t metric, at::ArrayRef<double> spacing, bool directed) {
  TORCH_CHECK(preds_in.is_cuda() && target_in.is_cuda(), name, ": expected GPU tensors");
  TORCH_CHECK(preds_in.device() == target_in.device(), name, ": preds and target on different devices");
  TORCH_CHECK(preds_in.dim() == (ONEHOT ? 4 : 3) && preds_in.sizes() == target_in.sizes(), name, ": expected matching shapes ",
              ONEHOT ? "[B, C, H, W]" : "[B, H, W]");
  TORCH_CHECK(num_classes >= 1 && num_classes <= INT32_MAX, name, ": num_classes must be positive");
  TORCH_CHECK(!ONEHOT || preds_in.size(1) == num_classes, name, ": expected ", num_classes, " channels");
  const int64_t c0 = include_background ? 0 : 1, kept = num_classes - c0;
  TORCH_CHECK(kept >= 1, name, ": no class left");
  TORCH_CHECK(metric >= kHdEuclidean && metric <= kHdTaxicab, name, ": metric must be 0, 1 or 2");
  TORCH_CHECK(spacing.empty() || spacing.size() == 2, name, ": spacing must be empty or (sy, sx)");
  const bool spaced = !spacing.empty();
  const float sy = spaced ? static_cast<float>(spacing[0]) : 1.f, sx = spaced ? static_cast<float>(spacing[1]) : 1.f;
  TORCH_CHECK(sy > 0.f && sx > 0.f && sy <= std::numeric_limits<float>::max() && sx <= std::numeric_limits<float>::max(), name,
              ": spacing must be positive and finite");
  hd_dispatch<ONEHOT>(preds_in.scalar_type(), name, [](auto) {});
  hd_dispatch<ONEHOT>(target_in.scalar_type(), name, [](auto) {});
  const int64_t B = preds_in.size(0), H = preds_in.size(-2), W = preds_in.size(-1), planes = B * kept;
  TORCH_CHECK(H >= 1 && W >= 1, name, ": empty plane");
  TORCH_CHECK(H <= kHdMaxH && W <= kHdMaxW, name, ": plane of ", H, " x ", W, " exceeds ", kHdMaxH, " x ", kHdMaxW);
  const at::DeviceGuard guard(preds_in.device());
  auto out = at::empty({B, kept}, preds_in.options().dtype(at::kFloat));
  if (planes == 0) return out;
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  auto words = at::zeros({planes, 2}, preds_in.options().dtype(at::kInt));

  const int64_t colblocks = (W + kHdCols - 1) / kHdCols, groups = (H + kHdRows - 1) / kHdRows;
  const int64_t plane_bytes = 2 * H * W * static_cast<int64_t>(sizeof(uint16_t));
  int64_t per_chunk = std::max<int64_t>(1, hd_scratch_bytes() / plane_bytes);
  per_chunk = std::min({per_chunk, planes, INT32_MAX / colblocks, INT32_MAX / groups});
  auto scratch = at::empty({per_chunk * 2 * H * W}, preds_in.options().dtype(at::kShort));
  uint16_t* G = reinterpret_cast<uint16_t*>(scratch.data_ptr());
  uint32_t* wp = reinterpret_cast<uint32_t*>(words.data_ptr());
  const size_t lds = static_cast<size_t>(kHdRows) * 4 * W * sizeof(uint16_t);

  for (int64_t plane0 = 0; plane0 < planes; plane0 += per_chunk) {
    const int64_t n = std::min(per_chunk, planes - plane0);
    const HdArgs a{plane0, kept, c0, num_classes, static_cast<int>(H), static_cast<int>(W), static_cast<int>(colblocks), directed ? 1 : 0, sy, sx};
    hd_dispatch<ONEHOT>(p.scalar_type(), name, [&](auto ptag) {
      hd_dispatch<ONEHOT>(t.scalar_type(), name, [&](auto ttag) {
        using TP = decltype(ptag);
        using TT = decltype(ttag);
        hipLaunchKernelGGL((hausdorff_columns_kernel<TP, TT, ONEHOT>), dim3(static_cast<unsigned>(n * colblocks)), dim3(kHdCols * kHdStrips), 0, stream(),
                           reinterpret_cast<const TP*>(p.data_ptr()), reinterpret_cast<const TT*>(t.data_ptr()), G, a);
        TMX_LAUNCH_CHECK();
      });
    });
    if (metric == kHdEuclidean) hd_launch_rows<kHdEuclidean>(spaced, n * groups, lds, G, wp, a);
    else if (metric == kHdChessboard) hd_launch_rows<kHdChessboard>(spaced, n * groups, lds, G, wp, a);
    else hd_launch_rows<kHdTaxicab>(spaced, n * groups, lds, G, wp, a);
  }
  hipLaunchKernelGGL(hausdorff_finish_kernel, dim3(static_cast<unsigned>((planes + 255) / 256)), dim3(256), 0, stream(), wp, out.data_ptr<float>(), planes,
                     static_cast<int>(metric), spaced, directed);
  TMX_LAUNCH_CHECK();
  return out;
}

}  // namespace

// (columns per workgroup of kernel 1, row strips of a column block, rows in flight per lane, rows per workgroup of kernel 2, largest W,
// largest H): what the tests need to place their edge shapes
std::vector<int64_t> hausdorff_tile() { return {kHdCols, kHdStrips, kHdBatch, kHdRows, kHdMaxW, kHdMaxH}; }

// fp32 [B, C'] Hausdorff distances of the classes c0 .. C - 1 of label maps preds / target [B, H, W]
at::Tensor hausdorff_index(const at::Tensor& preds, const at::Tensor& target, int64_t num_classes, bool include_background, int64_t metric,
                           at::ArrayRef<double> spacing, bool directed) {
  return hausdorff_impl<false>("hausdorff_index", preds, target, num_classes, include_background, metric, spacing, directed);
}

// ... of one-hot masks preds / target [B, C, H, W], nonzero = member
at::Tensor hausdorff_onehot(const at::Tensor& preds, const at::Tensor& target, int64_t num_classes, bool include_background, int64_t metric,
                            at::ArrayRef<double> spacing, bool directed) {
  return hausdorff_impl<true>("hausdorff_onehot", preds, target, num_classes, include_background, metric, spacing, directed);
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("hausdorff_index(Tensor preds, Tensor target, int num_classes, bool include_background, int metric, float[] spacing, bool directed) -> Tensor");
  m.def("hausdorff_onehot(Tensor preds, Tensor target, int num_classes, bool include_background, int metric, float[] spacing, bool directed) -> Tensor");
  m.def("hausdorff_tile() -> int[]", &tmx::hausdorff_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("hausdorff_index", &tmx::hausdorff_index);
  m.impl("hausdorff_onehot", &tmx::hausdorff_onehot);
}
