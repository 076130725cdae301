// All-pairs contingency tables and nominal association scores for gfx950, behind cramers_v_matrix, tschuprows_t_matrix,
// pearsons_contingency_coefficient_matrix, theils_u_matrix, their pair functionals and the four modules' compute():
// no per-pair host loop, no unique / sort, no boolean-mask indexing.
//
//   nominal_labels       matrix [N, V] (int64 / int32 / fp32, read in place with its strides) -> uint8 labels in a column-major
//                        plane [V, pitch] (pitch = N rounded up to 16, so every column starts 16-byte aligned), one 64-bit presence
//                        mask per column and a flag word.  Label rule per element: NaN becomes nan_replace, or under drop_nan the
//                        sentinel kNomDrop; the value is then truncated toward zero as .long() does.  A kept label outside [0, 64)
//                        sets flag bit 0 (its byte is the sentinel).  The rows pitch - N of padding hold the sentinel.
//   nominal_pair_tables  tables[i, j, a, b] = #{rows: col_j == a and col_i == b} for i < j, int32 [V, V, K, K]; a row where either
//                        label is the sentinel, or not below K, is skipped for that pair.  A workgroup owns nom_pairs(K) pairs and
//                        one chunk of kNomRows rows: it counts into LDS with integer LDS adds and flushes its non-zero cells with
//                        integer global atomics (exact, order-independent: two runs are bit-equal).  A pair whose labels (from the
//                        two presence masks) all lie below k' < K counts into a k' x k' table replicated min(32, slot / k'²) times
//                        across the lanes (slot = max(K², 1024) counters, copy c of a cell at cell * copies + c: a copy is an LDS
//                        bank), so that few categories do not serialise on a handful of LDS addresses.
//   nominal_scores       tables [P, K, K] (int32 / int64 / fp32 counts, any strides: a transposed view is read in place) -> fp32
//                        [P].  One wave per table, fp64 from the exact counts: marginals, the numbers r / c of non-empty rows /
//                        columns (empty rows add nothing to any sum, so nothing is dropped), n, df = (r - 1)(c - 1); then
//                        χ² (0 at df == 0; at df == 1 with bias correction every count moves half a count toward its expectation),
//                        φ² = χ² / n and
//                          kind 0 Cramér's V    sqrt(φ² / min(r - 1, c - 1));
//                          kind 1 Tschuprow's T sqrt(φ² / sqrt((r - 1)(c - 1)));
//                               with bias correction φ²c = max(φ² - df / (n - 1), 0), rc = r - (r - 1)² / (n - 1), cc alike, in place of
//                               φ², r, c; min(rc, cc) == 1 writes NaN and sets flag bit 1;
//                          kind 2 Pearson's C   sqrt(φ² / (1 + φ²));      all three clamped to [0, 1];
//                          kind 3 Theil's U     (s_x - s_xy) / s_x, s_x = -Σ_b p_b ln p_b over the columns, s_xy = Σ p_ab ln(p_a / p_ab)
//                               over the non-zero cells (p_a: row marginal); exactly 0 where s_x == 0.
//                        The fp64 value is rounded once to fp32.  Sums across lanes use the fixed tree of wave_sum.
//
// No floating-point atomics anywhere.  Grids are flat on x and decoded in the kernel.
#include "common.h"

#include <algorithm>
#include <limits>
#include <tuple>
#include <vector>

namespace tmx {

constexpr int kNomThreads = 256;
constexpr int kNomCap = 64;                 // labels 0 .. 63: one presence bit each
constexpr int kNomDrop = 255;               // the byte of a dropped (or out-of-range) element
constexpr int64_t kNomRows = 16384;         // rows per chunk of the pair kernel
constexpr int kNomLdsInts = 16384;          // 64 KiB of LDS tables per workgroup: two workgroups per CU
constexpr int kNomMaxCopies = 32;           // one copy per LDS bank of a ds_add
constexpr int kNomLabelRows = 256;          // rows per workgroup of the label kernel
constexpr int kNomLabelCols = 32;           // columns per workgroup of the label kernel

constexpr int nom_slot(int K) { return std::max(K * K, 1024); }  // LDS ints of one pair: room for copies of a small table
constexpr int nom_pairs(int K) { return std::min(16, kNomLdsInts / nom_slot(K)); }

// ---------------------------------------------------------------------------------------------------------- labels
template <typename T> __device__ __forceinline__ int nom_label(T v, bool, float, bool&) {
  return (v >= 0 && v < kNomCap) ? static_cast<int>(v) : -1;
}
template <> __device__ __forceinline__ int nom_label<float>(float v, bool drop_nan, float nan_replace, bool& dropped) {
  if (v != v) {
    if (drop_nan) {
      dropped = true;
      return -1;
    }
    v = nan_replace;
  }
  return (v > -1.f && v < static_cast<float>(kNomCap)) ? static_cast<int>(v) : -1;  // (-1, 0) truncates to 0; NaN fails both
}

template <typename T>
__global__ __launch_bounds__(kNomThreads) void nominal_labels_kernel(const T* __restrict__ matrix, int64_t s0, int64_t s1, int64_t N, int64_t V,
                                                                     int64_t pitch, int64_t col_blocks, bool drop_nan, float nan_replace,
                                                                     uint8_t* __restrict__ labels, unsigned long long* __restrict__ masks,
                                                                     int* __restrict__ flags) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kNomLabelCols][kNomLabelRows];
  __shared__ unsigned long long present[kNomLabelCols];
  __shared__ int bad;
  const int64_t wg = blockIdx.x;
  const int64_t r0 = (wg / col_blocks) * kNomLabelRows, c0 = (wg % col_blocks) * kNomLabelCols;
  const int cols = static_cast<int>(min(static_cast<int64_t>(kNomLabelCols), V - c0));
  const int rows = static_cast<int>(min(static_cast<int64_t>(kNomLabelRows), N - r0));
  if (threadIdx.x < kNomLabelCols) present[threadIdx.x] = 0ull;
  if (threadIdx.x == 0) bad = 0;
  for (int e = threadIdx.x; e < kNomLabelCols * kNomLabelRows / 4; e += kNomThreads) reinterpret_cast<uint32_t*>(&tile[0][0])[e] = 0xffffffffu;
  __syncthreads();

  // consecutive threads take consecutive columns of a row: the rows of a row-major matrix are read coalesced
  for (int e = threadIdx.x; e < rows * cols; e += kNomThreads) {
    const int row = e / cols, col = e % cols;
    bool dropped = false;
    const int lab = nom_label<T>(matrix[(r0 + row) * s0 + (c0 + col) * s1], drop_nan, nan_replace, dropped);
    if (lab >= 0) {
      tile[col][row] = static_cast<uint8_t>(lab);
      const unsigned long long bit = 1ull << lab;
      // a stale read only costs one more OR
      if ((*reinterpret_cast<volatile unsigned long long*>(&present[col]) & bit) == 0) atomicOr(&present[col], bit);
    } else if (!dropped) {
      bad = 1;
    }
  }
  __syncthreads();

  // 16 rows of one column per store; pitch and r0 are multiples of 16, so a vector lies wholly below pitch or wholly past it
  for (int e = threadIdx.x; e < cols * (kNomLabelRows / 16); e += kNomThreads) {
    const int col = e / (kNomLabelRows / 16), v = e % (kNomLabelRows / 16);
    const int64_t row = r0 + v * 16;
    if (row < pitch) *reinterpret_cast<uint4*>(labels + (c0 + col) * pitch + row) = *reinterpret_cast<const uint4*>(&tile[col][v * 16]);
  }
  if (threadIdx.x < cols && present[threadIdx.x] != 0ull) atomicOr(&masks[c0 + threadIdx.x], present[threadIdx.x]);
  if (threadIdx.x == 0 && bad) atomicOr(flags, 1);
}

// ------------------------------------------------------------------------------------------------------ pair tables
__device__ __forceinline__ void nom_next_pair(int& i, int& j, int V) {
  if (++j == V) {
    ++i;
    j = i + 1;
  }
}

// log2 of the table extent a pair counts in: the least power of two >= 2 above every label of the union mask, at most K
template <int K> __device__ __forceinline__ int nom_extent_log2(unsigned long long m) {
  constexpr int kLog2K = K == 64 ? 6 : (K == 32 ? 5 : (K == 16 ? 4 : (K == 8 ? 3 : (K == 4 ? 2 : 1))));
  const int top = m == 0ull ? 0 : 64 - __clzll(static_cast<long long>(m));  // labels < top
  int lg = 1;
  while ((1 << lg) < top && lg < kLog2K) ++lg;
  return lg;
}

template <int K> __device__ __forceinline__ int nom_copies_log2(int lg) {
  int copies = nom_slot(K) >> (2 * lg), lc = 0;
  copies = copies > kNomMaxCopies ? kNomMaxCopies : copies;
  while ((1 << (lc + 1)) <= copies) ++lc;
  return lc;
}

template <int K>
__global__ __launch_bounds__(kNomThreads) void nominal_pair_tables_kernel(const uint8_t* __restrict__ labels, const unsigned long long* __restrict__ masks,
                                                                          int64_t pitch, int V, int64_t P, int64_t chunks, int* __restrict__ tables) {
  constexpr int PT = nom_pairs(K);
  constexpr int kSlot = nom_slot(K);
  __shared__ int counts[PT * kSlot];
  const int64_t wg = blockIdx.x;
  const int64_t chunk = wg % chunks, p0 = (wg / chunks) * PT;
  const int np = static_cast<int>(min(static_cast<int64_t>(PT), P - p0));

  // pair p0 of the list (0, 1), (0, 2), ..., (0, V - 1), (1, 2), ...: the same walk in every thread
  int i0 = 0;
  int64_t rest = p0;
  while (rest >= V - 1 - i0) {
    rest -= V - 1 - i0;
    ++i0;
  }
  const int j0 = i0 + 1 + static_cast<int>(rest);

  for (int e = threadIdx.x; e < np * kSlot; e += kNomThreads) counts[e] = 0;
  __syncthreads();

  const int64_t row_begin = chunk * kNomRows, row_end = min(pitch, row_begin + kNomRows);
  int i = i0, j = j0;
  for (int s = 0; s < np; ++s) {
    const int lg = nom_extent_log2<K>(masks[i] | masks[j]);
    const int lc = nom_copies_log2<K>(lg);
    const unsigned limit = 1u << lg;
    const unsigned copy = threadIdx.x & ((1u << lc) - 1u);
    int* slot = counts + s * kSlot;
    const uint8_t* ci = labels + static_cast<int64_t>(i) * pitch;
    const uint8_t* cj = labels + static_cast<int64_t>(j) * pitch;
    for (int64_t row = row_begin + threadIdx.x * 16; row < row_end; row += kNomThreads * 16) {
      const uint4 a = *reinterpret_cast<const uint4*>(ci + row);
      const uint4 b = *reinterpret_cast<const uint4*>(cj + row);
      const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned li = (aw[w] >> (8 * k)) & 0xffu, lj = (bw[w] >> (8 * k)) & 0xffu;
          // limit is a power of two: (li | lj) < limit exactly when both are; the sentinel fails it.  The index is below
          // 4^lg * 2^lc <= kSlot: inside this pair's slot
          if ((li | lj) < limit) atomicAdd(&slot[(((lj << lg) | li) << lc) | copy], 1);
        }
      }
    }
    nom_next_pair(i, j, V);
  }
  __syncthreads();

  i = i0, j = j0;
  for (int s = 0; s < np; ++s) {
    const int lg = nom_extent_log2<K>(masks[i] | masks[j]);
    const int lc = nom_copies_log2<K>(lg);
    const int* slot = counts + s * kSlot;
    int* out = tables + (static_cast<int64_t>(i) * V + j) * (K * K);
    for (int cell = threadIdx.x; cell < (1 << (2 * lg)); cell += kNomThreads) {
      int sum = 0;
      for (int c = 0; c < (1 << lc); ++c) sum += slot[(cell << lc) | c];
      if (sum != 0) atomicAdd(&out[(cell >> lg) * K + (cell & ((1 << lg) - 1))], sum);
    }
    nom_next_pair(i, j, V);
  }
}

// ----------------------------------------------------------------------------------------------------------- scores
enum NomKind { kNomCramers = 0, kNomTschuprows = 1, kNomPearson = 2, kNomTheils = 3 };

template <typename T>
__global__ __launch_bounds__(kWave) void nominal_scores_kernel(const T* __restrict__ tables, int64_t s0, int64_t s1, int64_t s2, int K, int kind,
                                                               bool bias, float* __restrict__ out, int* __restrict__ flags) {
  const T* t = tables + static_cast<int64_t>(blockIdx.x) * s0;
  const int lane = threadIdx.x;
  const bool live = lane < K;
  // lane l: the sum of column l (rows read coalesced) and the sum of row l
  double col = 0.0, row = 0.0;
  if (live) {
    for (int a = 0; a < K; ++a) col += static_cast<double>(t[a * s1 + lane * s2]);
    for (int b = 0; b < K; ++b) row += static_cast<double>(t[lane * s1 + b * s2]);
  }
  const double n = wave_sum(col);
  const double r = wave_sum(row != 0.0 ? 1.0 : 0.0), c = wave_sum(col != 0.0 ? 1.0 : 0.0);
  const double df = (r - 1.0) * (c - 1.0);
  double value;

  if (kind == kNomTheils) {
    double sx = (live && col != 0.0) ? -(col / n) * log(col / n) : 0.0;
    sx = wave_sum(sx);
    double sxy = 0.0;
    for (int a = 0; a < K; ++a) {
      const double pa = __shfl(row, a, kWave) / n;
      if (live) {
        const double cell = static_cast<double>(t[a * s1 + lane * s2]);
        if (cell != 0.0) sxy += (cell / n) * log(pa / (cell / n));
      }
    }
    sxy = wave_sum(sxy);
    value = sx == 0.0 ? 0.0 : (sx - sxy) / sx;
  } else {
    const bool correct = bias && kind != kNomPearson;
    double chi = 0.0;
    if (df != 0.0) {
      const bool shift = correct && df == 1.0;
      for (int a = 0; a < K; ++a) {
        const double ra = __shfl(row, a, kWave);
        if (live && ra != 0.0 && col != 0.0) {
          const double expected = ra * col / n;
          double cell = static_cast<double>(t[a * s1 + lane * s2]);
          if (shift) cell += expected > cell ? 0.5 : (expected < cell ? -0.5 : 0.0);
          chi += (cell - expected) * (cell - expected) / expected;
        }
      }
      chi = wave_sum(chi);
    }
    double phi = chi / n, rr = r, cc = c;
    bool unable = false;
    if (correct) {
      phi = fmax(phi - df / (n - 1.0), 0.0);
      rr = r - (r - 1.0) * (r - 1.0) / (n - 1.0);
      cc = c - (c - 1.0) * (c - 1.0) / (n - 1.0);
      unable = fmin(rr, cc) == 1.0;
    }
    if (unable) {
      value = std::numeric_limits<double>::quiet_NaN();
      if (lane == 0) atomicOr(flags, 2);
    } else {
      if (kind == kNomCramers) {
        value = sqrt(phi / fmin(rr - 1.0, cc - 1.0));
      } else if (kind == kNomTschuprows) {
        value = sqrt(phi / sqrt((rr - 1.0) * (cc - 1.0)));
      } else {
        value = sqrt(phi / (1.0 + phi));
      }
      value = value != value ? value : fmin(fmax(value, 0.0), 1.0);  // clamp keeps NaN
    }
  }
  if (lane == 0) out[blockIdx.x] = static_cast<float>(value);
}

// ------------------------------------------------------------------------------------------------------------- host
// (rows per chunk of the pair kernel, threads per workgroup, pairs per tile at K = 2, 4, 8, 16, 32, 64, the label cap)
std::vector<int64_t> nominal_tile() {
  return {kNomRows, kNomThreads, nom_pairs(2), nom_pairs(4), nom_pairs(8), nom_pairs(16), nom_pairs(32), nom_pairs(64), kNomCap};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> nominal_labels(const at::Tensor& matrix, bool drop_nan, double nan_replace) {
  const char* name = "nominal_labels";
  TORCH_CHECK(matrix.is_cuda(), name, ": expected a GPU tensor");
  TORCH_CHECK(matrix.dim() == 2 && matrix.numel() > 0, name, ": expected a non-empty [N, V] matrix");
  const auto dtype = matrix.scalar_type();
  TORCH_CHECK(dtype == at::kLong || dtype == at::kInt || dtype == at::kFloat, name, ": unsupported dtype ", dtype);
  const int64_t N = matrix.size(0), V = matrix.size(1);
  TORCH_CHECK(N < (int64_t{1} << 31), name, ": expected fewer than 2^31 rows");
  const at::DeviceGuard guard(matrix.device());
  const int64_t pitch = (N + 15) / 16 * 16;
  const int64_t row_blocks = (pitch + kNomLabelRows - 1) / kNomLabelRows, col_blocks = (V + kNomLabelCols - 1) / kNomLabelCols;
  TORCH_CHECK(row_blocks * col_blocks <= INT32_MAX, name, ": too many workgroups for one launch");

  auto plane = at::empty({V, pitch}, matrix.options().dtype(at::kByte));
  auto masks = at::zeros({V}, matrix.options().dtype(at::kLong));
  auto flags = at::zeros({1}, matrix.options().dtype(at::kInt));
  auto launch = [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(nominal_labels_kernel<T>, dim3(static_cast<unsigned>(row_blocks * col_blocks)), dim3(kNomThreads), 0, stream(),
                       reinterpret_cast<const T*>(matrix.data_ptr()), matrix.stride(0), matrix.stride(1), N, V, pitch, col_blocks, drop_nan,
                       static_cast<float>(nan_replace), plane.data_ptr<uint8_t>(), reinterpret_cast<unsigned long long*>(masks.data_ptr<int64_t>()),
                       flags.data_ptr<int>());
    TMX_LAUNCH_CHECK();
  };
  if (dtype == at::kLong) launch(int64_t{});
  else if (dtype == at::kInt) launch(int32_t{});
  else launch(float{});
  return {plane.narrow(1, 0, N), masks, flags};
}

at::Tensor nominal_pair_tables(const at::Tensor& labels, const at::Tensor& masks, int64_t K) {
  const char* name = "nominal_pair_tables";
  TORCH_CHECK(labels.is_cuda() && masks.is_cuda() && labels.device() == masks.device(), name, ": expected GPU tensors on one device");
  TORCH_CHECK(labels.dim() == 2 && labels.scalar_type() == at::kByte && labels.numel() > 0, name, ": expected non-empty uint8 labels [V, N]");
  const int64_t V = labels.size(0), N = labels.size(1), pitch = labels.stride(0);
  TORCH_CHECK(V >= 2 && V <= INT32_MAX && N < (int64_t{1} << 31), name, ": expected at least two columns and fewer than 2^31 rows");
  TORCH_CHECK(labels.stride(1) == 1 && pitch % 16 == 0 && pitch >= N && pitch - N < 16 && (reinterpret_cast<uintptr_t>(labels.data_ptr()) & 15) == 0,
              name, ": expected the label plane of nominal_labels (16-byte aligned columns, padded with the drop byte)");
  TORCH_CHECK(masks.dim() == 1 && masks.size(0) == V && masks.scalar_type() == at::kLong && masks.is_contiguous(), name, ": expected int64 masks [V]");
  TORCH_CHECK(K == 2 || K == 4 || K == 8 || K == 16 || K == 32 || K == 64, name, ": K must be one of 2, 4, 8, 16, 32, 64");
  const at::DeviceGuard guard(labels.device());
  const int64_t P = V * (V - 1) / 2, chunks = (pitch + kNomRows - 1) / kNomRows;
  auto tables = at::zeros({V, V, K, K}, labels.options().dtype(at::kInt));
  auto launch = [&](auto k) {
    constexpr int K_ = decltype(k)::value;
    const int64_t tiles = (P + nom_pairs(K_) - 1) / nom_pairs(K_);
    TORCH_CHECK(tiles * chunks <= INT32_MAX, name, ": too many workgroups for one launch");
    hipLaunchKernelGGL(nominal_pair_tables_kernel<K_>, dim3(static_cast<unsigned>(tiles * chunks)), dim3(kNomThreads), 0, stream(),
                       labels.data_ptr<uint8_t>(), reinterpret_cast<const unsigned long long*>(masks.data_ptr<int64_t>()), pitch, static_cast<int>(V),
                       P, chunks, tables.data_ptr<int>());
    TMX_LAUNCH_CHECK();
  };
  switch (K) {
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 8: launch(std::integral_constant<int, 8>{}); break;
    case 16: launch(std::integral_constant<int, 16>{}); break;
    case 32: launch(std::integral_constant<int, 32>{}); break;
    default: launch(std::integral_constant<int, 64>{}); break;
  }
  return tables;
}

std::tuple<at::Tensor, at::Tensor> nominal_scores(const at::Tensor& tables, int64_t kind, bool bias_correction) {
  const char* name = "nominal_scores";
  TORCH_CHECK(tables.is_cuda(), name, ": expected a GPU tensor");
  TORCH_CHECK(tables.dim() == 3 && tables.size(1) == tables.size(2) && tables.numel() > 0, name, ": expected non-empty tables [P, K, K]");
  TORCH_CHECK(tables.size(2) <= kNomCap, name, ": at most ", kNomCap, " categories");
  TORCH_CHECK(kind >= 0 && kind <= 3, name, ": kind must be 0 (Cramer's V), 1 (Tschuprow's T), 2 (Pearson's C) or 3 (Theil's U)");
  const auto dtype = tables.scalar_type();
  TORCH_CHECK(dtype == at::kInt || dtype == at::kLong || dtype == at::kFloat, name, ": unsupported dtype ", dtype);
  const int64_t P = tables.size(0);
  TORCH_CHECK(P <= INT32_MAX, name, ": too many tables for one launch");
  const at::DeviceGuard guard(tables.device());
  auto out = at::empty({P}, tables.options().dtype(at::kFloat));
  auto flags = at::zeros({1}, tables.options().dtype(at::kInt));
  auto launch = [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(nominal_scores_kernel<T>, dim3(static_cast<unsigned>(P)), dim3(kWave), 0, stream(), reinterpret_cast<const T*>(tables.data_ptr()),
                       tables.stride(0), tables.stride(1), tables.stride(2), static_cast<int>(tables.size(2)), static_cast<int>(kind), bias_correction,
                       out.data_ptr<float>(), flags.data_ptr<int>());
    TMX_LAUNCH_CHECK();
  };
  if (dtype == at::kInt) launch(int32_t{});
  else if (dtype == at::kLong) launch(int64_t{});
  else launch(float{});
  return {out, flags};
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("nominal_labels(Tensor matrix, bool drop_nan, float nan_replace) -> (Tensor, Tensor, Tensor)");
  m.def("nominal_pair_tables(Tensor labels, Tensor masks, int K) -> Tensor");
  m.def("nominal_scores(Tensor tables, int kind, bool bias_correction) -> (Tensor, Tensor)");
  m.def("nominal_tile() -> int[]", &tmx::nominal_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("nominal_labels", &tmx::nominal_labels);
  m.impl("nominal_pair_tables", &tmx::nominal_pair_tables);
  m.impl("nominal_scores", &tmx::nominal_scores);
}
