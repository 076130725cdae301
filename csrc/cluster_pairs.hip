// Extrinsic clustering scores (mutual information, NMI, AMI, Rand, adjusted Rand, Fowlkes-Mallows, homogeneity,
// completeness, V-measure) on gfx950: all nine are functions of one [K_target, K_preds] contingency table of two label
// vectors.  Label ranks without a sort (cluster_scatter.hip), an integer pair table, one pass over the table, one small
// score launch.
//
// Reference: functional/clustering/utils.py::calculate_contingency_matrix (two torch.unique sorts, two host reads, one
// bincount) and the nine functionals (chains of small launches with host branches on device values, a second and third
// torch.unique + bincount for the entropies).
//
// Pair table.  cluster_pair_table_kernel: a workgroup of 256 threads owns a row chunk; a lane takes four consecutive ranks
// of each side per step (one 16-byte load per side where both pointers are 16-byte aligned, four dword loads in the generic
// instantiation: the same cells, so the same table), forms cell = t * K_p + p and merges consecutive equal cells into one
// add.  When all 256 ranks of a wave's step fall in one cell (sorted labels) the wave keeps the run in a wave-uniform
// register pair and lane 0 adds it when the cell changes: one add per run instead of 64 on one address.
//   LDS arm (cells <= LDS_CELLS): R = min(32, pow2 floor of LDS_CELLS / cells) replicas, cell-major (cell * R + lane % R):
//   the replicas of a cell sit in neighbouring banks.  Flush: sum the replicas, one global atomicAdd per non-zero cell.
//   Global arm (cells <= 2^20): integer atomicAdd into the L2-resident table.
// Integer adds only: two runs are bit-equal in both arms.  Ranks outside [0, K) are skipped, never used as an index.
//
// Table statistics.  cluster_pair_stats_kernel: a workgroup owns a tile of table rows; Cp = min(64, pow2 >= K_p) lanes walk
// one row (lane c takes columns c, c + Cp, ...: at most 16), 256 / Cp rows at a time.  Row sums by a butterfly over the Cp
// lanes (every row belongs to one lane group: no atomics), column sums in 16 registers folded through integer LDS adds,
// sum n^2 in int64 and sum n log n in fp64 in a fixed order (thread order, then a tree).  Any partial count is below
// 2^31, so the in-tile sums are 32-bit.  MI = log n + (sum n_ij log n_ij - sum a_i log a_i - sum b_j log b_j) / n needs
// nothing else from the cells.
//
// Fold and epilogue.  cluster_pair_score_kernel, one workgroup, phase 1: column partials in tile order -> b_j, n, sum a^2,
// sum b^2, the two sum c log c, the 2 x 2 pair matrix in int64, MI, H(preds), H(target), the fp64 marginals (AMI's EMI
// reads them).  Phase 2: the requested metric with the composition's edge rules, fp64, rounded once to fp32.  Rules that
// the composition applies to an fp32 value are applied to the fp32-rounded value.  A side with one cluster has MI = 0 and
// H = 0 exactly (an integer rule; the composition's fp32 sums give exact zeros there too).
#include "cluster.h"

#include <cstdlib>
#include <limits>

namespace tmx {
namespace {

constexpr int kCpThreads = 256;
constexpr int kCpPerLane = 4;                          // ranks per side per lane per step: one 16-byte load
constexpr int kCpStep = kCpThreads * kCpPerLane;       // ranks of one workgroup step
constexpr int kCpLdsCells = 16384;                     // most u32 cells of the LDS arm (64 KiB); TMX_CLUSTER_PAIR_LDS_CELLS is the A/B knob
constexpr int kCpReplicaCap = 32;
constexpr int kCpCellCap = 1 << 20;                    // largest table of the global arm (4 MiB: L2-resident)
constexpr int kCpCap = 1024;                           // most clusters per side (cluster_tile()'s cap)
constexpr int64_t kCpTargetGroups = 2048;              // workgroups the chunk rule aims for (256 CUs x 8)
constexpr int kCpColsPerLane = kCpCap / kWave;         // 16 column registers of the stats kernel
constexpr int kCpStatsCells = 4096;                    // cells a stats tile holds at least
constexpr int kCpMaxTiles = 64;                        // most stats tiles: bounds the one-workgroup fold
constexpr int kCpScoreThreads = 1024;
constexpr double kEpsF32 = 1.1920928955078125e-07;

enum : int { kMI = 0, kNMI, kAMI, kRand, kARI, kFM, kHomogeneity, kCompleteness, kVMeasure, kNumMetrics };
enum : int { kAvgMin = 0, kAvgGeometric, kAvgArithmetic, kAvgMax };
enum : int { kStMI = 0, kStHp, kStHt, kStN, kStTn, kStFp, kStFn, kStTp, kStSq, kStSa, kStSb, kStCount };

// ------------------------------------------------------------------------------------------------- pair table
// dynamic LDS (LDS arm): unsigned tab[cells << rep_log2]
template <bool VEC, bool LDS>
__global__ __launch_bounds__(kCpThreads) void cluster_pair_table_kernel(const int* __restrict__ inv_p, const int* __restrict__ inv_t, int N, int K_p,
                                                                        int K_t, int rep_log2, int rows_per_chunk, int* __restrict__ table) {
  extern __shared__ unsigned cp_lds[];
  const int t = threadIdx.x, lane = t & (kWave - 1);
  const int cells = K_p * K_t, rep = t & ((1 << rep_log2) - 1);
  if (LDS) {
    for (int i = t; i < (cells << rep_log2); i += kCpThreads) cp_lds[i] = 0u;
    __syncthreads();
  }
  auto add = [&](int cell, unsigned cnt) {
    if (LDS) atomicAdd(&cp_lds[(cell << rep_log2) + rep], cnt);
    else atomicAdd(&table[cell], static_cast<int>(cnt));
  };
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk, r1 = min<int64_t>(N, r0 + rows_per_chunk);
  int wcell = -1;      // the wave's pending run: wave-uniform
  unsigned wcnt = 0u;
  for (int64_t base = r0; base < r1; base += kCpStep) {  // every thread makes the same trips: the wave vote below stays whole
    const int64_t i = base + kCpPerLane * t;
    int p[kCpPerLane], q[kCpPerLane], c[kCpPerLane];
    if (VEC && i + kCpPerLane <= r1) {  // chunks start at multiples of the step: i is a multiple of four
      const int4 a = *reinterpret_cast<const int4*>(inv_p + i), b = *reinterpret_cast<const int4*>(inv_t + i);
      p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w;
      q[0] = b.x; q[1] = b.y; q[2] = b.z; q[3] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < kCpPerLane; ++j) {
        const bool in = i + j < r1;
        p[j] = in ? inv_p[i + j] : -1;
        q[j] = in ? inv_t[i + j] : -1;
      }
    }
#pragma unroll
    for (int j = 0; j < kCpPerLane; ++j)
      c[j] = (static_cast<unsigned>(p[j]) < static_cast<unsigned>(K_p) && static_cast<unsigned>(q[j]) < static_cast<unsigned>(K_t))
                 ? q[j] * K_p + p[j] : -1;
    const int first = __shfl(c[0], 0, kWave);
    const bool same = first >= 0 && c[0] == first && c[1] == first && c[2] == first && c[3] == first;
    if (__all(same)) {
      if (first != wcell) {
        if (wcnt != 0u && lane == 0) add(wcell, wcnt);
        wcell = first;
        wcnt = 0u;
      }
      wcnt += kCpPerLane * kWave;
      continue;
    }
    int cur = c[0];
    unsigned cnt = 1u;
#pragma unroll
    for (int j = 1; j < kCpPerLane; ++j) {
      if (c[j] == cur) { ++cnt; continue; }
      if (cur >= 0) add(cur, cnt);
      cur = c[j];
      cnt = 1u;
    }
    if (cur >= 0) add(cur, cnt);
  }
  if (wcnt != 0u && lane == 0) add(wcell, wcnt);
  if (LDS) {
    __syncthreads();
    for (int cell = t; cell < cells; cell += kCpThreads) {
      unsigned s = 0u;
      for (int r = 0; r < (1 << rep_log2); ++r) s += cp_lds[(cell << rep_log2) + r];
      if (s != 0u) atomicAdd(&table[cell], static_cast<int>(s));
    }
  }
}

// ------------------------------------------------------------------------------------------------- table statistics
// grid: tiles of rows_per_tile table rows.  row_sum [K_t], col_part [tiles, K_p], sq_part [tiles], nl_part [tiles]
__global__ __launch_bounds__(kCpThreads) void cluster_pair_stats_kernel(const int* __restrict__ table, int K_t, int K_p, int cp_log2, int rows_per_tile,
                                                                        long long* __restrict__ row_sum, long long* __restrict__ col_part,
                                                                        long long* __restrict__ sq_part, double* __restrict__ nl_part) {
  __shared__ unsigned s_col[kCpCap];
  __shared__ double s_nl[kCpThreads];
  __shared__ long long s_sq[kCpThreads];
  const int t = threadIdx.x, Cp = 1 << cp_log2, cl = t & (Cp - 1), slot = t >> cp_log2, slots = kCpThreads >> cp_log2;
  for (int c = t; c < K_p; c += kCpThreads) s_col[c] = 0u;
  __syncthreads();
  const int r0 = blockIdx.x * rows_per_tile, r1 = min(K_t, r0 + rows_per_tile);
  unsigned col[kCpColsPerLane];
#pragma unroll
  for (int j = 0; j < kCpColsPerLane; ++j) col[j] = 0u;
  long long sq = 0;
  double nl = 0.0;
  for (int base = r0; base < r1; base += slots) {  // every thread makes the same trips: the butterfly below stays whole
    const int r = base + slot;
    unsigned row = 0u;
    if (r < r1) {
      const int* __restrict__ tr = table + (int64_t)r * K_p;
#pragma unroll
      for (int j = 0; j < kCpColsPerLane; ++j) {
        const int c = cl + (j << cp_log2);
        if (c < K_p) {
          const unsigned n = static_cast<unsigned>(tr[c]);
          row += n;
          col[j] += n;
          sq += static_cast<long long>(n) * static_cast<long long>(n);
          if (n > 1u) nl += static_cast<double>(n) * log(static_cast<double>(n));
        }
      }
    }
    for (int off = Cp >> 1; off > 0; off >>= 1) row += __shfl_xor(row, off, kWave);
    if (r < r1 && cl == 0) row_sum[r] = static_cast<long long>(row);
  }
#pragma unroll
  for (int j = 0; j < kCpColsPerLane; ++j) {
    const int c = cl + (j << cp_log2);
    if (c < K_p && col[j] != 0u) atomicAdd(&s_col[c], col[j]);
  }
  s_nl[t] = nl;
  s_sq[t] = sq;
  __syncthreads();
  for (int c = t; c < K_p; c += kCpThreads) col_part[(int64_t)blockIdx.x * K_p + c] = static_cast<long long>(s_col[c]);
  for (int s = kCpThreads >> 1; s > 0; s >>= 1) {  // fixed-order tree
    if (t < s) { s_nl[t] += s_nl[t + s]; s_sq[t] += s_sq[t + s]; }
    __syncthreads();
  }
  if (t == 0) {
    sq_part[blockIdx.x] = s_sq[0];
    nl_part[blockIdx.x] = s_nl[0];
  }
}

// ------------------------------------------------------------------------------------------------- fold and epilogue
__device__ __forceinline__ double clogc(long long c) { return c > 1 ? static_cast<double>(c) * log(static_cast<double>(c)) : 0.0; }

// Fixed-order trees over the workgroup of kCpScoreThreads; every thread gets the result.
__device__ double score_fold(double v, double* sc) {
  const int t = threadIdx.x;
  sc[t] = v;
  __syncthreads();
  for (int s = kCpScoreThreads >> 1; s > 0; s >>= 1) {
    if (t < s) sc[t] += sc[t + s];
    __syncthreads();
  }
  const double r = sc[0];
  __syncthreads();
  return r;
}

__device__ long long score_fold(long long v, long long* sc) {
  const int t = threadIdx.x;
  sc[t] = v;
  __syncthreads();
  for (int s = kCpScoreThreads >> 1; s > 0; s >>= 1) {
    if (t < s) sc[t] += sc[t + s];
    __syncthreads();
  }
  const long long r = sc[0];
  __syncthreads();
  return r;
}

__device__ double generalized_mean(double hp, double ht, int average) {
  if (average == kAvgMin) return (ht < hp || ht != ht) ? ht : hp;
  if (average == kAvgMax) return (ht > hp || ht != ht) ? ht : hp;
  if (average == kAvgGeometric) return exp(0.5 * (log(hp) + log(ht)));
  return 0.5 * (hp + ht);
}

// The metric from the folded statistics, with the composition's edge rules.
__device__ double pair_metric(const double* st, int metric, int average, double beta, double emi, int K_t, int K_p) {
  const double mi = st[kStMI], hp = st[kStHp], ht = st[kStHt], n = st[kStN];
  const long long tn = __double_as_longlong(st[kStTn]), fp = __double_as_longlong(st[kStFp]), fn = __double_as_longlong(st[kStFn]),
                  tp = __double_as_longlong(st[kStTp]), sq = __double_as_longlong(st[kStSq]), sa = __double_as_longlong(st[kStSa]),
                  sb = __double_as_longlong(st[kStSb]);
  switch (metric) {
    case kMI: return mi;
    case kNMI: {
      if (fabsf(static_cast<float>(mi)) <= static_cast<float>(kEpsF32)) return mi;
      return mi / generalized_mean(hp, ht, average);
    }
    case kAMI: {
      double den = generalized_mean(hp, ht, average) - emi;
      if (den == den) den = static_cast<float>(den) < 0.0f ? fmin(den, -kEpsF32) : fmax(den, kEpsF32);
      return (mi - emi) / den;
    }
    case kRand: {
      const long long num = tn + tp, den = tn + fp + fn + tp;
      return (num == den || den == 0) ? 1.0 : static_cast<double>(num) / static_cast<double>(den);
    }
    case kARI: {
      if (fn == 0 && fp == 0) return 1.0;
      const double a = static_cast<double>(tn), b = static_cast<double>(fp), c = static_cast<double>(fn), d = static_cast<double>(tp);
      return 2.0 * (d * a - c * b) / ((d + c) * (c + a) + (d + b) * (b + a));
    }
    case kFM: {
      const long long nn = static_cast<long long>(n), tk = sq - nn;
      if (tk == 0) return 0.0;
      const double pk = static_cast<double>(sb - nn), qk = static_cast<double>(sa - nn);
      return sqrt(static_cast<double>(tk) / pk) * sqrt(static_cast<double>(tk) / qk);
    }
    default: {
      const double h = K_t == 1 ? 1.0 : mi / ht, c = K_p == 1 ? 1.0 : mi / hp;
      if (metric == kHomogeneity) return h;
      if (metric == kCompleteness) return c;
      if (static_cast<float>(h) + static_cast<float>(c) == 0.0f) return 1.0;
      return (1.0 + beta) * h * c / (beta * h + c);
    }
  }
}

// one workgroup.  phase bit 0: fold -> stats [kStCount], marg = {a fp64 [K_t], b fp64 [K_p]}; bit 1: epilogue -> resf
__global__ __launch_bounds__(kCpScoreThreads) void cluster_pair_score_kernel(const long long* __restrict__ row_sum, const long long* __restrict__ col_part,
                                                                             const long long* __restrict__ sq_part, const double* __restrict__ nl_part,
                                                                             int K_t, int K_p, int tiles, int phase, int metric, int average,
                                                                             double beta, const double* __restrict__ emi, double* marg,
                                                                             double* stats, float* __restrict__ resf) {
  __shared__ double sd[kCpScoreThreads];
  __shared__ long long sl[kCpScoreThreads];
  const int t = threadIdx.x;
  if (phase & 1) {
    long long na = 0, sa = 0, sb = 0;
    double la = 0.0, lb = 0.0;
    for (int i = t; i < K_t; i += kCpScoreThreads) {
      const long long a = row_sum[i];
      marg[i] = static_cast<double>(a);
      na += a;
      sa += a * a;
      la += clogc(a);
    }
    for (int j = t; j < K_p; j += kCpScoreThreads) {
      long long b = 0;
      for (int tile = 0; tile < tiles; ++tile) b += col_part[(int64_t)tile * K_p + j];
      marg[K_t + j] = static_cast<double>(b);
      sb += b * b;
      lb += clogc(b);
    }
    na = score_fold(na, sl);
    sa = score_fold(sa, sl);
    sb = score_fold(sb, sl);
    la = score_fold(la, sd);
    lb = score_fold(lb, sd);
    if (t == 0) {
      long long sq = 0;
      double nl = 0.0;
      for (int tile = 0; tile < tiles; ++tile) {  // tile order
        sq += sq_part[tile];
        nl += nl_part[tile];
      }
      const double n = static_cast<double>(na), log_n = log(n);
      const bool one = K_t == 1 || K_p == 1;
      stats[kStMI] = one ? 0.0 : log_n + (nl - la - lb) / n;
      stats[kStHp] = K_p == 1 ? 0.0 : log_n - lb / n;
      stats[kStHt] = K_t == 1 ? 0.0 : log_n - la / n;
      stats[kStN] = n;
      const long long fp = sa - sq, fn = sb - sq;  // calculate_pair_cluster_confusion_matrix: [0, 1] and [1, 0]
      stats[kStTn] = __longlong_as_double(na * na - fp - fn - sq);
      stats[kStFp] = __longlong_as_double(fp);
      stats[kStFn] = __longlong_as_double(fn);
      stats[kStTp] = __longlong_as_double(sq - na);
      stats[kStSq] = __longlong_as_double(sq);
      stats[kStSa] = __longlong_as_double(sa);
      stats[kStSb] = __longlong_as_double(sb);
    }
  }
  if ((phase & 2) && t == 0) resf[0] = static_cast<float>(pair_metric(stats, metric, average, beta, emi ? emi[0] : 0.0, K_t, K_p));
}

int log2_floor(int64_t v) {
  int l = 0;
  while ((int64_t(2) << l) <= v) ++l;
  return l;
}

// TMX_CLUSTER_PAIR_LDS_CELLS: the A/B knob of the LDS arm (README), read once per process; 4096, 8192 or 16384 (64 KiB of dynamic LDS)
int pair_lds_cells() {
  static const int cells = [] {
    const char* e = std::getenv("TMX_CLUSTER_PAIR_LDS_CELLS");
    const int64_t v = e ? std::atoll(e) : 0;
    return (v == 4096 || v == 8192 || v == 16384) ? static_cast<int>(v) : kCpLdsCells;
  }();
  return cells;
}

// replicas of a table of `cells` cells in the LDS arm, as a power of two; -1: the global arm
int pair_rep_log2(int64_t cells) {
  if (cells > pair_lds_cells()) return -1;
  return std::min(log2_floor(pair_lds_cells() / cells), log2_floor(kCpReplicaCap));
}

// rows per stats tile: at least kCpStatsCells cells, at most kCpMaxTiles tiles
int64_t pair_stats_rows(int64_t K_t, int64_t K_p) {
  const int64_t rows = std::max((kCpStatsCells + K_p - 1) / K_p, (K_t + kCpMaxTiles - 1) / kCpMaxTiles);
  return std::min(rows, K_t);
}

}  // namespace

// {threads, LDS cells, ranks per lane, replica cap, cell cap, cluster cap}: what the tests need to place their chunk, replica and arm edges
std::vector<int64_t> cluster_pair_tile() { return {kCpThreads, pair_lds_cells(), kCpPerLane, kCpReplicaCap, kCpCellCap, kCpCap}; }

// Ranks per workgroup of the table kernel for N label pairs and a table of `cells` cells: a function of the shape alone.
// Aims at kCpTargetGroups workgroups in whole steps of threads x ranks per lane; in the LDS arm a chunk holds at least as
// many ranks as the workgroup has LDS words to clear and flush.
int64_t cluster_pair_rows_per_chunk(int64_t N, int64_t cells) {
  TORCH_CHECK(N >= 1 && cells >= 1 && cells <= kCpCellCap, "cluster_pair_rows_per_chunk: expected a non-empty shape within the cell cap");
  const int rep = pair_rep_log2(cells);
  int64_t rows = (N + kCpTargetGroups - 1) / kCpTargetGroups;
  if (rep >= 0) rows = std::max(rows, cells << rep);
  return (rows + kCpStep - 1) / kCpStep * kCpStep;
}

// preds, target: integer labels [N] -> (inv_p, inv_t int32 [N], info int32 {K_p, wide_p, K_t, wide_t}): one host read serves both sides
std::tuple<at::Tensor, at::Tensor, at::Tensor> cluster_pair_ranks(const at::Tensor& preds, const at::Tensor& target) {
  TORCH_CHECK(preds.is_cuda() && target.is_cuda() && preds.device() == target.device(), "cluster_pair_ranks: expected labels on one GPU");
  TORCH_CHECK(preds.dim() == 1 && target.dim() == 1 && preds.numel() == target.numel(), "cluster_pair_ranks: expected two [N] label vectors");
  auto [inv_p, info_p] = cluster_label_ranks(preds);
  auto [inv_t, info_t] = cluster_label_ranks(target);
  return {inv_p, inv_t, at::cat({info_p, info_t})};
}

// inv_p, inv_t: int32 ranks [N] in [0, K_p) and [0, K_t) -> int32 table [K_t, K_p]
at::Tensor cluster_pair_table(const at::Tensor& inv_p_in, const at::Tensor& inv_t_in, int64_t K_p, int64_t K_t) {
  const char* name = "cluster_pair_table";
  TORCH_CHECK(inv_p_in.is_cuda() && inv_t_in.is_cuda() && inv_p_in.device() == inv_t_in.device(), name, ": expected ranks on one GPU");
  TORCH_CHECK(inv_p_in.dim() == 1 && inv_t_in.dim() == 1 && inv_p_in.numel() == inv_t_in.numel(), name, ": expected two [N] rank vectors");
  TORCH_CHECK(inv_p_in.scalar_type() == at::kInt && inv_t_in.scalar_type() == at::kInt, name, ": expected int32 ranks");
  const int64_t N = inv_p_in.numel(), cells = K_p * K_t;
  TORCH_CHECK(N >= 1 && N < INT32_MAX, name, ": unsupported number of labels ", N);
  TORCH_CHECK(K_p >= 1 && K_p <= kCpCap && K_t >= 1 && K_t <= kCpCap && cells <= kCpCellCap, name, ": unsupported table ", K_t, " x ", K_p);
  const at::DeviceGuard guard(inv_p_in.device());
  auto inv_p = inv_p_in.contiguous(), inv_t = inv_t_in.contiguous();
  auto table = at::zeros({K_t, K_p}, inv_p.options());
  const int rep = pair_rep_log2(cells);
  const int64_t rows = cluster_pair_rows_per_chunk(N, cells), chunks = (N + rows - 1) / rows;
  const bool vec = vec16_ok(kCpPerLane, sizeof(int), {inv_p.data_ptr(), inv_t.data_ptr()});
  const size_t lds = rep >= 0 ? (static_cast<size_t>(cells) << rep) * sizeof(unsigned) : 0;
  auto launch = [&](auto v, auto l) {
    hipLaunchKernelGGL((cluster_pair_table_kernel<decltype(v)::value, decltype(l)::value>), dim3(static_cast<unsigned>(chunks)), dim3(kCpThreads), lds,
                       stream(), inv_p.data_ptr<int>(), inv_t.data_ptr<int>(), static_cast<int>(N), static_cast<int>(K_p), static_cast<int>(K_t),
                       std::max(rep, 0), static_cast<int>(rows), table.data_ptr<int>());
  };
  if (vec && rep >= 0) launch(std::true_type{}, std::true_type{});
  else if (vec) launch(std::true_type{}, std::false_type{});
  else if (rep >= 0) launch(std::false_type{}, std::true_type{});
  else launch(std::false_type{}, std::false_type{});
  TMX_LAUNCH_CHECK();
  return table;
}

// table: int32 [K_t, K_p] of N label pairs -> the fp32 score (0-dim).  metric 0 MI, 1 NMI, 2 AMI, 3 Rand, 4 adjusted Rand,
// 5 Fowlkes-Mallows, 6 homogeneity, 7 completeness, 8 V-measure; average 0 min, 1 geometric, 2 arithmetic, 3 max.
at::Tensor cluster_pair_score(const at::Tensor& table_in, int64_t N, int64_t metric, int64_t average, double beta) {
  const char* name = "cluster_pair_score";
  TORCH_CHECK(table_in.is_cuda() && table_in.dim() == 2 && table_in.scalar_type() == at::kInt, name, ": expected an int32 [K_t, K_p] table on the GPU");
  const int64_t K_t = table_in.size(0), K_p = table_in.size(1);
  TORCH_CHECK(K_p >= 1 && K_p <= kCpCap && K_t >= 1 && K_t <= kCpCap, name, ": unsupported table ", K_t, " x ", K_p);
  TORCH_CHECK(N >= 1 && N < INT32_MAX, name, ": unsupported number of labels ", N);
  TORCH_CHECK(metric >= 0 && metric < kNumMetrics && average >= kAvgMin && average <= kAvgMax, name, ": unknown metric or average method");
  const at::DeviceGuard guard(table_in.device());
  auto table = table_in.contiguous();
  const auto i64 = table.options().dtype(at::kLong), f64 = table.options().dtype(at::kDouble);
  const int64_t rows = pair_stats_rows(K_t, K_p), tiles = (K_t + rows - 1) / rows;
  int cp_log2 = 0;
  while ((1 << cp_log2) < K_p && (1 << cp_log2) < kWave) ++cp_log2;
  auto ints = at::empty({K_t + tiles * K_p + tiles}, i64);  // row sums, column partials, sum n^2 partials
  auto reals = at::empty({tiles + K_t + K_p + kStCount}, f64);  // sum n log n partials, marginals, stats
  auto resf = at::empty({1}, table.options().dtype(at::kFloat));
  long long* row_sum = reinterpret_cast<long long*>(ints.data_ptr<int64_t>());
  long long* col_part = row_sum + K_t;
  long long* sq_part = col_part + tiles * K_p;
  double* nl_part = reals.data_ptr<double>();
  double* marg = nl_part + tiles;
  double* stats = marg + K_t + K_p;
  hipLaunchKernelGGL(cluster_pair_stats_kernel, dim3(static_cast<unsigned>(tiles)), dim3(kCpThreads), 0, stream(), table.data_ptr<int>(),
                     static_cast<int>(K_t), static_cast<int>(K_p), cp_log2, static_cast<int>(rows), row_sum, col_part, sq_part, nl_part);
  auto score = [&](int phase, const double* emi) {
    hipLaunchKernelGGL(cluster_pair_score_kernel, dim3(1), dim3(kCpScoreThreads), 0, stream(), row_sum, col_part, sq_part, nl_part,
                       static_cast<int>(K_t), static_cast<int>(K_p), static_cast<int>(tiles), phase, static_cast<int>(metric),
                       static_cast<int>(average), beta, emi, marg, stats, resf.data_ptr<float>());
  };
  if (metric == kAMI && K_t > 1 && K_p > 1) {  // the composition's EMI of a one-cluster side is 0
    score(1, nullptr);
    TMX_LAUNCH_CHECK();
    auto emi = expected_mutual_info(reals.narrow(0, tiles, K_t), reals.narrow(0, tiles + K_t, K_p), static_cast<double>(N));
    score(2, emi.data_ptr<double>());
  } else {
    score(3, nullptr);
  }
  TMX_LAUNCH_CHECK();
  return resf.reshape({});
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("cluster_pair_ranks(Tensor preds, Tensor target) -> (Tensor, Tensor, Tensor)");
  m.def("cluster_pair_table(Tensor inv_p, Tensor inv_t, int K_p, int K_t) -> Tensor");
  m.def("cluster_pair_score(Tensor table, int N, int metric, int average, float beta) -> Tensor");
  m.def("cluster_pair_tile() -> int[]", &tmx::cluster_pair_tile);
  m.def("cluster_pair_rows_per_chunk(int N, int cells) -> int", &tmx::cluster_pair_rows_per_chunk);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("cluster_pair_ranks", &tmx::cluster_pair_ranks);
  m.impl("cluster_pair_table", &tmx::cluster_pair_table);
  m.impl("cluster_pair_score", &tmx::cluster_pair_score);
}
