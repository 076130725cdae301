// Intrinsic clustering scores (Calinski-Harabasz, Davies-Bouldin, Dunn) on gfx950: label ranks without a sort, segmented
// fp64 sums without atomics, a second streaming pass for the scatter, one small score launch.
//
// Reference: functional/clustering/{calinski_harabasz_score,davies_bouldin_score,dunn_index}.py, which sort the labels
// (torch.unique), gather centroids[labels] into a second [N, D] tensor and segment-sum with atomics (index_add_).
//
// Labels -> ranks.  cluster_label_range_kernel folds min / max per workgroup and the last workgroup (a ticket) folds the
// partials and sets the wide flag when max - min >= 2^20.  cluster_label_bitmap_kernel ORs an LDS presence window into a
// 2^20-bit global bitmap (integer atomicOr: order-independent); cluster_label_prefix_kernel scans the words' popcounts
// and writes K; cluster_label_rank_kernel writes inv[i] = prefix[word] + popc(bits below).  A wide span writes nothing:
// the caller takes torch.unique's inverse and continues below.
//
// Sums.  A workgroup of 256 threads owns (row chunk, tile of 64 columns, window of KW clusters).  Thread t owns the fixed
// position (row slot t / Dp, column t % Dp), Dp = clamp(next pow2 >= D, 4, 64), and a private column of KW fp64
// accumulators acc[k][t] in LDS: lane t always hits bank pair t (no conflicts), no two threads share an accumulator (no
// atomics), and a thread adds its rows in row order (fixed order).  Rows whose label is outside the window are skipped
// before their data is loaded.  The slots of a column are folded in slot order into one fp64 partial [chunk, K, D];
// cluster_centroid_kernel adds the partials in chunk order and writes centroids, counts and the grand mean.
//
// Scatter.  Same (slot, column) mapping, all columns of a row in one workgroup: x - mu[label] in fp64, a butterfly over the
// row's Dp lanes, then per row d^2 (CH), d (DB) or the p-norm (Dunn).  CH needs only the total and Dunn only the largest
// radius, so they keep one register per slot; DB keeps acc[cluster][slot] in LDS over a cluster window.  One partial per
// workgroup; cluster_score_kernel folds them in order and evaluates the composition's formula and edge rules in fp64.
#include "cluster.h"

#include <cstdlib>
#include <limits>

namespace tmx {
namespace {

constexpr int kClThreads = 256;        // workgroup of the data kernels
constexpr int kClTD = 64;              // columns per sums tile
constexpr int kClKW = 16;              // clusters per sums window (default; TMX_CLUSTER_KW is the A/B knob)
constexpr int kClMinDp = 4;            // at most 64 row slots: the integer counts fit [KW][64]
constexpr int kClMaxSlots = kClThreads / kClMinDp;
constexpr int kClCap = 1024;           // most clusters the native route takes
constexpr int kClSpanLog2 = 20;        // presence bitmap: 2^20 bits
constexpr int kClWords = (1 << kClSpanLog2) / 32;
constexpr int kClLdsBits = 1 << 15;    // labels this close to the minimum go through the LDS window
constexpr int kClScoreThreads = 1024;
constexpr int kClDbLds = 4096;         // fp64 accumulators of the DB scatter (32 KiB): clusters per window = 4096 / slots
constexpr int64_t kClTargetGroups = 2048;  // workgroups the chunk rule aims for (256 CUs x 8)
constexpr int kClRangeBlocks = 256;

enum : int { kCH = 0, kDB = 1, kDunn1 = 2, kDunn2 = 3, kDunnP = 4 };

template <typename T> __device__ __forceinline__ double ld_f64(const T* p) { return static_cast<double>(to_f32(*p)); }

// 0: sum, 1: max, 2: min; max and min keep a NaN once one is seen (plain compare-select, not fmax / fmin)
template <int OP> __device__ __forceinline__ double fold_op(double a, double b) {
  if (OP == 0) return a + b;
  if (OP == 1) return (b > a || b != b) ? b : a;
  return (b < a || b != b) ? b : a;
}

// Fixed-order tree over the workgroup (blockDim.x a power of two); every thread gets the result.
template <int OP> __device__ double block_fold(double v, double* sc) {
  const int t = threadIdx.x;
  sc[t] = v;
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (t < s) sc[t] = fold_op<OP>(sc[t], sc[t + s]);
    __syncthreads();
  }
  const double r = sc[0];
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------------------------------------- label ranks
// info = {K, wide}; range = {min}
template <typename L>
__global__ __launch_bounds__(kClThreads) void cluster_label_range_kernel(const L* __restrict__ labels, int N, long long* pmin, long long* pmax,
                                                                         unsigned* ticket, long long* range, int* info) {
  __shared__ long long s_lo[kClThreads / kWave], s_hi[kClThreads / kWave];
  __shared__ bool s_last;
  const int t = threadIdx.x;
  long long lo = std::numeric_limits<long long>::max(), hi = std::numeric_limits<long long>::min();
  for (int64_t i = (int64_t)blockIdx.x * kClThreads + t; i < N; i += (int64_t)gridDim.x * kClThreads) {
    const long long v = static_cast<long long>(labels[i]);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  auto fold = [&](long long& a, long long& b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const long long oa = __shfl_xor(a, off, kWave), ob = __shfl_xor(b, off, kWave);
      a = oa < a ? oa : a;
      b = ob > b ? ob : b;
    }
    if ((t & (kWave - 1)) == 0) { s_lo[t / kWave] = a; s_hi[t / kWave] = b; }
    __syncthreads();
    a = s_lo[0]; b = s_hi[0];
    for (int w = 1; w < kClThreads / kWave; ++w) { a = s_lo[w] < a ? s_lo[w] : a; b = s_hi[w] > b ? s_hi[w] : b; }
    __syncthreads();
  };
  fold(lo, hi);
  if (t == 0) {
    __hip_atomic_store(&pmin[blockIdx.x], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&pmax[blockIdx.x], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  lo = std::numeric_limits<long long>::max(), hi = std::numeric_limits<long long>::min();
  for (int b = t; b < (int)gridDim.x; b += kClThreads) {
    const long long a = __hip_atomic_load(&pmin[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long c = __hip_atomic_load(&pmax[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lo = a < lo ? a : lo;
    hi = c > hi ? c : hi;
  }
  fold(lo, hi);
  if (t == 0) {
    range[0] = lo;
    info[0] = 0;
    info[1] = (static_cast<unsigned long long>(hi) - static_cast<unsigned long long>(lo)) >= (1ull << kClSpanLog2) ? 1 : 0;
  }
}

template <typename L>
__global__ __launch_bounds__(kClThreads) void cluster_label_bitmap_kernel(const L* __restrict__ labels, int N, const long long* __restrict__ range,
                                                                          const int* __restrict__ info, unsigned* bitmap) {
  __shared__ unsigned win[kClLdsBits / 32];
  if (info[1]) return;  // wide span: the pass writes nothing
  const int t = threadIdx.x;
  for (int w = t; w < kClLdsBits / 32; w += kClThreads) win[w] = 0u;
  __syncthreads();
  const long long lo = range[0];
  for (int64_t i = (int64_t)blockIdx.x * kClThreads + t; i < N; i += (int64_t)gridDim.x * kClThreads) {
    const unsigned long long off = static_cast<unsigned long long>(static_cast<long long>(labels[i])) - static_cast<unsigned long long>(lo);
    if (off < (unsigned long long)kClLdsBits) {
      atomicOr(&win[off >> 5], 1u << (off & 31));
    } else if (off < (1ull << kClSpanLog2)) {
      atomicOr(&bitmap[off >> 5], 1u << (off & 31));
    }
  }
  __syncthreads();
  for (int w = t; w < kClLdsBits / 32; w += kClThreads)
    if (win[w]) atomicOr(&bitmap[w], win[w]);
}

// one workgroup: exclusive scan of the words' popcounts -> prefix[word]; info[0] = K
__global__ __launch_bounds__(kClScoreThreads) void cluster_label_prefix_kernel(const unsigned* __restrict__ bitmap, int* __restrict__ prefix, int* info) {
  __shared__ int sc[kClScoreThreads];
  if (info[1]) return;
  constexpr int per = kClWords / kClScoreThreads;
  const int t = threadIdx.x;
  int mine = 0;
  for (int w = 0; w < per; ++w) mine += __popc(bitmap[t * per + w]);
  sc[t] = mine;
  __syncthreads();
  for (int off = 1; off < kClScoreThreads; off <<= 1) {  // inclusive Hillis-Steele scan
    const int add = t >= off ? sc[t - off] : 0;
    __syncthreads();
    sc[t] += add;
    __syncthreads();
  }
  int run = sc[t] - mine;
  for (int w = 0; w < per; ++w) {
    prefix[t * per + w] = run;
    run += __popc(bitmap[t * per + w]);
  }
  if (t == kClScoreThreads - 1) info[0] = sc[t];
}

template <typename L>
__global__ __launch_bounds__(kClThreads) void cluster_label_rank_kernel(const L* __restrict__ labels, int N, const long long* __restrict__ range,
                                                                        const int* __restrict__ info, const unsigned* __restrict__ bitmap,
                                                                        const int* __restrict__ prefix, int* __restrict__ inv) {
  if (info[1]) return;
  const long long lo = range[0];
  for (int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kClThreads) {
    unsigned long long off = static_cast<unsigned long long>(static_cast<long long>(labels[i])) - static_cast<unsigned long long>(lo);
    if (off >= (1ull << kClSpanLog2)) off = 0;  // cannot happen below the wide flag; keeps the reads in the tables
    const unsigned w = static_cast<unsigned>(off >> 5), b = static_cast<unsigned>(off & 31);
    inv[i] = prefix[w] + __popc(bitmap[w] & ((1u << b) - 1u));
  }
}

// ------------------------------------------------------------------------------------------------- sums
// grid (chunk, column tile, cluster window); dynamic LDS: double acc[KW][256], int cnt[KW][64]
template <typename T>
__global__ __launch_bounds__(kClThreads) void cluster_sums_kernel(const T* __restrict__ data, int64_t ld, const int* __restrict__ inv, int N, int D,
                                                                  int K, int KW, int dp_log2, int rows_per_chunk,
                                                                  double* __restrict__ part_sums, int* __restrict__ part_counts) {
  extern __shared__ double cl_lds[];
  double* acc = cl_lds;
  int* cnt = reinterpret_cast<int*>(cl_lds + (size_t)KW * kClThreads);
  const int t = threadIdx.x, Dp = 1 << dp_log2, col = t & (Dp - 1), slot = t >> dp_log2, slots = kClThreads >> dp_log2;
  const int chunk = blockIdx.x, tile = blockIdx.y, k0 = blockIdx.z * KW;
  const int kw = min(KW, K - k0);
  const int c = tile * kClTD + col;
  const bool counting = tile == 0 && col == 0;
  for (int k = 0; k < KW; ++k) acc[k * kClThreads + t] = 0.0;
  if (col == 0)
    for (int k = 0; k < KW; ++k) cnt[k * kClMaxSlots + slot] = 0;
  const int64_t r0 = (int64_t)chunk * rows_per_chunk, r1 = min<int64_t>(N, r0 + rows_per_chunk);
  if (c < D) {
    for (int64_t r = r0 + slot; r < r1; r += 4 * slots) {
      int lab[4];
      double x[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t rr = r + (int64_t)j * slots;
        lab[j] = rr < r1 ? inv[rr] - k0 : -1;
        const bool in = static_cast<unsigned>(lab[j]) < static_cast<unsigned>(kw);
        if (!in) lab[j] = -1;
        x[j] = in ? ld_f64(data + rr * ld + c) : 0.0;  // rows of other windows are not loaded
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (lab[j] >= 0) {
          acc[lab[j] * kClThreads + t] += x[j];
          if (counting) cnt[lab[j] * kClMaxSlots + slot] += 1;
        }
      }
    }
  }
  __syncthreads();
  for (int i = t; i < (kw << dp_log2); i += kClThreads) {
    const int k = i >> dp_log2, cc = i & (Dp - 1), c2 = tile * kClTD + cc;
    if (c2 >= D) continue;
    double s = 0.0;
    for (int sl = 0; sl < slots; ++sl) s += acc[k * kClThreads + (sl << dp_log2) + cc];
    part_sums[((int64_t)chunk * K + k0 + k) * D + c2] = s;
  }
  if (tile == 0) {
    for (int k = t; k < kw; k += kClThreads) {
      int n = 0;
      for (int sl = 0; sl < slots; ++sl) n += cnt[k * kClMaxSlots + sl];
      part_counts[(int64_t)chunk * K + k0 + k] = n;
    }
  }
}

// one workgroup per column: partials in chunk order -> centroid[k][c]; counts[k]; mean[c] from the same sums
__global__ __launch_bounds__(kClThreads) void cluster_centroid_kernel(const double* __restrict__ part_sums, const int* __restrict__ part_counts,
                                                                      int chunks, int N, int D, int K, double* __restrict__ centroid,
                                                                      double* __restrict__ counts, double* __restrict__ mean) {
  __shared__ double sc[kClThreads];
  const int t = threadIdx.x, c = blockIdx.x;
  double mine = 0.0;
  for (int k = t; k < K; k += kClThreads) {
    double s = 0.0;
    long long n = 0;
    for (int ch = 0; ch < chunks; ++ch) {
      s += part_sums[((int64_t)ch * K + k) * D + c];
      n += part_counts[(int64_t)ch * K + k];
    }
    centroid[(int64_t)k * D + c] = s / static_cast<double>(n);
    if (c == 0) counts[k] = static_cast<double>(n);
    mine += s;
  }
  const double total = block_fold<0>(mine, sc);
  if (t == 0) mean[c] = total / static_cast<double>(N);
}

// ------------------------------------------------------------------------------------------------- scatter
// grid (chunk, DB cluster window); dynamic LDS: double fold[256], then DB's acc[KS][slots]
template <typename T, int MODE>
__global__ __launch_bounds__(kClThreads) void cluster_scatter_kernel(const T* __restrict__ data, int64_t ld, const int* __restrict__ inv, int N,
                                                                     int D, int K, int KS, int dp_log2, int rows_per_chunk,
                                                                     const double* __restrict__ centroid, double p, double* __restrict__ part) {
  extern __shared__ double cl_lds[];
  double* fold = cl_lds;
  double* acc = cl_lds + kClThreads;
  const int t = threadIdx.x, Dp = 1 << dp_log2, col = t & (Dp - 1), slot = t >> dp_log2, slots = kClThreads >> dp_log2;
  const int chunk = blockIdx.x, k0 = MODE == kDB ? blockIdx.y * KS : 0;
  const int kw = MODE == kDB ? min(KS, K - k0) : K;
  if (MODE == kDB) {
    for (int i = t; i < kw * slots; i += kClThreads) acc[i] = 0.0;
    __syncthreads();
  }
  double mine = MODE == kCH ? 0.0 : -std::numeric_limits<double>::infinity();
  const int64_t r0 = (int64_t)chunk * rows_per_chunk, r1 = min<int64_t>(N, r0 + rows_per_chunk);
  for (int64_t base = r0; base < r1; base += slots) {  // every thread makes the same trips: the butterfly below stays whole
    const int64_t r = base + slot;
    const int lab = r < r1 ? inv[r] - k0 : -1;
    const bool in = static_cast<unsigned>(lab) < static_cast<unsigned>(kw);
    double s = 0.0;
    if (in) {
      const T* row = data + r * ld;
      const double* mu = centroid + (int64_t)(lab + k0) * D;
      for (int c = col; c < D; c += Dp) {
        const double d = ld_f64(row + c) - mu[c];
        if (MODE == kCH || MODE == kDB || MODE == kDunn2) s += d * d;
        else if (MODE == kDunn1) s += fabs(d);
        else s += pow(fabs(d), p);
      }
    }
    for (int off = Dp >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
    if (MODE == kDB || MODE == kDunn2) s = sqrt(s);
    if (MODE == kDunnP) s = pow(s, 1.0 / p);
    if (in) {
      if (MODE == kCH) mine += s;
      else if (MODE == kDB) { if (col == 0) acc[lab * slots + slot] += s; }
      else mine = fold_op<1>(mine, s);
    }
  }
  if (MODE == kDB) {
    __syncthreads();
    for (int k = t; k < kw; k += kClThreads) {
      double s = 0.0;
      for (int sl = 0; sl < slots; ++sl) s += acc[k * slots + sl];
      part[(int64_t)chunk * K + k0 + k] = s;
    }
  } else {
    fold[t] = mine;
    __syncthreads();
    if (t == 0) {  // the slots' column-0 lanes in slot order
      double s = fold[0];
      for (int sl = 1; sl < slots; ++sl) s = fold_op<MODE == kCH ? 0 : 1>(s, fold[sl << dp_log2]);
      part[chunk] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------------- score
__device__ __forceinline__ double centroid_dist(const double* __restrict__ a, const double* __restrict__ b, int D, int mode, double p) {
  double s = 0.0;
  for (int c = 0; c < D; ++c) {
    const double d = a[c] - b[c];
    if (mode == kDunn1) s += fabs(d);
    else if (mode == kDunnP) s += pow(fabs(d), p);
    else s += d * d;
  }
  if (mode == kDunn1) return s;
  return mode == kDunnP ? pow(s, 1.0 / p) : sqrt(s);
}

// one workgroup; res = {score, edge rule taken}, resf = the score in fp32
__global__ __launch_bounds__(kClScoreThreads) void cluster_score_kernel(const double* __restrict__ part, int chunks, const double* __restrict__ centroid,
                                                                        const double* __restrict__ counts, const double* __restrict__ mean, int N,
                                                                        int D, int K, int mode, double p, double* __restrict__ res,
                                                                        float* __restrict__ resf) {
  __shared__ double sc[kClScoreThreads];
  __shared__ double sk[kClCap];
  const int t = threadIdx.x;
  const double inf = std::numeric_limits<double>::infinity();
  double score = 0.0, edge = 0.0;
  if (mode == kCH) {
    double w = 0.0, b = 0.0;
    for (int i = t; i < chunks; i += kClScoreThreads) w += part[i];
    const double within = block_fold<0>(w, sc);
    for (int k = t; k < K; k += kClScoreThreads) {
      double q = 0.0;
      for (int c = 0; c < D; ++c) {
        const double d = centroid[(int64_t)k * D + c] - mean[c];
        q += d * d;
      }
      b += q * counts[k];
    }
    const double between = block_fold<0>(b, sc);
    edge = within == 0.0 ? 1.0 : 0.0;
    score = within == 0.0 ? 1.0 : between * static_cast<double>(N - K) / (within * (static_cast<double>(K) - 1.0));
  } else {
    // thread (i, jp) walks j = jp, jp + P, ... of centroid i's row of the K x K terms; P partitions per row
    const int P = min(32, max(1, kClScoreThreads / K));
    const int i = t / P, jp = t % P;
    const bool active = i < K;
    double far_s = 0.0, far_d = 0.0;  // 1 when some s / some d_ij is not within allclose's default atol of zero
    if (mode == kDB) {
      for (int k = t; k < K; k += kClScoreThreads) {
        double s = 0.0;
        for (int ch = 0; ch < chunks; ++ch) s += part[(int64_t)ch * K + k];
        sk[k] = s / counts[k];
        if (!(fabs(sk[k]) <= 1e-8)) far_s = 1.0;
      }
      __syncthreads();
    }
    double best = mode == kDB ? -inf : inf;
    if (active) {
      for (int j = mode == kDB ? jp : i + 1 + jp; j < K; j += P) {
        double d = j == i ? 0.0 : centroid_dist(centroid + (int64_t)i * D, centroid + (int64_t)j * D, D, mode, p);
        if (mode == kDB) {
          if (!(fabs(d) <= 1e-8)) far_d = 1.0;
          if (d == 0.0) d = inf;
          best = fold_op<1>(best, (sk[i] + sk[j]) / d);
        } else {
          best = fold_op<2>(best, d);
        }
      }
    }
    sc[t] = best;
    __syncthreads();
    double row = 0.0;
    if (active && jp == 0) {
      row = sc[t];
      for (int q = 1; q < P; ++q) row = mode == kDB ? fold_op<1>(row, sc[t + q]) : fold_op<2>(row, sc[t + q]);
    }
    __syncthreads();
    if (mode == kDB) {
      const double total = block_fold<0>(active && jp == 0 ? row : 0.0, sc);
      const double any_s = block_fold<1>(far_s, sc), any_d = block_fold<1>(far_d, sc);
      edge = (any_s == 0.0 || any_d == 0.0) ? 1.0 : 0.0;
      score = edge != 0.0 ? 0.0 : total / static_cast<double>(K);
    } else {
      const double inter = block_fold<2>(active && jp == 0 ? row : inf, sc);
      double m = -inf;
      for (int q = t; q < chunks; q += kClScoreThreads) m = fold_op<1>(m, part[q]);
      score = inter / block_fold<1>(m, sc);
    }
  }
  if (t == 0) {
    res[0] = score;
    res[1] = edge;
    resf[0] = static_cast<float>(score);
  }
}

int64_t env_knob(const char* name, int64_t fallback) {
  const char* e = std::getenv(name);
  const int64_t v = e ? std::atoll(e) : 0;
  return v > 0 ? v : fallback;
}

// TMX_CLUSTER_KW: the A/B knob of the cluster window (README), read once per process; 8, 16 or 24 (dynamic LDS below 64 KiB)
int cluster_kw() {
  static const int kw = [] {
    const int64_t v = env_knob("TMX_CLUSTER_KW", kClKW);
    return (v == 8 || v == 16 || v == 24) ? static_cast<int>(v) : kClKW;
  }();
  return kw;
}

int dp_log2_for(int64_t D) {
  int l = 2;  // kClMinDp
  while ((1 << l) < D && (1 << l) < kClTD) ++l;
  return l;
}

template <typename F>
void dispatch_label(at::ScalarType dtype, const char* name, F&& f) {
  switch (dtype) {
    case at::kByte: f(uint8_t{}); break;
    case at::kChar: f(int8_t{}); break;
    case at::kShort: f(int16_t{}); break;
    case at::kInt: f(int32_t{}); break;
    case at::kLong: f(int64_t{}); break;
    default: TORCH_CHECK(false, name, ": unsupported label dtype ", dtype);
  }
}

}  // namespace

// {threads, TD, KW, min Dp, bitmap span, cluster cap}: what the tests need to place their column, window and span edges
std::vector<int64_t> cluster_tile() { return {kClThreads, kClTD, cluster_kw(), kClMinDp, int64_t(1) << kClSpanLog2, kClCap}; }

// Rows per chunk of a [N, D] call with K clusters: a function of the shape alone.  pass 0: sums, 1: CH / Dunn scatter, 2: DB scatter.
// Aims at kClTargetGroups workgroups; a chunk holds at least 16 K rows wherever it writes a [K, ...] partial, so the
// partials stay below 8 K / (16 K * 2) = 1/4 (16-bit) or 1/8 (fp32) of the input's bytes.
int64_t cluster_rows_per_chunk(int64_t N, int64_t D, int64_t K, int64_t pass) {
  TORCH_CHECK(N >= 1 && D >= 1 && K >= 1 && pass >= 0 && pass <= 2, "cluster_rows_per_chunk: expected a non-empty shape and pass 0..2");
  static const int64_t target = env_knob("TMX_CLUSTER_TARGET_GROUPS", kClTargetGroups);
  const int slots = kClThreads >> dp_log2_for(D);
  int64_t groups = 1, floor_rows = kClThreads;
  if (pass == 0) groups = ((D + kClTD - 1) / kClTD) * ((K + cluster_kw() - 1) / cluster_kw());
  if (pass == 2) groups = (K + kClDbLds / slots - 1) / (kClDbLds / slots);
  if (pass != 1) floor_rows = std::max<int64_t>(floor_rows, 16 * K);
  const int64_t want = std::max<int64_t>(1, target / groups);
  return std::max<int64_t>((N + want - 1) / want, floor_rows);
}

// labels: any integer dtype [N] -> (inv int32 [N], info int32 {K, wide}); with wide set inv is not written
std::tuple<at::Tensor, at::Tensor> cluster_label_ranks(const at::Tensor& labels_in) {
  const char* name = "cluster_label_ranks";
  TORCH_CHECK(labels_in.is_cuda() && labels_in.dim() == 1, name, ": expected 1-D labels on the GPU");
  const int64_t N = labels_in.numel();
  TORCH_CHECK(N >= 1 && N < INT32_MAX, name, ": unsupported number of labels ", N);
  const at::DeviceGuard guard(labels_in.device());
  auto labels = labels_in.contiguous();
  const auto i32 = labels.options().dtype(at::kInt), i64 = labels.options().dtype(at::kLong);
  auto zeroed = at::zeros({kClWords + 1}, i32);  // the bitmap, then the ticket
  auto prefix = at::empty({kClWords}, i32);
  auto part = at::empty({2 * kClRangeBlocks + 1}, i64);  // pmin, pmax, range
  auto info = at::empty({2}, i32);
  auto inv = at::empty({N}, i32);
  unsigned* bitmap = reinterpret_cast<unsigned*>(zeroed.data_ptr<int>());
  long long* pm = reinterpret_cast<long long*>(part.data_ptr<int64_t>());
  long long* range = pm + 2 * kClRangeBlocks;
  const int range_grid = grid_for(N, kClThreads, kClRangeBlocks), grid = grid_for(N, kClThreads);
  dispatch_label(labels.scalar_type(), name, [&](auto tag) {
    using L = decltype(tag);
    const L* lp = reinterpret_cast<const L*>(labels.data_ptr());
    hipLaunchKernelGGL(cluster_label_range_kernel<L>, dim3(range_grid), dim3(kClThreads), 0, stream(), lp, static_cast<int>(N), pm,
                       pm + kClRangeBlocks, bitmap + kClWords, range, info.data_ptr<int>());
    hipLaunchKernelGGL(cluster_label_bitmap_kernel<L>, dim3(grid), dim3(kClThreads), 0, stream(), lp, static_cast<int>(N), range,
                       info.data_ptr<int>(), bitmap);
    hipLaunchKernelGGL(cluster_label_prefix_kernel, dim3(1), dim3(kClScoreThreads), 0, stream(), bitmap, prefix.data_ptr<int>(),
                       info.data_ptr<int>());
    hipLaunchKernelGGL(cluster_label_rank_kernel<L>, dim3(grid), dim3(kClThreads), 0, stream(), lp, static_cast<int>(N), range,
                       info.data_ptr<int>(), bitmap, prefix.data_ptr<int>(), inv.data_ptr<int>());
  });
  TMX_LAUNCH_CHECK();
  return {inv, info};
}

// data [N, D] fp32 / bf16 / fp16 (unit column stride), inv int32 [N] in [0, K); mode 0 CH, 1 DB, 2 Dunn with norm p.
// Returns (res fp64 {score, edge rule taken}, resf fp32 {score}).
std::tuple<at::Tensor, at::Tensor> cluster_intrinsic_score(const at::Tensor& data_in, const at::Tensor& inv_in, int64_t K, int64_t metric,
                                                           double p) {
  const char* name = "cluster_intrinsic_score";
  TORCH_CHECK(data_in.is_cuda() && inv_in.is_cuda() && data_in.device() == inv_in.device(), name, ": expected tensors on one GPU");
  TORCH_CHECK(data_in.dim() == 2 && inv_in.dim() == 1 && inv_in.numel() == data_in.size(0), name, ": expected [N, D] data and [N] ranks");
  TORCH_CHECK(inv_in.scalar_type() == at::kInt, name, ": expected int32 ranks");
  const int64_t N = data_in.size(0), D = data_in.size(1);
  TORCH_CHECK(N >= 1 && N < INT32_MAX && D >= 1 && D <= kClTD * kMaxGridPlanes, name, ": unsupported shape");
  TORCH_CHECK(K >= 2 && K <= kClCap, name, ": unsupported number of clusters ", K);
  TORCH_CHECK(metric >= 0 && metric <= 2, name, ": unknown metric ", metric);
  TORCH_CHECK(metric != 2 || (p >= 1.0 && p < std::numeric_limits<double>::infinity()), name, ": expected a finite p >= 1");
  const at::DeviceGuard guard(data_in.device());
  auto data = data_in.stride(1) == 1 || D == 1 ? data_in : data_in.contiguous();
  auto inv = inv_in.contiguous();
  const int64_t ld = data.stride(0);
  const int mode = metric == 0 ? kCH : metric == 1 ? kDB : p == 1.0 ? kDunn1 : p == 2.0 ? kDunn2 : kDunnP;
  const int dpl = dp_log2_for(D), slots = kClThreads >> dpl, KW = cluster_kw();
  const auto f64 = data.options().dtype(at::kDouble);

  const int64_t rows0 = cluster_rows_per_chunk(N, D, K, 0), chunks0 = (N + rows0 - 1) / rows0;
  auto part_sums = at::empty({chunks0, K, D}, f64);
  auto part_counts = at::empty({chunks0, K}, data.options().dtype(at::kInt));
  auto centroid = at::empty({K, D}, f64);
  auto counts = at::empty({K}, f64);
  auto mean = at::empty({D}, f64);
  const int KS = kClDbLds / slots;
  const int64_t rows1 = cluster_rows_per_chunk(N, D, K, mode == kDB ? 2 : 1), chunks1 = (N + rows1 - 1) / rows1;
  auto part = at::empty({mode == kDB ? chunks1 * K : chunks1}, f64);
  auto res = at::empty({2}, f64);
  auto resf = at::empty({1}, data.options().dtype(at::kFloat));
  TORCH_CHECK(rows0 < INT32_MAX && rows1 < INT32_MAX, name, ": chunk too long");

  const dim3 grid0(static_cast<unsigned>(chunks0), static_cast<unsigned>((D + kClTD - 1) / kClTD), static_cast<unsigned>((K + KW - 1) / KW));
  const size_t lds0 = (size_t)KW * kClThreads * sizeof(double) + (size_t)KW * kClMaxSlots * sizeof(int);
  const dim3 grid1(static_cast<unsigned>(chunks1), mode == kDB ? static_cast<unsigned>((K + KS - 1) / KS) : 1u);
  const size_t lds1 = (kClThreads + (mode == kDB ? (size_t)std::min<int64_t>(KS, K) * slots : 0)) * sizeof(double);
  dispatch_float3(data.scalar_type(), name, [&](auto tag) {
    using T = decltype(tag);
    const T* dp = reinterpret_cast<const T*>(data.data_ptr());
    hipLaunchKernelGGL(cluster_sums_kernel<T>, grid0, dim3(kClThreads), lds0, stream(), dp, ld, inv.data_ptr<int>(), static_cast<int>(N),
                       static_cast<int>(D), static_cast<int>(K), KW, dpl, static_cast<int>(rows0), part_sums.data_ptr<double>(),
                       part_counts.data_ptr<int>());
    hipLaunchKernelGGL(cluster_centroid_kernel, dim3(static_cast<unsigned>(D)), dim3(kClThreads), 0, stream(), part_sums.data_ptr<double>(),
                       part_counts.data_ptr<int>(), static_cast<int>(chunks0), static_cast<int>(N), static_cast<int>(D), static_cast<int>(K),
                       centroid.data_ptr<double>(), counts.data_ptr<double>(), mean.data_ptr<double>());
    auto scatter = [&](auto m) {
      hipLaunchKernelGGL((cluster_scatter_kernel<T, decltype(m)::value>), grid1, dim3(kClThreads), lds1, stream(), dp, ld, inv.data_ptr<int>(),
                         static_cast<int>(N), static_cast<int>(D), static_cast<int>(K), KS, dpl, static_cast<int>(rows1),
                         centroid.data_ptr<double>(), p, part.data_ptr<double>());
    };
    switch (mode) {
      case kCH: scatter(std::integral_constant<int, kCH>{}); break;
      case kDB: scatter(std::integral_constant<int, kDB>{}); break;
      case kDunn1: scatter(std::integral_constant<int, kDunn1>{}); break;
      case kDunn2: scatter(std::integral_constant<int, kDunn2>{}); break;
      default: scatter(std::integral_constant<int, kDunnP>{}); break;
    }
  });
  hipLaunchKernelGGL(cluster_score_kernel, dim3(1), dim3(kClScoreThreads), 0, stream(), part.data_ptr<double>(), static_cast<int>(chunks1),
                     centroid.data_ptr<double>(), counts.data_ptr<double>(), mean.data_ptr<double>(), static_cast<int>(N), static_cast<int>(D),
                     static_cast<int>(K), mode, p, res.data_ptr<double>(), resf.data_ptr<float>());
  TMX_LAUNCH_CHECK();
  return {res, resf};
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("cluster_label_ranks(Tensor labels) -> (Tensor, Tensor)");
  m.def("cluster_intrinsic_score(Tensor data, Tensor inv, int K, int metric, float p) -> (Tensor, Tensor)");
  m.def("cluster_tile() -> int[]", &tmx::cluster_tile);
  m.def("cluster_rows_per_chunk(int N, int D, int K, int which) -> int", &tmx::cluster_rows_per_chunk);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("cluster_label_ranks", &tmx::cluster_label_ranks);
  m.impl("cluster_intrinsic_score", &tmx::cluster_intrinsic_score);
}
