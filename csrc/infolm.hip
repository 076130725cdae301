// InfoLM's scoring side and the row-pair reductions of the regression metrics (KL divergence, cosine similarity).
//
// tmx::infolm_accumulate: acc[owner[r], :] += weight[r] * softmax(logits[r, pos[r], :] / T) for every row r.
//   The composition gathers the masked rows into a copy, divides, softmaxes, casts, scales and index_adds: about ten passes over
//   rows * V elements and an atomic scatter.  Here the logits are read in place, twice:
//   1. infolm_row_stats_kernel: one workgroup per row streams the row once with the online (max, sum exp) pair of
//      online_softmax.h and writes m_r = max(x / T) and c_r = weight_r / sum exp(x / T - m_r).
//   2. infolm_accumulate_kernel: one workgroup owns a tile of kIlTile vocabulary columns of ONE sentence.  It looks the sentence's row
//      run [r0, r1) up in an offset table (infolm_offsets_kernel: a lower bound per sentence in the non-decreasing owner list), walks
//      the run in row order with the next row's loads in flight while this row's exponentials are evaluated (two register buffers),
//      keeps sum_r c_r * exp(x / T - m_r) in registers and ends with one read-modify-write of acc.  Every acc element has one owner:
//      no atomics, two calls are bit-equal, and a sentence without rows leaves its acc row untouched.
//   Row starts are (r * row_stride + pos * seq_stride) elements from the base, so consecutive rows differ in alignment (V = 30522: fp32
//   rows alternate between 16- and 8-byte alignment).  Each row is loaded with the widest of 16 / 8 / 4-byte loads its address allows.
//   Special values follow softmax: a -inf logit adds 0, a NaN logit makes c_r NaN and with it the row's whole contribution, a +inf logit or
//   a row of -inf gives NaN through exp(inf - inf).  A position outside [0, S) poisons the row with NaN without reading out of bounds.
//
// tmx::row_pair_measure: out[n] = measure(p[n, :], t[n, :]) for the nine InfoLM information measures, KL divergence on probabilities and
//   on log-probabilities, and cosine similarity.  One kernel template over the kind, two splits chosen by V:
//   * row_pair_wave_kernel: G lanes per row pair (8 for V <= kRpSmallLimit, else a whole wave; 256 / G rows per workgroup), shuffles only;
//   * row_pair_block_kernel: a workgroup per row pair for V > kRpWaveLimit, 16-byte loads after a scalar head that aligns both rows,
//     wave shuffles and one LDS exchange.
//   Element terms are evaluated in fp32 as the composition writes them (accurate logf / powf / expf / sqrtf, IEEE semantics at 0 and inf);
//   per-thread sums, the tree and the epilogue (logs, quotients, acos, nan_to_num) are fp64, rounded once to fp32.  KL on probabilities is
//   single-pass, sum xlogy(p, p / q) / P - log(P / Q) with P = sum p and Q = sum q; its element term is fp64, since the two parts cancel.
#include "common.h"
#include "online_softmax.h"

#include <cfloat>
#include <vector>

namespace tmx {

constexpr int kIlThreads = 256;
constexpr int kIlCols = 8;                       // vocabulary columns per thread of the accumulate kernel
constexpr int kIlTile = kIlThreads * kIlCols;    // columns per workgroup
constexpr int kRpThreads = 256;
constexpr int kRpSmallLimit = 16;                // rows up to here: 8 lanes per row pair
constexpr int kRpWaveLimit = 1024;               // rows up to here: a wave per row pair
constexpr int kRpTile = kRpThreads * kIlCols;    // elements a workgroup of the block route covers per step

// Eight consecutive elements of a row, as loaded.
template <typename T>
struct alignas(16) Raw8 {
  T v[kIlCols];
};

template <typename T, typename W>
__device__ __forceinline__ void load_words(Raw8<T>& dst, const T* src) {
  constexpr int n = sizeof(Raw8<T>) / sizeof(W);
  W* d = reinterpret_cast<W*>(&dst);
  const W* s = reinterpret_cast<const W*>(src);
#pragma unroll
  for (int k = 0; k < n; ++k) d[k] = s[k];
}

// src[0 .. n) into dst (n <= 8; elements from n on stay zero): the widest loads the address allows when all eight exist.
template <typename T>
__device__ __forceinline__ void load8(Raw8<T>& dst, const T* src, int n) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src);
  if (n == kIlCols && a % 16 == 0) {
    load_words<T, uint4>(dst, src);
  } else if (n == kIlCols && a % 8 == 0) {
    load_words<T, uint2>(dst, src);
  } else if (n == kIlCols && sizeof(T) < 4 && a % 4 == 0) {
    load_words<T, uint32_t>(dst, src);
  } else {
    dst = Raw8<T>{};
#pragma unroll
    for (int k = 0; k < kIlCols; ++k)
      if (k < n) dst.v[k] = src[k];
  }
}

// ------------------------------------------------------------------------------------------------------------ infolm_accumulate

// offs[b] = first row whose owner is >= b, for b in [0, B]: sentence b owns the rows [offs[b], offs[b + 1]).
__global__ void infolm_offsets_kernel(const int64_t* __restrict__ owner, int64_t R, int64_t B, int64_t* __restrict__ offs) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b > B) return;
  int64_t lo = 0, hi = R;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (owner[mid] < b) lo = mid + 1;
    else hi = mid;
  }
  offs[b] = lo;
}

template <typename T>
__device__ __forceinline__ const T* infolm_row(const T* logits, int64_t sr, int64_t ss, int64_t S, const int64_t* pos, int64_t r, bool& ok) {
  const int64_t p = pos[r];
  ok = p >= 0 && p < S;
  return logits + r * sr + (ok ? p : 0) * ss;
}

template <typename T>
__global__ __launch_bounds__(kIlThreads) void infolm_row_stats_kernel(const T* __restrict__ logits, int64_t sr, int64_t ss, int64_t S, int64_t V,
                                                                      const int64_t* __restrict__ pos, const float* __restrict__ weight,
                                                                      float temperature, float* __restrict__ row_m, float* __restrict__ row_c) {
  const int64_t r = blockIdx.x;
  bool ok;
  const T* x = infolm_row(logits, sr, ss, S, pos, r, ok);
  MaxSum<float> acc{-INFINITY, 0.f};
  // scalar head up to the first 16-byte boundary, 16-byte body, scalar tail
  constexpr int kVec = 16 / sizeof(T);
  int64_t head = static_cast<int64_t>(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / sizeof(T));
  if (head > V) head = V;
  const int64_t nvec = (V - head) / kVec;
  if (static_cast<int64_t>(threadIdx.x) < head) ms_push(acc, to_f32<T>(x[threadIdx.x]) / temperature);
  struct alignas(16) Pack { T v[kVec]; };
  const Pack* xp = reinterpret_cast<const Pack*>(x + head);
  for (int64_t i = threadIdx.x; i < nvec; i += kIlThreads) {
    const Pack pk = xp[i];
#pragma unroll
    for (int k = 0; k < kVec; ++k) ms_push(acc, to_f32<T>(pk.v[k]) / temperature);
  }
  for (int64_t i = head + nvec * kVec + threadIdx.x; i < V; i += kIlThreads) ms_push(acc, to_f32<T>(x[i]) / temperature);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    MaxSum<float> o{__shfl_xor(acc.m, off, kWave), __shfl_xor(acc.s, off, kWave)};
    acc = ms_merge(acc, o);
  }
  __shared__ float sm[kIlThreads / kWave], ss_[kIlThreads / kWave];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) {
    sm[wave] = acc.m;
    ss_[wave] = acc.s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    MaxSum<float> tot{sm[0], ss_[0]};
    for (int w = 1; w < kIlThreads / kWave; ++w) tot = ms_merge(tot, MaxSum<float>{sm[w], ss_[w]});
    row_m[r] = tot.m;
    row_c[r] = ok ? weight[r] / tot.s : NAN;
  }
}

template <typename T>
__global__ __launch_bounds__(kIlThreads) void infolm_accumulate_kernel(const T* __restrict__ logits, int64_t sr, int64_t ss, int64_t S, int64_t V,
                                                                       const int64_t* __restrict__ pos, const int64_t* __restrict__ offs,
                                                                       const float* __restrict__ row_m, const float* __restrict__ row_c,
                                                                       float temperature, int tiles, float* __restrict__ acc) {
  const int64_t b = blockIdx.x / tiles;
  const int64_t col0 = static_cast<int64_t>(blockIdx.x % tiles) * kIlTile + static_cast<int64_t>(threadIdx.x) * kIlCols;
  const int64_t r0 = offs[b], r1 = offs[b + 1];
  if (r0 >= r1 || col0 >= V) return;
  const int ncol = V - col0 < kIlCols ? static_cast<int>(V - col0) : kIlCols;
  float sum[kIlCols];
#pragma unroll
  for (int k = 0; k < kIlCols; ++k) sum[k] = 0.f;
  bool ok;
  Raw8<T> cur, nxt{};
  load8(cur, infolm_row(logits, sr, ss, S, pos, r0, ok) + col0, ncol);
  float m = row_m[r0], c = row_c[r0];
  for (int64_t r = r0; r < r1; ++r) {
    float m_n = 0.f, c_n = 0.f;
    if (r + 1 < r1) {  // the next row's loads are issued before this row's exponentials
      load8(nxt, infolm_row(logits, sr, ss, S, pos, r + 1, ok) + col0, ncol);
      m_n = row_m[r + 1];
      c_n = row_c[r + 1];
    }
#pragma unroll
    for (int k = 0; k < kIlCols; ++k) sum[k] += c * expf(to_f32<T>(cur.v[k]) / temperature - m);
    cur = nxt;
    m = m_n;
    c = c_n;
  }
  float* out = acc + b * V + col0;
#pragma unroll
  for (int k = 0; k < kIlCols; ++k)
    if (k < ncol) out[k] += sum[k];
}

void infolm_accumulate(const at::Tensor& logits, const at::Tensor& pos_in, const at::Tensor& owner_in, const at::Tensor& weight_in,
                       double temperature, at::Tensor& acc) {
  TORCH_CHECK(logits.is_cuda() && pos_in.is_cuda() && owner_in.is_cuda() && weight_in.is_cuda() && acc.is_cuda(), "infolm_accumulate: expected GPU tensors");
  TORCH_CHECK(logits.dim() == 3 && acc.dim() == 2, "infolm_accumulate: expected logits [R, S, V] and acc [B, V]");
  const int64_t R = logits.size(0), S = logits.size(1), V = logits.size(2), B = acc.size(0);
  TORCH_CHECK(acc.size(1) == V && acc.scalar_type() == at::kFloat && acc.is_contiguous(), "infolm_accumulate: acc must be contiguous fp32 [B, V]");
  TORCH_CHECK(V == 1 || logits.stride(2) == 1, "infolm_accumulate: the vocabulary dim of logits must be contiguous");
  TORCH_CHECK(pos_in.dim() == 1 && owner_in.dim() == 1 && weight_in.dim() == 1 && pos_in.size(0) == R && owner_in.size(0) == R && weight_in.size(0) == R,
              "infolm_accumulate: pos, owner and weight must be [R]");
  TORCH_CHECK(pos_in.scalar_type() == at::kLong && owner_in.scalar_type() == at::kLong && weight_in.scalar_type() == at::kFloat,
              "infolm_accumulate: pos / owner must be int64 and weight fp32");
  TORCH_CHECK(temperature > 0, "infolm_accumulate: temperature must be positive");
  if (R == 0 || B == 0) return;
  TORCH_CHECK(S > 0 && V > 0, "infolm_accumulate: empty logits");
  const int64_t tiles = (V + kIlTile - 1) / kIlTile;
  TORCH_CHECK(R < (int64_t{1} << 31) && tiles * B < (int64_t{1} << 31), "infolm_accumulate: too many rows or tiles");
  const at::DeviceGuard guard(logits.device());
  auto pos = pos_in.contiguous(), owner = owner_in.contiguous(), weight = weight_in.contiguous();
  auto offs = at::empty({B + 1}, owner.options());
  auto stats = at::empty({2, R}, weight.options());
  float* row_m = stats.data_ptr<float>();
  float* row_c = row_m + R;
  const float temp = static_cast<float>(temperature);
  hipLaunchKernelGGL(infolm_offsets_kernel, dim3(static_cast<unsigned>((B + 1 + 255) / 256)), dim3(256), 0, stream(), owner.data_ptr<int64_t>(), R, B,
                     offs.data_ptr<int64_t>());
  dispatch_float3(logits.scalar_type(), "infolm_accumulate", [&](auto tag) {
    using T = decltype(tag);
    const T* x = reinterpret_cast<const T*>(logits.data_ptr());
    hipLaunchKernelGGL(infolm_row_stats_kernel<T>, dim3(static_cast<unsigned>(R)), dim3(kIlThreads), 0, stream(), x, logits.stride(0), logits.stride(1), S,
                       V, pos.data_ptr<int64_t>(), weight.data_ptr<float>(), temp, row_m, row_c);
    hipLaunchKernelGGL(infolm_accumulate_kernel<T>, dim3(static_cast<unsigned>(tiles * B)), dim3(kIlThreads), 0, stream(), x, logits.stride(0),
                       logits.stride(1), S, V, pos.data_ptr<int64_t>(), offs.data_ptr<int64_t>(), row_m, row_c, temp, static_cast<int>(tiles),
                       acc.data_ptr<float>());
  });
  TMX_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------------------- row_pair_measure

enum RpKind : int {
  kRpKl = 0, kRpAlpha, kRpAb, kRpRenyi, kRpL1, kRpL2, kRpLinf, kRpFisherRao,  // information measures: nan_to_num applied
  kRpKlProb, kRpKlLogProb, kRpCosine,                                           // regression metrics: no nan_to_num
  kRpKinds
};

template <int K>
constexpr int rp_sums() {
  return (K == kRpAb || K == kRpKlProb || K == kRpCosine) ? 3 : 1;
}

// a maximum that keeps a NaN once it has seen one
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

template <int K>
__device__ __forceinline__ double rp_join(double a, double b) {
  if constexpr (K == kRpLinf) return nan_max(a, b);
  else return a + b;
}

// e0 / e1 / e2: the fp32 exponents of the power family (alpha, 1 - alpha | alpha, beta, alpha + beta)
template <int K>
__device__ __forceinline__ void rp_term(float p, float t, float e0, float e1, float e2, double (&s)[rp_sums<K>()]) {
  if constexpr (K == kRpKl) {
    s[0] += static_cast<double>(t * logf(p / t));
  } else if constexpr (K == kRpAlpha || K == kRpRenyi) {
    s[0] += static_cast<double>(powf(t, e0) * powf(p, e1));
  } else if constexpr (K == kRpAb) {
    s[0] += static_cast<double>(powf(t, e2));
    s[1] += static_cast<double>(powf(p, e2));
    s[2] += static_cast<double>(powf(t, e0) * powf(p, e1));
  } else if constexpr (K == kRpL1) {
    s[0] += static_cast<double>(fabsf(t - p));
  } else if constexpr (K == kRpL2) {
    const float d = t - p;
    s[0] += static_cast<double>(d * d);
  } else if constexpr (K == kRpLinf) {
    s[0] = nan_max(s[0], static_cast<double>(fabsf(t - p)));
  } else if constexpr (K == kRpFisherRao) {
    s[0] += static_cast<double>(sqrtf(p * t));
  } else if constexpr (K == kRpKlProb) {  // t is q
    s[0] += static_cast<double>(p);
    s[1] += static_cast<double>(t);
    // fp64, as the epilogue's log(P / Q) is: the two parts cancel
    const double dp = p;
    s[2] += p == 0.f ? 0.0 : dp * log(dp / static_cast<double>(t));
  } else if constexpr (K == kRpKlLogProb) {
    s[0] += static_cast<double>(expf(p) * (p - t));
  } else {
    const double dp = p, dt = t;
    s[0] = fma(dp, dt, s[0]);
    s[1] = fma(dp, dp, s[1]);
    s[2] = fma(dt, dt, s[2]);
  }
}

// (sum - P log(P / Q)) / P.  The product is rounded on its own, never fused into the subtraction: a one-element row, whose sum is that same
// product, then gives exactly 0 as the composition does (the empty asm keeps the product in a register of its own).
__device__ __forceinline__ double kl_prob_finish(double sum, double P, double Q) {
  double pl = P * log(P / Q);
  asm volatile("" : "+v"(pl));
  return (sum - pl) / P;
}

template <int K>
__device__ __forceinline__ float rp_finish(const double (&s)[rp_sums<K>()], double a, double b) {
  double r;
  if constexpr (K == kRpAlpha) r = (1.0 - s[0]) / (a * (a - 1.0));
  else if constexpr (K == kRpAb) r = log(s[0]) / (b * (b + a)) + log(s[1]) / (a * (b + a)) - log(s[2]) / (a * b);
  else if constexpr (K == kRpRenyi) r = log(s[0]) / (a - 1.0);
  else if constexpr (K == kRpL2) r = sqrt(s[0]);
  else if constexpr (K == kRpFisherRao) r = 2.0 * acos(s[0] < 0.0 ? 0.0 : (s[0] > 1.0 ? 1.0 : s[0]));  // a NaN passes the clamp, as torch.clamp's
  else if constexpr (K == kRpKlProb) r = kl_prob_finish(s[2], s[0], s[1]);
  else if constexpr (K == kRpCosine) r = s[0] / (sqrt(s[1]) * sqrt(s[2]));
  else r = s[0];
  float f = static_cast<float>(r);
  if constexpr (K < kRpKlProb) {  // nan_to_num
    if (f != f) f = 0.f;
    else if (f == INFINITY) f = FLT_MAX;
    else if (f == -INFINITY) f = -FLT_MAX;
  }
  return f;
}

struct RpArgs {
  int64_t N, V;
  double alpha, beta;
  float e0, e1, e2;
};

// G lanes per row pair, kRpThreads / G row pairs per workgroup, shuffles only.
template <typename T, int K, int G>
__global__ __launch_bounds__(kRpThreads) void row_pair_wave_kernel(const T* __restrict__ p, const T* __restrict__ t, RpArgs a, float* __restrict__ out) {
  constexpr int NS = rp_sums<K>();
  const int64_t row = static_cast<int64_t>(blockIdx.x) * (kRpThreads / G) + threadIdx.x / G;
  const int lane = threadIdx.x % G;
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  if (row < a.N) {
    const T* pr = p + row * a.V;
    const T* tr = t + row * a.V;
    for (int64_t i = lane; i < a.V; i += G) rp_term<K>(to_f32<T>(pr[i]), to_f32<T>(tr[i]), a.e0, a.e1, a.e2, s);
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = rp_join<K>(s[k], __shfl_xor(s[k], off, kWave));
  }
  if (row < a.N && lane == 0) out[row] = rp_finish<K>(s, a.alpha, a.beta);
}

// A workgroup per row pair: scalar head up to the rows' common 16-byte boundary, 16-byte body, scalar tail.
template <typename T, int K>
__global__ __launch_bounds__(kRpThreads) void row_pair_block_kernel(const T* __restrict__ p, const T* __restrict__ t, RpArgs a, float* __restrict__ out) {
  constexpr int NS = rp_sums<K>();
  const int64_t row = blockIdx.x;
  const T* pr = p + row * a.V;
  const T* tr = t + row * a.V;
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  const uintptr_t ap = reinterpret_cast<uintptr_t>(pr) & 15, at_ = reinterpret_cast<uintptr_t>(tr) & 15;
  int64_t done = 0;
  if (ap == at_) {  // both rows reach a 16-byte boundary after the same number of elements
    int64_t head = static_cast<int64_t>(((16 - ap) & 15) / sizeof(T));
    if (head > a.V) head = a.V;
    if (static_cast<int64_t>(threadIdx.x) < head) rp_term<K>(to_f32<T>(pr[threadIdx.x]), to_f32<T>(tr[threadIdx.x]), a.e0, a.e1, a.e2, s);
    const int64_t ngroup = (a.V - head) / kIlCols;
    for (int64_t g = threadIdx.x; g < ngroup; g += kRpThreads) {
      Raw8<T> rp, rt;
      load_words<T, uint4>(rp, pr + head + g * kIlCols);
      load_words<T, uint4>(rt, tr + head + g * kIlCols);
#pragma unroll
      for (int k = 0; k < kIlCols; ++k) rp_term<K>(to_f32<T>(rp.v[k]), to_f32<T>(rt.v[k]), a.e0, a.e1, a.e2, s);
    }
    done = head + ngroup * kIlCols;
  }
  for (int64_t i = done + threadIdx.x; i < a.V; i += kRpThreads) rp_term<K>(to_f32<T>(pr[i]), to_f32<T>(tr[i]), a.e0, a.e1, a.e2, s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = rp_join<K>(s[k], __shfl_xor(s[k], off, kWave));
  }
  __shared__ double part[kRpThreads / kWave][NS];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) part[wave][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kRpThreads / kWave; ++w) {
#pragma unroll
      for (int k = 0; k < NS; ++k) s[k] = rp_join<K>(s[k], part[w][k]);
    }
    out[row] = rp_finish<K>(s, a.alpha, a.beta);
  }
}

template <typename T, int K>
void rp_launch(const at::Tensor& p, const at::Tensor& t, const RpArgs& a, at::Tensor& out) {
  const T* pp = reinterpret_cast<const T*>(p.data_ptr());
  const T* tp = reinterpret_cast<const T*>(t.data_ptr());
  float* op = out.data_ptr<float>();
  if (a.V <= kRpSmallLimit) {
    constexpr int rows = kRpThreads / 8;
    hipLaunchKernelGGL((row_pair_wave_kernel<T, K, 8>), dim3(static_cast<unsigned>((a.N + rows - 1) / rows)), dim3(kRpThreads), 0, stream(), pp, tp, a, op);
  } else if (a.V <= kRpWaveLimit) {
    constexpr int rows = kRpThreads / kWave;
    hipLaunchKernelGGL((row_pair_wave_kernel<T, K, kWave>), dim3(static_cast<unsigned>((a.N + rows - 1) / rows)), dim3(kRpThreads), 0, stream(), pp, tp, a, op);
  } else {
    hipLaunchKernelGGL((row_pair_block_kernel<T, K>), dim3(static_cast<unsigned>(a.N)), dim3(kRpThreads), 0, stream(), pp, tp, a, op);
  }
}

template <typename T, int K = 0>
void rp_dispatch_kind(int64_t kind, const at::Tensor& p, const at::Tensor& t, const RpArgs& a, at::Tensor& out) {
  if constexpr (K < kRpKinds) {
    if (kind == K) rp_launch<T, K>(p, t, a, out);
    else rp_dispatch_kind<T, K + 1>(kind, p, t, a, out);
  }
}

at::Tensor row_pair_measure(const at::Tensor& p_in, const at::Tensor& t_in, int64_t kind, double alpha, double beta) {
  TORCH_CHECK(p_in.is_cuda() && t_in.is_cuda(), "row_pair_measure: expected GPU tensors");
  TORCH_CHECK(p_in.dim() == 2 && p_in.sizes() == t_in.sizes() && p_in.scalar_type() == t_in.scalar_type(),
              "row_pair_measure: expected two [N, V] tensors of one dtype");
  TORCH_CHECK(kind >= 0 && kind < kRpKinds, "row_pair_measure: unknown kind ", kind);
  const at::DeviceGuard guard(p_in.device());
  auto p = p_in.contiguous(), t = t_in.contiguous();
  RpArgs a{p.size(0), p.size(1), alpha, beta, 0.f, 0.f, 0.f};
  TORCH_CHECK(a.N < (int64_t{1} << 31), "row_pair_measure: too many rows");
  if (kind == kRpAb) {
    a.e0 = static_cast<float>(alpha);
    a.e1 = static_cast<float>(beta);
    a.e2 = static_cast<float>(beta + alpha);
  } else {
    a.e0 = static_cast<float>(alpha);
    a.e1 = static_cast<float>(1.0 - alpha);
  }
  auto out = at::empty({a.N}, p.options().dtype(at::kFloat));
  if (a.N == 0) return out;
  dispatch_float3(p.scalar_type(), "row_pair_measure", [&](auto tag) { rp_dispatch_kind<decltype(tag)>(kind, p, t, a, out); });
  TMX_LAUNCH_CHECK();
  return out;
}

// (columns per workgroup of the accumulate kernel, its threads, largest V of the 8-lane split, largest V of the wave split, elements per
// step of the workgroup split): what the tests need to place their edge shapes
std::vector<int64_t> infolm_tile() { return {kIlTile, kIlThreads, kRpSmallLimit, kRpWaveLimit, kRpTile}; }

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("infolm_accumulate(Tensor logits, Tensor pos, Tensor owner, Tensor weight, float temperature, Tensor(a!) acc) -> ()");
  m.def("row_pair_measure(Tensor p, Tensor t, int kind, float alpha, float beta) -> Tensor");
  m.def("infolm_tile() -> int[]", &tmx::infolm_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("infolm_accumulate", &tmx::infolm_accumulate);
  m.impl("row_pair_measure", &tmx::row_pair_measure);
}
