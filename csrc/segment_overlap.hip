// Class-overlap counts for gfx950 behind the segmentation metrics (mean IoU, Dice, generalized Dice): per sample b and class c
//   I[b, c] = pixels in class c on both sides,  P[b, c] = pixels in class c in preds,  T[b, c] = pixels in class c in target,
// as one int64 [B, C, 3] tensor, and the fp64 scores of those counts.  Labels and masks are read in place, once: no one-hot
// expansion, no [B, C, n] temporary.
//
// segment_overlap_index   preds / target [B, n] label maps (uint8 / int16 / int32 / int64, the two may differ).  A label outside
//                         [0, C) is in no class on its side.  Grid: flat on x over (sample, chunk), decoded in the kernel.  A
//                         workgroup counts its chunk into three C-entry u32 arrays in LDS (a chunk is at most 2^30 pixels, so
//                         no entry can wrap) and adds the nonzero entries to the zero-initialised result with 64-bit device
//                         atomics: integer adds commute, so two runs are bit-equal.
// segment_overlap_onehot  preds / target [B·C, n] masks (bool / uint8 / int32 / int64, the two may differ), nonzero = member.
//                         One workgroup per (plane, chunk); per-lane u32 counts, one wave sum, three atomics per workgroup.
//                         Two 1-byte sides count 16 pixels per 16-byte load with byte-wise bit operations and a population count.
// segment_scores          one wave per sample: [B, C, 3] -> fp64 IoU / Dice / generalized Dice in every reduction the
//                         functionals offer.
//
// Loads.  A lane takes runs of R = 16 / max(itemsize) consecutive pixels: the wider side reads a run with one 16-byte load, the
// narrower side with one naturally aligned load of R·itemsize bytes, and the 64 runs of a wave-instruction are contiguous on both
// sides.  A step of a workgroup is kSegThreads·kSegPixels pixels: 16 / R runs per lane and side in flight.  The vector
// instantiation needs 16-byte aligned bases and rows whose byte length is a multiple of 16 on both sides (or a single row); a run
// cut by the end of the row is read by scalar loads.  Everything else takes the generic instantiation: scalar loads, any
// alignment, the same pixels on the same lanes.  No unaligned vector load is ever issued.
//
// LDS contention.  Label maps are spatially coherent: neighbouring lanes hold the same label and their LDS atomics on one
// address serialise.  mode 2 (the default) merges runs per lane: a lane keeps its current (preds, target) label pair and a
// count in registers and touches LDS only when the pair changes.  A lane's pixels lie R apart in a row and a step apart
// between steps, so a lane stays inside one region for many pixels.  mode 1 is the wave-uniform fast path (when all lanes hold
// one pair, one lane adds the ballot's population), mode 0 plain per-pixel atomics; both exist for the A/B of
// tools/segmentation_bench.py (TMX_SEGMENT_MODE, read per call).
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace tmx {

constexpr int kSegThreads = 256;
constexpr int kSegPixels = 16;                                   // pixels per lane per step
constexpr int64_t kSegAlign = kSegThreads * kSegPixels;          // chunk lengths are multiples of a step: chunk starts keep the row's alignment
constexpr int64_t kSegChunkMin = 2 * kSegAlign;                  // the host's own chunking never cuts a row finer than this
constexpr int64_t kSegChunkMax = int64_t{1} << 30;               // a u32 LDS counter holds a whole chunk
constexpr int64_t kSegTargetGroups = 2048;                       // rows are split into chunks until the grid has about this many workgroups
constexpr int64_t kSegMaxClasses = 4096;                         // three u32 arrays: 48 KiB of a workgroup's 64 KiB of LDS

enum SegMode { kSegPlain = 0, kSegWaveUniform = 1, kSegRunMerge = 2 };

struct SegArgs {
  int64_t n, per_chunk, chunks;  // pixels per row, pixels per chunk, chunks per row
  int C, mode;
};

template <typename T, int R> struct SegRun { typedef T type __attribute__((ext_vector_type(R))); };

// R consecutive elements.  VEC and a whole run: one aligned load of R·sizeof(T) bytes; else scalar loads of the first ``valid``.
template <typename T, int R, bool VEC>
__device__ __forceinline__ void seg_load(const T* __restrict__ src, int valid, T (&o)[R]) {
  if (VEC && valid == R) {
    const typename SegRun<T, R>::type v = *reinterpret_cast<const typename SegRun<T, R>::type*>(src);
#pragma unroll
    for (int j = 0; j < R; ++j) o[j] = v[j];
  } else {
#pragma unroll
    for (int j = 0; j < R; ++j) o[j] = j < valid ? src[j] : T(0);
  }
}

// class of a label, -1 when it is outside [0, C): one unsigned compare on the widened value
template <typename T> __device__ __forceinline__ int seg_class(T v, int C) {
  const uint64_t w = static_cast<uint64_t>(static_cast<int64_t>(v));  // uint8 zero-extends, the signed types sign-extend
  return w < static_cast<uint64_t>(C) ? static_cast<int>(w) : -1;
}

__device__ __forceinline__ void seg_add(uint32_t* sI, uint32_t* sP, uint32_t* sT, int cp, int ct, uint32_t count) {
  if (cp >= 0) {
    atomicAdd(&sP[cp], count);
    if (cp == ct) atomicAdd(&sI[cp], count);
  }
  if (ct >= 0) atomicAdd(&sT[ct], count);
}

template <typename TP, typename TT, bool VEC>
__device__ __forceinline__ void segment_index_body(const TP* __restrict__ preds, const TT* __restrict__ target, int64_t* __restrict__ out, const SegArgs& a) {
  constexpr int R = 16 / static_cast<int>(sizeof(TP) > sizeof(TT) ? sizeof(TP) : sizeof(TT));
  constexpr int U = kSegPixels / R;
  extern __shared__ uint32_t seg_lds[];
  uint32_t* sI = seg_lds;
  uint32_t* sP = sI + a.C;
  uint32_t* sT = sP + a.C;
  for (int i = threadIdx.x; i < 3 * a.C; i += kSegThreads) seg_lds[i] = 0u;
  __syncthreads();

  const int64_t wg = blockIdx.x;
  const int64_t b = wg / a.chunks, chunk = wg % a.chunks;
  const TP* p = preds + b * a.n;
  const TT* t = target + b * a.n;
  const int64_t e0 = chunk * a.per_chunk, e1 = min(a.n, e0 + a.per_chunk);

  int rp = -1, rt = -1;  // mode 2: the lane's current pair and how many pixels of it are not in LDS yet
  uint32_t rn = 0u;
  for (int64_t base = e0; base < e1; base += kSegAlign) {
    TP lp[U][R];
    TT lt[U][R];
    int valid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t at = base + (static_cast<int64_t>(u) * kSegThreads + threadIdx.x) * R;
      valid[u] = at < e1 ? static_cast<int>(min(static_cast<int64_t>(R), e1 - at)) : 0;
      seg_load<TP, R, VEC>(p + at, valid[u], lp[u]);  // valid == 0: nothing is read
      seg_load<TT, R, VEC>(t + at, valid[u], lt[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        // a pixel past the chunk is in no class on either side: it adds nothing in any mode, and every lane gets here
        const int cp = j < valid[u] ? seg_class<TP>(lp[u][j], a.C) : -1;
        const int ct = j < valid[u] ? seg_class<TT>(lt[u][j], a.C) : -1;
        if (a.mode == kSegRunMerge) {
          if (cp == rp && ct == rt) {
            ++rn;
          } else {
            if (rn != 0u) seg_add(sI, sP, sT, rp, rt, rn);
            rp = cp, rt = ct, rn = 1u;
          }
        } else if (a.mode == kSegWaveUniform) {
          const int fp = __builtin_amdgcn_readfirstlane(cp), ft = __builtin_amdgcn_readfirstlane(ct);
          if (__all(cp == fp && ct == ft)) {
            const uint32_t lanes = static_cast<uint32_t>(__popcll(__ballot(1)));
            if ((threadIdx.x & (kWave - 1)) == 0) seg_add(sI, sP, sT, fp, ft, lanes);
          } else {
            seg_add(sI, sP, sT, cp, ct, 1u);
          }
        } else {
          seg_add(sI, sP, sT, cp, ct, 1u);
        }
      }
    }
  }
  if (rn != 0u) seg_add(sI, sP, sT, rp, rt, rn);
  __syncthreads();

  int64_t* o = out + b * a.C * 3;
  for (int c = threadIdx.x; c < a.C; c += kSegThreads) {
    const uint32_t vi = sI[c], vp = sP[c], vt = sT[c];
    if (vi != 0u) atomic_add_i64(o + c * 3 + 0, vi);
    if (vp != 0u) atomic_add_i64(o + c * 3 + 1, vp);
    if (vt != 0u) atomic_add_i64(o + c * 3 + 2, vt);
  }
}

template <typename TP, typename TT>
__global__ __launch_bounds__(kSegThreads) void segment_overlap_index_vec_kernel(const TP* __restrict__ preds, const TT* __restrict__ target,
                                                                                int64_t* __restrict__ out, SegArgs a) {
  segment_index_body<TP, TT, true>(preds, target, out, a);
}

template <typename TP, typename TT>
__global__ __launch_bounds__(kSegThreads) void segment_overlap_index_generic_kernel(const TP* __restrict__ preds, const TT* __restrict__ target,
                                                                                    int64_t* __restrict__ out, SegArgs a) {
  segment_index_body<TP, TT, false>(preds, target, out, a);
}

// 0x80 in every byte of w that is nonzero
__device__ __forceinline__ uint32_t seg_nonzero_bytes(uint32_t w) { return (w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u; }

template <typename TP, typename TT, bool VEC>
__device__ __forceinline__ void segment_onehot_body(const TP* __restrict__ preds, const TT* __restrict__ target, int64_t* __restrict__ out, const SegArgs& a) {
  constexpr int R = 16 / static_cast<int>(sizeof(TP) > sizeof(TT) ? sizeof(TP) : sizeof(TT));
  constexpr int U = kSegPixels / R;
  constexpr bool kBytes = sizeof(TP) == 1 && sizeof(TT) == 1;  // R == 16, U == 1
  const int64_t wg = blockIdx.x;
  const int64_t plane = wg / a.chunks, chunk = wg % a.chunks;
  const TP* p = preds + plane * a.n;
  const TT* t = target + plane * a.n;
  const int64_t e0 = chunk * a.per_chunk, e1 = min(a.n, e0 + a.per_chunk);

  uint32_t ci = 0u, cp = 0u, ct = 0u;  // a lane sees at most a chunk's pixels
  for (int64_t base = e0; base < e1; base += kSegAlign) {
    if constexpr (kBytes) {
      const int64_t at = base + static_cast<int64_t>(threadIdx.x) * R;
      const int valid = at < e1 ? static_cast<int>(min(static_cast<int64_t>(R), e1 - at)) : 0;
      if (VEC && valid == R) {
        const uint4 vp = *reinterpret_cast<const uint4*>(p + at);
        const uint4 vt = *reinterpret_cast<const uint4*>(t + at);
        const uint32_t wp[4] = {vp.x, vp.y, vp.z, vp.w}, wt[4] = {vt.x, vt.y, vt.z, vt.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t mp = seg_nonzero_bytes(wp[k]), mt = seg_nonzero_bytes(wt[k]);
          ci += __popc(mp & mt), cp += __popc(mp), ct += __popc(mt);
        }
      } else {
        for (int j = 0; j < valid; ++j) {
          const bool bp = p[at + j] != TP(0), bt = t[at + j] != TT(0);
          ci += bp && bt, cp += bp, ct += bt;
        }
      }
    } else {
      TP lp[U][R];
      TT lt[U][R];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t at = base + (static_cast<int64_t>(u) * kSegThreads + threadIdx.x) * R;
        const int valid = at < e1 ? static_cast<int>(min(static_cast<int64_t>(R), e1 - at)) : 0;
        seg_load<TP, R, VEC>(p + at, valid, lp[u]);  // elements past ``valid`` read as 0: not a member
        seg_load<TT, R, VEC>(t + at, valid, lt[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const bool bp = lp[u][j] != TP(0), bt = lt[u][j] != TT(0);
          ci += bp && bt, cp += bp, ct += bt;
        }
      }
    }
  }

  __shared__ long long part[kSegThreads / kWave][3];
  const long long wi = wave_sum(static_cast<long long>(ci)), wp = wave_sum(static_cast<long long>(cp)), wt = wave_sum(static_cast<long long>(ct));
  const int wave = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) part[wave][0] = wi, part[wave][1] = wp, part[wave][2] = wt;
  __syncthreads();
  if (threadIdx.x < 3) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kSegThreads / kWave; ++w) s += part[w][threadIdx.x];
    if (s != 0) atomic_add_i64(out + plane * 3 + threadIdx.x, s);
  }
}

template <typename TP, typename TT>
__global__ __launch_bounds__(kSegThreads) void segment_overlap_onehot_vec_kernel(const TP* __restrict__ preds, const TT* __restrict__ target,
                                                                                 int64_t* __restrict__ out, SegArgs a) {
  segment_onehot_body<TP, TT, true>(preds, target, out, a);
}

template <typename TP, typename TT>
__global__ __launch_bounds__(kSegThreads) void segment_overlap_onehot_generic_kernel(const TP* __restrict__ preds, const TT* __restrict__ target,
                                                                                     int64_t* __restrict__ out, SegArgs a) {
  segment_onehot_body<TP, TT, false>(preds, target, out, a);
}

// ------------------------------------------------------------------------------------------------------------ scores
enum SegMetric { kSegIoU = 0, kSegDice = 1, kSegGeneralizedDice = 2 };
// option: IoU 0 mean over classes, 1 per class; Dice 0 micro, 1 macro, 2 weighted, 3 per class;
// generalized Dice weight + 3·per_class with weight 0 square, 1 simple, 2 linear

__device__ __forceinline__ double seg_sdiv(double a, double b) { return b != 0.0 ? a / b : 0.0; }
__device__ __forceinline__ double seg_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
  return v;
}
__device__ __forceinline__ double seg_weight(double T, int weight) { return weight == 0 ? 1.0 / (T * T) : (weight == 1 ? 1.0 / T : 1.0); }

// One wave per sample; lane l takes the classes c0 + l, c0 + l + 64, ...  out: [B] or [B, C - c0].
__global__ __launch_bounds__(kWave) void segment_scores_kernel(const int64_t* __restrict__ counts, double* __restrict__ out, int64_t C, int c0,
                                                               int metric, int option, bool per_class) {
  const int64_t b = blockIdx.x;
  const int64_t* k = counts + b * C * 3;
  const int64_t kept = C - c0;
  double* o = out + (per_class ? b * kept : b);
  const int weight = option % 3;

  double first = 0.0;  // generalized Dice: the largest finite weight of this sample; weighted Dice: Σ T
  if (metric == kSegGeneralizedDice && weight != 2) {
    for (int64_t c = c0 + threadIdx.x; c < C; c += kWave) {
      const double T = static_cast<double>(k[c * 3 + 2]);
      if (T != 0.0) first = fmax(first, seg_weight(T, weight));
    }
    first = seg_wave_max(first);
  } else if (metric == kSegDice && option == 2) {
    for (int64_t c = c0 + threadIdx.x; c < C; c += kWave) first += static_cast<double>(k[c * 3 + 2]);
    first = wave_sum(first);
  }

  double s0 = 0.0, s1 = 0.0;
  for (int64_t c = c0 + threadIdx.x; c < C; c += kWave) {
    const double I = static_cast<double>(k[c * 3]), P = static_cast<double>(k[c * 3 + 1]), T = static_cast<double>(k[c * 3 + 2]);
    double v = 0.0;  // the per-class value where the form has one
    if (metric == kSegIoU) {
      v = seg_sdiv(I, P + T - I);
      s0 += v;
    } else if (metric == kSegDice) {
      v = seg_sdiv(2.0 * I, P + T);
      if (option == 0) s0 += 2.0 * I, s1 += P + T;
      else if (option == 2) s0 += seg_sdiv(T, first) * v;
      else s0 += v;
    } else {
      const double w = (weight == 2 || T != 0.0) ? seg_weight(T, weight) : first;
      v = seg_sdiv(2.0 * I * w, (P + T) * w);
      s0 += 2.0 * I * w, s1 += (P + T) * w;
    }
    if (per_class) o[c - c0] = v;
  }
  if (per_class) return;
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if (threadIdx.x != 0) return;
  if (metric == kSegIoU || (metric == kSegDice && option == 1)) o[0] = s0 / static_cast<double>(kept);
  else if (metric == kSegDice && option == 2) o[0] = s0;
  else o[0] = seg_sdiv(s0, s1);
}

// ------------------------------------------------------------------------------------------------------------- host
namespace {

// pixels per chunk of a row when ``rows`` rows share the grid: a multiple of kSegAlign, at most kSegChunkMax.  TMX_SEGMENT_CHUNK
// (read per call, rounded up to the alignment) overrides it: it lets a test place chunk edges inside a tiny map.
int64_t segment_per_chunk(int64_t rows, int64_t n) {
  if (const char* env = std::getenv("TMX_SEGMENT_CHUNK")) {
    const long long v = std::atoll(env);
    if (v > 0) return (std::min<int64_t>(v, kSegChunkMax) + kSegAlign - 1) / kSegAlign * kSegAlign;
  }
  const int64_t want = std::max<int64_t>(1, (kSegTargetGroups + rows - 1) / rows);
  const int64_t most = std::max<int64_t>(1, n / kSegChunkMin);
  const int64_t chunks = std::min(want, most);
  const int64_t per = (n + chunks - 1) / chunks;
  return std::min((per + kSegAlign - 1) / kSegAlign * kSegAlign, kSegChunkMax);
}

int segment_mode() {
  if (const char* env = std::getenv("TMX_SEGMENT_MODE")) {
    const int v = std::atoi(env);
    if (v >= kSegPlain && v <= kSegRunMerge) return v;
  }
  return kSegRunMerge;
}

bool segment_vec_ok(const at::Tensor& p, const at::Tensor& t, int64_t rows, int64_t n) {
  const bool aligned = (reinterpret_cast<uintptr_t>(p.data_ptr()) & 15) == 0 && (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
  const bool rows_ok = rows == 1 || ((n * static_cast<int64_t>(p.element_size())) % 16 == 0 && (n * static_cast<int64_t>(t.element_size())) % 16 == 0);
  return aligned && rows_ok;
}

template <typename F>
void dispatch_label(at::ScalarType dtype, const char* name, F&& f) {
  switch (dtype) {
    case at::kByte: f(uint8_t{}); break;
    case at::kShort: f(int16_t{}); break;
    case at::kInt: f(int32_t{}); break;
    case at::kLong: f(int64_t{}); break;
    default: TORCH_CHECK(false, name, ": unsupported label dtype ", dtype);
  }
}

template <typename F>
void dispatch_mask(at::ScalarType dtype, const char* name, F&& f) {
  switch (dtype) {
    case at::kBool:  // one byte, nonzero = member: the uint8 instantiation
    case at::kByte: f(uint8_t{}); break;
    case at::kInt: f(int32_t{}); break;
    case at::kLong: f(int64_t{}); break;
    default: TORCH_CHECK(false, name, ": unsupported mask dtype ", dtype);
  }
}

void segment_check_pair(const char* name, const at::Tensor& preds, const at::Tensor& target, int64_t min_dim) {
  TORCH_CHECK(preds.is_cuda() && target.is_cuda(), name, ": expected GPU tensors");
  TORCH_CHECK(preds.device() == target.device(), name, ": preds and target on different devices");
  TORCH_CHECK(preds.dim() >= min_dim && preds.sizes() == target.sizes(), name, ": expected matching shapes with at least ", min_dim, " dims");
}

}  // namespace

// (threads per workgroup, pixels per lane per step, class cap of the index form, chunk alignment in pixels: the least
// TMX_SEGMENT_CHUNK): what the tests need to place their edge shapes
std::vector<int64_t> segment_overlap_tile() { return {kSegThreads, kSegPixels, kSegMaxClasses, kSegAlign}; }

// How many chunks the overlap kernels split every row of n pixels into (index form: B rows; one-hot form: B·C rows): a
// function of the shape alone (and of TMX_SEGMENT_CHUNK where a test sets it).  Only the last chunk may be short.
int64_t segment_overlap_chunks(int64_t B, int64_t n, int64_t C, bool onehot) {
  TORCH_CHECK(B >= 1 && n >= 1 && C >= 1, "segment_overlap_chunks: expected a non-empty shape");
  const int64_t per = segment_per_chunk(onehot ? B * C : B, n);
  return (n + per - 1) / per;
}

// int64 [B, C, 3] counts (I, P, T) of label maps preds / target [B, *spatial].
at::Tensor segment_overlap_index(const at::Tensor& preds_in, const at::Tensor& target_in, int64_t num_classes) {
  const char* name = "segment_overlap_index";
  segment_check_pair(name, preds_in, target_in, 2);
  TORCH_CHECK(num_classes >= 1 && num_classes <= kSegMaxClasses, name, ": num_classes must be in 1 .. ", kSegMaxClasses, ", got ", num_classes);
  const at::DeviceGuard guard(preds_in.device());
  const int64_t B = preds_in.size(0), n = B > 0 ? preds_in.numel() / B : 0, C = num_classes;
  auto out = at::zeros({B, C, 3}, preds_in.options().dtype(at::kLong));
  // dtypes are checked before the early return
  dispatch_label(preds_in.scalar_type(), name, [](auto) {});
  dispatch_label(target_in.scalar_type(), name, [](auto) {});
  if (B == 0 || n == 0) return out;
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  const int64_t per_chunk = segment_per_chunk(B, n), chunks = (n + per_chunk - 1) / per_chunk;
  TORCH_CHECK(B * chunks <= INT32_MAX, name, ": too many workgroups for one launch");
  const bool vec = segment_vec_ok(p, t, B, n);
  const SegArgs a{n, per_chunk, chunks, static_cast<int>(C), segment_mode()};
  const size_t lds = 3 * static_cast<size_t>(C) * sizeof(uint32_t);
  dispatch_label(p.scalar_type(), name, [&](auto ptag) {
    dispatch_label(t.scalar_type(), name, [&](auto ttag) {
      using TP = decltype(ptag);
      using TT = decltype(ttag);
      auto kernel = vec ? segment_overlap_index_vec_kernel<TP, TT> : segment_overlap_index_generic_kernel<TP, TT>;
      hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(B * chunks)), dim3(kSegThreads), lds, stream(), reinterpret_cast<const TP*>(p.data_ptr()),
                         reinterpret_cast<const TT*>(t.data_ptr()), out.data_ptr<int64_t>(), a);
      TMX_LAUNCH_CHECK();
    });
  });
  return out;
}

// int64 [B, C, 3] counts (I, P, T) of one-hot masks preds / target [B, C, *spatial], nonzero = member.
at::Tensor segment_overlap_onehot(const at::Tensor& preds_in, const at::Tensor& target_in) {
  const char* name = "segment_overlap_onehot";
  segment_check_pair(name, preds_in, target_in, 3);
  const at::DeviceGuard guard(preds_in.device());
  const int64_t B = preds_in.size(0), C = preds_in.size(1), planes = B * C, n = planes > 0 ? preds_in.numel() / planes : 0;
  auto out = at::zeros({B, C, 3}, preds_in.options().dtype(at::kLong));
  dispatch_mask(preds_in.scalar_type(), name, [](auto) {});
  dispatch_mask(target_in.scalar_type(), name, [](auto) {});
  if (planes == 0 || n == 0) return out;
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  const int64_t per_chunk = segment_per_chunk(planes, n), chunks = (n + per_chunk - 1) / per_chunk;
  TORCH_CHECK(planes * chunks <= INT32_MAX, name, ": too many workgroups for one launch");
  const bool vec = segment_vec_ok(p, t, planes, n);
  const SegArgs a{n, per_chunk, chunks, static_cast<int>(C), 0};
  dispatch_mask(p.scalar_type(), name, [&](auto ptag) {
    dispatch_mask(t.scalar_type(), name, [&](auto ttag) {
      using TP = decltype(ptag);
      using TT = decltype(ttag);
      auto kernel = vec ? segment_overlap_onehot_vec_kernel<TP, TT> : segment_overlap_onehot_generic_kernel<TP, TT>;
      hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(planes * chunks)), dim3(kSegThreads), 0, stream(), reinterpret_cast<const TP*>(p.data_ptr()),
                         reinterpret_cast<const TT*>(t.data_ptr()), out.data_ptr<int64_t>(), a);
      TMX_LAUNCH_CHECK();
    });
  });
  return out;
}

// fp64 scores of counts [B, C, 3]: [B], or [B, C'] for the per-class forms (C' = C, or C - 1 without the background class).
at::Tensor segment_scores(const at::Tensor& counts_in, int64_t metric, int64_t option, bool include_background) {
  const char* name = "segment_scores";
  TORCH_CHECK(counts_in.is_cuda(), name, ": expected a GPU tensor");
  TORCH_CHECK(counts_in.scalar_type() == at::kLong && counts_in.dim() == 3 && counts_in.size(2) == 3, name, ": expected int64 counts [B, C, 3]");
  TORCH_CHECK(metric >= kSegIoU && metric <= kSegGeneralizedDice, name, ": metric must be 0, 1 or 2");
  const int64_t options = metric == kSegIoU ? 2 : (metric == kSegDice ? 4 : 6);
  TORCH_CHECK(option >= 0 && option < options, name, ": option out of range for this metric");
  const int64_t B = counts_in.size(0), C = counts_in.size(1);
  const int c0 = include_background ? 0 : 1;
  TORCH_CHECK(C - c0 >= 1, name, ": no class left");
  TORCH_CHECK(B <= INT32_MAX, name, ": too many samples for one launch");
  const at::DeviceGuard guard(counts_in.device());
  const bool per_class = (metric == kSegIoU && option == 1) || (metric == kSegDice && option == 3) || (metric == kSegGeneralizedDice && option >= 3);
  const auto f64 = counts_in.options().dtype(at::kDouble);
  at::Tensor out = per_class ? at::empty({B, C - c0}, f64) : at::empty({B}, f64);
  if (B == 0) return out;
  auto counts = counts_in.contiguous();
  hipLaunchKernelGGL(segment_scores_kernel, dim3(static_cast<unsigned>(B)), dim3(kWave), 0, stream(), counts.data_ptr<int64_t>(), out.data_ptr<double>(), C, c0,
                     static_cast<int>(metric), static_cast<int>(option), per_class);
  TMX_LAUNCH_CHECK();
  return out;
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("segment_overlap_index(Tensor preds, Tensor target, int num_classes) -> Tensor");
  m.def("segment_overlap_onehot(Tensor preds, Tensor target) -> Tensor");
  m.def("segment_scores(Tensor counts, int metric, int option, bool include_background) -> Tensor");
  m.def("segment_overlap_chunks(int B, int n, int C, bool onehot) -> int", &tmx::segment_overlap_chunks);
  m.def("segment_overlap_tile() -> int[]", &tmx::segment_overlap_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("segment_overlap_index", &tmx::segment_overlap_index);
  m.impl("segment_overlap_onehot", &tmx::segment_overlap_onehot);
  m.impl("segment_scores", &tmx::segment_scores);
}
