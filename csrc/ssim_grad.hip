// Backward of the fused separable-window SSIM (csrc/image.hip ssim_sums) for gfx950.
//
// Per plane the forward returns S = Σ sim and CS = Σ cs over the valid KS×KS windows, both functions of the five
// window moments m0 = E[p], m1 = E[t], m2 = E[p²], m3 = E[t²], m4 = E[pt].  With upstream gradients gs, gc of the
// two sums, ω = gs·lum + gc and
//   U = 2(m4 − m0·m1) + c2    L = (m2 − m0²) + (m3 − m1²) + c2    A = 2·m0·m1 + c1    B = m0² + m1² + c1
// the moment coefficients of every window are (the E[p²] and E[t²] coefficients are equal)
//   a4 = 2ω/L    a2 = −ω·cs/L
//   a0 = ω(−2·m1 + 2·m0·cs)/L + gs·cs·(2·m1 − 2·m0·lum)/B
//   a1 = ω(−2·m0 + 2·m1·cs)/L + gs·cs·(2·m0 − 2·m1·lum)/B
// and with F(a)[y,x] = Σ_k Σ_l wy[k]·wx[l]·a[y−k, x−l] (zero outside the Hv×Wv map: the transposed window pass)
//   grad_p = F(a0) + 2p·F(a2) + t·F(a4)        grad_t = F(a1) + 2t·F(a2) + p·F(a4)
//
// Two kernels per chunk of planes:
//   ssim_coef_kernel    the forward's structure (256 columns per block, staged row segment in LDS, register ring of
//                       the last KS horizontal sums, compile-time KS) — writes the coefficient maps instead of
//                       reducing sim / cs: fp32 [chunk, NM, Hv, Wv], NM = 4 (both sides) or 3 (one side).
//   ssim_gather_kernel  one thread per output column, the same ring over the coefficient rows (zeros outside the
//                       map), NM horizontal sums per row, the vertical pass in registers, then the combination with
//                       p and t.  Gather only — no atomics, the result is deterministic.
// The planes are processed in chunks so the maps stay under a fixed scratch cap (TMX_SSIM_GRAD_SCRATCH_MB).
#include "common.h"
#include "window_moments.h"

#include <algorithm>
#include <cstdlib>
#include <tuple>
#include <type_traits>
#include <utility>

namespace tmx {

constexpr int kGradThreads = 256;  // columns per block (both kernels)
constexpr int kGradRows = 64;      // output rows per block (both kernels); each strip re-reads a KS − 1 row halo

template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ __hip_bfloat16 from_f32<__hip_bfloat16>(float v) { return __float2bfloat16(v); }
template <> __device__ __forceinline__ __half from_f32<__half>(float v) { return __float2half_rn(v); }

// maps: [chunk, NM, Hv, Wv] with NM = 2 + NP + NT, order (a0 if NP) (a1 if NT) a2 a4
template <typename T, int KS, bool NP, bool NT>
__global__ __launch_bounds__(kGradThreads) void ssim_coef_kernel(const T* __restrict__ preds, const T* __restrict__ target, int H,
                                                                 int W, const float* __restrict__ wx, const float* __restrict__ wy,
                                                                 const float* __restrict__ consts, const float* __restrict__ grad_sim,
                                                                 const float* __restrict__ grad_cs, float* __restrict__ maps) {
  constexpr int kSeg = kGradThreads + KS - 1;
  constexpr int NM = 2 + (NP ? 1 : 0) + (NT ? 1 : 0);
  __shared__ float sp[2][kSeg];
  __shared__ float st[2][kSeg];
  __shared__ float s_w[KS];

  const int Hv = H - KS + 1, Wv = W - KS + 1;
  const int64_t plane = blockIdx.z;  // within the chunk: preds / target / grads are offset by the host
  const int x0 = blockIdx.x * kGradThreads;
  const int y0 = blockIdx.y * kGradRows;
  const int tid = threadIdx.x;
  const T* P = preds + plane * static_cast<int64_t>(H) * W;
  const T* Tt = target + plane * static_cast<int64_t>(H) * W;
  float* M = maps + plane * NM * static_cast<int64_t>(Hv) * Wv;
  const int64_t map_stride = static_cast<int64_t>(Hv) * Wv;
  const float c1 = consts[0], c2 = consts[1];
  const float gs = grad_sim[plane], gc = grad_cs[plane];
  if (tid < KS) s_w[tid] = wx[tid];

  float wyr[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) wyr[k] = wy[k];

  float ring[KS][5];
#pragma unroll
  for (int k = 0; k < KS; ++k)
#pragma unroll
    for (int q = 0; q < 5; ++q) ring[k][q] = 0.f;

  const int out_rows = min(kGradRows, Hv - y0);
  const int in_rows = out_rows + KS - 1;  // input rows y0 .. y0 + in_rows - 1 (all < H)
  const bool col_ok = (x0 + tid) < Wv;

  auto stage = [&](int r, int buf) {
    const int64_t row = static_cast<int64_t>(y0 + r) * W;
    for (int i = tid; i < kSeg; i += kGradThreads) {
      const int x = x0 + i;
      const bool ok = x < W;
      sp[buf][i] = ok ? to_f32<T>(P[row + x]) : 0.f;
      st[buf][i] = ok ? to_f32<T>(Tt[row + x]) : 0.f;
    }
  };

  if (in_rows > 0) stage(0, 0);
  __syncthreads();

  for (int base = 0; base < in_rows; base += KS) {
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int r = base + j;
      if (r < in_rows) {  // uniform across the block
        const int buf = r & 1;
        if (r + 1 < in_rows) stage(r + 1, buf ^ 1);
        float hp = 0.f, ht = 0.f, hpp = 0.f, htt = 0.f, hpt = 0.f;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          const float w = s_w[k];
          const float p = sp[buf][tid + k];
          const float t = st[buf][tid + k];
          const float wp = w * p, wt = w * t;
          hp += wp;
          ht += wt;
          hpp = fmaf(wp, p, hpp);
          htt = fmaf(wt, t, htt);
          hpt = fmaf(wp, t, hpt);
        }
        ring[j][0] = hp;
        ring[j][1] = ht;
        ring[j][2] = hpp;
        ring[j][3] = htt;
        ring[j][4] = hpt;
        if (r >= KS - 1 && col_ok) {
          // vertical pass: rows r-KS+1 .. r live in ring[(j+1+k) % KS] (oldest first)
          float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int k = 0; k < KS; ++k) {
            const int slot = (j + 1 + k) % KS;
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] = fmaf(wyr[k], ring[slot][q], m[q]);
          }
          const SsimTerms s = ssim_terms(m[0], m[1], m[2], m[3], m[4], c2);
          const float a = 2.f * s.mu_pt + c1;
          const float b = s.mu_pp + s.mu_tt + c1;
          const float cs = s.upper / s.lower;
          const float lum = a / b;
          const float omega = fmaf(gs, lum, gc);
          const float ol = omega / s.lower;   // ω / L
          const float gb = gs * cs / b;     // gs·cs / B
          const int64_t o = static_cast<int64_t>(y0 + r - (KS - 1)) * Wv + (x0 + tid);
          int q = 0;
          if (NP) M[(q++) * map_stride + o] = 2.f * (ol * (m[0] * cs - m[1]) + gb * (m[1] - m[0] * lum));
          if (NT) M[(q++) * map_stride + o] = 2.f * (ol * (m[1] * cs - m[0]) + gb * (m[0] - m[1] * lum));
          M[(q++) * map_stride + o] = -ol * cs;
          M[q * map_stride + o] = 2.f * ol;
        }
        __syncthreads();  // staged row r+1 visible; buffer r free for r+2
      }
    }
  }
}

// One block = kGradThreads output columns x kGradRows output rows of one plane.  Output row y takes the coefficient
// rows y-KS+1 .. y, output column x the coefficient columns x-KS+1 .. x (zeros outside [0,Hv) x [0,Wv)).
template <typename T, int KS, bool NP, bool NT>
__global__ __launch_bounds__(kGradThreads) void ssim_gather_kernel(const T* __restrict__ preds, const T* __restrict__ target, int H,
                                                                   int W, const float* __restrict__ wx, const float* __restrict__ wy,
                                                                   const float* __restrict__ maps, T* __restrict__ grad_p,
                                                                   T* __restrict__ grad_t) {
  constexpr int kSeg = kGradThreads + KS - 1;
  constexpr int NM = 2 + (NP ? 1 : 0) + (NT ? 1 : 0);
  __shared__ float sm[2][NM][kSeg];
  __shared__ float s_w[KS];

  const int Hv = H - KS + 1, Wv = W - KS + 1;
  const int64_t plane = blockIdx.z;
  const int x0 = blockIdx.x * kGradThreads;
  const int y0 = blockIdx.y * kGradRows;
  const int tid = threadIdx.x;
  const int64_t map_stride = static_cast<int64_t>(Hv) * Wv;
  const float* M = maps + plane * NM * map_stride;
  const int64_t img = plane * static_cast<int64_t>(H) * W;
  // tap l of output column x reads coefficient column x - l = segment index tid + (KS-1) - l: reversed weights
  if (tid < KS) s_w[tid] = wx[KS - 1 - tid];

  float wyr[KS];  // slot order is oldest row first: row y - (KS-1) + k carries wy[KS-1-k]
#pragma unroll
  for (int k = 0; k < KS; ++k) wyr[k] = wy[KS - 1 - k];

  float ring[KS][NM];
#pragma unroll
  for (int k = 0; k < KS; ++k)
#pragma unroll
    for (int q = 0; q < NM; ++q) ring[k][q] = 0.f;

  const int out_rows = min(kGradRows, H - y0);
  const int in_rows = out_rows + KS - 1;  // coefficient rows cy0 .. cy0 + in_rows - 1, cy0 = y0 - (KS-1)
  const int cy0 = y0 - (KS - 1);
  const int cx0 = x0 - (KS - 1);
  const bool col_ok = (x0 + tid) < W;

  auto stage = [&](int r, int buf) {
    const int cy = cy0 + r;
    const bool row_ok = cy >= 0 && cy < Hv;
    const int64_t row = static_cast<int64_t>(cy) * Wv;
    for (int i = tid; i < kSeg; i += kGradThreads) {
      const int cx = cx0 + i;
      const bool ok = row_ok && cx >= 0 && cx < Wv;
#pragma unroll
      for (int q = 0; q < NM; ++q) sm[buf][q][i] = ok ? M[q * map_stride + row + cx] : 0.f;
    }
  };

  if (in_rows > 0) stage(0, 0);
  __syncthreads();

  for (int base = 0; base < in_rows; base += KS) {
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int r = base + j;
      if (r < in_rows) {  // uniform across the block
        const int buf = r & 1;
        if (r + 1 < in_rows) stage(r + 1, buf ^ 1);
        float h[NM];
#pragma unroll
        for (int q = 0; q < NM; ++q) h[q] = 0.f;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
          const float w = s_w[k];
#pragma unroll
          for (int q = 0; q < NM; ++q) h[q] = fmaf(w, sm[buf][q][tid + k], h[q]);
        }
#pragma unroll
        for (int q = 0; q < NM; ++q) ring[j][q] = h[q];
        if (r >= KS - 1 && col_ok) {
          float f[NM];
#pragma unroll
          for (int q = 0; q < NM; ++q) f[q] = 0.f;
#pragma unroll
          for (int k = 0; k < KS; ++k) {
            const int slot = (j + 1 + k) % KS;
#pragma unroll
            for (int q = 0; q < NM; ++q) f[q] = fmaf(wyr[k], ring[slot][q], f[q]);
          }
          const int64_t o = img + static_cast<int64_t>(cy0 + r) * W + (x0 + tid);  // output row y = cy0 + r in [y0, H)
          const float p = to_f32<T>(preds[o]);
          const float t = to_f32<T>(target[o]);
          const float f2 = f[NM - 2], f4 = f[NM - 1];
          if (NP) grad_p[o] = from_f32<T>(fmaf(2.f * p, f2, fmaf(t, f4, f[0])));
          if (NT) grad_t[o] = from_f32<T>(fmaf(2.f * t, f2, fmaf(p, f4, f[NP ? 1 : 0])));
        }
        __syncthreads();  // staged row r+1 visible; buffer r free for r+2
      }
    }
  }
}

template <typename T, int KS, bool NP, bool NT>
void launch_ssim_grad(const at::Tensor& p, const at::Tensor& t, const at::Tensor& wx, const at::Tensor& wy, const at::Tensor& consts,
                      const at::Tensor& gs, const at::Tensor& gc, at::Tensor& maps, at::Tensor& gp, at::Tensor& gt, int64_t plane0,
                      int64_t nplanes, int H, int W) {
  const int Hv = H - KS + 1, Wv = W - KS + 1;
  const int64_t off = plane0 * static_cast<int64_t>(H) * W;
  const T* pp = reinterpret_cast<const T*>(p.data_ptr()) + off;
  const T* tp = reinterpret_cast<const T*>(t.data_ptr()) + off;
  T* gpp = NP ? reinterpret_cast<T*>(gp.data_ptr()) + off : nullptr;
  T* gtp = NT ? reinterpret_cast<T*>(gt.data_ptr()) + off : nullptr;
  dim3 cgrid(static_cast<unsigned>((Wv + kGradThreads - 1) / kGradThreads), static_cast<unsigned>((Hv + kGradRows - 1) / kGradRows),
             static_cast<unsigned>(nplanes));
  hipLaunchKernelGGL((ssim_coef_kernel<T, KS, NP, NT>), cgrid, kGradThreads, 0, stream(), pp, tp, H, W, wx.data_ptr<float>(),
                     wy.data_ptr<float>(), consts.data_ptr<float>(), gs.data_ptr<float>() + plane0, gc.data_ptr<float>() + plane0,
                     maps.data_ptr<float>());
  dim3 ggrid(static_cast<unsigned>((W + kGradThreads - 1) / kGradThreads), static_cast<unsigned>((H + kGradRows - 1) / kGradRows),
             static_cast<unsigned>(nplanes));
  hipLaunchKernelGGL((ssim_gather_kernel<T, KS, NP, NT>), ggrid, kGradThreads, 0, stream(), pp, tp, H, W, wx.data_ptr<float>(),
                     wy.data_ptr<float>(), maps.data_ptr<float>(), gpp, gtp);
}

template <typename T, int KS, typename... Args>
void launch_ssim_grad_sides(bool np, bool nt, Args&&... args) {
  if (np && nt)
    launch_ssim_grad<T, KS, true, true>(std::forward<Args>(args)...);
  else if (np)
    launch_ssim_grad<T, KS, true, false>(std::forward<Args>(args)...);
  else
    launch_ssim_grad<T, KS, false, true>(std::forward<Args>(args)...);
}

// scratch cap of the coefficient maps in MB.  512 measured fastest of 64 / 128 / 512 at 32 x 3 x 1024² (forward + backward
// 4.49 / 2.82 / 2.14 ms, tools/ssim_grad_bench.py, profiles/ssim_backward_r7.json): a chunk of 1024² planes under 128 MB is
// 7 to 10 planes, too few workgroups to fill the 256 CUs, and that costs more than reading the maps back from HBM
static int64_t grad_scratch_bytes() {
  static const int64_t mb = [] {
    const char* e = std::getenv("TMX_SSIM_GRAD_SCRATCH_MB");
    const long v = e ? std::atol(e) : 0;
    return static_cast<int64_t>(v > 0 ? std::min(v, 16384L) : 512);
  }();
  return mb << 20;
}

// preds/target [P, H, W]; wx/wy fp32 [KS]; consts (c1, c2[, data range]) on the device; grad_sim/grad_cs [P]: the upstream
// gradients of ssim_sums' two per-plane sums.  Returns (grad_preds, grad_target) in the input dtype; a side that is
// not needed comes back as an empty tensor.
std::tuple<at::Tensor, at::Tensor> ssim_sums_backward(const at::Tensor& preds_in, const at::Tensor& target_in, const at::Tensor& wx_in,
                                                      const at::Tensor& wy_in, const at::Tensor& consts_in, const at::Tensor& grad_sim_in,
                                                      const at::Tensor& grad_cs_in, bool need_preds, bool need_target) {
  TORCH_CHECK(preds_in.is_cuda() && target_in.is_cuda(), "ssim_sums_backward: expected GPU tensors");
  TORCH_CHECK(preds_in.dim() == 3 && preds_in.sizes() == target_in.sizes(), "ssim_sums_backward: expected matching [P, H, W]");
  TORCH_CHECK(preds_in.scalar_type() == target_in.scalar_type(), "ssim_sums_backward: dtype mismatch");
  const auto dt = preds_in.scalar_type();
  TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16 || dt == at::kHalf, "ssim_sums_backward: unsupported dtype ", dt);
  const int64_t KS = wx_in.numel();
  TORCH_CHECK(wy_in.numel() == KS, "ssim_sums_backward: window size mismatch");
  TORCH_CHECK(KS % 2 == 1 && KS >= 3 && KS <= 15, "ssim_sums_backward: unsupported window size ", KS);
  const int64_t P = preds_in.size(0), H = preds_in.size(1), W = preds_in.size(2);
  TORCH_CHECK(H >= KS && W >= KS, "ssim_sums_backward: image smaller than the window");
  TORCH_CHECK(H < (int64_t{1} << 30) && W < (int64_t{1} << 30), "ssim_sums_backward: plane too large");
  TORCH_CHECK(consts_in.numel() >= 2, "ssim_sums_backward: consts holds (c1, c2[, data range])");
  TORCH_CHECK(grad_sim_in.numel() == P && grad_cs_in.numel() == P, "ssim_sums_backward: expected [P] upstream gradients");
  for (const at::Tensor* x : {&wx_in, &wy_in, &consts_in, &grad_sim_in, &grad_cs_in})
    TORCH_CHECK(x->device() == preds_in.device(), "ssim_sums_backward: every tensor must be on the inputs' device");
  TORCH_CHECK(target_in.device() == preds_in.device(), "ssim_sums_backward: every tensor must be on the inputs' device");
  const at::DeviceGuard guard(preds_in.device());
  auto empty = [&] { return at::empty({0}, preds_in.options()); };
  if (!need_preds && !need_target) return {empty(), empty()};
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  auto wx = wx_in.to(at::kFloat).contiguous();
  auto wy = wy_in.to(at::kFloat).contiguous();
  auto consts = consts_in.to(at::kFloat).contiguous();
  auto gs = grad_sim_in.reshape(-1).to(at::kFloat).contiguous();
  auto gc = grad_cs_in.reshape(-1).to(at::kFloat).contiguous();
  auto gp = need_preds ? at::empty_like(p) : empty();
  auto gt = need_target ? at::empty_like(t) : empty();
  if (P == 0) return {gp, gt};
  const int64_t Hv = H - KS + 1, Wv = W - KS + 1;
  const int64_t nm = 2 + (need_preds ? 1 : 0) + (need_target ? 1 : 0);
  const int64_t per_plane = nm * Hv * Wv;  // floats
  // (the planes of a chunk are the grid's z axis: at most kMaxGridPlanes of them, whatever the scratch would hold)
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({P, kMaxGridPlanes, grad_scratch_bytes() / 4 / per_plane}));
  auto maps = at::empty({chunk * per_plane}, p.options().dtype(at::kFloat));
  for (int64_t p0 = 0; p0 < P; p0 += chunk) {
    const int64_t n = std::min(chunk, P - p0);
    dispatch_float3(dt, "ssim_sums_backward", [&](auto tag) {
      dispatch_odd_window(KS, "ssim_sums_backward", [&](auto ks) {
        launch_ssim_grad_sides<decltype(tag), decltype(ks)::value>(need_preds, need_target, p, t, wx, wy, consts, gs, gc, maps, gp, gt, p0,
                                                                   n, static_cast<int>(H), static_cast<int>(W));
      });
    });
    TMX_LAUNCH_CHECK();
  }
  return {gp, gt};
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def(
      "ssim_sums_backward(Tensor preds, Tensor target, Tensor wx, Tensor wy, Tensor consts, Tensor grad_sim, Tensor grad_cs, "
      "bool need_preds, bool need_target) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) { m.impl("ssim_sums_backward", &tmx::ssim_sums_backward); }
