// Separable-window moment code shared by the SSIM, 3-D SSIM, SSIM-backward and VIF kernels (csrc/image.hip via
// ssim_kernels.h, ssim3d.hip, ssim_grad.hip, vif.hip) and the block sum they and the LPIPS heads end with.
// Device code only, no torch headers: tools/kexp/ssim_mfma_exp.hip includes it through ssim_kernels.h.
// The five window moments of a pixel pair (p, t) are m0 = E[p], m1 = E[t], m2 = E[pp], m3 = E[tt], m4 = E[pt].
// Everything here was checked to leave the kernels' register, scratch and LDS use as it was.  Two things were tried and
// are NOT here, because hipcc (ROCm 7.2, gfx950) then allocates the kernels differently:
//   * the scalar row march of ssim_valid_kernel / ssim_coef_kernel as one function template: even the unchanged body
//     of ssim_valid_kernel moved into a force-inlined device function changes its VGPR count (bf16 KS 11: 130 -> 134),
//     and with the per-window functor the fp32 KS 9 kernel went from 96 to over 108 VGPRs;
//   * one loop for the second (LDS to register) pass of ssim3d_kernel / vif_scale_kernel: 2 more VGPRs in every
//     ssim3d_kernel.  Those loops stay in their kernels, on Moments5::add.
#pragma once

#include "device_common.h"

#include <type_traits>

namespace tmx {

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 splat2(float w) { return f2{w, w}; }

// The five moments on packed fp32 pairs (v_pk_mul / v_pk_add / v_pk_fma): (mu_p, mu_t) and (E[pp], E[tt]) share
// instructions, E[pt] is scalar.  Every loop below takes the weight of tap k as w(k): a float, or a pair that the caller
// splatted beforehand (ssim_v2_kernel keeps its weights that way: no per-tap register moves).
struct Moments5 {
  f2 m01 = f2{0.f, 0.f}, m23 = f2{0.f, 0.f};
  float m4 = 0.f;

  // one tap of the first pass over v = (p, t)
  __device__ __forceinline__ void tap(f2 w2, f2 v) {
    const f2 wv = w2 * v;                            // (w p, w t)
    m01 += wv;
    m23 = __builtin_elementwise_fma(wv, v, m23);     // (w p p, w t t)
    m4 = fmaf(wv.x, v.y, m4);                        // w p t
  }
  __device__ __forceinline__ void tap(float w, f2 v) { tap(splat2(w), v); }
  // one tap of a later pass over already filtered moments (sources by reference: each is loaded where it is used,
  // as in the loops this replaces; loading all three first cost ssim3d_kernel two VGPRs)
  __device__ __forceinline__ void add(f2 w2, float w, const f2& s01, const f2& s23, const float& s4) {
    m01 = __builtin_elementwise_fma(w2, s01, m01);
    m23 = __builtin_elementwise_fma(w2, s23, m23);
    m4 = fmaf(w, s4, m4);
  }
  __device__ __forceinline__ void add(f2 w2, const f2& s01, const f2& s23, const float& s4) { add(w2, w2.x, s01, s23, s4); }
  __device__ __forceinline__ void add(float w, const f2& s01, const f2& s23, const float& s4) { add(splat2(w), w, s01, s23, s4); }
};

// first pass: n taps over consecutive (p, t) pairs in LDS.  n is known at compile time (std::integral_constant<int, N>:
// the loop is unrolled) or at run time (int), as each caller had it.
template <typename Count, typename Wt>
__device__ __forceinline__ Moments5 moments5_taps(const f2* src, Count n, Wt w) {
  Moments5 h;
  if constexpr (std::is_same_v<Count, int>) {
    for (int k = 0; k < n; ++k) h.tap(w(k), src[k]);
  } else {
#pragma unroll
    for (int k = 0; k < Count::value; ++k) h.tap(w(k), src[k]);
  }
  return h;
}

// last pass over a register ring of the last KS results (rm, rq, rx: the three members, one array each), slot j written
// last: slot (j + 1 + k) % KS is the k-th oldest.  The caller's loop over j is unrolled by KS, so every slot index is a
// compile-time constant.
template <int KS, typename Wt>
__device__ __forceinline__ Moments5 moments5_ring(const f2 (&rm)[KS], const f2 (&rq)[KS], const float (&rx)[KS], int j, Wt w) {
  Moments5 m;
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    const int slot = (j + 1 + k) % KS;  // oldest first
    m.add(w(k), rm[slot], rq[slot], rx[slot]);
  }
  return m;
}

// ------------------------------------------------------------------------------------------------------------
// The terms of one window's SSIM.  The two finishes round differently and stay distinct: IEEE divisions
// (ssim_valid_kernel, ssim3d_kernel, ssim_coef_kernel) and hardware reciprocals (ssim_v2_kernel).
struct SsimTerms {
  float mu_pp, mu_tt, mu_pt, upper, lower;
};

__device__ __forceinline__ SsimTerms ssim_terms(float m0, float m1, float m2, float m3, float m4, float c2) {
  SsimTerms s;
  s.mu_pp = m0 * m0, s.mu_tt = m1 * m1, s.mu_pt = m0 * m1;
  s.upper = 2.f * (m4 - s.mu_pt) + c2;
  s.lower = (m2 - s.mu_pp) + (m3 - s.mu_tt) + c2;
  return s;
}

__device__ __forceinline__ void ssim_finish_ieee(const SsimTerms& s, float c1, float& sim, float& cs) {
  cs = s.upper / s.lower;
  sim = (2.f * s.mu_pt + c1) * s.upper / ((s.mu_pp + s.mu_tt + c1) * s.lower);
}

// hardware reciprocals (1 ulp) instead of two IEEE divisions (~10 instructions each)
__device__ __forceinline__ void ssim_finish_rcp(const SsimTerms& s, float c1, float& sim, float& cs) {
  cs = s.upper * __builtin_amdgcn_rcpf(s.lower);
  sim = (2.f * s.mu_pt + c1) * cs * __builtin_amdgcn_rcpf(s.mu_pp + s.mu_tt + c1);
}

// ------------------------------------------------------------------------------------------------------------
// Block sum of N per-thread fp64 values: wave shuffles, one LDS slot per (value, wave), one barrier, then thread 0 adds
// the waves in index order and stores value n to out[n][index()] (index is a functor: only thread 0 evaluates it).
// Deterministic: no atomics.  Every thread of the block must call it.  ssim_valid_kernel and ssim_v2_kernel keep this
// written out: with the call their SGPR spill counts change.
template <int N, int kThreads, typename Idx>
__device__ __forceinline__ void block_sum_store(double (&v)[N], double* const (&out)[N], Idx index) {
  __shared__ double red[N][kThreads / kWave];
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = wave_sum(v[n]);
  const int tid = threadIdx.x;
  const int wave = tid / kWave, lane = tid & (kWave - 1);
  if (lane == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) red[n][wave] = v[n];
  }
  __syncthreads();
  if (tid == 0) {
    double s[N];
#pragma unroll
    for (int n = 0; n < N; ++n) s[n] = 0.0;
    for (int w = 0; w < kThreads / kWave; ++w) {
#pragma unroll
      for (int n = 0; n < N; ++n) s[n] += red[n][w];
    }
    const int64_t idx = index();
#pragma unroll
    for (int n = 0; n < N; ++n) out[n][idx] = s[n];
  }
}

}  // namespace tmx
