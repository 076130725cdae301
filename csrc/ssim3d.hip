// Fused separable-window SSIM of volumes ([P, D, H, W] planes, P = B*C) for gfx950: tmx::ssim3d_sums.
//
// The reference reflect-pads both volumes in 3-D, stacks (p, t, p², t², p·t) into a 5·B batch, runs one dense grouped
// conv3d (KS³ taps) and crops the padded border.  As in 2-D (csrc/image.hip) the cropped region is exactly the set of
// windows that lie fully inside the volume, so the per-volume SSIM is the mean over all *valid* windows of a separable
// window: 5·(KSd + KSh + KSw) MACs per output voxel instead of 5·KSd·KSh·KSw, and no temporary in HBM.
//
// Chosen constants (exported to Python by tmx::ssim3d_tile):
//   kS3TH x kS3TW = 16 x 16 output footprint per 256-thread workgroup, one output pixel per thread.  Measured at op level
//     (gaussian 11-tap windows, fp32, 4 x 64^3 / 4 x 128^3 / 1 x 256^3, tools/ssim3d_bench.py --op-lib): 16 x 16
//     0.050 / 0.130 / 0.218 ms, 8 x 32 0.059 / 0.150 / 0.251 ms, 4 x 64 0.074 / 0.189 / 0.312 ms.  The square footprint
//     restages the least halo (2.6x the outputs at KS = 11, 3.0x for 8 x 32) and runs the W pass over the fewest tile
//     rows (26 / 16 against 18 / 8 per output row), which outweighs the 2-way bank conflicts of its W-pass reads
//     (two 16-pixel rows per 32-lane group; 8 x 32 reads one contiguous row and is conflict-free);
//   strip: output slices per workgroup along D, chosen on the host (see ssim3d_sums), minimum 1; TMX_SSIM3D_STRIP
//     overrides it;
//   ring: the last KSd slices' five 2-D-filtered moments live in registers (5·KSd VGPRs per thread), addressed with
//     compile-time indices: the slice loop is unrolled by KSd and the kernel is a template on KSd only (7 window sizes
//     x 3 dtypes).  KSh and KSw are run-time bounds of the LDS loops.
//
// A workgroup owns one footprint of one volume and one strip of output slices and marches along D.  Per input slice:
//   1. the (16 + KSh − 1) x (16 + KSw − 1) tile of (p, t), prefetched into registers during the previous slice, is
//      stored to LDS interleaved as float2;
//   2. W pass: every (tile row, output column) item reads KSw float2 from LDS and writes the five row moments
//      (mu_p, mu_t), (E[pp], E[tt]), E[pt] to an LDS intermediate (packed fp32 arithmetic as ssim_v2_kernel);
//   3. H pass: every thread reads KSh rows of the intermediate for its own output pixel;
//   4. the result enters the register ring; once KSd slices are in, the D pass runs from the ring, then the epilogue
//      of ssim_valid_kernel (IEEE divisions) and the fp64 accumulation.
// Two barriers per slice, no double buffers: the tile store of slice r + 1 follows the barrier that ends the W pass of
// slice r, and the W pass of slice r + 1 follows the barrier that every thread reaches after its H pass of slice r.
// One fp64 partial pair per workgroup, folded by a sum on the host side of the op: no atomics, deterministic.
#include "common.h"
#include "window_moments.h"

#include <cstdlib>
#include <vector>

namespace tmx {

constexpr int kS3Threads = 256;
#ifndef TMX_SSIM3D_TH  // (compile-time A/B of the footprint: tools/ssim3d_bench.py --op-lib; TH x TW must stay 256)
#define TMX_SSIM3D_TH 16
#define TMX_SSIM3D_TW 16
#endif
constexpr int kS3TH = TMX_SSIM3D_TH, kS3TW = TMX_SSIM3D_TW;
constexpr int kS3MinStrip = 1;
constexpr int kS3MaxKS = 15;
constexpr int kS3MaxRows = kS3TH + kS3MaxKS - 1;                                    // 30 tile rows
constexpr int kS3MaxSeg = kS3TW + kS3MaxKS - 1;                                     // 30 tile columns
constexpr int kS3StagePer = (kS3MaxRows * kS3MaxSeg + kS3Threads - 1) / kS3Threads;  // 4 staged pixels per thread
constexpr int kS3RowPer = (kS3MaxRows * kS3TW + kS3Threads - 1) / kS3Threads;        // 2 W-pass items per thread
static_assert(kS3TH * kS3TW == kS3Threads, "one output pixel per thread");

// grid: x = ((plane * n_strips + strip) * tiles_h + tile_y) * tiles_w + tile_x, which is also the partial's index
template <typename T, int KSD>
__global__ __launch_bounds__(kS3Threads) void ssim3d_kernel(const T* __restrict__ preds, const T* __restrict__ target, int D, int H,
                                                            int W, int KSH, int KSW, int strip, int n_strips, int tiles_h,
                                                            int tiles_w, const float* __restrict__ wd, const float* __restrict__ wh,
                                                            const float* __restrict__ ww, const float* __restrict__ consts,
                                                            double* __restrict__ part_sim, double* __restrict__ part_cs) {
  __shared__ f2 s_pt[kS3MaxRows * kS3MaxSeg];
  __shared__ f2 s_m01[kS3MaxRows * kS3TW];
  __shared__ f2 s_m23[kS3MaxRows * kS3TW];
  __shared__ float s_m4[kS3MaxRows * kS3TW];
  __shared__ float s_wh[kS3MaxKS], s_ww[kS3MaxKS];

  const int tid = threadIdx.x;
  unsigned b = blockIdx.x;
  const int x0 = static_cast<int>(b % tiles_w) * kS3TW;
  b /= tiles_w;
  const int y0 = static_cast<int>(b % tiles_h) * kS3TH;
  b /= tiles_h;
  const int z0 = static_cast<int>(b % n_strips) * strip;
  const int64_t plane = b / n_strips;

  const int Dv = D - KSD + 1, Hv = H - KSH + 1, Wv = W - KSW + 1;
  const int out_slices = min(strip, Dv - z0);
  const int in_slices = out_slices + KSD - 1;  // input slices z0 .. z0 + in_slices - 1 (< D)
  const int rows = kS3TH + KSH - 1, seg = kS3TW + KSW - 1;
  const int n_stage = rows * seg, n_row = rows * kS3TW;
  const int64_t slice = static_cast<int64_t>(H) * W;
  const T* P = preds + (plane * D + z0) * slice;
  const T* Tt = target + (plane * D + z0) * slice;
  const float c1 = consts[0], c2 = consts[1];
  if (tid < KSH) s_wh[tid] = wh[tid];
  if (tid < KSW) s_ww[tid] = ww[tid];
  float wdr[KSD];
#pragma unroll
  for (int k = 0; k < KSD; ++k) wdr[k] = wd[k];

  // this thread's staged pixels: offset inside a slice, or -1 outside the tile / the volume (zero-filled: such
  // pixels only reach windows that are masked below)
  int off[kS3StagePer];
#pragma unroll
  for (int i = 0; i < kS3StagePer; ++i) {
    const int e = tid + i * kS3Threads;
    const int r = e / seg, c = e - r * seg;
    const int y = y0 + r, x = x0 + c;
    off[i] = (e < n_stage && y < H && x < W) ? y * W + x : -1;
  }
  float pre_p[kS3StagePer], pre_t[kS3StagePer];
  auto fetch = [&](int z) {
    const T* Pz = P + z * slice;
    const T* Tz = Tt + z * slice;
#pragma unroll
    for (int i = 0; i < kS3StagePer; ++i) {
      const bool ok = off[i] >= 0;
      pre_p[i] = ok ? to_f32<T>(Pz[off[i]]) : 0.f;
      pre_t[i] = ok ? to_f32<T>(Tz[off[i]]) : 0.f;
    }
  };

  // ring of H·W-filtered moments of the last KSD slices: (mu_p, mu_t), (E[pp], E[tt]) packed, E[pt] scalar
  f2 rm[KSD], rq[KSD];
  float rx[KSD];
#pragma unroll
  for (int k = 0; k < KSD; ++k) {
    rm[k] = f2{0.f, 0.f};
    rq[k] = f2{0.f, 0.f};
    rx[k] = 0.f;
  }
  const int ty = tid / kS3TW, tx = tid % kS3TW;
  const bool px_ok = y0 + ty < Hv && x0 + tx < Wv;
  double acc_sim = 0.0, acc_cs = 0.0;

  if (in_slices > 0) fetch(0);
  for (int base = 0; base < in_slices; base += KSD) {
#pragma unroll
    for (int j = 0; j < KSD; ++j) {
      const int r = base + j;
      if (r < in_slices) {  // uniform across the workgroup
#pragma unroll
        for (int i = 0; i < kS3StagePer; ++i) {
          const int e = tid + i * kS3Threads;
          if (e < n_stage) s_pt[e] = f2{pre_p[i], pre_t[i]};
        }
        __syncthreads();  // tile of slice r visible; every thread has finished the H pass of slice r - 1
        if (r + 1 < in_slices) fetch(r + 1);  // in flight during this slice's arithmetic
        // W pass
#pragma unroll
        for (int i = 0; i < kS3RowPer; ++i) {
          const int e = tid + i * kS3Threads;
          if (e < n_row) {
            const Moments5 h = moments5_taps(s_pt + (e / kS3TW) * seg + (e % kS3TW), KSW, [&](int k) { return s_ww[k]; });
            s_m01[e] = h.m01;
            s_m23[e] = h.m23;
            s_m4[e] = h.m4;
          }
        }
        __syncthreads();  // row moments visible; the tile buffer is free for slice r + 1
        // H pass for this thread's output pixel
        Moments5 v;
        for (int k = 0; k < KSH; ++k) {
          const int idx = (ty + k) * kS3TW + tx;
          v.add(s_wh[k], s_m01[idx], s_m23[idx], s_m4[idx]);
        }
        rm[j] = v.m01;
        rq[j] = v.m23;
        rx[j] = v.m4;
        if (r >= KSD - 1 && px_ok) {
          // D pass: slices r - KSD + 1 .. r live in ring slot (j + 1 + k) % KSD (oldest first)
          const Moments5 m = moments5_ring(rm, rq, rx, j, [&](int k) { return wdr[k]; });
          float sim, cs;
          ssim_finish_ieee(ssim_terms(m.m01.x, m.m01.y, m.m23.x, m.m23.y, m.m4, c2), c1, sim, cs);
          acc_sim += static_cast<double>(sim);
          acc_cs += static_cast<double>(cs);
        }
      }
    }
  }

  double acc[2] = {acc_sim, acc_cs};
  block_sum_store<2, kS3Threads>(acc, {part_sim, part_cs}, [&] { return blockIdx.x; });
}

template <typename T, int KSD, typename... Args>
void launch_ssim3d_ks(const at::Tensor& p, const at::Tensor& t, unsigned grid, Args... args) {
  hipLaunchKernelGGL((ssim3d_kernel<T, KSD>), dim3(grid), dim3(kS3Threads), 0, stream(), reinterpret_cast<const T*>(p.data_ptr()),
                     reinterpret_cast<const T*>(t.data_ptr()), args...);
}

// (footprint rows, footprint columns, smallest strip): what the tests need to build their edge shapes
std::vector<int64_t> ssim3d_tile() { return {kS3TH, kS3TW, kS3MinStrip}; }

// preds/target [P, D, H, W] volumes (P = B*C), fp32 / bf16 / fp16; wd/wh/ww fp32 1-D windows of the D, H and W axes (odd
// lengths 3 .. 15, possibly different); consts fp32 (c1, c2) on the device.
// Returns fp64 [2, P]: per-volume sums of SSIM and contrast sensitivity over all valid windows.
at::Tensor ssim3d_sums(const at::Tensor& preds_in, const at::Tensor& target_in, const at::Tensor& wd_in, const at::Tensor& wh_in,
                       const at::Tensor& ww_in, const at::Tensor& consts_in) {
  TORCH_CHECK(preds_in.is_cuda() && target_in.is_cuda() && wd_in.is_cuda() && wh_in.is_cuda() && ww_in.is_cuda() && consts_in.is_cuda(),
              "ssim3d_sums: expected GPU tensors");
  TORCH_CHECK(preds_in.dim() == 4 && preds_in.sizes() == target_in.sizes(), "ssim3d_sums: expected matching [P, D, H, W]");
  TORCH_CHECK(preds_in.scalar_type() == target_in.scalar_type(), "ssim3d_sums: dtype mismatch");
  const auto dtype = preds_in.scalar_type();
  TORCH_CHECK(dtype == at::kFloat || dtype == at::kBFloat16 || dtype == at::kHalf, "ssim3d_sums: unsupported dtype ", dtype);
  TORCH_CHECK(consts_in.numel() >= 2, "ssim3d_sums: consts must hold (c1, c2)");
  const int64_t KSd = wd_in.numel(), KSh = wh_in.numel(), KSw = ww_in.numel();
  for (const int64_t ks : {KSd, KSh, KSw})
    TORCH_CHECK(ks % 2 == 1 && ks >= 3 && ks <= kS3MaxKS, "ssim3d_sums: unsupported window size ", ks, " (odd, 3 .. 15)");
  const at::DeviceGuard guard(preds_in.device());
  auto p = preds_in.contiguous();
  auto t = target_in.contiguous();
  auto wd = wd_in.to(at::kFloat).contiguous();
  auto wh = wh_in.to(at::kFloat).contiguous();
  auto ww = ww_in.to(at::kFloat).contiguous();
  auto consts = consts_in.to(at::kFloat).contiguous();
  const int64_t P = p.size(0), D = p.size(1), H = p.size(2), W = p.size(3);
  TORCH_CHECK(D >= KSd && H >= KSh && W >= KSw, "ssim3d_sums: volume smaller than the window");
  TORCH_CHECK(H * W <= INT32_MAX && D <= INT32_MAX, "ssim3d_sums: slice too large");
  auto opts = p.options().dtype(at::kDouble);
  if (P == 0) return at::zeros({2, 0}, opts);
  const int64_t Dv = D - KSd + 1, Hv = H - KSh + 1, Wv = W - KSw + 1;
  const int64_t tiles_h = (Hv + kS3TH - 1) / kS3TH, tiles_w = (Wv + kS3TW - 1) / kS3TW;
  const int64_t tiles = tiles_h * tiles_w;
  // Output slices per workgroup.  A strip reads strip + KSd - 1 input slices, so short strips recompute: the host cuts D
  // into as many strips as still fit one resident wave of workgroups (256 CUs x 4, the occupancy the 110 VGPRs of
  // KSd = 11 allow; one more strip than that starts a second, mostly empty wave: with the 8 x 32 footprint a whole call
  // at 1 x 256^3 took 0.44 ms with 5 strips and 0.37 ms with 4; the sweep is in profiles/ssim3d_bench.json) and never goes below KSd - 1 slices (at most twice the work) unless D
  // itself is shorter.  Read per call, so a test can place a strip edge in a tiny volume.
  int64_t strip;
  if (const char* env = std::getenv("TMX_SSIM3D_STRIP")) {
    strip = std::min<int64_t>(Dv, std::max<int64_t>(kS3MinStrip, std::atoll(env)));
  } else {
    constexpr int64_t kResidentGroups = 4 * 256;
    const int64_t want_strips = std::max<int64_t>(1, std::min<int64_t>(Dv, kResidentGroups / (P * tiles)));
    strip = (Dv + want_strips - 1) / want_strips;
    strip = std::min<int64_t>(Dv, std::max<int64_t>(strip, KSd - 1));
  }
  const int64_t n_strips = (Dv + strip - 1) / strip;
  const int64_t groups = P * n_strips * tiles;  // all in grid.x: no 65535 limit on planes x strips
  TORCH_CHECK(groups <= INT32_MAX, "ssim3d_sums: too many workgroups for one launch (", groups, ")");
  auto partial = at::empty({2, P, n_strips * tiles}, opts);
  double* ps = partial.data_ptr<double>();
  double* pc = ps + groups;
  dispatch_float3(dtype, "ssim3d_sums", [&](auto tag) {
    dispatch_odd_window(KSd, "ssim3d_sums", [&](auto ksd) {
      launch_ssim3d_ks<decltype(tag), decltype(ksd)::value>(
          p, t, static_cast<unsigned>(groups), static_cast<int>(D), static_cast<int>(H), static_cast<int>(W), static_cast<int>(KSh),
          static_cast<int>(KSw), static_cast<int>(strip), static_cast<int>(n_strips), static_cast<int>(tiles_h), static_cast<int>(tiles_w),
          wd.data_ptr<float>(), wh.data_ptr<float>(), ww.data_ptr<float>(), consts.data_ptr<float>(), ps, pc);
    });
  });
  TMX_LAUNCH_CHECK();
  return partial.sum(2);
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("ssim3d_sums(Tensor preds, Tensor target, Tensor wd, Tensor wh, Tensor ww, Tensor consts) -> Tensor");
  m.def("ssim3d_tile() -> int[]", &tmx::ssim3d_tile);
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) { m.impl("ssim3d_sums", &tmx::ssim3d_sums); }
