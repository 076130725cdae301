// fp32 3x3 convolution (stride 1, zero padding 1) on the f16 matrix cores: the LPIPS VGG16 trunk.
//
// The product is the split-f16 one of pairwise.hip's x3 kernels: every fp32 value t (scaled by a power of two so that the
// largest lands in [2^14, 2^15)) is hi = f16(t), lo = f16(t - hi), and a dot product is hi·lo + lo·hi + hi·hi on
// v_mfma_f32_16x16x32_f16 with fp32 accumulation (the small terms first; the dropped lo·lo is below 2^-22 of |x||w|).
// A 3x3 convolution is that product with M = pixels, N = C_out, K = 9 C_in; this file adds the implicit-GEMM data movement.
//
//  * Activations stay fp32 NHWC (channels_last) in HBM and are split while they are staged into LDS.  The scale has to be
//    constant along K and a GEMM row is a 3x3 neighbourhood, so it is one power of two per IMAGE, from ``x_absmax[b]``.  Every
//    launch gathers its output's per-image max |y| in the epilogue (one atomicMax on the bit pattern per workgroup), so only
//    the network input needs a reduction launch of its own (conv3x3_absmax_kernel).
//  * Weights are split once (conv3x3_pack_kernel), one shift per output channel, into [C_in/32][tap 0..8][C_out][hi 32 | lo 32]
//    halves: the K loop walks that array front to back, one [C_out tile][64] block per step.
//  * A workgroup (256 threads, 4 waves) owns an 8 x 16 patch of one image x NT output channels (NT = 128: 2 x 2 waves of
//    64 couts x 64 pixels, 4 x 4 MFMA tiles; NT = 64: 4 waves of 64 couts x 32 pixels).  The MFMA's A operand is the weight
//    block, B the pixels: a lane then ends with four consecutive output channels of one pixel, one 16-byte NHWC store.
//  * K loop: per 32-channel slice the 10 x 18 halo patch (both planes, rows padded to 72 halves like pairwise.hip's tiles) is
//    staged once, out-of-image pixels as zeros without a load; the nine taps read their pixel fragments from it at shifted
//    offsets, so the 9-fold reuse happens in LDS.  The weight block of the next step and the fp32 patch of the next slice
//    wait in registers during the MFMAs.  LDS: 25.9 KB patch + 2 x 18.4 KB weights (NT = 128): two workgroups per CU.
//  * C_in = 3 (K = 27) is one step: the 128 x 27 im2col block is gathered straight into LDS, columns 27..31 as zeros.
//
// Non-finite activations: an image whose max is inf / NaN is staged unscaled, so its own outputs go non-finite where the
// composition's would; no other image reads its scale.  Weights are checked finite when packed.
#include "conv_split.h"

#include <algorithm>

namespace tmx {

constexpr int kCvTH = 8, kCvTW = 16, kCvHaloW = kCvTW + 2, kCvHalo = (kCvTH + 2) * kCvHaloW;  // 180 halo pixels

// max |x| per image as a bit pattern (NaN orders above inf there, so a NaN anywhere makes the image's max NaN).
// x: [B][n] fp32, out: [B] zero-initialised; chunks workgroups per image.
__global__ __launch_bounds__(kCvThreads) void conv3x3_absmax_kernel(const float* __restrict__ x, int64_t n, int chunks,
                                                                    unsigned int* __restrict__ out) {
  __shared__ unsigned int red[kCvThreads / kWave];
  const int64_t b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const float* __restrict__ xb = x + b * n;
  unsigned int m = 0;
  for (int64_t i = chunk * kCvThreads + threadIdx.x; i < n; i += static_cast<int64_t>(chunks) * kCvThreads)
    m = max(m, __float_as_uint(fabsf(xb[i])));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out + b, max(max(red[0], red[1]), max(red[2], red[3])));
}

// One wave per output channel: w [C_out][C_in][3][3] fp32 -> planes (layout above; C_in = 3: [C_out][hi 32 | lo 32] with
// k = 3 tap + ci, zeros from 27), shift[C_out]; nonfinite[0] = 1 if any weight is inf / NaN.
__global__ __launch_bounds__(kCvThreads) void conv3x3_pack_kernel(const float* __restrict__ w, int C_in, int C_out,
                                                                  __half* __restrict__ planes, int* __restrict__ shift,
                                                                  int* __restrict__ nonfinite) {
  const int lane = threadIdx.x & (kWave - 1);
  const int co = blockIdx.x * (kCvThreads / kWave) + threadIdx.x / kWave;
  if (co >= C_out) return;
  const int K = C_in * 9;
  const float* __restrict__ wr = w + static_cast<int64_t>(co) * K;
  unsigned int m = 0;
  for (int e = lane; e < K; e += kWave) m = max(m, __float_as_uint(fabsf(wr[e])));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, kWave));
  const float mx = __uint_as_float(m);
  const int s = cv_shift(mx);
  if (lane == 0) {
    shift[co] = s;
    if (!(mx <= FLT_MAX)) nonfinite[0] = 1;
  }
  short* __restrict__ dst = reinterpret_cast<short*>(planes);
  if (C_in == 3) {
    if (lane < kCvK) {
      short hi = 0, lo = 0;
      if (lane < 27) cv_split(wr[(lane % 3) * 9 + lane / 3], s, hi, lo);
      dst[static_cast<int64_t>(co) * 64 + lane] = hi;
      dst[static_cast<int64_t>(co) * 64 + 32 + lane] = lo;
    }
    return;
  }
  for (int e = lane; e < K; e += kWave) {
    const int ci = e / 9, tap = e - ci * 9;
    short hi, lo;
    cv_split(wr[e], s, hi, lo);
    const int64_t row = (static_cast<int64_t>(ci / kCvK) * 9 + tap) * C_out + co;
    dst[row * 64 + (ci & (kCvK - 1))] = hi;
    dst[row * 64 + 32 + (ci & (kCvK - 1))] = lo;
  }
}

template <int NT, bool C3>
__global__ __launch_bounds__(kCvThreads, 2) void conv3x3_kernel(const float* __restrict__ x, const __half* __restrict__ wp,
                                                                const int* __restrict__ wshift, const float* __restrict__ bias,
                                                                const float* __restrict__ x_absmax, float* __restrict__ y,
                                                                unsigned int* __restrict__ y_absmax, int H, int W, int C_in, int C_out,
                                                                int tiles_x, int tiles_y, bool relu) {
  constexpr int MJ = NT == 128 ? 4 : 2;                // pixel rows (MFMA tiles of 16 pixels) per wave
  constexpr int kBChunks = NT * 8 / kCvThreads;        // 16-byte chunks of a weight block per thread
  constexpr int kAChunks = (kCvHalo * 8 + kCvThreads - 1) / kCvThreads;  // float4 chunks of an fp32 halo slice per thread
  __shared__ __attribute__((aligned(16))) short lds_a[kCvHalo * kCvLd];  // [halo pixel | C3: tile pixel][hi 32 | lo 32]
  __shared__ __attribute__((aligned(16))) short lds_b[2][NT * kCvLd];    // [buffer][cout][hi 32 | lo 32]
  __shared__ unsigned int red[kCvThreads / kWave];
  // consecutive ids (the C_out tiles of one patch, then the next patch) stay on one XCD's L2
  const int64_t nwg = gridDim.x, orig = blockIdx.x, xcd = orig % 8, q = nwg / 8, rr = nwg % 8;
  int64_t id = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + orig / 8;
  const int nct = C_out / NT;
  const int co0 = static_cast<int>(id % nct) * NT;
  id /= nct;
  const int x0 = static_cast<int>(id % tiles_x) * kCvTW;
  id /= tiles_x;
  const int y0 = static_cast<int>(id % tiles_y) * kCvTH;
  const int64_t b = id / tiles_y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int wr = NT == 128 ? wave >> 1 : wave, wc = NT == 128 ? wave & 1 : 0;
  const int fr = lane & 15, fk = 8 * (lane >> 4);
  const float* __restrict__ xb = x + b * H * W * C_in;
  const int s_img = cv_shift(x_absmax[b]);
  const int nsl = C3 ? 1 : C_in / kCvK, steps = C3 ? 1 : 9 * nsl;

  cv_frag8 rb[kBChunks];
  auto load_b = [&](int step) {  // weight block of one step: NT rows of 64 halves, contiguous
    const cv_frag8* __restrict__ src = reinterpret_cast<const cv_frag8*>(wp + (static_cast<int64_t>(step) * C_out + co0) * 64);
#pragma unroll
    for (int i = 0; i < kBChunks; ++i) rb[i] = src[tid + kCvThreads * i];
  };
  auto store_b = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kBChunks; ++i) {
      const int c = tid + kCvThreads * i;
      *reinterpret_cast<cv_frag8*>(&lds_b[buf][(c >> 3) * kCvLd + 8 * (c & 7)]) = rb[i];
    }
  };
  // halo chunk i of this thread: pixel offset inside the image, -1 outside it (stored as zeros, never loaded)
  int aoff[kAChunks];
  float4 ra[kAChunks];
  if constexpr (!C3) {
#pragma unroll
    for (int i = 0; i < kAChunks; ++i) {
      const int hp = (tid + kCvThreads * i) >> 3, hy = hp / kCvHaloW, hx = hp - hy * kCvHaloW;
      const int iy = y0 + hy - 1, ix = x0 + hx - 1;
      aoff[i] = (hp < kCvHalo && iy >= 0 && iy < H && ix >= 0 && ix < W) ? iy * W + ix : -1;
    }
  }
  auto load_a = [&](int sl) {
#pragma unroll
    for (int i = 0; i < kAChunks; ++i) {
      ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (aoff[i] >= 0)
        ra[i] = *reinterpret_cast<const float4*>(xb + static_cast<int64_t>(aoff[i]) * C_in + sl * kCvK + 4 * (tid & 7));
    }
  };
  auto store_a = [&]() {
#pragma unroll
    for (int i = 0; i < kAChunks; ++i) {
      const int c = tid + kCvThreads * i;
      if (c >= kCvHalo * 8) continue;
      short hi[4], lo[4];
      cv_split(ra[i].x, s_img, hi[0], lo[0]);
      cv_split(ra[i].y, s_img, hi[1], lo[1]);
      cv_split(ra[i].z, s_img, hi[2], lo[2]);
      cv_split(ra[i].w, s_img, hi[3], lo[3]);
      *reinterpret_cast<cv_frag4*>(&lds_a[(c >> 3) * kCvLd + 4 * (c & 7)]) = cv_frag4{hi[0], hi[1], hi[2], hi[3]};
      *reinterpret_cast<cv_frag4*>(&lds_a[(c >> 3) * kCvLd + 32 + 4 * (c & 7)]) = cv_frag4{lo[0], lo[1], lo[2], lo[3]};
    }
  };

  load_b(0);
  if constexpr (C3) {  // im2col of the tile: row = pixel, k = 3 tap + ci, zeros from 27 and outside the image
    for (int e = tid; e < kCvTH * kCvTW * kCvK; e += kCvThreads) {
      const int p = e >> 5, k = e & 31, tap = k / 3, ci = k - 3 * tap;
      const int iy = y0 + (p >> 4) + tap / 3 - 1, ix = x0 + (p & 15) + tap % 3 - 1;
      short hi = 0, lo = 0;
      if (k < 27 && iy >= 0 && iy < H && ix >= 0 && ix < W) cv_split(xb[(static_cast<int64_t>(iy) * W + ix) * 3 + ci], s_img, hi, lo);
      lds_a[p * kCvLd + k] = hi;
      lds_a[p * kCvLd + 32 + k] = lo;
    }
  } else {
    load_a(0);
    store_a();
  }
  store_b(0);
  __syncthreads();

  cv_acc4 acc[4][MJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] = cv_acc4{0.f, 0.f, 0.f, 0.f};
  int tap = 0, sl = 0;
  for (int step = 0; step < steps; ++step) {
    const int buf = step & 1;
    const bool more = step + 1 < steps;
    if (more) load_b(step + 1);
    if constexpr (!C3)
      if (tap == 0 && sl + 1 < nsl) load_a(sl + 1);
    const int ky = tap / 3, kx = tap - 3 * ky;
    const short* B = lds_b[buf];
    cv_frag8 wh[4], wl[4], ph[MJ], pl[MJ];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wh[i] = *reinterpret_cast<const cv_frag8*>(B + (wc * 64 + 16 * i + fr) * kCvLd + fk);
      wl[i] = *reinterpret_cast<const cv_frag8*>(B + (wc * 64 + 16 * i + fr) * kCvLd + 32 + fk);
    }
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      const int py = wr * MJ + j;
      const int row = C3 ? py * kCvTW + fr : (py + ky) * kCvHaloW + kx + fr;
      ph[j] = *reinterpret_cast<const cv_frag8*>(lds_a + row * kCvLd + fk);
      pl[j] = *reinterpret_cast<const cv_frag8*>(lds_a + row * kCvLd + 32 + fk);
    }
    // the small terms first, as in pairwise.hip
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < MJ; ++j) acc[i][j] = cv_mma(wh[i], pl[j], acc[i][j]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < MJ; ++j) acc[i][j] = cv_mma(wl[i], ph[j], acc[i][j]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < MJ; ++j) acc[i][j] = cv_mma(wh[i], ph[j], acc[i][j]);
    if (more) store_b(buf ^ 1);
    if constexpr (!C3) {
      if (tap == 8 && sl + 1 < nsl) {  // every wave has read the last tap of this slice before the patch is replaced
        __syncthreads();
        store_a();
      }
    }
    __syncthreads();
    if (++tap == 9) {
      tap = 0;
      ++sl;
    }
  }

  // epilogue: a lane holds couts co .. co + 3 of pixel (py, fr) in acc[i][j]
  unsigned int m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = co0 + wc * 64 + 16 * i + (lane >> 4) * 4;
    const int4 sc = *reinterpret_cast<const int4*>(wshift + co);
    const float4 bs = *reinterpret_cast<const float4*>(bias + co);
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      const int oy = y0 + wr * MJ + j, ox = x0 + fr;
      if (oy >= H || ox >= W) continue;
      float4 v;
      v.x = ldexpf(acc[i][j][0], -(s_img + sc.x)) + bs.x;
      v.y = ldexpf(acc[i][j][1], -(s_img + sc.y)) + bs.y;
      v.z = ldexpf(acc[i][j][2], -(s_img + sc.z)) + bs.z;
      v.w = ldexpf(acc[i][j][3], -(s_img + sc.w)) + bs.w;
      if (relu) {  // (keeps NaN, as torch's relu does)
        v.x = v.x < 0.f ? 0.f : v.x;
        v.y = v.y < 0.f ? 0.f : v.y;
        v.z = v.z < 0.f ? 0.f : v.z;
        v.w = v.w < 0.f ? 0.f : v.w;
      }
      m = max(max(m, __float_as_uint(fabsf(v.x))), __float_as_uint(fabsf(v.y)));
      m = max(max(m, __float_as_uint(fabsf(v.z))), __float_as_uint(fabsf(v.w)));
      *reinterpret_cast<float4*>(y + ((b * H + oy) * W + ox) * C_out + co) = v;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, kWave));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (tid == 0) atomicMax(y_absmax + b, max(max(red[0], red[1]), max(red[2], red[3])));
}

// fp32 [B] max |x| per image of a [B, C, H, W] tensor (any dense layout)
at::Tensor conv3x3_absmax(const at::Tensor& x_in) {
  TORCH_CHECK(x_in.is_cuda() && x_in.scalar_type() == at::kFloat && x_in.dim() == 4, "conv3x3_absmax: expected a GPU fp32 [B, C, H, W] tensor");
  const at::DeviceGuard guard(x_in.device());
  auto x = x_in.is_contiguous(at::MemoryFormat::ChannelsLast) ? x_in : x_in.contiguous();
  const int64_t B = x.size(0), n = B ? x.numel() / B : 0;
  auto out = at::zeros({B}, x.options());
  if (B == 0 || n == 0) return out;
  const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((n + 16 * kCvThreads - 1) / (16 * kCvThreads), 2048 / B));
  TORCH_CHECK(B * chunks < (int64_t(1) << 31), "conv3x3_absmax: batch too large");
  hipLaunchKernelGGL(conv3x3_absmax_kernel, dim3(static_cast<unsigned>(B * chunks)), kCvThreads, 0, stream(), x.data_ptr<float>(), n,
                     static_cast<int>(chunks), reinterpret_cast<unsigned int*>(out.data_ptr<float>()));
  TMX_LAUNCH_CHECK();
  return out;
}

// w [C_out, C_in, 3, 3] fp32 -> (f16 planes, int32 [C_out] shifts, int32 [1] non-finite flag)
std::tuple<at::Tensor, at::Tensor, at::Tensor> conv3x3_pack(const at::Tensor& w_in) {
  TORCH_CHECK(w_in.is_cuda() && w_in.scalar_type() == at::kFloat, "conv3x3_pack: expected a GPU fp32 weight");
  TORCH_CHECK(w_in.dim() == 4 && w_in.size(2) == 3 && w_in.size(3) == 3, "conv3x3_pack: expected [C_out, C_in, 3, 3]");
  const int64_t C_out = w_in.size(0), C_in = w_in.size(1);
  TORCH_CHECK(C_in == 3 || (C_in > 0 && C_in % kCvK == 0), "conv3x3_pack: C_in must be 3 or a multiple of 32, got ", C_in);
  TORCH_CHECK(C_out > 0 && C_out % 64 == 0, "conv3x3_pack: C_out must be a multiple of 64, got ", C_out);
  TORCH_CHECK(C_in * 9 * C_out < (int64_t(1) << 31), "conv3x3_pack: weight too large");
  const at::DeviceGuard guard(w_in.device());
  auto w = w_in.contiguous();
  const int64_t rows = C_in == 3 ? C_out : (C_in / kCvK) * 9 * C_out;
  auto planes = at::empty({rows, 64}, w.options().dtype(at::kHalf));
  auto shift = at::empty({C_out}, w.options().dtype(at::kInt));
  auto flag = at::zeros({1}, w.options().dtype(at::kInt));
  hipLaunchKernelGGL(conv3x3_pack_kernel, dim3(static_cast<unsigned>(C_out / (kCvThreads / kWave))), kCvThreads, 0, stream(),
                     w.data_ptr<float>(), static_cast<int>(C_in), static_cast<int>(C_out), reinterpret_cast<__half*>(planes.data_ptr()),
                     shift.data_ptr<int>(), flag.data_ptr<int>());
  TMX_LAUNCH_CHECK();
  return {planes, shift, flag};
}

// x [B, C_in, H, W] fp32 (read as channels_last), packed weights, bias [C_out], x_absmax [B] -> (y channels_last, y_absmax [B])
std::tuple<at::Tensor, at::Tensor> conv3x3_relu(const at::Tensor& x_in, const at::Tensor& w_planes, const at::Tensor& w_shift,
                                                const at::Tensor& bias_in, const at::Tensor& x_absmax, bool relu) {
  TORCH_CHECK(x_in.is_cuda() && x_in.scalar_type() == at::kFloat && x_in.dim() == 4, "conv3x3_relu: expected a GPU fp32 [B, C, H, W] input");
  const auto dev = x_in.device();
  TORCH_CHECK(w_planes.device() == dev && w_shift.device() == dev && bias_in.device() == dev && x_absmax.device() == dev,
              "conv3x3_relu: tensors on different devices");
  const int64_t B = x_in.size(0), C_in = x_in.size(1), H = x_in.size(2), W = x_in.size(3), C_out = w_shift.numel();
  TORCH_CHECK(C_in == 3 || (C_in > 0 && C_in % kCvK == 0), "conv3x3_relu: C_in must be 3 or a multiple of 32, got ", C_in);
  TORCH_CHECK(C_out > 0 && C_out % 64 == 0, "conv3x3_relu: C_out must be a multiple of 64, got ", C_out);
  const int64_t rows = C_in == 3 ? C_out : (C_in / kCvK) * 9 * C_out;
  TORCH_CHECK(w_planes.scalar_type() == at::kHalf && w_planes.is_contiguous() && w_planes.numel() == rows * 64,
              "conv3x3_relu: the packed weights do not match C_in = ", C_in, ", C_out = ", C_out);
  TORCH_CHECK(w_shift.scalar_type() == at::kInt && w_shift.is_contiguous(), "conv3x3_relu: expected int32 shifts");
  TORCH_CHECK(bias_in.numel() == C_out, "conv3x3_relu: bias / C_out mismatch");
  TORCH_CHECK(x_absmax.scalar_type() == at::kFloat && x_absmax.is_contiguous() && x_absmax.numel() == B, "conv3x3_relu: expected fp32 x_absmax [B]");
  const at::DeviceGuard guard(dev);
  auto x = x_in.contiguous(at::MemoryFormat::ChannelsLast);
  auto bias = bias_in.to(at::kFloat).contiguous();
  auto y = at::empty({B, C_out, H, W}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto y_absmax = at::zeros({B}, x.options());
  if (y.numel() == 0) return {y, y_absmax};
  TORCH_CHECK(H * W < (int64_t(1) << 31), "conv3x3_relu: image plane too large");
  const int64_t tiles_x = (W + kCvTW - 1) / kCvTW, tiles_y = (H + kCvTH - 1) / kCvTH;
  const int nt = C_out % 128 == 0 ? 128 : 64;
  const int64_t nwg = B * tiles_y * tiles_x * (C_out / nt);
  TORCH_CHECK(nwg < (int64_t(1) << 31), "conv3x3_relu: too many tiles for one launch");
  // (the three-channel input is gathered by scalar loads: a batch slice of it may start at any multiple of 4 bytes)
  for (const void* p : {C_in == 3 ? nullptr : x.data_ptr(), w_planes.data_ptr(), w_shift.data_ptr(), bias.data_ptr(), y.data_ptr()})
    TORCH_CHECK((reinterpret_cast<uintptr_t>(p) & 15) == 0, "conv3x3_relu: expected 16-byte aligned tensors");
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(nwg)), kCvThreads, 0, stream(), x.data_ptr<float>(),
                       reinterpret_cast<const __half*>(w_planes.data_ptr()), w_shift.data_ptr<int>(), bias.data_ptr<float>(),
                       x_absmax.data_ptr<float>(), y.data_ptr<float>(), reinterpret_cast<unsigned int*>(y_absmax.data_ptr<float>()),
                       static_cast<int>(H), static_cast<int>(W), static_cast<int>(C_in), static_cast<int>(C_out),
                       static_cast<int>(tiles_x), static_cast<int>(tiles_y), relu);
  };
  if (C_in == 3) {
    if (nt == 128) launch(conv3x3_kernel<128, true>);
    else launch(conv3x3_kernel<64, true>);
  } else {
    if (nt == 128) launch(conv3x3_kernel<128, false>);
    else launch(conv3x3_kernel<64, false>);
  }
  TMX_LAUNCH_CHECK();
  return {y, y_absmax};
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("conv3x3_relu(Tensor x, Tensor w_planes, Tensor w_shift, Tensor bias, Tensor x_absmax, bool relu) -> (Tensor, Tensor)");
  m.def("conv3x3_pack(Tensor w) -> (Tensor, Tensor, Tensor)");
  m.def("conv3x3_absmax(Tensor x) -> Tensor");
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("conv3x3_relu", &tmx::conv3x3_relu);
  m.impl("conv3x3_pack", &tmx::conv3x3_pack);
  m.impl("conv3x3_absmax", &tmx::conv3x3_absmax);
}
