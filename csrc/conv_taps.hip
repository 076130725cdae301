// fp32 stride-1 convolutions with folded batch norm and ReLU on the f16 matrix cores: the Inception-v3 trunk of FID / KID / IS / MiFID.
//
// The product is conv_split.h's (as in conv3x3.hip): operands scaled by a power of two and split into f16 hi / lo planes,
// hi·lo + lo·hi + hi·hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation.  Activations stay fp32 channels_last in HBM and are
// split while they are staged; the weights are the MFMA's A operand, so a lane ends with four consecutive output channels
// of one pixel: one 16-byte store.  What this file adds over conv3x3.hip:
//
//  * conv_pack_kernel folds eval-mode batch norm into the weights in fp64 (w' = w γ / sqrt(var + eps), b' = β − mean γ / sqrt(var + eps),
//    each rounded once to fp32) before the split, and writes [ceil(C_in / 32)][tap][C_out][hi 32 | lo 32]; channels past C_in in
//    the last slice are zeros, which serves C_in % 16 == 0 (48, 80, 160, 208 ...) without a second MFMA shape.
//  * conv_pointwise_kernel<NT>: the 1x1 case is a plain GEMM over M = B·H·W flat pixels, 128 per workgroup, no halo and no
//    per-plane tile waste.  The scale only has to be constant along K, so every GEMM row (pixel) is staged and rescaled by the
//    shift of its own image and a tile may span images.  A and B are double-buffered in LDS (one barrier per K slice), the next
//    slice waits in registers during the MFMAs.  LDS: 2 x 18.4 KB pixels + 2 x 9.2 / 18.4 KB weights (NT = 64 / 128).
//  * conv_taps_kernel<KH, KW, NT, MJ>: implicit GEMM over a TH x TW output patch of one image x NT output channels.  The patch
//    shape is a launch argument, not a constant: a lane's pixel slot q maps to (q / TW, q % TW) once, before the K loop, so any
//    TH·TW <= slots costs nothing inside it.  The host takes the shape that covers the output plane in the fewest workgroups
//    under the 256-pixel halo budget (35 x 35: 7 x 18, 96 % of the MFMA rows live; 17 x 17: 6 x 17, 75 %, against 38 % for an
//    8 x 16 patch; 8 x 8: one 64-slot patch per image, MJ = 2 with NT = 128).  Per 32-channel slice the (TH + KH − 1) x (TW + KW − 1)
//    halo is staged once, both planes, out-of-image pixels and padded channels as zeros without a load; the KH·KW taps read
//    their fragments at shifted offsets.  LDS: 36.9 KB halo + 2 x 9.2 / 18.4 KB weights: two workgroups per CU.
//  * Output-channel tiles that overhang C_out (C_out % 16 == 0) are zeros in the weight load, skipped per 16-channel MFMA tile
//    (wave-uniform) and masked in the store.
//  * The output is a channel range [c_off, c_off + C_out) of a wider channels_last block: the branches of a Mixed block write
//    into one tensor and there is no concatenation.  Every launch takes atomicMax of its per-image output maximum (bit
//    pattern, NaN above inf) into the block's one [B] buffer, which is the next block's scale.
//
// Non-finite activations: an image whose maximum is inf / NaN is staged unscaled; no other image reads its scale.
#include "conv_split.h"

#include <algorithm>

namespace tmx {

constexpr int kTpSlots = 128;  // pixel slots (GEMM rows) of a full workgroup tile
constexpr int kTpHalo = 256;   // halo pixels a taps workgroup can stage: 256 x 144 B = 36.9 KB

// One wave per output channel: w [C_out][C_in][T] fp32 and the batch-norm vectors -> planes (layout above), shift[C_out],
// bias[C_out] (b'); nonfinite[0] = 1 if a folded weight or bias is inf / NaN.
__global__ __launch_bounds__(kCvThreads) void conv_pack_kernel(const float* __restrict__ w, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ mean,
                                                               const float* __restrict__ var, double eps, int C_in, int C_out, int T,
                                                               __half* __restrict__ planes, int* __restrict__ shift,
                                                               float* __restrict__ bias, int* __restrict__ nonfinite) {
  const int lane = threadIdx.x & (kWave - 1);
  const int co = blockIdx.x * (kCvThreads / kWave) + threadIdx.x / kWave;
  if (co >= C_out) return;
  const int K = C_in * T;
  const float* __restrict__ wr = w + static_cast<int64_t>(co) * K;
  const double g = static_cast<double>(gamma[co]) / sqrt(static_cast<double>(var[co]) + eps);
  const float b = static_cast<float>(static_cast<double>(beta[co]) - static_cast<double>(mean[co]) * g);
  unsigned int m = 0;
  for (int e = lane; e < K; e += kWave) m = max(m, __float_as_uint(fabsf(static_cast<float>(wr[e] * g))));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, kWave));
  const float mx = __uint_as_float(m);
  const int s = cv_shift(mx);
  if (lane == 0) {
    shift[co] = s;
    bias[co] = b;
    if (!(mx <= FLT_MAX) || !(fabsf(b) <= FLT_MAX)) nonfinite[0] = 1;
  }
  short* __restrict__ dst = reinterpret_cast<short*>(planes);
  const int Kp = (C_in + kCvK - 1) / kCvK * kCvK * T;
  for (int e = lane; e < Kp; e += kWave) {
    const int ci = e / T, tap = e - ci * T;
    short hi = 0, lo = 0;
    if (ci < C_in) cv_split(static_cast<float>(wr[e] * g), s, hi, lo);
    const int64_t row = (static_cast<int64_t>(ci / kCvK) * T + tap) * C_out + co;
    dst[row * 64 + (ci & (kCvK - 1))] = hi;
    dst[row * 64 + 32 + (ci & (kCvK - 1))] = lo;
  }
}

// consecutive ids (the C_out tiles of one pixel tile, then the next pixel tile) stay on one XCD's L2
__device__ __forceinline__ int64_t tp_workgroup_id() {
  const int64_t nwg = gridDim.x, orig = blockIdx.x, xcd = orig % 8, q = nwg / 8, rr = nwg % 8;
  return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + orig / 8;
}

// weight block of one K step: NT rows of 64 halves, rows from C_out on as zeros
template <int NT>
__device__ __forceinline__ void tp_load_b(cv_frag8 (&rb)[NT * 8 / kCvThreads], const __half* __restrict__ wp, int64_t step, int C_out,
                                          int co0) {
  const cv_frag8* __restrict__ src = reinterpret_cast<const cv_frag8*>(wp + (step * C_out + co0) * 64);
#pragma unroll
  for (int i = 0; i < NT * 8 / kCvThreads; ++i) {
    const int c = threadIdx.x + kCvThreads * i;
    rb[i] = cv_frag8{0, 0, 0, 0, 0, 0, 0, 0};
    if (co0 + (c >> 3) < C_out) rb[i] = src[c];
  }
}

template <int NT>
__device__ __forceinline__ void tp_store_b(const cv_frag8 (&rb)[NT * 8 / kCvThreads], short* __restrict__ lds) {
#pragma unroll
  for (int i = 0; i < NT * 8 / kCvThreads; ++i) {
    const int c = threadIdx.x + kCvThreads * i;
    *reinterpret_cast<cv_frag8*>(&lds[(c >> 3) * kCvLd + 8 * (c & 7)]) = rb[i];
  }
}

// four fp32 channels of one pixel, split by that pixel's image shift into LDS row `row`
__device__ __forceinline__ void tp_store_a(short* __restrict__ lds, int row, int chunk, float4 v, int s) {
  short hi[4], lo[4];
  cv_split(v.x, s, hi[0], lo[0]);
  cv_split(v.y, s, hi[1], lo[1]);
  cv_split(v.z, s, hi[2], lo[2]);
  cv_split(v.w, s, hi[3], lo[3]);
  *reinterpret_cast<cv_frag4*>(&lds[row * kCvLd + 4 * chunk]) = cv_frag4{hi[0], hi[1], hi[2], hi[3]};
  *reinterpret_cast<cv_frag4*>(&lds[row * kCvLd + 32 + 4 * chunk]) = cv_frag4{lo[0], lo[1], lo[2], lo[3]};
}

// One K = 32 step of a wave: its `nci` live 16-channel tiles x MJ pixel tiles, the small terms first.  `bw` is the wave's
// weight row of lane (fr, fk) in LDS, `a` the pixel rows, `prow[j]` the lane's pixel row offset of tile j (halves, fk included).
template <int MJ>
__device__ __forceinline__ void tp_step(const short* __restrict__ bw, const short* __restrict__ a, const int (&prow)[MJ], int nci,
                                        cv_acc4 (&acc)[4][MJ]) {
  cv_frag8 wh[4], wl[4], ph[MJ], pl[MJ];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    wh[i] = wl[i] = cv_frag8{0, 0, 0, 0, 0, 0, 0, 0};
    if (i < nci) {
      wh[i] = *reinterpret_cast<const cv_frag8*>(bw + 16 * i * kCvLd);
      wl[i] = *reinterpret_cast<const cv_frag8*>(bw + 16 * i * kCvLd + 32);
    }
  }
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    ph[j] = *reinterpret_cast<const cv_frag8*>(a + prow[j]);
    pl[j] = *reinterpret_cast<const cv_frag8*>(a + prow[j] + 32);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nci)
#pragma unroll
      for (int j = 0; j < MJ; ++j) acc[i][j] = cv_mma(wh[i], pl[j], acc[i][j]);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nci)
#pragma unroll
      for (int j = 0; j < MJ; ++j) acc[i][j] = cv_mma(wl[i], ph[j], acc[i][j]);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nci)
#pragma unroll
      for (int j = 0; j < MJ; ++j) acc[i][j] = cv_mma(wh[i], ph[j], acc[i][j]);
}

// A lane holds channels co .. co + 3 of pixel opix[j] (-1: no such output pixel) in acc[i][j]: rescale by the pixel's image
// shift and the channel shifts, add b', ReLU (NaN kept), store; m[j] = max bit pattern of what the lane stored for tile j.
template <int MJ>
__device__ __forceinline__ void tp_epilogue(const cv_acc4 (&acc)[4][MJ], int co_wave, int C_out, const int* __restrict__ wshift,
                                            const float* __restrict__ bias, const int64_t (&opix)[MJ], const int (&simg)[MJ],
                                            float* __restrict__ y, int64_t ldy, unsigned int (&m)[MJ]) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int j = 0; j < MJ; ++j) m[j] = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = co_wave + 16 * i + (lane >> 4) * 4;
    if (co >= C_out) continue;
    const int4 sc = *reinterpret_cast<const int4*>(wshift + co);
    const float4 bs = *reinterpret_cast<const float4*>(bias + co);
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      if (opix[j] < 0) continue;
      float4 v;
      v.x = ldexpf(acc[i][j][0], -(simg[j] + sc.x)) + bs.x;
      v.y = ldexpf(acc[i][j][1], -(simg[j] + sc.y)) + bs.y;
      v.z = ldexpf(acc[i][j][2], -(simg[j] + sc.z)) + bs.z;
      v.w = ldexpf(acc[i][j][3], -(simg[j] + sc.w)) + bs.w;
      v.x = v.x < 0.f ? 0.f : v.x;  // (keeps NaN, as torch's relu does)
      v.y = v.y < 0.f ? 0.f : v.y;
      v.z = v.z < 0.f ? 0.f : v.z;
      v.w = v.w < 0.f ? 0.f : v.w;
      m[j] = max(max(m[j], __float_as_uint(fabsf(v.x))), __float_as_uint(fabsf(v.y)));
      m[j] = max(max(m[j], __float_as_uint(fabsf(v.z))), __float_as_uint(fabsf(v.w)));
      *reinterpret_cast<float4*>(y + opix[j] * ldy + co) = v;
    }
  }
}

// 1x1: y[p][c_off + co] = relu(sum_ci x[p][ci] w'[co][ci] + b'[co]) over the M = B·HW flat pixels p.  NT = 128: 2 x 2 waves of
// 64 channels x 64 pixels; NT = 64: 4 waves of 64 channels x 32 pixels.  y already points at channel c_off.
template <int NT>
__global__ __launch_bounds__(kCvThreads, 2) void conv_pointwise_kernel(const float* __restrict__ x, const __half* __restrict__ wp,
                                                                       const int* __restrict__ wshift, const float* __restrict__ bias,
                                                                       const float* __restrict__ x_absmax, float* __restrict__ y,
                                                                       unsigned int* __restrict__ y_absmax, int64_t M, int HW, int C_in,
                                                                       int C_out, int64_t ldy) {
  constexpr int MJ = NT == 128 ? 4 : 2;
  constexpr int kAChunks = kTpSlots * 8 / kCvThreads;  // float4 chunks of an fp32 pixel slice per thread
  __shared__ __attribute__((aligned(16))) short lds_a[2][kTpSlots * kCvLd];  // [buffer][pixel slot][hi 32 | lo 32]
  __shared__ __attribute__((aligned(16))) short lds_b[2][NT * kCvLd];        // [buffer][cout][hi 32 | lo 32]
  __shared__ unsigned int img_max[kTpSlots];  // per image of this tile (at most one image per pixel slot)
  int64_t id = tp_workgroup_id();
  const int nct = (C_out + NT - 1) / NT;
  const int co0 = static_cast<int>(id % nct) * NT;
  const int64_t p0 = id / nct * kTpSlots;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int wr = NT == 128 ? wave >> 1 : wave, wc = NT == 128 ? wave & 1 : 0;
  const int fr = lane & 15, fk = 8 * (lane >> 4);
  const int nsl = (C_in + kCvK - 1) / kCvK;
  const int nci = min(4, max(0, (C_out - co0 - wc * 64) / 16));
  const bool last_ok = 4 * (tid & 7) < C_in - (nsl - 1) * kCvK;  // this thread's channels exist in the last, maybe padded, slice
  if (tid < kTpSlots) img_max[tid] = 0;

  // chunk i of this thread is channels 4 (tid & 7) .. + 3 of pixel slot (tid >> 3) + 32 i, in every slice
  const float* asrc[kAChunks];
  int sa[kAChunks];
  float4 ra[kAChunks];
  cv_frag8 rb[NT * 8 / kCvThreads];
#pragma unroll
  for (int i = 0; i < kAChunks; ++i) {
    const int64_t p = p0 + (tid >> 3) + 32 * i;
    asrc[i] = p < M ? x + p * C_in + 4 * (tid & 7) : nullptr;
    sa[i] = p < M ? cv_shift(x_absmax[p / HW]) : 0;
  }
  auto load_a = [&](int sl) {
#pragma unroll
    for (int i = 0; i < kAChunks; ++i) {
      ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (asrc[i] != nullptr && (sl + 1 < nsl || last_ok)) ra[i] = *reinterpret_cast<const float4*>(asrc[i] + sl * kCvK);
    }
  };
  auto store_a = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kAChunks; ++i) tp_store_a(lds_a[buf], (tid >> 3) + 32 * i, tid & 7, ra[i], sa[i]);
  };

  load_a(0);
  tp_load_b<NT>(rb, wp, 0, C_out, co0);
  store_a(0);
  tp_store_b<NT>(rb, lds_b[0]);
  __syncthreads();

  cv_acc4 acc[4][MJ];
  int prow[MJ];
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    prow[j] = ((wr * MJ + j) * 16 + fr) * kCvLd + fk;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][j] = cv_acc4{0.f, 0.f, 0.f, 0.f};
  }
  for (int sl = 0; sl < nsl; ++sl) {
    const int buf = sl & 1;
    const bool more = sl + 1 < nsl;
    if (more) {
      load_a(sl + 1);
      tp_load_b<NT>(rb, wp, sl + 1, C_out, co0);
    }
    tp_step<MJ>(lds_b[buf] + (wc * 64 + fr) * kCvLd + fk, lds_a[buf], prow, nci, acc);
    if (more) {  // the other buffer: every wave left it at the barrier that ended the previous slice
      store_a(buf ^ 1);
      tp_store_b<NT>(rb, lds_b[buf ^ 1]);
    }
    __syncthreads();
  }

  int64_t opix[MJ];
  int simg[MJ], img[MJ];
  unsigned int m[MJ];
  const int64_t b0 = p0 / HW;
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    const int64_t p = p0 + (wr * MJ + j) * 16 + fr;
    opix[j] = p < M ? p : -1;
    img[j] = p < M ? static_cast<int>(p / HW - b0) : 0;
    simg[j] = p < M ? cv_shift(x_absmax[p / HW]) : 0;
  }
  tp_epilogue<MJ>(acc, co0 + wc * 64, C_out, wshift, bias, opix, simg, y, ldy, m);
  // the four lanes of a pixel (other channels) first, then one LDS atomic per pixel into its image's slot
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    m[j] = max(m[j], __shfl_xor(m[j], 16, kWave));
    m[j] = max(m[j], __shfl_xor(m[j], 32, kWave));
    if (lane < 16 && opix[j] >= 0) atomicMax(&img_max[img[j]], m[j]);
  }
  __syncthreads();
  if (tid < kTpSlots && img_max[tid] != 0) atomicMax(y_absmax + b0 + tid, img_max[tid]);
}

// KH x KW taps, stride 1, zero padding (pad_h, pad_w): a TH x TW patch of output pixels of one image x NT output channels.
// Pixel slots: (NT = 128 ? 2 : 4) wave rows x MJ tiles x 16; slots from TH·TW on are dead (never stored, their waves skip the MFMAs).
template <int KH, int KW, int NT, int MJ>
__global__ __launch_bounds__(kCvThreads, 2) void conv_taps_kernel(const float* __restrict__ x, const __half* __restrict__ wp,
                                                                  const int* __restrict__ wshift, const float* __restrict__ bias,
                                                                  const float* __restrict__ x_absmax, float* __restrict__ y,
                                                                  unsigned int* __restrict__ y_absmax, int H, int W, int C_in, int C_out,
                                                                  int Ho, int Wo, int pad_h, int pad_w, int TH, int TW, int tiles_x,
                                                                  int tiles_y, int64_t ldy) {
  constexpr int T = KH * KW;
  constexpr int kAChunks = kTpHalo * 8 / kCvThreads;  // float4 chunks of an fp32 halo slice per thread
  __shared__ __attribute__((aligned(16))) short lds_a[kTpHalo * kCvLd];  // [halo pixel][hi 32 | lo 32]
  __shared__ __attribute__((aligned(16))) short lds_b[2][NT * kCvLd];    // [buffer][cout][hi 32 | lo 32]
  __shared__ unsigned int red[kCvThreads / kWave];
  int64_t id = tp_workgroup_id();
  const int nct = (C_out + NT - 1) / NT;
  const int co0 = static_cast<int>(id % nct) * NT;
  id /= nct;
  const int x0 = static_cast<int>(id % tiles_x) * TW;
  id /= tiles_x;
  const int y0 = static_cast<int>(id % tiles_y) * TH;
  const int64_t b = id / tiles_y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int wr = NT == 128 ? wave >> 1 : wave, wc = NT == 128 ? wave & 1 : 0;
  const int fr = lane & 15, fk = 8 * (lane >> 4);
  const int halo_w = TW + KW - 1, halo_n = (TH + KH - 1) * halo_w;
  const float* __restrict__ xb = x + b * H * W * C_in;
  const int s_img = cv_shift(x_absmax[b]);
  const int nsl = (C_in + kCvK - 1) / kCvK, steps = T * nsl;
  const int nci = wr * MJ * 16 < TH * TW ? min(4, max(0, (C_out - co0 - wc * 64) / 16)) : 0;
  const bool last_ok = 4 * (tid & 7) < C_in - (nsl - 1) * kCvK;  // this thread's channels exist in the last, maybe padded, slice

  // halo chunk i of this thread: pixel offset inside the image, -1 outside it and past the halo (stored as zeros, never loaded)
  int aoff[kAChunks];
  float4 ra[kAChunks];
  cv_frag8 rb[NT * 8 / kCvThreads];
#pragma unroll
  for (int i = 0; i < kAChunks; ++i) {
    const int hp = (tid >> 3) + 32 * i, hy = hp / halo_w, hx = hp - hy * halo_w;
    const int iy = y0 + hy - pad_h, ix = x0 + hx - pad_w;
    aoff[i] = (hp < halo_n && iy >= 0 && iy < H && ix >= 0 && ix < W) ? iy * W + ix : -1;
  }
  auto load_a = [&](int sl) {
#pragma unroll
    for (int i = 0; i < kAChunks; ++i) {
      ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (aoff[i] >= 0 && (sl + 1 < nsl || last_ok))
        ra[i] = *reinterpret_cast<const float4*>(xb + static_cast<int64_t>(aoff[i]) * C_in + sl * kCvK + 4 * (tid & 7));
    }
  };
  auto store_a = [&]() {
#pragma unroll
    for (int i = 0; i < kAChunks; ++i) tp_store_a(lds_a, (tid >> 3) + 32 * i, tid & 7, ra[i], s_img);
  };

  tp_load_b<NT>(rb, wp, 0, C_out, co0);
  load_a(0);
  store_a();
  tp_store_b<NT>(rb, lds_b[0]);
  __syncthreads();

  // the lane's pixel of tile j: slot -> (py, px) of the patch; a dead slot reads halo pixel 0 and stores nothing
  cv_acc4 acc[4][MJ];
  int prow[MJ], ptap[MJ];
  int64_t opix[MJ];
  int simg[MJ];
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    const int q = (wr * MJ + j) * 16 + fr, py = q / TW, px = q - py * TW;
    const bool live = q < TH * TW;
    prow[j] = live ? (py * halo_w + px) * kCvLd + fk : fk;
    opix[j] = live && y0 + py < Ho && x0 + px < Wo ? (b * Ho + y0 + py) * Wo + x0 + px : -1;
    simg[j] = s_img;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][j] = cv_acc4{0.f, 0.f, 0.f, 0.f};
  }
  int tap = 0, sl = 0;
  for (int step = 0; step < steps; ++step) {
    const int buf = step & 1;
    const bool more = step + 1 < steps;
    if (more) tp_load_b<NT>(rb, wp, step + 1, C_out, co0);
    if (tap == 0 && sl + 1 < nsl) load_a(sl + 1);
    const int shift_rows = ((tap / KW) * halo_w + tap % KW) * kCvLd;
#pragma unroll
    for (int j = 0; j < MJ; ++j) ptap[j] = prow[j] + shift_rows;
    tp_step<MJ>(lds_b[buf] + (wc * 64 + fr) * kCvLd + fk, lds_a, ptap, nci, acc);
    if (more) tp_store_b<NT>(rb, lds_b[buf ^ 1]);
    if (tap == T - 1 && sl + 1 < nsl) {  // every wave has read the last tap of this slice before the patch is replaced
      __syncthreads();
      store_a();
    }
    __syncthreads();
    if (++tap == T) {
      tap = 0;
      ++sl;
    }
  }

  unsigned int m[MJ];
  tp_epilogue<MJ>(acc, co0 + wc * 64, C_out, wshift, bias, opix, simg, y, ldy, m);
  unsigned int mm = m[0];
#pragma unroll
  for (int j = 1; j < MJ; ++j) mm = max(mm, m[j]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mm = max(mm, __shfl_xor(mm, off, kWave));
  if (lane == 0) red[wave] = mm;
  __syncthreads();
  if (tid == 0) atomicMax(y_absmax + b, max(max(red[0], red[1]), max(red[2], red[3])));
}

// conv weight [C_out, C_in, KH, KW] fp32 and eval-mode batch norm -> (f16 planes, int32 [C_out] shifts, fp32 [C_out] b', int32 [1] non-finite flag)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> conv_pack(const at::Tensor& w_in, const at::Tensor& bn_weight,
                                                                     const at::Tensor& bn_bias, const at::Tensor& bn_mean,
                                                                     const at::Tensor& bn_var, double eps) {
  TORCH_CHECK(w_in.is_cuda() && w_in.scalar_type() == at::kFloat && w_in.dim() == 4, "conv_pack: expected a GPU fp32 [C_out, C_in, KH, KW] weight");
  const int64_t C_out = w_in.size(0), C_in = w_in.size(1), T = w_in.size(2) * w_in.size(3);
  TORCH_CHECK(C_in > 0 && C_in % 16 == 0, "conv_pack: C_in must be a multiple of 16, got ", C_in);
  TORCH_CHECK(C_out > 0 && C_out % 16 == 0, "conv_pack: C_out must be a multiple of 16, got ", C_out);
  const int64_t nsl = (C_in + kCvK - 1) / kCvK;
  TORCH_CHECK(T > 0 && nsl * kCvK * T * C_out < (int64_t(1) << 31), "conv_pack: weight too large");
  at::Tensor bn[4];
  int k = 0;
  for (const at::Tensor* t : {&bn_weight, &bn_bias, &bn_mean, &bn_var}) {
    TORCH_CHECK(t->device() == w_in.device() && t->scalar_type() == at::kFloat && t->numel() == C_out,
                "conv_pack: expected fp32 [C_out] batch-norm tensors on the weight's device");
    bn[k++] = t->contiguous();
  }
  const at::DeviceGuard guard(w_in.device());
  auto w = w_in.contiguous();
  auto planes = at::empty({nsl * T * C_out, 64}, w.options().dtype(at::kHalf));
  auto shift = at::empty({C_out}, w.options().dtype(at::kInt));
  auto bias = at::empty({C_out}, w.options());
  auto flag = at::zeros({1}, w.options().dtype(at::kInt));
  constexpr int kPerWg = kCvThreads / kWave;
  hipLaunchKernelGGL(conv_pack_kernel, dim3(static_cast<unsigned>((C_out + kPerWg - 1) / kPerWg)), kCvThreads, 0, stream(),
                     w.data_ptr<float>(), bn[0].data_ptr<float>(), bn[1].data_ptr<float>(), bn[2].data_ptr<float>(), bn[3].data_ptr<float>(),
                     eps, static_cast<int>(C_in), static_cast<int>(C_out), static_cast<int>(T), reinterpret_cast<__half*>(planes.data_ptr()),
                     shift.data_ptr<int>(), bias.data_ptr<float>(), flag.data_ptr<int>());
  TMX_LAUNCH_CHECK();
  return {planes, shift, bias, flag};
}

// The TH x TW (TH·TW <= slots, halo within kTpHalo) that covers an Ho x Wo plane in the fewest patches; ties: the smaller halo.
static void tp_patch(int64_t Ho, int64_t Wo, int kh, int kw, int slots, int& TH, int& TW) {
  int64_t best_tiles = INT64_MAX, best_halo = 0;
  for (int64_t th = 1; th <= std::min<int64_t>(slots, Ho); ++th) {
    for (int64_t tw = std::min<int64_t>(slots / th, Wo); tw >= 1; --tw) {
      const int64_t halo = (th + kh - 1) * (tw + kw - 1), tiles = ((Ho + th - 1) / th) * ((Wo + tw - 1) / tw);
      if (halo > kTpHalo) continue;
      if (tiles < best_tiles || (tiles == best_tiles && halo < best_halo)) {
        best_tiles = tiles, best_halo = halo;
        TH = static_cast<int>(th), TW = static_cast<int>(tw);
      }
    }
  }
}

// y[:, c_off : c_off + C_out] = relu(bn(conv(x))) for weights packed by conv_pack; x [B, C_in, H, W] and y [B, C_y, Ho, Wo] fp32
// channels_last, x_absmax [B]; the per-image maximum of what was written is folded into y_absmax [B] (atomicMax).
void conv_bn_relu(const at::Tensor& x, const at::Tensor& w_planes, const at::Tensor& w_shift, const at::Tensor& bias,
                  const at::Tensor& x_absmax, at::Tensor& y, at::Tensor& y_absmax, int64_t c_off, int64_t kh, int64_t kw, int64_t pad_h,
                  int64_t pad_w) {
  const auto CL = at::MemoryFormat::ChannelsLast;
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 4 && x.is_contiguous(CL),
              "conv_bn_relu: expected a GPU fp32 channels_last [B, C, H, W] input");
  TORCH_CHECK(y.scalar_type() == at::kFloat && y.dim() == 4 && y.is_contiguous(CL), "conv_bn_relu: expected an fp32 channels_last [B, C, H, W] output");
  const auto dev = x.device();
  for (const at::Tensor* t : std::initializer_list<const at::Tensor*>{&w_planes, &w_shift, &bias, &x_absmax, &y, &y_absmax})
    TORCH_CHECK(t->device() == dev, "conv_bn_relu: tensors on different devices");
  const int64_t B = x.size(0), C_in = x.size(1), H = x.size(2), W = x.size(3), C_out = w_shift.numel(), C_y = y.size(1);
  const bool same = pad_h == (kh - 1) / 2 && pad_w == (kw - 1) / 2;
  const bool served = (kh == 1 && kw == 1) || (kh == 3 && kw == 3) || (kh == 5 && kw == 5) || (kh == 1 && kw == 7) || (kh == 7 && kw == 1) ||
                      (kh == 1 && kw == 3) || (kh == 3 && kw == 1);
  TORCH_CHECK(served, "conv_bn_relu: taps ", kh, " x ", kw, " are not served");
  TORCH_CHECK(same || (pad_h == 0 && pad_w == 0), "conv_bn_relu: padding is (0, 0) or same, got (", pad_h, ", ", pad_w, ")");
  const int64_t Ho = H + 2 * pad_h - kh + 1, Wo = W + 2 * pad_w - kw + 1, T = kh * kw, nsl = (C_in + kCvK - 1) / kCvK;
  TORCH_CHECK(C_in > 0 && C_in % 16 == 0, "conv_bn_relu: C_in must be a multiple of 16, got ", C_in);
  TORCH_CHECK(C_out > 0 && C_out % 16 == 0, "conv_bn_relu: C_out must be a multiple of 16, got ", C_out);
  TORCH_CHECK(w_planes.scalar_type() == at::kHalf && w_planes.is_contiguous() && w_planes.numel() == nsl * T * C_out * 64,
              "conv_bn_relu: the packed weights do not match C_in = ", C_in, ", C_out = ", C_out, ", taps ", kh, " x ", kw);
  TORCH_CHECK(w_shift.scalar_type() == at::kInt && w_shift.is_contiguous(), "conv_bn_relu: expected int32 shifts");
  TORCH_CHECK(bias.scalar_type() == at::kFloat && bias.is_contiguous() && bias.numel() == C_out, "conv_bn_relu: expected fp32 bias [C_out]");
  for (const at::Tensor* t : std::initializer_list<const at::Tensor*>{&x_absmax, &y_absmax})
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == B, "conv_bn_relu: expected fp32 [B] maxima");
  TORCH_CHECK(y.size(0) == B && y.size(2) == Ho && y.size(3) == Wo, "conv_bn_relu: the output block is not [B, C, ", Ho, ", ", Wo, "]");
  TORCH_CHECK(c_off >= 0 && c_off % 4 == 0 && C_y % 4 == 0 && c_off + C_out <= C_y, "conv_bn_relu: channels [", c_off, ", ", c_off + C_out,
              ") do not fit the block's ", C_y, " (offset and width in multiples of 4)");
  if (B == 0 || Ho <= 0 || Wo <= 0) return;
  TORCH_CHECK(H * W < (int64_t(1) << 31) && Ho * Wo < (int64_t(1) << 31), "conv_bn_relu: image plane too large");
  for (const void* p : {x.data_ptr(), w_planes.data_ptr(), w_shift.data_ptr(), bias.data_ptr(), y.data_ptr()})
    TORCH_CHECK((reinterpret_cast<uintptr_t>(p) & 15) == 0, "conv_bn_relu: expected 16-byte aligned tensors");
  const at::DeviceGuard guard(dev);
  const float* xp = x.data_ptr<float>();
  const __half* wp = reinterpret_cast<const __half*>(w_planes.data_ptr());
  float* yp = y.data_ptr<float>() + c_off;
  unsigned int* ymax = reinterpret_cast<unsigned int*>(y_absmax.data_ptr<float>());
  constexpr int64_t kFill = 512;  // workgroups that fill the device twice over: below it the narrower channel tile spreads wider

  if (T == 1) {
    const int64_t M = B * H * W, mt = (M + kTpSlots - 1) / kTpSlots;
    const bool wide = C_out % 128 == 0 && mt * (C_out / 128) >= kFill;
    const int64_t nwg = mt * ((C_out + (wide ? 127 : 63)) / (wide ? 128 : 64));
    TORCH_CHECK(nwg < (int64_t(1) << 31), "conv_bn_relu: too many tiles for one launch");
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(nwg)), kCvThreads, 0, stream(), xp, wp, w_shift.data_ptr<int>(),
                         bias.data_ptr<float>(), x_absmax.data_ptr<float>(), yp, ymax, M, static_cast<int>(H * W), static_cast<int>(C_in),
                         static_cast<int>(C_out), C_y);
    };
    if (wide) launch(conv_pointwise_kernel<128>);
    else launch(conv_pointwise_kernel<64>);
    TMX_LAUNCH_CHECK();
    return;
  }

  // 0: NT = 64, 128 slots; 1: NT = 128, 128 slots; 2: NT = 128, 64 slots (a plane of at most 64 pixels, one patch per image)
  int TH = 1, TW = 1;
  tp_patch(Ho, Wo, static_cast<int>(kh), static_cast<int>(kw), kTpSlots, TH, TW);
  int64_t tiles = B * ((Ho + TH - 1) / TH) * ((Wo + TW - 1) / TW);
  int variant = C_out % 128 == 0 && tiles * (C_out / 128) >= kFill ? 1 : 0;
  if (Ho * Wo <= kTpSlots / 2 && C_out >= 128) {
    variant = 2;
    tp_patch(Ho, Wo, static_cast<int>(kh), static_cast<int>(kw), kTpSlots / 2, TH, TW);
  }
  const int64_t tiles_x = (Wo + TW - 1) / TW, tiles_y = (Ho + TH - 1) / TH;
  const int64_t nwg = B * tiles_y * tiles_x * ((C_out + (variant ? 127 : 63)) / (variant ? 128 : 64));
  TORCH_CHECK(nwg < (int64_t(1) << 31), "conv_bn_relu: too many tiles for one launch");
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(nwg)), kCvThreads, 0, stream(), xp, wp, w_shift.data_ptr<int>(), bias.data_ptr<float>(),
                       x_absmax.data_ptr<float>(), yp, ymax, static_cast<int>(H), static_cast<int>(W), static_cast<int>(C_in),
                       static_cast<int>(C_out), static_cast<int>(Ho), static_cast<int>(Wo), static_cast<int>(pad_h), static_cast<int>(pad_w), TH,
                       TW, static_cast<int>(tiles_x), static_cast<int>(tiles_y), C_y);
  };
  auto shape = [&](auto khc, auto kwc) {
    constexpr int KH = decltype(khc)::value, KW = decltype(kwc)::value;
    if (variant == 0) launch(conv_taps_kernel<KH, KW, 64, 2>);
    else if (variant == 1) launch(conv_taps_kernel<KH, KW, 128, 4>);
    else launch(conv_taps_kernel<KH, KW, 128, 2>);
  };
  using std::integral_constant;
  if (kh == 3 && kw == 3) shape(integral_constant<int, 3>{}, integral_constant<int, 3>{});
  else if (kh == 5) shape(integral_constant<int, 5>{}, integral_constant<int, 5>{});
  else if (kw == 7) shape(integral_constant<int, 1>{}, integral_constant<int, 7>{});
  else if (kh == 7) shape(integral_constant<int, 7>{}, integral_constant<int, 1>{});
  else if (kw == 3) shape(integral_constant<int, 1>{}, integral_constant<int, 3>{});
  else shape(integral_constant<int, 3>{}, integral_constant<int, 1>{});
  TMX_LAUNCH_CHECK();
}

}  // namespace tmx

TORCH_LIBRARY_FRAGMENT(tmx, m) {
  m.def("conv_pack(Tensor w, Tensor bn_weight, Tensor bn_bias, Tensor bn_mean, Tensor bn_var, float eps) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def(
      "conv_bn_relu(Tensor x, Tensor w_planes, Tensor w_shift, Tensor bias, Tensor x_absmax, Tensor(a!) y, Tensor(b!) y_absmax, int c_off, "
      "int kh, int kw, int pad_h, int pad_w) -> ()");
}

TORCH_LIBRARY_IMPL(tmx, CUDA, m) {
  m.impl("conv_pack", &tmx::conv_pack);
  m.impl("conv_bn_relu", &tmx::conv_bn_relu);
}
