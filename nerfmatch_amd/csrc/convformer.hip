// The memory-bound kernels of the ConvFormer image backbone (modules/convformer.py): stem plus stages 0 and 1 of a MetaFormer whose
// token mixer is a separable convolution.  Activations are channel-last rows (B*H*W, C) from the stem to the two returned maps, so every
// 1x1 convolution is nm_linear and every LayerNorm nm_layernorm as they stand; this file holds what those two do not cover:
//
//   nm_conv_patches   the k x k patches of a strided convolution as GEMM rows (the 7x7 stem and the 3x3 downsample are then nm_linear)
//   nm_dwconv7_nhwc   the 7x7 depthwise convolution of the token mixer, with StarReLU applied to its input on the way into LDS
//   nm_star_relu      StarReLU between the two 1x1 convolutions of the channel MLP
//   nm_nhwc_to_nchw   the returned maps as the planes the matcher's contract names
//
// Depthwise kernel.  One workgroup makes a tile of DW_TH x DW_TW outputs of DW_CS = 32 channels.  The (DW_TH + 6) x (DW_TW + 6) input
// pixels of those channels go to LDS once, 128 contiguous bytes per pixel, activated as they are staged (an out-of-image pixel is staged as
// zero: the padding comes behind the activation) -- stage_tile of convformer_tile.h, which the backward kernels stage with too; the sums
// are dw_tile_body of that header, shared with the input-gradient kernel.  A lane owns four channels and a run of DW_RUN = 8 outputs
// along x of one row; per kernel row it reads the run's 14 inputs and the row's 7 weights as 16-byte LDS words and issues 8 x 7 x 4 fused multiply-adds, so an output
// costs (7 * 14 + 49) / 8 = 18 LDS reads instead of 98, and an output's sum is one fmaf chain over the taps in (ky, kx) order whatever
// tile it falls in.  LDS pitch: 23 pixels (odd) -- the run slots of the 16 lanes that one ds_read_b128 cycle serves (two rows x two runs)
// then start on both 128-byte halves of the 256-byte bank row; with an even pitch all four start on the same half (2-way conflict).
// Arithmetic intensity: 98 flop per 8 bytes of compulsory traffic; at the chip's copy rate that is close to the rate of unpacked fp32
// FMAs, so the kernel is expected to sit between the two bounds, not at the copy rate.
#include "convformer_tile.h"

namespace {

static_assert((DW_IH * DW_PITCH + 49) * DW_CS * 4 <= 80 * 1024, "two workgroups per compute unit");

// T: fp32, or fp16 in AND out (the fp16 inference walk): the typed load of stage_tile widens exactly, the LDS image, the activation and the
// sums are those of the fp32 kernel, and the store rounds the sum once to fp16 (round to nearest even, overflow to infinity; a sum that was
// finite and is stored as infinity is counted into `overflow`).  So the fp16 kernel's result is the fp32 kernel's on the widened input, rounded.
__device__ __forceinline__ void store_quad(float* p, f32x4 v, int&) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void store_quad(_Float16* p, f32x4 v, int& events) {
  f16x4 h;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = (_Float16)v[e];
    events += f16_overflowed(v[e], h[e]) ? 1 : 0;
  }
  *reinterpret_cast<f16x4*>(p) = h;
}

template <class T>
__global__ void __launch_bounds__(DW_THREADS) dwconv7_nhwc_kernel(const T* __restrict__ x, const float* __restrict__ w49c,
                                                                  const float* __restrict__ act_scale, const float* __restrict__ act_bias,
                                                                  int H, int W, int C, int tiles_x, T* __restrict__ y, int* overflow) {
  __shared__ f32x4 in_s[DW_IH * DW_PITCH * DW_QUADS];
  __shared__ f32x4 w_s[49 * DW_QUADS];
  const int tid = threadIdx.x;
  const int ty0 = (blockIdx.x / tiles_x) * DW_TH, tx0 = (blockIdx.x % tiles_x) * DW_TW;
  const int c0 = blockIdx.y * DW_CS;
  const size_t img = (size_t)blockIdx.z * H * W;  // pixels in front of this image
  const bool act = act_scale != nullptr;
  const float sc = act ? act_scale[0] : 0.f, bi = act ? act_bias[0] : 0.f;

  for (int i = tid; i < 49 * DW_QUADS; i += DW_THREADS)
    w_s[i] = *reinterpret_cast<const f32x4*>(w49c + (size_t)(i / DW_QUADS) * C + c0 + 4 * (i % DW_QUADS));
  stage_tile<DW_IH, DW_IW, DW_PITCH>(x, img, ty0 - 3, tx0 - 3, c0, H, W, C, act, sc, bi, in_s, tid);
  __syncthreads();

  const int q = tid % DW_QUADS, slot = tid / DW_QUADS;
  const int run = slot % (DW_TW / DW_RUN), row = slot / (DW_TW / DW_RUN);
  const int oy = ty0 + row, ox0 = tx0 + run * DW_RUN;
  if (oy >= H || ox0 >= W) return;
  f32x4 acc[DW_RUN];
  dw_tile_body(in_s, w_s, q, run, row, acc);
  T* out = y + (img + (size_t)oy * W + ox0) * C + c0 + 4 * q;
  int events = 0;
#pragma unroll
  for (int r = 0; r < DW_RUN; ++r)
    if (ox0 + r < W) store_quad(out + (size_t)r * C, acc[r], events);
  if (events && overflow) atomicAdd(overflow, events);
}

constexpr int SR_THREADS = 256;

__global__ void __launch_bounds__(SR_THREADS) star_relu_kernel(const float* x, const float* __restrict__ scale, const float* __restrict__ bias,
                                                               size_t n, float* y) {
  const float sc = scale[0], bi = bias[0];
  const size_t n4 = n / 4, i = (size_t)blockIdx.x * SR_THREADS + threadIdx.x;
  if (i < n4) reinterpret_cast<f32x4*>(y)[i] = star_relu4(reinterpret_cast<const f32x4*>(x)[i], sc, bi);
  if (i < n - 4 * n4) y[4 * n4 + i] = star_relu1(x[4 * n4 + i], sc, bi);  // the scalar tail (at most three elements)
}

// rows [B Ho Wo][ld]: column (ky k + kx) C + c of row (b, oy, ox) = x[b, c, oy s - p + ky, ox s - p + kx], zero outside the image and in
// the columns from k k C on.  One thread per four columns.  VEC: channel-last input with C % 4 == 0 -- the four columns are one 16-byte word
// of one pixel.
template <bool VEC>
__global__ void __launch_bounds__(256) conv_patches_kernel(const float* __restrict__ x, int layout, int C, int H, int W, int Ho, int Wo, int k,
                                                           int stride, int pad, int ld, size_t total4, float* __restrict__ rows) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int ld4 = ld / 4;
  const size_t row = i / ld4;
  const int col0 = (int)(i - row * ld4) * 4;
  const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho);
  const size_t b = row / ((size_t)Wo * Ho);
  const int kkc = k * k * C;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    if (col0 < kkc) {
      const int tap = col0 / C, c = col0 - tap * C, ky = tap / k, kx = tap - ky * k;
      const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *reinterpret_cast<const f32x4*>(x + ((b * H + iy) * W + ix) * C + c);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = col0 + j;
      if (col >= kkc) continue;
      const int tap = col / C, c = col - tap * C, ky = tap / k, kx = tap - ky * k;
      const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      v[j] = layout ? x[((b * H + iy) * W + ix) * C + c] : x[((b * C + c) * H + iy) * W + ix];
    }
  }
  *reinterpret_cast<f32x4*>(rows + row * ld + col0) = v;
}

// The same gather with fp16 rows: one thread per eight columns (one 16-byte word of the row).  LAYOUT 0: fp32 planes, each value rounded to
// fp16 as it is gathered (an image value that was finite and is stored as infinity is counted into `overflow`); LAYOUT 1: fp16 channel-last
// rows with C % 8 == 0 -- the eight columns are one 16-byte word of one pixel, copied as it is.
template <int LAYOUT>
__global__ void __launch_bounds__(256) conv_patches_f16_kernel(const void* __restrict__ xv, int C, int H, int W, int Ho, int Wo, int k, int stride,
                                                               int pad, int ld, size_t total8, _Float16* __restrict__ rows, int* overflow) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total8) return;
  const int ld8 = ld / 8;
  const size_t row = i / ld8;
  const int col0 = (int)(i - row * ld8) * 8;
  const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho);
  const size_t b = row / ((size_t)Wo * Ho);
  const int kkc = k * k * C;
  u32x4 out = {0u, 0u, 0u, 0u};
  if (LAYOUT == 1) {
    const _Float16* x = static_cast<const _Float16*>(xv);
    if (col0 < kkc) {
      const int tap = col0 / C, c = col0 - tap * C, ky = tap / k, kx = tap - ky * k;
      const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) out = *reinterpret_cast<const u32x4*>(x + ((b * H + iy) * W + ix) * C + c);
    }
  } else {
    const float* x = static_cast<const float*>(xv);
    f16x8 h = {0, 0, 0, 0, 0, 0, 0, 0};
    int events = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = col0 + j;
      if (col >= kkc) continue;
      const int tap = col / C, c = col - tap * C, ky = tap / k, kx = tap - ky * k;
      const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const float v = x[((b * C + c) * H + iy) * W + ix];
      h[j] = (_Float16)v;
      events += f16_overflowed(v, h[j]) ? 1 : 0;
    }
    out = __builtin_bit_cast(u32x4, h);
    if (events && overflow) atomicAdd(overflow, events);
  }
  *reinterpret_cast<u32x4*>(rows + row * ld + col0) = out;
}

constexpr int TR_TILE = 64;

// y[b][c][p] = x[b][p][c]: a 64 x 64 tile through LDS (pitch 65 words: the column reads touch 64 banks); 16-byte reads along c, the lanes of
// a wavefront write 256 contiguous bytes along p (a plane's rows start at any multiple of 4 bytes, so the writes stay single words)
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const float* __restrict__ x, int HW, int C, float* __restrict__ y) {
  __shared__ float tile[TR_TILE][TR_TILE + 1];
  const int tid = threadIdx.x;
  const int p0 = blockIdx.x * TR_TILE, c0 = blockIdx.y * TR_TILE;
  const size_t base = (size_t)blockIdx.z * HW * C;
  for (int i = tid; i < TR_TILE * (TR_TILE / 4); i += 256) {
    const int cq = i % (TR_TILE / 4), p = i / (TR_TILE / 4);
    if (p0 + p < HW && c0 + 4 * cq < C) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + base + (size_t)(p0 + p) * C + c0 + 4 * cq);
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[p][4 * cq + j] = v[j];
    }
  }
  __syncthreads();
  for (int i = tid; i < TR_TILE * TR_TILE; i += 256) {
    const int p = i % TR_TILE, c = i / TR_TILE;
    if (p0 + p < HW && c0 + c < C) y[base + (size_t)(c0 + c) * HW + p0 + p] = tile[p][c];
  }
}

}  // namespace

extern "C" int nm_dwconv7_nhwc(const float* x, const float* w49c, const float* act_scale, const float* act_bias, int B, int H, int W, int C,
                               float* y, nmStream_t stream) {
  NM_CHECK_ARG(x && w49c && y && x != y && B > 0 && H > 0 && W > 0 && C > 0 && (act_scale != nullptr) == (act_bias != nullptr));
  NM_CHECK_ARG(aligned16(x) && aligned16(w49c) && aligned16(y));
  if (!dw_supported(B, H, W, C)) return NM_ERR_UNSUPPORTED;
  const DwTiles t = dw_tiles(H, W, DW_TH);
  dwconv7_nhwc_kernel<float><<<dim3(t.x * t.y, C / DW_CS, B), DW_THREADS, 0, (hipStream_t)stream>>>(x, w49c, act_scale, act_bias, H, W, C, t.x, y, nullptr);
  return nm_launch_status();
}

extern "C" int nm_dwconv7_nhwc_f16(const void* x, const float* w49c, const float* act_scale, const float* act_bias, int B, int H, int W, int C,
                                   void* y, int* overflow, nmStream_t stream) {
  NM_CHECK_ARG(x && w49c && y && x != y && B > 0 && H > 0 && W > 0 && C > 0 && (act_scale != nullptr) == (act_bias != nullptr));
  NM_CHECK_ARG(aligned16(x) && aligned16(w49c) && aligned16(y));
  if (!dw_supported(B, H, W, C)) return NM_ERR_UNSUPPORTED;
  const DwTiles t = dw_tiles(H, W, DW_TH);
  dwconv7_nhwc_kernel<_Float16><<<dim3(t.x * t.y, C / DW_CS, B), DW_THREADS, 0, (hipStream_t)stream>>>(
      static_cast<const _Float16*>(x), w49c, act_scale, act_bias, H, W, C, t.x, static_cast<_Float16*>(y), overflow);
  return nm_launch_status();
}

extern "C" int nm_star_relu(const float* x, const float* scale, const float* bias, size_t n, float* y, nmStream_t stream) {
  NM_CHECK_ARG(x && scale && bias && y && n > 0);
  NM_CHECK_ARG(aligned16(x) && aligned16(y));
  const size_t blocks = (n / 4 + SR_THREADS) / SR_THREADS;  // (>= 1, and block 0 also holds the tail's three lanes)
  if (blocks > 0x7fffffffu) return NM_ERR_UNSUPPORTED;
  star_relu_kernel<<<(unsigned)blocks, SR_THREADS, 0, (hipStream_t)stream>>>(x, scale, bias, n, y);
  return nm_launch_status();
}

extern "C" int nm_conv_patches(const float* x, int layout, int B, int C, int H, int W, int k, int stride, int pad, int ld, float* rows,
                               nmStream_t stream) {
  // the NCHW gather reads single floats: a batch slice of odd-sized images starts at any multiple of 4 bytes
  const bool aligned = ((uintptr_t)x & 3) == 0 && (layout == 0 || aligned16(x)) && aligned16(rows);
  int Ho, Wo;
  if (const int err = conv_patch_args(x, rows, aligned, true, layout, B, C, H, W, k, stride, pad, ld, &Ho, &Wo)) return err;
  const size_t total4 = (size_t)B * Ho * Wo * (ld / 4), blocks = (total4 + 255) / 256;
  if (blocks > 0x7fffffffu) return NM_ERR_UNSUPPORTED;
  if (layout == 1 && C % 4 == 0)
    conv_patches_kernel<true><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, layout, C, H, W, Ho, Wo, k, stride, pad, ld, total4, rows);
  else
    conv_patches_kernel<false><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, layout, C, H, W, Ho, Wo, k, stride, pad, ld, total4, rows);
  return nm_launch_status();
}

extern "C" int nm_conv_patches_f16(const void* x, int layout, int B, int C, int H, int W, int k, int stride, int pad, int ld, void* rows,
                                   int* overflow, nmStream_t stream) {
  // (layout 0: fp32 planes read as single floats, as nm_conv_patches reads them; layout 1: fp16 pixels read in 16-byte words)
  const bool aligned = ((uintptr_t)x & 3) == 0 && (layout == 0 || aligned16(x)) && aligned16(rows);
  int Ho, Wo;
  if (const int err = conv_patch_args(x, rows, aligned, layout == 0 || C % 8 == 0, layout, B, C, H, W, k, stride, pad, ld, &Ho, &Wo)) return err;
  const size_t total8 = (size_t)B * Ho * Wo * (ld / 8), blocks = (total8 + 255) / 256;
  if (blocks > 0x7fffffffu) return NM_ERR_UNSUPPORTED;
  _Float16* r16 = static_cast<_Float16*>(rows);
  if (layout == 1) conv_patches_f16_kernel<1><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, C, H, W, Ho, Wo, k, stride, pad, ld, total8, r16, overflow);
  else conv_patches_f16_kernel<0><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, C, H, W, Ho, Wo, k, stride, pad, ld, total8, r16, overflow);
  return nm_launch_status();
}

extern "C" int nm_nhwc_to_nchw(const float* x, int B, int HW, int C, float* y, nmStream_t stream) {
  NM_CHECK_ARG(x && y && x != y && B > 0 && HW > 0 && C > 0);
  NM_CHECK_ARG(aligned16(x) && aligned16(y));
  if (C % 4 || C > 65535 * TR_TILE || B > 65535) return NM_ERR_UNSUPPORTED;
  const dim3 grid((HW + TR_TILE - 1) / TR_TILE, (C + TR_TILE - 1) / TR_TILE, B);
  nhwc_to_nchw_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, HW, C, y);
  return nm_launch_status();
}
