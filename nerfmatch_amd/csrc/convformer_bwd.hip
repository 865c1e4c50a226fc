// Backward of the four kernels of convformer.hip (the training path of modules/convformer.py).  Notation: a(x) = scale * relu(x)^2 + bias,
// r = relu(x), tap t = ky * 7 + kx; images are zero outside their bounds and the padding comes behind the activation.
//
//   nm_dwconv7_nhwc_bwd_input    da[b,h,w,c] = sum_t w49c[t,c] dy[b, h-ky+3, w-kx+3, c];  dx = da * (2 * (scale * r(x))), dscale = sum da r^2,
//                                dbias = sum da (without the activation: dx = da)
//   nm_dwconv7_nhwc_bwd_weight   dw49c[t,c] = sum_(b,h,w) dy[b,h,w,c] a(x[b, h+ky-3, w+kx-3, c])
//   nm_star_relu_bwd             dx = dy * (2 * (scale * r(x))), dscale = sum dy r^2, dbias = sum dy
//   nm_conv_patches_bwd          the adjoint of the channel-last patch gather, itself a gather: one thread per 16-byte word of dx
//
// Every reduction is ordered: a workgroup writes its partial sums to the caller's workspace and a finishing kernel adds them in index
// order.  No floating-point atomics, the same bits on every run.
//
// Input gradient.  The forward tile kernel -- stage_tile and dw_tile_body of convformer_tile.h, the same text for both -- with dy staged
// in place of x and the taps loaded mirrored (LDS slot t holds tap 48 - t), so da is one fmaf chain per element whatever tile it falls in;
// the epilogue reads x at the lane's own outputs, multiplies and keeps the two
// scalar sums, reduced over the workgroup (xor butterfly per wavefront, the four wavefronts in order) into one partial pair.
//
// Weight gradient.  The sum runs over pixels, so a lane that owns pixels (the forward's plan) needs all 49 x 4 sums of its channel quad
// live at once: 196 accumulators next to 32 registers of dy and 56 of staged inputs are more than the 256 registers that still allow two
// wavefronts per SIMD, and the 49 x 32-lane reduction would come once per tile.  Here a lane owns TAPS instead: channel quad q, kernel row
// ky and one of four row groups of the tile -- 7 x 4 = 28 accumulators, kept in registers while the workgroup walks a whole strip of tiles
// along x.  Both operands then come from LDS: the activated inputs with their halo, staged by the forward kernel's stage_tile, and the
// tile's dy.
// A wavefront is one row group: its lanes are (q, ky) with ky = 7 idle (one lane in eight), they read the same dy word per q (a broadcast)
// and input rows row + ky, which the odd pitch spreads over both halves of the bank row as in the forward kernel.  Per run of 8 pixels a
// lane reads 8 + 14 LDS words for 224 fused multiply-adds.  Tile: BW_TH x 16 pixels with BW_TH = 8, so that inputs (14 x 23 pixels) and
// dy (8 x 16) take 56 KB and two workgroups share a compute unit.  At the end of the strip the four row groups are added through LDS in
// group order and the workgroup writes one (49, 32) partial: (B * ceil(H / 8)) partials per channel slice, not one per tile.
#include "convformer_tile.h"

namespace {

constexpr int BW_TH = 8;                                   // rows of the weight-gradient tile
constexpr int BW_IH = BW_TH + 6;
constexpr int BW_GROUPS = DW_THREADS / 64;                 // row groups = wavefronts
constexpr int BW_ROWS = BW_TH / BW_GROUPS;                 // rows of a group
constexpr int SRB_QUADS = 8;                               // nm_star_relu_bwd: 16-byte words per thread
constexpr int RED_THREADS = 256;

static_assert(BW_TH % BW_GROUPS == 0 && DW_TW % DW_RUN == 0, "whole rows and runs per group");
static_assert((BW_IH * DW_PITCH + BW_TH * DW_TW) * DW_CS * 4 <= 80 * 1024, "two workgroups per compute unit");
static_assert(BW_GROUPS * 49 <= BW_IH * DW_PITCH, "the group sums fit into the input tile's LDS");

// StarReLU's derivative, op for op: returns dx and adds this element's terms of dscale and dbias to ps and pb
__device__ __forceinline__ float star_relu_bwd1(float x, float dy, float sc, float& ps, float& pb) {
  const float r = x < 0.f ? 0.f : x;
  ps += dy * (r * r);
  pb += dy;
  return dy * (2.f * (sc * r));
}

// sum of v over the workgroup's DW_THREADS lanes, valid in thread 0: butterfly per wavefront, then the wavefronts in order
__device__ __forceinline__ float block_sum(float v, float* red_s, int tid) {
  v = wave_sum(v);
  __syncthreads();  // (red_s may still be read from the previous call)
  if (tid % 64 == 0) red_s[tid / 64] = v;
  __syncthreads();
  float s = red_s[0];
#pragma unroll
  for (int i = 1; i < DW_THREADS / 64; ++i) s += red_s[i];
  return s;
}

// part: the caller's workspace [2][workgroups] (dscale partials, then dbias partials), null when the scalars are not wanted
__global__ void __launch_bounds__(DW_THREADS, 2) dwconv7_bwd_input_kernel(const float* __restrict__ dy, const float* __restrict__ w49c,
                                                                       const float* __restrict__ x, const float* __restrict__ act_scale, int H,
                                                                       int W, int C, int tiles_x, float* __restrict__ dx,
                                                                       float* __restrict__ part) {
  __shared__ f32x4 in_s[DW_IH * DW_PITCH * DW_QUADS];
  __shared__ f32x4 w_s[49 * DW_QUADS];
  __shared__ float red_s[DW_THREADS / 64];
  const int tid = threadIdx.x;
  const int ty0 = (blockIdx.x / tiles_x) * DW_TH, tx0 = (blockIdx.x % tiles_x) * DW_TW;
  const int c0 = blockIdx.y * DW_CS;
  const size_t img = (size_t)blockIdx.z * H * W;  // pixels in front of this image
  const bool act = x != nullptr;
  const float sc = act ? act_scale[0] : 0.f;

  for (int i = tid; i < 49 * DW_QUADS; i += DW_THREADS)  // mirrored: dy[h - ky + 3] = dy[h + (6 - ky) - 3]
    w_s[i] = *reinterpret_cast<const f32x4*>(w49c + (size_t)(48 - i / DW_QUADS) * C + c0 + 4 * (i % DW_QUADS));
  stage_tile<DW_IH, DW_IW, DW_PITCH>(dy, img, ty0 - 3, tx0 - 3, c0, H, W, C, false, 0.f, 0.f, in_s, tid);
  __syncthreads();

  const int q = tid % DW_QUADS, slot = tid / DW_QUADS;
  const int run = slot % (DW_TW / DW_RUN), row = slot / (DW_TW / DW_RUN);
  const int oy = ty0 + row, ox0 = tx0 + run * DW_RUN;
  const bool valid = oy < H && ox0 < W;
  float ps = 0.f, pb = 0.f;
  if (valid) {
    f32x4 acc[DW_RUN];
    dw_tile_body(in_s, w_s, q, run, row, acc);
    const size_t o = (img + (size_t)oy * W + ox0) * C + c0 + 4 * q;
#pragma unroll
    for (int r = 0; r < DW_RUN; ++r) {
      if (ox0 + r >= W) continue;
      f32x4 g = acc[r];
      if (act) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + o + (size_t)r * C);
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] = star_relu_bwd1(xv[c], acc[r][c], sc, ps, pb);
      }
      *reinterpret_cast<f32x4*>(dx + o + (size_t)r * C) = g;
    }
  }
  if (part == nullptr) return;  // (uniform over the workgroup)
  const size_t wgs = (size_t)gridDim.x * gridDim.y * gridDim.z;
  const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  ps = block_sum(ps, red_s, tid);
  pb = block_sum(pb, red_s, tid);
  if (tid == 0) {
    part[wg] = ps;
    part[wgs + wg] = pb;
  }
}

// grid (tile rows, channel slices, images); part: [images * tile rows][49][C]
__global__ void __launch_bounds__(DW_THREADS, 2) dwconv7_bwd_weight_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                        const float* __restrict__ act_scale, const float* __restrict__ act_bias,
                                                                        int H, int W, int C, int tiles_x, float* __restrict__ part) {
  __shared__ f32x4 in_s[BW_IH * DW_PITCH * DW_QUADS];
  __shared__ f32x4 dy_s[BW_TH * DW_TW * DW_QUADS];
  const int tid = threadIdx.x;
  const int ty0 = blockIdx.x * BW_TH;
  const int c0 = blockIdx.y * DW_CS;
  const size_t img = (size_t)blockIdx.z * H * W;
  const bool act = act_scale != nullptr;
  const float sc = act ? act_scale[0] : 0.f, bi = act ? act_bias[0] : 0.f;
  const int q = tid % DW_QUADS, ky = (tid % 64) / DW_QUADS, grp = tid / 64;
  const bool active = ky < 7;

  f32x4 acc[7];
#pragma unroll
  for (int kx = 0; kx < 7; ++kx) acc[kx] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int tile = 0; tile < tiles_x; ++tile) {
    const int tx0 = tile * DW_TW;
    if (tile) __syncthreads();  // (the previous tile has been read)
    stage_tile<BW_IH, DW_IW, DW_PITCH>(x, img, ty0 - 3, tx0 - 3, c0, H, W, C, act, sc, bi, in_s, tid);
    stage_tile<BW_TH, DW_TW, DW_TW>(dy, img, ty0, tx0, c0, H, W, C, false, 0.f, 0.f, dy_s, tid);
    __syncthreads();
    if (active) {
#pragma unroll 1
      for (int rr = 0; rr < BW_ROWS; ++rr) {
        const int row = grp * BW_ROWS + rr;
#pragma unroll 1
        for (int run = 0; run < DW_TW / DW_RUN; ++run) {
          f32x4 in[DW_RUN + 6], d[DW_RUN];
          const f32x4* src = in_s + ((row + ky) * DW_PITCH + run * DW_RUN) * DW_QUADS + q;
          const f32x4* dsrc = dy_s + (row * DW_TW + run * DW_RUN) * DW_QUADS + q;
#pragma unroll
          for (int i = 0; i < DW_RUN + 6; ++i) in[i] = src[i * DW_QUADS];
#pragma unroll
          for (int r = 0; r < DW_RUN; ++r) d[r] = dsrc[r * DW_QUADS];
#pragma unroll
          for (int kx = 0; kx < 7; ++kx)
#pragma unroll
            for (int r = 0; r < DW_RUN; ++r)
#pragma unroll
              for (int c = 0; c < 4; ++c) acc[kx][c] = NM_FMA(d[r][c], in[r + kx][c], acc[kx][c]);
        }
      }
    }
  }
  __syncthreads();
  f32x4* red_s = in_s;  // [group][tap][quad]
  if (active)
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) red_s[(grp * 49 + ky * 7 + kx) * DW_QUADS + q] = acc[kx];
  __syncthreads();
  float* out = part + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * 49 * C;
  for (int i = tid; i < 49 * DW_QUADS; i += DW_THREADS) {
    f32x4 s = red_s[i];
#pragma unroll
    for (int g = 1; g < BW_GROUPS; ++g) s += red_s[g * 49 * DW_QUADS + i];
    *reinterpret_cast<f32x4*>(out + (size_t)(i / DW_QUADS) * C + c0 + 4 * (i % DW_QUADS)) = s;
  }
}

// out[i] = the sum over `parts` rows of part[., i], i < n, rows added in index order (four interleaved sums, then (s0 + s1) + (s2 + s3))
__global__ void __launch_bounds__(RED_THREADS) sum_rows_kernel(const float* __restrict__ part, int parts, int n, float* __restrict__ out) {
  const int i = blockIdx.x * RED_THREADS + threadIdx.x;
  if (i >= n) return;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < parts; ++p) s[p & 3] += part[(size_t)p * n + i];
  out[i] = (s[0] + s[1]) + (s[2] + s[3]);
}

// out[j] = the sum of part[j][0 .. parts), j = blockIdx.x: strided sums per thread, then a tree through LDS -- a fixed order
__global__ void __launch_bounds__(RED_THREADS) sum_scalars_kernel(const float* __restrict__ part, size_t parts, float* __restrict__ out) {
  __shared__ float red_s[RED_THREADS];
  const int tid = threadIdx.x;
  const float* p = part + blockIdx.x * parts;
  float s = 0.f;
  for (size_t i = tid; i < parts; i += RED_THREADS) s += p[i];
  red_s[tid] = s;
  __syncthreads();
  for (int o = RED_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red_s[tid] += red_s[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = red_s[0];
}

// a workgroup covers DW_THREADS * SRB_QUADS 16-byte words; block 0 also holds the scalar tail's (at most three) lanes; part as in
// dwconv7_bwd_input_kernel
__global__ void __launch_bounds__(DW_THREADS, 4) star_relu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                      const float* __restrict__ scale, size_t n, float* __restrict__ dx,
                                                                      float* __restrict__ part) {
  __shared__ float red_s[DW_THREADS / 64];
  const int tid = threadIdx.x;
  const float sc = scale[0];
  const size_t n4 = n / 4;
  float ps = 0.f, pb = 0.f;
  const size_t i0 = (size_t)blockIdx.x * (DW_THREADS * SRB_QUADS) + tid;
#pragma unroll
  for (int u = 0; u < SRB_QUADS; ++u) {
    const size_t i = i0 + (size_t)u * DW_THREADS;
    if (i >= n4) break;
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i], dv = reinterpret_cast<const f32x4*>(dy)[i];
    f32x4 g;
#pragma unroll
    for (int c = 0; c < 4; ++c) g[c] = star_relu_bwd1(xv[c], dv[c], sc, ps, pb);
    reinterpret_cast<f32x4*>(dx)[i] = g;
  }
  if (blockIdx.x == 0 && (size_t)tid < n - 4 * n4) dx[4 * n4 + tid] = star_relu_bwd1(x[4 * n4 + tid], dy[4 * n4 + tid], sc, ps, pb);
  if (part == nullptr) return;
  ps = block_sum(ps, red_s, tid);
  pb = block_sum(pb, red_s, tid);
  if (tid == 0) {
    part[blockIdx.x] = ps;
    part[(size_t)gridDim.x + blockIdx.x] = pb;
  }
}

// one thread per 16-byte word of dx [B,H,W,C]: the sum over the patches (b, oy, ox) and taps (ky, kx) that read it, ascending in (ky, kx)
__global__ void __launch_bounds__(256) conv_patches_bwd_kernel(const float* __restrict__ drows, int C, int H, int W, int Ho, int Wo, int k,
                                                               int stride, int pad, int ld, size_t total4, float* __restrict__ dx) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int c4 = C / 4;
  const int c = (int)(i % c4) * 4;
  const size_t pix = i / c4;
  const int ix = (int)(pix % W), iy = (int)((pix / W) % H);
  const size_t b = pix / ((size_t)W * H);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int ky = 0; ky < k; ++ky) {
    const int ty = iy + pad - ky;
    if (ty < 0 || ty % stride || ty / stride >= Ho) continue;
    for (int kx = 0; kx < k; ++kx) {
      const int tx = ix + pad - kx;
      if (tx < 0 || tx % stride || tx / stride >= Wo) continue;
      const size_t row = (b * Ho + ty / stride) * Wo + tx / stride;
      s += *reinterpret_cast<const f32x4*>(drows + row * ld + (size_t)(ky * k + kx) * C + c);
    }
  }
  *reinterpret_cast<f32x4*>(dx + i * 4) = s;
}

size_t input_workgroups(DwTiles t, int B, int C) { return (size_t)t.x * t.y * (C / DW_CS) * B; }
size_t star_blocks(size_t n) { return (n / 4 + DW_THREADS * SRB_QUADS - 1) / (DW_THREADS * SRB_QUADS) + (n < 4 ? 1 : 0); }

}  // namespace

extern "C" size_t nm_dwconv7_nhwc_bwd_input_workspace_bytes(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || !dw_supported(B, H, W, C)) return 0;
  return 2 * input_workgroups(dw_tiles(H, W, DW_TH), B, C) * sizeof(float);
}

extern "C" int nm_dwconv7_nhwc_bwd_input(const float* dy, const float* w49c, const float* x, const float* act_scale, int B, int H, int W, int C,
                                         float* dx, float* dscale_dbias, void* workspace, size_t workspace_bytes, nmStream_t stream) {
  NM_CHECK_ARG(dy && w49c && dx && dx != dy && dx != x && B > 0 && H > 0 && W > 0 && C > 0 && (x != nullptr) == (act_scale != nullptr));
  NM_CHECK_ARG(x || !dscale_dbias);
  NM_CHECK_ARG(aligned16(dy) && aligned16(w49c) && aligned16(dx) && aligned16(x));
  if (!dw_supported(B, H, W, C)) return NM_ERR_UNSUPPORTED;
  const DwTiles t = dw_tiles(H, W, DW_TH);
  const size_t wgs = input_workgroups(t, B, C);
  if (dscale_dbias && (!workspace || workspace_bytes < 2 * wgs * sizeof(float))) return NM_ERR_WORKSPACE;
  float* part = dscale_dbias ? (float*)workspace : nullptr;
  dwconv7_bwd_input_kernel<<<dim3(t.x * t.y, C / DW_CS, B), DW_THREADS, 0, (hipStream_t)stream>>>(dy, w49c, x, act_scale, H, W, C, t.x, dx, part);
  if (part) sum_scalars_kernel<<<2, RED_THREADS, 0, (hipStream_t)stream>>>(part, wgs, dscale_dbias);
  return nm_launch_status();
}

extern "C" size_t nm_dwconv7_nhwc_bwd_weight_workspace_bytes(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || !dw_supported(B, H, W, C)) return 0;
  return (size_t)B * dw_tiles(H, W, BW_TH).y * 49 * C * sizeof(float);
}

extern "C" int nm_dwconv7_nhwc_bwd_weight(const float* dy, const float* x, const float* act_scale, const float* act_bias, int B, int H, int W,
                                          int C, float* dw49c, void* workspace, size_t workspace_bytes, nmStream_t stream) {
  NM_CHECK_ARG(dy && x && dw49c && dw49c != dy && dw49c != x && B > 0 && H > 0 && W > 0 && C > 0 &&
               (act_scale != nullptr) == (act_bias != nullptr));
  NM_CHECK_ARG(aligned16(dy) && aligned16(x) && aligned16(dw49c) && aligned16(workspace));
  if (!dw_supported(B, H, W, C)) return NM_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < nm_dwconv7_nhwc_bwd_weight_workspace_bytes(B, H, W, C)) return NM_ERR_WORKSPACE;
  const DwTiles t = dw_tiles(H, W, BW_TH);
  const size_t parts = (size_t)B * t.y;
  if (parts > 0x7fffffffu) return NM_ERR_UNSUPPORTED;
  float* part = (float*)workspace;
  dwconv7_bwd_weight_kernel<<<dim3(t.y, C / DW_CS, B), DW_THREADS, 0, (hipStream_t)stream>>>(dy, x, act_scale, act_bias, H, W, C, t.x, part);
  sum_rows_kernel<<<(49 * C + RED_THREADS - 1) / RED_THREADS, RED_THREADS, 0, (hipStream_t)stream>>>(part, (int)parts, 49 * C, dw49c);
  return nm_launch_status();
}

extern "C" size_t nm_star_relu_bwd_workspace_bytes(size_t n) { return n ? 2 * star_blocks(n) * sizeof(float) : 0; }

extern "C" int nm_star_relu_bwd(const float* x, const float* dy, const float* scale, size_t n, float* dx, float* dscale_dbias, void* workspace,
                                size_t workspace_bytes, nmStream_t stream) {
  NM_CHECK_ARG(x && dy && scale && dx && dx != x && dx != dy && n > 0);
  NM_CHECK_ARG(aligned16(x) && aligned16(dy) && aligned16(dx));
  const size_t blocks = star_blocks(n);
  if (blocks > 0x7fffffffu) return NM_ERR_UNSUPPORTED;
  if (dscale_dbias && (!workspace || workspace_bytes < 2 * blocks * sizeof(float))) return NM_ERR_WORKSPACE;
  float* part = dscale_dbias ? (float*)workspace : nullptr;
  star_relu_bwd_kernel<<<(unsigned)blocks, DW_THREADS, 0, (hipStream_t)stream>>>(x, dy, scale, n, dx, part);
  if (part) sum_scalars_kernel<<<2, RED_THREADS, 0, (hipStream_t)stream>>>(part, blocks, dscale_dbias);
  return nm_launch_status();
}

extern "C" int nm_conv_patches_bwd(const float* drows, int layout, int B, int C, int H, int W, int k, int stride, int pad, int ld, float* dx,
                                   nmStream_t stream) {
  int Ho, Wo;  // (the adjoint exists for channel-last words only)
  if (const int err = conv_patch_args(drows, dx, aligned16(drows) && aligned16(dx), layout == 1 && C % 4 == 0, layout, B, C, H, W, k, stride, pad,
                                      ld, &Ho, &Wo))
    return err;
  const size_t total4 = (size_t)B * H * W * (C / 4), blocks = (total4 + 255) / 256;
  if (blocks > 0x7fffffffu) return NM_ERR_UNSUPPORTED;
  conv_patches_bwd_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(drows, C, H, W, Ho, Wo, k, stride, pad, ld, total4, dx);
  return nm_launch_status();
}
