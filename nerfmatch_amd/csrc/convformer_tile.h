// The depthwise tile of the ConvFormer backbone, owned here for the forward (convformer.hip) and backward (convformer_bwd.hip) kernels:
// its geometry, its one staging loop (stage_tile), its one body (dw_tile_body), StarReLU's arithmetic, and the argument rules and grid
// arithmetic that the entry points of both files share.
#pragma once
#include "common.h"

namespace {

constexpr int DW_TH = NM_DWCONV_TILE_H, DW_TW = NM_DWCONV_TILE_W;
constexpr int DW_CS = 32;                 // channels of a workgroup (8 lanes x 4 channels = 128 B per pixel)
constexpr int DW_RUN = 8;                 // outputs along x per lane
constexpr int DW_THREADS = 256;
constexpr int DW_LOADS = 8;               // staging: 16-byte loads of a thread in flight together
constexpr int DW_IH = DW_TH + 6, DW_IW = DW_TW + 6;
constexpr int DW_PITCH = DW_IW | 1;       // pixels per staged row (odd, see convformer.hip)
constexpr int DW_QUADS = DW_CS / 4;       // 16-byte words per pixel
constexpr int DW_MAX_SIDE = 8192, DW_MAX_C = 1024;

static_assert((DW_TW / DW_RUN) * DW_TH * DW_QUADS == DW_THREADS, "one run of outputs per lane");

// StarReLU, op for op (three roundings; a NaN passes through the comparison)
__device__ __forceinline__ float star_relu1(float x, float scale, float bias) {
  const float r = x < 0.f ? 0.f : x;
  float t = r * r;
  t = scale * t;
  return t + bias;
}
__device__ __forceinline__ f32x4 star_relu4(f32x4 v, float scale, float bias) {
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = star_relu1(v[i], scale, bias);
  return o;
}

// ROWS x COLS pixels of DW_CS channels from (y0, x0) on to LDS, PITCH pixels per row; pixels outside the image are staged as zero, the
// others activated when `act` (the padding comes behind the activation).  Without branches: every load is issued, at the address
// clamped into the image, and a word from outside is replaced by zeros behind the activation.  DW_LOADS global loads of a thread are in
// flight together: one at a time, a 22 x 22 tile's 16 rounds each wait out a memory latency.
// `src` is fp32 or fp16 (load_quad: fp16 -> fp32 is exact); the LDS image is fp32 either way.
__device__ __forceinline__ f32x4 load_quad(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load_quad(const _Float16* p) {
  const f16x4 h = *reinterpret_cast<const f16x4*>(p);
  return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

template <int ROWS, int COLS, int PITCH, class T>
__device__ __forceinline__ void stage_tile(const T* __restrict__ src, size_t img, int y0, int x0, int c0, int H, int W, int C, bool act,
                                           float sc, float bi, f32x4* __restrict__ dst_s, int tid) {
  constexpr int N = ROWS * COLS * DW_QUADS;
  constexpr int LOADS = N < DW_LOADS * DW_THREADS ? (N + DW_THREADS - 1) / DW_THREADS : DW_LOADS;
  for (int base = 0; base < N; base += LOADS * DW_THREADS) {
    f32x4 v[LOADS];
    int dst[LOADS];
    bool inside[LOADS];
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      const int i = min(base + u * DW_THREADS + tid, N - 1);  // (past the end: the last word once more)
      const int q = i % DW_QUADS, p = i / DW_QUADS, px = p % COLS, py = p / COLS;
      const int gy = y0 + py, gx = x0 + px;
      dst[u] = (py * PITCH + px) * DW_QUADS + q;
      inside[u] = gy >= 0 && gy < H && gx >= 0 && gx < W;
      const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);
      v[u] = load_quad(src + (img + (size_t)cy * W + cx) * C + c0 + 4 * q);
    }
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      if (act) v[u] = star_relu4(v[u], sc, bi);
      dst_s[dst[u]] = inside[u] ? v[u] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

// The tile body.  in_s: a staged DW_IH x DW_IW tile at pitch DW_PITCH; w_s: 49 staged taps.  The lane (q, run, row) -- channel quad,
// run of DW_RUN outputs along x, tile row -- fills acc[r] with output (row, run * DW_RUN + r): one fmaf chain from 0 over the LDS tap
// slots t = ky * 7 + kx in that order, slot t against input (row + ky, x + kx), whatever tile the output falls in.  Which tap a slot
// holds is the caller's choice: in order for the convolution, mirrored for its input gradient.
__device__ __forceinline__ void dw_tile_body(const f32x4* in_s, const f32x4* w_s, int q, int run, int row, f32x4 (&acc)[DW_RUN]) {
#pragma unroll
  for (int r = 0; r < DW_RUN; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1  // (one kernel row's 21 LDS words live at a time: unrolled, the scheduler hoists all 147 and spills)
  for (int ky = 0; ky < 7; ++ky) {
    f32x4 in[DW_RUN + 6], wk[7];
    const f32x4* src = in_s + ((row + ky) * DW_PITCH + run * DW_RUN) * DW_QUADS + q;
#pragma unroll
    for (int i = 0; i < DW_RUN + 6; ++i) in[i] = src[i * DW_QUADS];
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) wk[kx] = w_s[(ky * 7 + kx) * DW_QUADS + q];
#pragma unroll
    for (int kx = 0; kx < 7; ++kx)
#pragma unroll
      for (int r = 0; r < DW_RUN; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = NM_FMA(in[r + kx][c], wk[kx][c], acc[r][c]);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- host side: what the entry points of both files check and count the same way
inline bool dw_supported(int B, int H, int W, int C) { return C % 64 == 0 && C <= DW_MAX_C && H <= DW_MAX_SIDE && W <= DW_MAX_SIDE && B <= 65535; }

// tiles along x and y of an H x W map cut into tiles of th rows (DW_TH, or the weight gradient's BW_TH) and DW_TW columns
struct DwTiles {
  int x, y;
};
inline DwTiles dw_tiles(int H, int W, int th) { return {(W + DW_TW - 1) / DW_TW, (H + th - 1) / th}; }

// The argument rules of the patch gather and its adjoint, in their order: the operands (aligned: the caller's own alignment rule),
// then the limits (supported: the caller's own, on top of the shared ones), then ld, then the image against the kernel.  NM_OK: Ho, Wo
// are the patch grid.
inline int conv_patch_args(const void* src, const void* dst, bool aligned, bool supported, int layout, int B, int C, int H, int W, int k,
                           int stride, int pad, int ld, int* Ho, int* Wo) {
  NM_CHECK_ARG(src && dst && src != dst && (layout == 0 || layout == 1) && B > 0 && C > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0);
  NM_CHECK_ARG(aligned);
  if (!supported || k > 7 || stride > 8 || pad >= k || C > DW_MAX_C || H > DW_MAX_SIDE || W > DW_MAX_SIDE) return NM_ERR_UNSUPPORTED;
  NM_CHECK_ARG(ld % 8 == 0 && ld >= k * k * C);
  NM_CHECK_ARG(H + 2 * pad >= k && W + 2 * pad >= k);
  *Ho = (H + 2 * pad - k) / stride + 1, *Wo = (W + 2 * pad - k) / stride + 1;
  return NM_OK;
}

}  // namespace
