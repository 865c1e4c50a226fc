// What the forward (convformer.hip) and backward (convformer_bwd.hip) kernels of the ConvFormer backbone share: the depthwise tile's
// geometry, the limits of the entry points and StarReLU's arithmetic.
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

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
