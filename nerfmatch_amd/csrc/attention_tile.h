// The head-dim-32 tile vocabulary of the matrix-core attention kernels (attention*.hip; gemm_bf16.hip writes their K / V operands):
// the K / V slot layout, the XCD-aware work mapping with its grid, and the row helpers (row loads, hi / lo split of an accumulator,
// scaled row store).  A kernel whose code changed when one of these pieces became a call keeps that piece written out and says so;
// waits on in-flight loads are kernel-specific and stay in the .hip files.
#pragma once
#include "bf16x3.h"

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// Operand slots: one per (batch, head, tile), tiles of one (batch, head) contiguous -- slot index ((b H + h) nt + t), times the slot size.
__host__ __device__ __forceinline__ constexpr size_t tile_slot(int b, int H, int h, int nt, int t) { return ((size_t)b * H + h) * nt + t; }

// K / V slot of the split-bf16 forward kernel: NM_SLOT8K_BYTES per 32-key tile = 8 pieces of 64 lanes x 16 bytes (8 bf16), piece =
// {K, V^T} x {k-step 0, 1} x {hi, lo}.  K: lane (key r, half) holds dims 16 ks + 8 half + i; V^T: lane (dim r, half) holds keys
// nrow(8 ks + i, half).  Writers: kv_presplit_kernel, epilogue_keys / epilogue_values (gemm_bf16.hip); reader: attn32_v3_kernel.
enum { AT_K = 0, AT_VT = 1, AT_HI = 0, AT_LO = 1 };
constexpr int AT_PIECE_BYTES = 64 * 16;
__host__ __device__ __forceinline__ constexpr int at_piece(int which, int ks, int hl) { return which * 4 + ks * 2 + hl; }
static_assert(at_piece(AT_K, 0, AT_HI) == 0 && at_piece(AT_K, 0, AT_LO) == 1 && at_piece(AT_K, 1, AT_HI) == 2, "K pieces 0..3");
static_assert(at_piece(AT_VT, 0, AT_HI) == 4 && at_piece(AT_VT, 1, AT_HI) == 6 && at_piece(AT_VT, 1, AT_LO) == 7, "V^T pieces 4..7");
static_assert(at_piece(AT_VT, 1, AT_LO) == at_piece(AT_VT, 1, AT_HI) + 1, "a lo piece follows its hi piece");
static_assert(8 * AT_PIECE_BYTES == NM_SLOT8K_BYTES, "8 pieces fill the slot");

// XCD-aware 1-D grid, block 256 = 4 wavefronts x 32 rows: consecutive workgroup ids go round robin to the 8 XCDs (each with its own
// 4 MiB L2), so id -> (xcd = id % 8, row block = (id / 8) % nblk, (batch, head) = 8 (id / (8 nblk)) + xcd): all row blocks of one
// (batch, head) run on ONE XCD, whose L2 then holds the slots they all stream.  false: padding (B H is rounded up to a multiple of 8).
__host__ __device__ __forceinline__ constexpr int row_blocks(int n) { return ((n + 31) / 32 + 3) / 4; }
__device__ __forceinline__ bool map_work(int nblk, int BH, int& bh, int& blk) {
  const int xcd = blockIdx.x & 7, jj = blockIdx.x >> 3;
  bh = 8 * (jj / nblk) + xcd;
  blk = jj % nblk;
  return bh < BH;
}
// its grid; false (grid untouched) if the workgroup count does not fit
__host__ __forceinline__ bool map_work_grid(int BH, int nblk, unsigned& grid) {
  const long long g = (long long)((BH + 7) / 8) * 8 * nblk;
  if (g > 0x7fffffffLL) return false;
  grid = (unsigned)g;
  return true;
}

// a lane's share of a row as B operand of the fp32 MFMA, scaled: dims 8c + 4hi + t (p already offset by 4hi)
__device__ __forceinline__ void load16(const float* p, float s, float (&reg)[16]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4 t4 = *reinterpret_cast<const f32x4*>(p + 8 * c);
#pragma unroll
    for (int t = 0; t < 4; ++t) reg[4 * c + t] = t4[t] * s;
  }
}
// ... and of the 16-wide k-steps m = 0, 1: dims 16 m + 8 half + i (p already offset by 8 half); load_split: as bf16 hi / lo
__device__ __forceinline__ void load8(const float* p, float s, float (&v8)[8]) {
  const f32x4 a4 = *reinterpret_cast<const f32x4*>(p), b4 = *reinterpret_cast<const f32x4*>(p + 4);
  v8[0] = a4[0] * s; v8[1] = a4[1] * s; v8[2] = a4[2] * s; v8[3] = a4[3] * s; v8[4] = b4[0] * s; v8[5] = b4[1] * s; v8[6] = b4[2] * s; v8[7] = b4[3] * s;
}
__device__ __forceinline__ void load_row(const float* p, float s, float (&v)[2][8]) {
#pragma unroll
  for (int m = 0; m < 2; ++m) load8(p + 16 * m, s, v[m]);
}
__device__ __forceinline__ void load_split(const float* p, float s, bf16x8 (&h)[2], bf16x8 (&l)[2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    float v8[8];
    load8(p + 16 * m, s, v8);
    split8(v8, h[m], l[m]);
  }
}

// 16 accumulator values -> the B operands of the next product's two k-steps
__device__ __forceinline__ void split16(const f32x16& v, bf16x8 (&h)[2], bf16x8 (&l)[2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const float v8[8] = {v[8 * m], v[8 * m + 1], v[8 * m + 2], v[8 * m + 3], v[8 * m + 4], v[8 * m + 5], v[8 * m + 6], v[8 * m + 7]};
    split8(v8, h[m], l[m]);
  }
}

// row epilogue: register 4g+e <-> dim 8g + 4hi + e (p already offset by 4hi), scaled, as four 16-byte stores
__device__ __forceinline__ void store16(float* p, const f32x16& a, float s) {
#pragma unroll
  for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(p + 8 * g) = f32x4{a[4 * g] * s, a[4 * g + 1] * s, a[4 * g + 2] * s, a[4 * g + 3] * s};
}
