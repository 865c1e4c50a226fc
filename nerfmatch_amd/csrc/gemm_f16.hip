// y[M,N] = epi(x[M,K] . w[N,K]^T) with fp16 operands and ONE product per K-step on v_mfma_f32_32x32x16_f16, fp32 accumulation: the GEMM of
// the ConvFormer backbone's fp16 inference walk (modules/convformer.py).  The structure is gemm_bf16.hip's:
//
//   * the weights are rounded to fp16 (round to nearest even, overflow to infinity) and laid out once (nm_linear_pack_f16, on the device) into
//     8 KiB slots = one 32-wide K-step (two MFMA K-steps) of a chunk of 128 output features, in A-operand order;
//   * a workgroup = 4 wavefronts x 32 rows computes a 128-row x 128-column tile: the slots are streamed through the LDS ring with
//     global_load_lds one slot ahead (one full s_waitcnt + one s_barrier per slot: see `step`); the rows of x arrive as 16-byte fp16 pieces
//     that already are B operands -- a lane reads 32 contiguous bytes per slot, k = 32 s + 16 half .. + 15, the first 8 for the slot's first
//     MFMA K-step and the last 8 for its second (the order of k inside a product is free as long as both operands agree);
//   * result layout lane = row, register = feature; the epilogue transposes the tile through the (by then idle) LDS ring and writes row
//     segments (gemm_bf16.hip's header has the measurement behind that: the lane = row store pattern halves the throughput as soon as
//     it is mixed with loads).  fp32 output: 256-byte segments, the residual read in the same layout.  fp16 output: 128-byte segments.
//   * epilogue: the bias is the accumulators' starting value; StarReLU (scale * relu(v)^2 + bias, op for op star_relu1) is applied to the
//     fp32 accumulator, then -- fp16 output -- rounded once, round to nearest even, no saturation.  Every stored fp16 value that is not
//     finite while the accumulator it came from was is counted into `overflow` (one vector atomic add per lane that saw one).
//
// A row's result does not depend on M or on the row's place in the tile: column j of an MFMA is a function of column j of its B operand.
// The kernel is byte-bound at the backbone's shapes (K <= 1152: at most 72 MFMAs of 16 passes per wavefront against 32 rows x (K + N) x 2..4
// bytes), hence no small-grid form and no hand scheduling.
#include "convformer_tile.h"

namespace {

constexpr int GH_ROWS = 128;          // rows per workgroup
constexpr int GH_COLS = 128;          // output features per workgroup (4 blocks of 32)
constexpr int GH_KSLOT = 32;          // K per slot
constexpr int GH_SLOT_BYTES = 8192;   // 2 K-steps x 4 blocks x 64 lanes x 16 bytes
constexpr int GH_SLOT_FLOATS = GH_SLOT_BYTES / 4;
constexpr int GH_RING = 4;            // (one slot ahead needs two positions; the epilogue's transposition buffer needs the four)

struct GemmHArgs {
  const _Float16* x;
  const char* blob;
  const float* bias;
  const float* star;  // StarReLU's scale and bias, one device float each (STAR kernels)
  const float* star_bias;
  const float* res;
  void* y;
  int* overflow;
  int M, N, K, nks;
};

// slot g of the stream -> ring position g % GH_RING: two 1 KiB pieces per wavefront (cf. dma_slot_8k of bf16x3.h)
__device__ __forceinline__ void dma_slot(const char* slots, int g, float* ring, int wave, int lane) {
  const unsigned voff = (unsigned)(wave * 2048 + lane * 16);
  const auto* src = (const __attribute__((address_space(1))) void*)(slots + (size_t)g * GH_SLOT_BYTES + voff);
  auto* dst = (__attribute__((address_space(3))) void*)(ring + (g & (GH_RING - 1)) * GH_SLOT_FLOATS + wave * 512);
  __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
  __builtin_amdgcn_global_load_lds(src, dst, 16, 1024, 0);
}

struct XRowH {
  u32x4 a, b;  // x[m][32 s + 16 half .. + 7], .. + 8 .. + 15
};

// OUT16: fp16 output (no residual); STAR: StarReLU on the accumulator
template <bool OUT16, bool STAR>
__global__ void __launch_bounds__(256, 4) gemm_f16_kernel(GemmHArgs a) {
  __shared__ __attribute__((aligned(16))) float ring[GH_RING * GH_SLOT_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hi = lane >> 5;
  // XCD-aware 1-D grid, as gemm_bf16x3_kernel: the column chunks of one row tile run back to back on one XCD
  const int chunks = (a.N + GH_COLS - 1) / GH_COLS;
  const int g = blockIdx.x >> 3, chunk = g % chunks, row_tile = 8 * (g / chunks) + (blockIdx.x & 7);
  if (row_tile * GH_ROWS >= a.M) return;  // (whole workgroup: the row tiles are padded to a multiple of 8)
  const int m = row_tile * GH_ROWS + wave * 32 + r;
  const int mc = m < a.M ? m : a.M - 1;
  const int nks = a.nks;
  const char* slots = a.blob + (size_t)chunk * nks * GH_SLOT_BYTES;
  const _Float16* xrow = a.x + (size_t)mc * a.K;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  // K is a multiple of 8: an 8-wide piece is inside the row or entirely outside.  A piece from outside is loaded at the row's first bytes
  // (no branch around a load) and replaced by zeros where it is consumed, a step later: a use right behind the load would wait for it there.
  auto xload = [&](int s) {
    XRowH v;
    const int k = GH_KSLOT * s + 16 * hi;
    v.a = *reinterpret_cast<const u32x4*>(xrow + (k < a.K ? k : 0));
    v.b = *reinterpret_cast<const u32x4*>(xrow + (k + 8 < a.K ? k + 8 : 0));
    return v;
  };
  // accumulator start: register 4q+e of block ob <- bias[128 chunk + 32 ob + 8 q + 4 half + e]
  f32x16 acc[4];
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n0 = chunk * GH_COLS + 4 * hi + 32 * ob + 8 * q;
      f32x4 b = {0.f, 0.f, 0.f, 0.f};
      if (a.bias && n0 < a.N) b = *reinterpret_cast<const f32x4*>(a.bias + n0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] = b[e];
    }

  // One step = one slot: full wait + barrier (slot s is in LDS for everybody, x piece s in this lane's registers; nobody reads slot s-1 any
  // more), the requests of slot s+1, the products of slot s.  The requests of a step have that step's MFMAs to land; the rest of a
  // memory round trip is hidden by the other wavefronts of the SIMD (4 at 116 registers), which is what gemm_bf16.hip's loop amounts to as
  // compiled: beside LDS DMA the compiler answers every use of an ordinary load's result with a full wait, counted waits or not.  The wait
  // is the builtin, which the compiler's own request counting sees: it adds none of its own behind the new requests.  Two register sets
  // take turns (xc is consumed, xn requested), so no loaded value is copied -- a copy is a use.
  auto step = [&](int s, XRowH& xc, XRowH& xn) {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0); expcnt / lgkmcnt: no wait
    __builtin_amdgcn_s_barrier();
    if (s + 1 < nks) {
      dma_slot(slots, s + 1, ring, wave, lane);
      xn = xload(s + 1);
    }
    const int k = GH_KSLOT * s + 16 * hi;
    const f16x8 xa = __builtin_bit_cast(f16x8, k < a.K ? xc.a : zero4), xb = __builtin_bit_cast(f16x8, k + 8 < a.K ? xc.b : zero4);
    const u32x4* s4 = reinterpret_cast<const u32x4*>(ring + (s & (GH_RING - 1)) * GH_SLOT_FLOATS) + lane;
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) {
      const f16x8 wa = __builtin_bit_cast(f16x8, s4[ob * 64]);
      const f16x8 wb = __builtin_bit_cast(f16x8, s4[(4 + ob) * 64]);
      acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa, xa, acc[ob], 0, 0, 0);
      acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wb, xb, acc[ob], 0, 0, 0);
    }
  };
  dma_slot(slots, 0, ring, wave, lane);
  XRowH xA = xload(0), xB = {zero4, zero4};
  for (int s = 0; s < nks; s += 2) {
    step(s, xA, xB);
    if (s + 1 < nks) step(s + 1, xB, xA);
  }

  // ---- epilogue: `tb` = this wavefront's 8 KiB of the ring (32 rows x 16 pieces of 16 bytes, piece index XOR-swizzled with the row so that
  // both the row-wise writes and the piece-wise reads are conflict free), half a tile (64 columns) at a time
  __builtin_amdgcn_s_barrier();  // every wavefront is done with the ring: it becomes the transposition buffer
  float* tb = ring + wave * 2048;
  const int m0 = row_tile * GH_ROWS + wave * 32, n_chunk = chunk * GH_COLS;
  const int rrow = lane >> 4, rpiece = lane & 15;  // read side: row 4 i + rrow, piece rpiece
  float sc = 0.f, bi = 0.f;
  if (STAR) sc = a.star[0], bi = a.star_bias[0];
  int events = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int obl = 0; obl < 2; ++obl)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ob = 2 * h + obl;
        const f32x4 v = {acc[ob][4 * q], acc[ob][4 * q + 1], acc[ob][4 * q + 2], acc[ob][4 * q + 3]};
        const int p = obl * 8 + 2 * q + hi;
        *reinterpret_cast<f32x4*>(tb + r * 64 + ((p ^ (r & 15)) << 2)) = v;
      }
    const int n0 = n_chunk + 64 * h + 4 * rpiece;
    if (n0 < a.N) {  // N a multiple of 8, n0 of 4: a piece is inside or outside
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {  // 16 rows at a time
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = 4 * (4 * ib + j) + rrow;
          v[j] = *reinterpret_cast<const f32x4*>(tb + row * 64 + ((rpiece ^ (row & 15)) << 2));
        }
        if (OUT16) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int mm = m0 + 4 * (4 * ib + j) + rrow;
            const f32x4 o = STAR ? star_relu4(v[j], sc, bi) : v[j];
            f16x4 h4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              h4[e] = (_Float16)o[e];
              events += (mm < a.M && f16_overflowed(v[j][e], h4[e])) ? 1 : 0;
            }
            if (mm < a.M) *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(a.y) + (size_t)mm * a.N + n0) = h4;
          }
        } else {
          if (a.res) {
            f32x4 rr[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int mm = m0 + 4 * (4 * ib + j) + rrow;
              rr[j] = *reinterpret_cast<const f32x4*>(a.res + (size_t)(mm < a.M ? mm : a.M - 1) * a.N + n0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (STAR ? star_relu4(v[j], sc, bi) : v[j]) + rr[j];
          } else if (STAR) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = star_relu4(v[j], sc, bi);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int mm = m0 + 4 * (4 * ib + j) + rrow;
            if (mm < a.M) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.y) + (size_t)mm * a.N + n0) = v[j];
          }
        }
      }
    }
  }
  if (OUT16 && events && a.overflow) atomicAdd(a.overflow, events);
}

// blob element (chunk, s, j, ob, lane, i) = fp16(w[128 chunk + 32 ob + (lane & 31)][32 s + 16 (lane >> 5) + 8 j + i]), zero outside the matrix
__global__ void linear_pack_f16_kernel(const float* __restrict__ w, int N, int K, int nks, _Float16* __restrict__ blob, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int i = idx & 7, lane = (idx >> 3) & 63, ob = (idx >> 9) & 3, j = (idx >> 11) & 1;
  const size_t slot = idx >> 12;
  const int s = slot % nks, chunk = slot / nks;
  const int n = 128 * chunk + 32 * ob + (lane & 31), k = GH_KSLOT * s + 16 * (lane >> 5) + 8 * j + i;
  blob[idx] = (_Float16)((n < N && k < K) ? w[(size_t)n * K + k] : 0.f);
}

unsigned gemm_f16_grid(int M, int N) {
  const int row_tiles = (M + GH_ROWS - 1) / GH_ROWS, chunks = (N + GH_COLS - 1) / GH_COLS;
  return (unsigned)(((row_tiles + 7) / 8) * 8 * chunks);
}

}  // namespace

extern "C" size_t nm_linear_blob_bytes_f16(int N, int K) {
  if (N <= 0 || K <= 0) return 0;
  return (size_t)((N + GH_COLS - 1) / GH_COLS) * ((K + GH_KSLOT - 1) / GH_KSLOT) * GH_SLOT_BYTES;
}

extern "C" int nm_linear_pack_f16(const float* w, int N, int K, void* blob, nmStream_t stream) {
  NM_CHECK_ARG(w && blob && N > 0 && K > 0);
  const int nks = (K + GH_KSLOT - 1) / GH_KSLOT;
  const size_t total = (size_t)((N + GH_COLS - 1) / GH_COLS) * nks * (GH_SLOT_BYTES / 2);
  linear_pack_f16_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, N, K, nks, (_Float16*)blob, total);
  return nm_launch_status();
}

extern "C" int nm_linear_f16(const void* x, const void* blob, const float* bias, const float* star_scale, const float* star_bias,
                             const float* residual, int M, int N, int K, int out_f16, void* y, int* overflow, nmStream_t stream) {
  NM_CHECK_ARG(x && blob && y && x != y && M > 0 && N > 0 && K > 0 && (out_f16 == 0 || out_f16 == 1));
  NM_CHECK_ARG((star_scale != nullptr) == (star_bias != nullptr) && !(out_f16 && residual));
  NM_CHECK_ARG(aligned16(x) && aligned16(blob) && aligned16(y) && aligned16(bias) && aligned16(residual));
  if (K % 8 != 0 || N % 8 != 0) return NM_ERR_UNSUPPORTED;  // 16-byte row pieces on the input side, whole 4-wide pieces on the output side
  GemmHArgs a{};
  a.x = (const _Float16*)x; a.blob = (const char*)blob; a.bias = bias; a.star = star_scale; a.star_bias = star_bias; a.res = residual;
  a.y = y; a.overflow = overflow; a.M = M; a.N = N; a.K = K; a.nks = (K + GH_KSLOT - 1) / GH_KSLOT;
  const unsigned grid = gemm_f16_grid(M, N);
  hipStream_t s = (hipStream_t)stream;
  if (out_f16 && star_scale) gemm_f16_kernel<true, true><<<grid, 256, 0, s>>>(a);
  else if (out_f16) gemm_f16_kernel<true, false><<<grid, 256, 0, s>>>(a);
  else if (star_scale) gemm_f16_kernel<false, true><<<grid, 256, 0, s>>>(a);
  else gemm_f16_kernel<false, false><<<grid, 256, 0, s>>>(a);
  return nm_launch_status();
}
