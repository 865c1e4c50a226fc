// The skeleton of the encoder-tail kernels (encoder_tail.hip: forward, forward that keeps its intermediates; encoder_tail_bwd.hip:
// backward): a chain of three 256 x 256 split-bf16 products in which every wavefront owns 32 rows from end to end.  Constants, the
// 48-K-step weight stream through the LDS ring with its counted waits, and the software-pipelined K-step.
// The helpers take what they use (the three weight blobs), not a kernel's argument block: each kernel has its own.
// NOT here: the coalesced store of a finished tile.  Each kernel keeps its own copy (inline in encoder_tail_kernel, a `store_rows` lambda in
// the other two): as one device function, forced inline or not, it changes the instruction schedule of all three kernels.
#pragma once
#include "bf16x3.h"

constexpr int ET_ROWS = 128;
constexpr int ET_D = 256;                 // model dim = inner dim = FFN hidden dim
constexpr int ET_NKS = ET_D / 16;         // K-steps per product
constexpr int ET_SLOT_BYTES = 8192;       // one K-step of one 128-column chunk (linear blob format)
constexpr int ET_STEP_FLOATS = 2 * ET_SLOT_BYTES / 4;  // both chunks of a K-step: 16 KiB
// K-steps of the weight stream in flight ahead of the matrix work.  Round 5 measured 6 (ring of 8, 128 KiB) against 3: 40.6 vs 38.2 us at 4800 rows,
// 276 vs 255 us at 153,600 -- the kernel already uses all 512 registers and the deeper bookkeeping spills 49 of them to scratch; the stream is not what a
// K-step waits for (profiles/r5_ab_encoder_tail_ahead.log).  The wait counts below are derived from ET_AHEAD for any depth.
constexpr int ET_AHEAD = 3;
constexpr int ET_RING = ET_AHEAD > 3 ? 8 : 4;    // ring positions (a power of two > ET_AHEAD)

// the weight stream: blob[g / 16] holds product g / 16's [chunk][ks] slots of 8 KiB (product 0 in standard K order, 1 and 2 in accumulator K order)
typedef const char* const (&TailBlobs)[3];

// K-step g of the 48-step weight stream (product g / 16): both chunks, 4 x 1 KiB pieces per wavefront
__device__ __forceinline__ void dma_step(TailBlobs blobs, int g, float* ring, int wave, int lane) {
  const char* blob = blobs[g >> 4];
  const int ks = g & 15;
  float* dst0 = ring + (g & (ET_RING - 1)) * ET_STEP_FLOATS + wave * 512;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const char* base = blob + ((size_t)c * ET_NKS + ks) * ET_SLOT_BYTES + wave * 2048 + lane * 16;
    const auto* src = (const __attribute__((address_space(1))) void*)base;
    auto* dst = (__attribute__((address_space(3))) void*)(dst0 + c * (ET_SLOT_BYTES / 4));
    __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds(src, dst, 16, 1024, 0);
  }
}

// A operands of one 128-column chunk of a K-step: 4 blocks x (hi, lo) = 8 x 16 bytes per lane
struct OpsC {
  u32x4 h[4], l[4];
};
__device__ __forceinline__ void read_chunk(OpsC& o, const float* step, int lane, int c) {
  const u32x4* s4 = reinterpret_cast<const u32x4*>(step) + lane;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    o.h[b] = s4[(c * 8 + b * 2 + 0) * 64];
    o.l[b] = s4[(c * 8 + b * 2 + 1) * 64];
  }
}
// 12 MFMAs of one chunk (accumulators acc[4c .. 4c+3]; an accumulator is touched again after three others), one `item(j)` of
// other traffic issued right behind MFMA j: with ONE wavefront per SIMD and in-order issue nothing overlaps the matrix pipe
// unless it is interleaved with it (a first version that issued a K-step's DMA pieces and operand reads in front of its 24 MFMAs
// ran at ~1300 cycles per K-step against 768 of matrix time).
template <class Items>
__device__ __forceinline__ void half_step(f32x16 (&acc)[8], int c, const OpsC& o, const bf16x8& xh, const bf16x8& xl, Items items) {
#define NM_SB __builtin_amdgcn_sched_barrier(0)
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    acc[4 * c + b] = MFMA_BF16(__builtin_bit_cast(bf16x8, o.h[b]), xh, acc[4 * c + b]); NM_SB;
    items(b); NM_SB;
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    acc[4 * c + b] = MFMA_BF16(__builtin_bit_cast(bf16x8, o.h[b]), xl, acc[4 * c + b]); NM_SB;
    items(4 + b); NM_SB;
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    acc[4 * c + b] = MFMA_BF16(__builtin_bit_cast(bf16x8, o.l[b]), xh, acc[4 * c + b]); NM_SB;
    items(8 + b); NM_SB;
  }
#undef NM_SB
}

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[8]) {
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[ob][i] = 0.f;
}

// Ring protocol, one K-step AHEAD of the matrix work: while the MFMAs of step g run on operands already in registers, step
// g + 1's pieces have landed (at most allow(g) younger VMEM operations remain in flight), one barrier, step g + 3 is requested
// into the position of step g - 1 (everybody consumed it an iteration ago), step g + 1's operands go into the other buffer.
// Issue order per iteration: [wait] [barrier] [DMA g+3: 4 ops] [operand reads g+1] [att row pieces of step g+2: 2 ops, product 0
// only]; prologue: rows 0, 1, DMA 0, 1, 2.  Counting the operations issued after DMA g+1 gives:
// VMEM operations a K-step issues behind its mid-step wait, in this order: DMA of step g + 3 (4 pieces), input row pieces of step
// g + 4 (2, product 0), tile pieces (4 per step: the 32 pieces of a [32, 256] row tile in accumulator layout)
__device__ __forceinline__ constexpr int n_dma(int g) { return g + ET_AHEAD < 3 * ET_NKS ? 4 : 0; }
__device__ __forceinline__ constexpr int n_row(int g) { return g + 4 < ET_NKS ? 2 : 0; }
// SCHED 0: one tile, during the second half of product 0 (encoder_tail_kernel: the residual xh).  SCHED 1: a second one during the second
// half of product 1 (encoder_tail_bwd_kernel: the pre-GELU tile, then the pre-LayerNorm tile; encoder_tail_save_kernel: the residual, twice)
template <int SCHED>
__device__ __forceinline__ constexpr int n_res(int g) { return ((g >= 8 && g < ET_NKS) || (SCHED == 1 && g >= ET_NKS + 8 && g < 2 * ET_NKS)) ? 4 : 0; }
// operations younger than the DMA of step g + 1 at the mid-step wait of step g (prologue: rows 0..3, DMA 0, 1, 2)
template <int SCHED>
__device__ __forceinline__ constexpr int allow_of(int g) {
  // the DMA of step g + 1 was issued in the prologue (g + 1 < ET_AHEAD: younger = the prologue's later DMAs + everything the loop issued so
  // far) or behind the wait of step g + 1 - ET_AHEAD (younger = that step's row / tile pieces + everything of the steps since)
  int n = 0;
  if (g + 1 < ET_AHEAD) {
    n = (ET_AHEAD - 1 - (g + 1)) * 4;
    for (int t = 0; t < g; ++t) n += n_dma(t) + n_row(t) + n_res<SCHED>(t);
  } else {
    const int t0 = g + 1 - ET_AHEAD;
    n = n_row(t0) + n_res<SCHED>(t0);
    for (int t = t0 + 1; t < g; ++t) n += n_dma(t) + n_row(t) + n_res<SCHED>(t);
  }
  return n;
}
template <int N>
__device__ __forceinline__ void wait_vm_n() {
#ifdef NM_SAFE_WAIT
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (checker build: every counted wait becomes a full wait, see common.h)
#else
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#endif
}
__device__ __forceinline__ void wait_vm(int allow) {
  switch (allow) {  // (g is a compile-time constant wherever this is called: the switch folds; every count is even)
#define NM_CASE(n) case n: wait_vm_n<n>(); break;
    NM_CASE(0) NM_CASE(2) NM_CASE(4) NM_CASE(6) NM_CASE(8) NM_CASE(10) NM_CASE(12) NM_CASE(14) NM_CASE(16) NM_CASE(18) NM_CASE(20) NM_CASE(22)
    NM_CASE(24) NM_CASE(26) NM_CASE(28) NM_CASE(30) NM_CASE(32) NM_CASE(34) NM_CASE(36) NM_CASE(38) NM_CASE(40) NM_CASE(42) NM_CASE(44) NM_CASE(46)
    NM_CASE(48) NM_CASE(50) NM_CASE(52) NM_CASE(54) NM_CASE(56) NM_CASE(58) NM_CASE(60) NM_CASE(62)
#undef NM_CASE
    default: wait_vm_n<0>(); break;  // (conservative)
  }
}

// K-step g of the 48-step stream, software pipelined over its two chunks ("consume first", as in nerf_split_chain.h):
//   chunk 0 MFMAs (operands c0, fetched during the previous step)  |  behind them: the 8 operand reads of chunk 1 of THIS step
//   wait: step g + 1 landed; barrier (=> for everybody; and everybody is past step g - 1)
//   chunk 1 MFMAs  |  behind them: the 4 DMA pieces of step g + 3 (ring position of step g - 1), the 8 operand reads of chunk 0
//   of step g + 1, and `tail()` (product 0: the input row pieces of step g + 2 -- issued after the DMA pieces, the order allow_of counts)
template <int SCHED, class Tail>
__device__ __forceinline__ void kstep(TailBlobs blobs, int g, float* ring, int wave, int lane, f32x16 (&acc)[8], OpsC& c0, OpsC& c1,
                                      const bf16x8& xh, const bf16x8& xl, Tail tail) {
  const u32x4* cur = reinterpret_cast<const u32x4*>(ring + (g & (ET_RING - 1)) * ET_STEP_FLOATS) + lane;
  half_step(acc, 0, c0, xh, xl, [&](int j) {
    if (j < 8) {
      const int b = j >> 1;
      if (j & 1) c1.l[b] = cur[(8 + b * 2 + 1) * 64];
      else c1.h[b] = cur[(8 + b * 2 + 0) * 64];
    }
  });
  const bool more = g + 1 < 3 * ET_NKS;
  if (more) {
    wait_vm(allow_of<SCHED>(g));
    __builtin_amdgcn_s_barrier();
  }
  const int q = g + ET_AHEAD;
  const bool dma = q < 3 * ET_NKS;
  const char* src0 = nullptr;
  float* dst = nullptr;
  if (dma) {
    src0 = blobs[q >> 4] + (size_t)(q & 15) * ET_SLOT_BYTES + wave * 2048 + lane * 16;
    dst = ring + (q & (ET_RING - 1)) * ET_STEP_FLOATS + wave * 512;
  }
  const u32x4* nxt = reinterpret_cast<const u32x4*>(ring + ((g + 1) & (ET_RING - 1)) * ET_STEP_FLOATS) + lane;
  half_step(acc, 1, c1, xh, xl, [&](int j) {
    if (j < 4) {
      if (dma) {
        const auto* src = (const __attribute__((address_space(1))) void*)(src0 + (size_t)(j >> 1) * ET_NKS * ET_SLOT_BYTES);
        auto* d = (__attribute__((address_space(3))) void*)(dst + (j >> 1) * (ET_SLOT_BYTES / 4));
        if (j & 1) __builtin_amdgcn_global_load_lds(src, d, 16, 1024, 0);
        else __builtin_amdgcn_global_load_lds(src, d, 16, 0, 0);
      }
    } else if (more) {
      const int b = (j - 4) >> 1;
      if ((j - 4) & 1) c0.l[b] = nxt[(b * 2 + 1) * 64];
      else c0.h[b] = nxt[(b * 2 + 0) * 64];
    }
  });
  tail();
  __builtin_amdgcn_sched_barrier(0);
}
