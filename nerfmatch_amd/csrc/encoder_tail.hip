// The part of a pre-norm encoder layer that follows the attention, as ONE kernel (round 3):
//
//     y = xh + FFN(LN2(xh + att . Wo^T)),   FFN(a) = W2 . gelu(W1 . a + b1) + b2
//
// reference: GenericEncoderLayer.forward_pre_norm, nerfmatch/modules/attention.py:229-241 (`out = x + out` with x the NORMALISED
// input, norm2, feedforward, second residual again onto the normalised input), MultiHeadAttention's bias-free proj_out :131-133,
// FeedForwardNetwork :136-154 (exact-erf GELU).  Unfused this is nm_linear_bf16x3 + nm_layernorm + 2 x nm_linear_bf16x3: four
// launches that move ten [rows, 256] fp32 tensors through HBM (0.42 ms at 153,600 rows); here three tensors move (att and xh
// in, y out) and the three 256 x 256 products are chained in registers:
//   * workgroup = 4 wavefronts x 32 rows, every wavefront owns its rows for the whole chain (all 256 features: 8 blocks of 32,
//     128 accumulator registers); arithmetic = the split-bf16 products of gemm_bf16.hip (w_hi x_hi + w_hi x_lo + w_lo x_hi);
//   * the accumulator layout (lane = row, register r of block ob <-> feature 32 ob + (r & 3) + 8 (r >> 2) + 4 half) makes 8
//     consecutive registers the 8 K-slots of one MFMA step of the NEXT product if that product's weight slots are packed in the
//     matching K order (nm_linear_pack_perm_bf16x3) -- the trick of the fused NeRF kernel: bias / LayerNorm / GELU / hi-lo
//     re-packing are lane local, no LDS, no shuffles except the two xor-32 row reductions of the LayerNorm;
//   * weights: 48 K-steps of 16 KiB (both 128-column chunks of a product) streamed by LDS DMA through a 4-deep ring, two K-steps
//     ahead, ONE continuous stream across the three products so that the hand-overs do not drain it;
//   * y leaves through the LDS-transposed, coalesced epilogue of gemm_bf16.hip; the residual row is read ONCE, in the
//     accumulator layout (prefetched behind the MFMAs of the first product, kept in registers for the last one).
// One wavefront per SIMD (320 registers): the hand-overs are exposed; what it buys is the HBM traffic.
#include "encoder_tail_chain.h"

namespace {

struct TailArgs {
  const float* att;
  const float* xh;
  const char* blob[3];  // Wo (standard K order), W1, W2 (accumulator K order): [chunk][ks] slots of 8 KiB
  const float* gamma;
  const float* beta;
  const float* b1;
  const float* b2;
  float* y;
  int R;
  float eps;
};

__global__ void __launch_bounds__(256, 1) encoder_tail_kernel(TailArgs a) {
  // ONE __shared__ object on purpose.  With two (ring, vectors) the LDS lowering attaches alias scopes, the compiler's waitcnt pass starts to
  // track the weight stream's LDS-DMA as "stores into `ring`" and puts an s_waitcnt vmcnt(0) in front of every ds_read of `ring` that
  // follows a DMA request -- i.e. right behind the request of step g + 3, every K-step, in the middle of the MFMA stream (26 of them in the
  // disassembly; a tile ran at 2.7 k cycles per K-step against 768 of matrix time).  The ring's own counted waits (wait_vm / allow_of) are
  // the synchronisation; tests/test_safe_wait_gpu.py checks them against the vmcnt(0) build.
  __shared__ __attribute__((aligned(16))) float lds[ET_RING * ET_STEP_FLOATS + 4 * ET_D];
  float* const ring = lds;                                   // 64 KiB
  float* const sm_vec = lds + ET_RING * ET_STEP_FLOATS;      // gamma, beta, b1, b2
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hi = lane >> 5;
  const int m0 = blockIdx.x * ET_ROWS + wave * 32;
  const int m = m0 + r, mc = m < a.R ? m : a.R - 1;
  sm_vec[tid] = a.gamma[tid];
  sm_vec[ET_D + tid] = a.beta[tid];
  sm_vec[2 * ET_D + tid] = a.b1[tid];
  sm_vec[3 * ET_D + tid] = a.b2[tid];
  // ---- product 0: a = xh + att . Wo^T; rows of att go global -> registers two K-steps ahead, split on the fly
  const float* xp = a.att + (size_t)mc * ET_D + 8 * hi;
  struct XRow {
    f32x4 p, q;
  };
  auto xload = [&](int ks) {
    XRow v;
    v.p = *reinterpret_cast<const f32x4*>(xp + 16 * ks);
    v.q = *reinterpret_cast<const f32x4*>(xp + 16 * ks + 4);
    return v;
  };
  XRow xr[ET_NKS];  // (unrolled: five are live at a time)
  xr[0] = xload(0);
  xr[1] = xload(1);
  xr[2] = xload(2);
  xr[3] = xload(3);
  // the residual xh in the accumulator layout: 32 pieces of 16 bytes per lane, requested during the second half of product 0
  // and kept until product 2 starts from b2 + xh (the row is not read a second time)
  f32x4 res[32];
  const float* rp = a.xh + (size_t)mc * ET_D + 4 * hi;
#pragma unroll
  for (int g0 = 0; g0 < ET_AHEAD; ++g0) dma_step(a.blob, g0, ring, wave, lane);
  f32x16 acc[8];
  zero_acc(acc);
  OpsC c0, c1;
  wait_vm(4 * (ET_AHEAD - 1));  // step 0 landed (steps 1 .. ET_AHEAD - 1 in flight)
  __builtin_amdgcn_s_barrier();
  read_chunk(c0, ring, lane, 0);
#pragma unroll
  for (int ks = 0; ks < ET_NKS; ++ks) {
    bf16x8 xh, xl;
    {
      const XRow& x0 = xr[ks];
      const float v8[8] = {x0.p[0], x0.p[1], x0.p[2], x0.p[3], x0.q[0], x0.q[1], x0.q[2], x0.q[3]};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const __bf16 h = (__bf16)v8[i];
        xh[i] = h;
        xl[i] = (__bf16)(v8[i] - (float)h);
      }
    }
    kstep<0>(a.blob, ks, ring, wave, lane, acc, c0, c1, xh, xl, [&]() {
      if (ks + 4 < ET_NKS) xr[ks + 4] = xload(ks + 4);
      if (ks >= 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = 4 * (ks - 8) + j;  // piece i = (block i / 4, quad i % 4)
          res[i] = *reinterpret_cast<const f32x4*>(rp + 32 * (i >> 2) + 8 * (i & 3));
        }
      }
    });
  }
  // residual in the accumulator layout, LayerNorm over the row (the lane pair r, r + 32 owns it), re-pack
  Unit un[16];
  {
    float s = 0.f;
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 rr = res[4 * ob + q];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[ob][4 * q + e] += rr[e];
          s += acc[ob][4 * q + e];
        }
      }
    s += nm_shfl_xor32(s);
    const float mean = s * (1.0f / ET_D);
    float vs = 0.f;
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float d = acc[ob][i] - mean;
        acc[ob][i] = d;
        vs = NM_FMA(d, d, vs);
      }
    vs += nm_shfl_xor32(vs);
    const float rstd = 1.0f / sqrtf(vs * (1.0f / ET_D) + a.eps);
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(sm_vec + 32 * ob + 8 * q + 4 * hi);
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(sm_vec + ET_D + 32 * ob + 8 * q + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] = (acc[ob][4 * q + e] * rstd) * g4[e] + b4[e];
      }
    repack(acc, un);
  }
  // ---- product 1: h = gelu(W1 . a_n + b1)
  zero_acc(acc);
#pragma unroll
  for (int ks = 0; ks < ET_NKS; ++ks)
    kstep<0>(a.blob, ET_NKS + ks, ring, wave, lane, acc, c0, c1, __builtin_bit_cast(bf16x8, un[ks].h), __builtin_bit_cast(bf16x8, un[ks].l), [] {});
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(sm_vec + 2 * ET_D + 32 * ob + 8 * q + 4 * hi);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] = gelu_erf(acc[ob][4 * q + e] + b4[e]);
    }
  repack(acc, un);
  // ---- product 2: y = xh + W2 . h + b2   (b2 + xh = the accumulators' starting value)
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(sm_vec + 3 * ET_D + 32 * ob + 8 * q + 4 * hi);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] = b4[e] + res[4 * ob + q][e];
    }
#pragma unroll
  for (int ks = 0; ks < ET_NKS; ++ks)
    kstep<0>(a.blob, 2 * ET_NKS + ks, ring, wave, lane, acc, c0, c1, __builtin_bit_cast(bf16x8, un[ks].h), __builtin_bit_cast(bf16x8, un[ks].l), [] {});
  __builtin_amdgcn_s_barrier();  // the ring becomes the transposition buffer: 16 KiB per wavefront
  // coalesced epilogue (cf. epilogue_coalesced in gemm_bf16.hip): 64 columns at a time through this wavefront's LDS region
  // (32 rows x 16 pieces of 16 bytes, piece index XOR-swizzled with the row), then 256-byte row segments + residual
  float* tb = ring + wave * 4096;
  const int rrow = lane >> 4, rpiece = lane & 15;
#pragma unroll
  for (int hq = 0; hq < 4; ++hq) {  // 64-column quarter: blocks 2 hq, 2 hq + 1
#pragma unroll
    for (int obl = 0; obl < 2; ++obl)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ob = 2 * hq + obl;
        const f32x4 v = {acc[ob][4 * q], acc[ob][4 * q + 1], acc[ob][4 * q + 2], acc[ob][4 * q + 3]};
        const int p = obl * 8 + 2 * q + hi;
        *reinterpret_cast<f32x4*>(tb + (hq & 1) * 2048 + r * 64 + ((p ^ (r & 15)) << 2)) = v;
      }
    const int n0 = 64 * hq + 4 * rpiece;
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) {
      f32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 4 * (4 * ib + j) + rrow;
        v[j] = *reinterpret_cast<const f32x4*>(tb + (hq & 1) * 2048 + row * 64 + ((rpiece ^ (row & 15)) << 2));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int mm = m0 + 4 * (4 * ib + j) + rrow;
        if (mm < a.R) *reinterpret_cast<f32x4*>(a.y + (size_t)mm * ET_D + n0) = v[j];
      }
    }
  }
}

// Argument block of encoder_tail_save_kernel.  The kernel was written against the block it shared with encoder_tail_bwd_kernel, and the kernarg
// offsets are part of its code: the fields keep that order, the backward kernel's own ones are unused slots here.
struct SaveArgs {
  const float *dy_, *a_pre_, *u_pre_;  // (unused: encoder_tail_bwd_kernel's inputs)
  const char* blob[3];                 // Wo (standard K order), W1, W2 (accumulator K order): [chunk][ks] slots of 8 KiB
  const float* gamma;
  float *d_att_, *d_xh_;               // (unused: encoder_tail_bwd_kernel's outputs)
  int R;
  float eps;
  const float *att, *xh, *beta, *b1, *b2;
  float *y, *a_out, *u_out;            // a = xh + att . Wo^T (the LayerNorm's input), u = W1 . LN2(a) + b1 (the GELU's input)
};

// The FORWARD of the tail for the frozen-parameter passes, as one launch that also KEEPS what the backward kernel (encoder_tail_bwd.hip) needs:
// encoder_tail_kernel above (same arithmetic, same order) with a (the LayerNorm's input) and u (the GELU's input) leaving mid-chain through a
// transposition buffer of its own (the ring keeps streaming).  Five launches before (GEMM + residual, LayerNorm, GEMM, GELU, GEMM + residual).
__global__ void __launch_bounds__(256, 1) encoder_tail_save_kernel(SaveArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[ET_RING * ET_STEP_FLOATS + 4 * ET_D + 4 * 4096];
  float* const ring = lds;
  float* const sm_vec = lds + ET_RING * ET_STEP_FLOATS;  // gamma, beta, b1, b2
  float* const tbuf = sm_vec + 4 * ET_D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hi = lane >> 5;
  const int m0 = blockIdx.x * ET_ROWS + wave * 32;
  const int m = m0 + r, mc = m < a.R ? m : a.R - 1;
  sm_vec[tid] = a.gamma[tid];
  sm_vec[ET_D + tid] = a.beta[tid];
  sm_vec[2 * ET_D + tid] = a.b1[tid];
  sm_vec[3 * ET_D + tid] = a.b2[tid];
  const float* xp = a.att + (size_t)mc * ET_D + 8 * hi;
  struct XRow {
    f32x4 p, q;
  };
  auto xload = [&](int ks) {
    XRow v;
    v.p = *reinterpret_cast<const f32x4*>(xp + 16 * ks);
    v.q = *reinterpret_cast<const f32x4*>(xp + 16 * ks + 4);
    return v;
  };
  XRow xr[ET_NKS];
  xr[0] = xload(0);
  xr[1] = xload(1);
  xr[2] = xload(2);
  xr[3] = xload(3);
  f32x4 res[32];
  const float* rp = a.xh + (size_t)mc * ET_D + 4 * hi;
#pragma unroll
  for (int g0 = 0; g0 < ET_AHEAD; ++g0) dma_step(a.blob, g0, ring, wave, lane);
  f32x16 acc[8];
  zero_acc(acc);
  OpsC c0, c1;
  wait_vm(4 * (ET_AHEAD - 1));
  __builtin_amdgcn_s_barrier();
  read_chunk(c0, ring, lane, 0);
#pragma unroll
  for (int ks = 0; ks < ET_NKS; ++ks) {
    bf16x8 xh, xl;
    {
      const XRow& x0 = xr[ks];
      const float v8[8] = {x0.p[0], x0.p[1], x0.p[2], x0.p[3], x0.q[0], x0.q[1], x0.q[2], x0.q[3]};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const __bf16 h = (__bf16)v8[i];
        xh[i] = h;
        xl[i] = (__bf16)(v8[i] - (float)h);
      }
    }
    kstep<1>(a.blob, ks, ring, wave, lane, acc, c0, c1, xh, xl, [&]() {
      if (ks + 4 < ET_NKS) xr[ks + 4] = xload(ks + 4);
      if (ks >= 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = 4 * (ks - 8) + j;
          res[i] = *reinterpret_cast<const f32x4*>(rp + 32 * (i >> 2) + 8 * (i & 3));
        }
      }
    });
  }
  float* tb = tbuf + wave * 4096;
  const int rrow = lane >> 4, rpiece = lane & 15;
  auto store_rows = [&](float* __restrict__ dst) {
#pragma unroll
    for (int hq = 0; hq < 4; ++hq) {
#pragma unroll
      for (int obl = 0; obl < 2; ++obl)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ob = 2 * hq + obl;
          const f32x4 v = {acc[ob][4 * q], acc[ob][4 * q + 1], acc[ob][4 * q + 2], acc[ob][4 * q + 3]};
          const int p = obl * 8 + 2 * q + hi;
          *reinterpret_cast<f32x4*>(tb + (hq & 1) * 2048 + r * 64 + ((p ^ (r & 15)) << 2)) = v;
        }
      const int n0 = 64 * hq + 4 * rpiece;
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = 4 * (4 * ib + j) + rrow;
          v[j] = *reinterpret_cast<const f32x4*>(tb + (hq & 1) * 2048 + row * 64 + ((rpiece ^ (row & 15)) << 2));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int mm = m0 + 4 * (4 * ib + j) + rrow;
          if (mm < a.R) *reinterpret_cast<f32x4*>(dst + (size_t)mm * ET_D + n0) = v[j];
        }
      }
    }
  };
  Unit un[16];
  {
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 rr = res[4 * ob + q];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] += rr[e];
      }
    store_rows(a.a_out);  // a = xh + att . Wo^T leaves here
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (see encoder_tail_bwd_kernel: the counted waits that follow stay on the safe side)
    float s = 0.f;
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int i = 0; i < 16; ++i) s += acc[ob][i];
    s += nm_shfl_xor32(s);
    const float mean = s * (1.0f / ET_D);
    float vs = 0.f;
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float d = acc[ob][i] - mean;
        acc[ob][i] = d;
        vs = NM_FMA(d, d, vs);
      }
    vs += nm_shfl_xor32(vs);
    const float rstd = 1.0f / sqrtf(vs * (1.0f / ET_D) + a.eps);
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(sm_vec + 32 * ob + 8 * q + 4 * hi);
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(sm_vec + ET_D + 32 * ob + 8 * q + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] = (acc[ob][4 * q + e] * rstd) * g4[e] + b4[e];
      }
    repack(acc, un);
  }
  zero_acc(acc);
  // (the residual row is read a SECOND time during the second half of this product, for product 2's starting value: kept in registers across
  // the two mid-chain stores it spilled 58 of them to scratch -- encoder_tail_kernel has no store before its end)
#pragma unroll
  for (int ks = 0; ks < ET_NKS; ++ks)
    kstep<1>(a.blob, ET_NKS + ks, ring, wave, lane, acc, c0, c1, __builtin_bit_cast(bf16x8, un[ks].h), __builtin_bit_cast(bf16x8, un[ks].l), [&]() {
      if (ks >= 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = 4 * (ks - 8) + j;
          res[i] = *reinterpret_cast<const f32x4*>(rp + 32 * (i >> 2) + 8 * (i & 3));
        }
      }
    });
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(sm_vec + 2 * ET_D + 32 * ob + 8 * q + 4 * hi);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] += b4[e];
    }
  store_rows(a.u_out);  // u = W1 . LN2(a) + b1 leaves here
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[ob][i] = gelu_erf(acc[ob][i]);
  repack(acc, un);
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(sm_vec + 3 * ET_D + 32 * ob + 8 * q + 4 * hi);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] = b4[e] + res[4 * ob + q][e];
    }
#pragma unroll
  for (int ks = 0; ks < ET_NKS; ++ks)
    kstep<1>(a.blob, 2 * ET_NKS + ks, ring, wave, lane, acc, c0, c1, __builtin_bit_cast(bf16x8, un[ks].h), __builtin_bit_cast(bf16x8, un[ks].l), [] {});
  store_rows(a.y);
}

// blob element (chunk, ks, ob, hl, lane, i) = split(w[128 chunk + 32 ob + (lane & 31)][32 (ks >> 1) + nrow(8 (ks & 1) + i, lane >> 5)]):
// the K order in which the accumulator registers of the PREVIOUS product hold its output features
__global__ void linear_pack_perm_kernel(const float* __restrict__ w, int N, int K, int nks, unsigned short* __restrict__ blob, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int i = idx & 7, lane = (idx >> 3) & 63, ob = (idx >> 9) & 3;
  const size_t slot = idx >> 11;
  const int ks = slot % nks, chunk = slot / nks;
  const int n = 128 * chunk + 32 * ob + (lane & 31), k = 32 * (ks >> 1) + nrow(8 * (ks & 1) + i, lane >> 5);
  const float v = (n < N && k < K) ? w[(size_t)n * K + k] : 0.f;
  const __bf16 h = (__bf16)v;
  const __bf16 l = (__bf16)(v - (float)h);
  unsigned short* s = blob + slot * (ET_SLOT_BYTES / 2);
  s[((ob * 2 + 0) * 64 + lane) * 8 + i] = __builtin_bit_cast(unsigned short, h);
  s[((ob * 2 + 1) * 64 + lane) * 8 + i] = __builtin_bit_cast(unsigned short, l);
}

}  // namespace

extern "C" int nm_linear_pack_perm_bf16x3(const float* w, int N, int K, void* blob, nmStream_t stream) {
  NM_CHECK_ARG(w && blob && N > 0 && K > 0);
  if (K % 32 != 0) return NM_ERR_UNSUPPORTED;
  const int nks = K / 16;
  const size_t total = (size_t)((N + 127) / 128) * nks * (ET_SLOT_BYTES / 4);
  linear_pack_perm_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, N, K, nks, (unsigned short*)blob, total);
  return nm_launch_status();
}

extern "C" int nm_encoder_tail_bf16x3(const float* att, const float* xh, const void* wo_blob, const void* w1_perm_blob, const void* w2_perm_blob,
                                      const float* gamma2, const float* beta2, const float* b1, const float* b2, int rows, int dim, float eps,
                                      float* y, nmStream_t stream) {
  NM_CHECK_ARG(att && xh && wo_blob && w1_perm_blob && w2_perm_blob && gamma2 && beta2 && b1 && b2 && y && rows > 0);
  if (dim != ET_D) return NM_ERR_UNSUPPORTED;
  TailArgs a{};
  a.att = att; a.xh = xh; a.blob[0] = (const char*)wo_blob; a.blob[1] = (const char*)w1_perm_blob; a.blob[2] = (const char*)w2_perm_blob;
  a.gamma = gamma2; a.beta = beta2; a.b1 = b1; a.b2 = b2; a.y = y; a.R = rows; a.eps = eps;
  encoder_tail_kernel<<<(rows + ET_ROWS - 1) / ET_ROWS, 256, 0, (hipStream_t)stream>>>(a);
  return nm_launch_status();
}

extern "C" int nm_encoder_tail_save_bf16x3(const float* att, const float* xh, const void* wo_blob, const void* w1_perm_blob, const void* w2_perm_blob,
                                           const float* gamma2, const float* beta2, const float* b1, const float* b2, int rows, int dim, float eps,
                                           float* y, float* a_out, float* u_out, nmStream_t stream) {
  NM_CHECK_ARG(att && xh && wo_blob && w1_perm_blob && w2_perm_blob && gamma2 && beta2 && b1 && b2 && y && a_out && u_out && rows > 0);
  if (dim != ET_D) return NM_ERR_UNSUPPORTED;
  SaveArgs a{};
  a.att = att; a.xh = xh; a.blob[0] = (const char*)wo_blob; a.blob[1] = (const char*)w1_perm_blob; a.blob[2] = (const char*)w2_perm_blob;
  a.gamma = gamma2; a.beta = beta2; a.b1 = b1; a.b2 = b2; a.y = y; a.a_out = a_out; a.u_out = u_out; a.R = rows; a.eps = eps;
  encoder_tail_save_kernel<<<(rows + ET_ROWS - 1) / ET_ROWS, 256, 0, (hipStream_t)stream>>>(a);
  return nm_launch_status();
}
