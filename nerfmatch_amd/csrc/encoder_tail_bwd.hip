// Backward of the encoder tail for FROZEN parameters, as ONE kernel (round 6) -- the mirror image of encoder_tail.hip:
//
//     forward:  a = xh + att . Wo^T;   u = W1 . LN2(a) + b1;   y = xh + W2 . gelu(u) + b2
//     backward: g1 = dy . W2;  du = g1 o gelu'(u);  g2 = du . W1;  d_a = LN2'(a; g2);  d_xh = dy + d_a;  d_att = d_a . Wo
//
// (reference: torch autograd through GenericEncoderLayer.forward_pre_norm, nerfmatch/modules/attention.py:229-241, as the iNeRF refinement's
// matching term runs it with the matcher's parameters frozen, nerfmatch_evaluator.py:429-441: input gradients only, no dW.)  Unfused this is
// three GEMM launches, nm_gelu_bwd, nm_layernorm_bwd and two elementwise adds per layer.  Same skeleton as the forward kernel (encoder_tail_chain.h): workgroup = 4
// wavefronts x 32 rows, every wavefront owns its rows through the chain of three 256 x 256 split-bf16 products, the accumulator layout of one
// product is the K order of the next (weights of products 1 and 2 packed with nm_linear_pack_perm_bf16x3 from the TRANSPOSED matrices), one
// 48-K-step weight stream through the 4-deep LDS ring.  What is new: two row tiles arrive in the accumulator layout during the second halves
// of products 0 and 1 (u for GELU', a for the LayerNorm backward: its statistics are recomputed, four xor-32 row reductions), d_xh leaves in
// the MIDDLE of the chain through an LDS transposition buffer of its own (the ring keeps streaming product 2's weights) with dy re-read in the
// coalesced store layout, d_att leaves at the end through the same buffer.
#include "encoder_tail_chain.h"

namespace {

struct TailArgs {
  const float* dy;      // gradient of the tail's output y [R, 256]
  const float* a_pre;   // a = xh + att . Wo^T, the input of LayerNorm 2 (saved by the forward pass)
  const float* u_pre;   // u = W1 . LN2(a) + b1, the input of the GELU (saved by the forward pass)
  const char* blob[3];  // W2^T (standard K order), W1^T, Wo^T (accumulator K order): [chunk][ks] slots of 8 KiB
  const float* gamma;
  float* d_att;
  float* d_xh;
  int R;
  float eps;
  // (unused slots: this block used to serve encoder_tail_save_kernel as well -- now SaveArgs in encoder_tail.hip; the kernarg size is part of the code)
  const float *att_, *xh_, *beta_, *b1_, *b2_;
  float *y_, *a_out_, *u_out_;
};

// d/dv of the exact-erf GELU: Phi(v) + v phi(v), erf by Abramowitz & Stegun 7.1.26 as in gelu_erf (bf16x3.h) (the exponential it needs IS
// exp(-v^2 / 2), the Gaussian of the second term)
__device__ __forceinline__ float gelu_grad(float v) {
  const float x = fabsf(v) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(NM_FMA(0.3275911f, x, 1.0f));
  float p = NM_FMA(1.061405429f, t, -1.453152027f);
  p = NM_FMA(p, t, 1.421413741f);
  p = NM_FMA(p, t, -0.284496736f);
  p = NM_FMA(p, t, 0.254829592f);
  const float ex = __builtin_amdgcn_exp2f(-(x * x) * 1.44269504088896340736f);  // exp(-v^2 / 2)
  const float e = 1.0f - (p * t) * ex;
  return NM_FMA(v * 0.39894228040143267794f, ex, 0.5f * (1.0f + copysignf(e, v)));
}

__global__ void __launch_bounds__(256, 1) encoder_tail_bwd_kernel(TailArgs a) {
  // (ONE __shared__ object: see encoder_tail_kernel, encoder_tail.hip)  ring 64 KiB | gamma 1 KiB | transposition buffer 4 x 16 KiB
  __shared__ __attribute__((aligned(16))) float lds[ET_RING * ET_STEP_FLOATS + ET_D + 4 * 4096];
  float* const ring = lds;
  float* const sm_gamma = lds + ET_RING * ET_STEP_FLOATS;
  float* const tbuf = sm_gamma + ET_D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hi = lane >> 5;
  const int m0 = blockIdx.x * ET_ROWS + wave * 32;
  const int m = m0 + r, mc = m < a.R ? m : a.R - 1;
  sm_gamma[tid] = a.gamma[tid];
  // ---- product 0: g1 = dy . W2; rows of dy go global -> registers two K-steps ahead, split on the fly
  const float* xp = a.dy + (size_t)mc * ET_D + 8 * hi;
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
  // a row tile in the accumulator layout: 32 pieces of 16 bytes per lane (first u, then a)
  f32x4 tile[32];
  const float* up = a.u_pre + (size_t)mc * ET_D + 4 * hi;
  const float* ap = a.a_pre + (size_t)mc * ET_D + 4 * hi;
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
          tile[i] = *reinterpret_cast<const f32x4*>(up + 32 * (i >> 2) + 8 * (i & 3));
        }
      }
    });
  }
  // du = g1 o gelu'(u), re-pack
  Unit un[16];
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 u4 = tile[4 * ob + q];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] *= gelu_grad(u4[e]);
    }
  repack(acc, un);
  // ---- product 1: g2 = du . W1; the pre-LayerNorm tile a arrives during its second half
  zero_acc(acc);
#pragma unroll
  for (int ks = 0; ks < ET_NKS; ++ks)
    kstep<1>(a.blob, ET_NKS + ks, ring, wave, lane, acc, c0, c1, __builtin_bit_cast(bf16x8, un[ks].h), __builtin_bit_cast(bf16x8, un[ks].l), [&]() {
      if (ks >= 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = 4 * (ks - 8) + j;
          tile[i] = *reinterpret_cast<const f32x4*>(ap + 32 * (i >> 2) + 8 * (i & 3));
        }
      }
    });
  // LayerNorm backward over the row (the lane pair r, r + 32 owns it): statistics of a as in the forward kernel, then
  //   d_a = rstd (g - mean(g) - xhat mean(g xhat)),   g = g2 gamma,   xhat = (a - mean) rstd
  {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) s += tile[i][e];
    s += nm_shfl_xor32(s);
    const float mean = s * (1.0f / ET_D);
    float vs = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = tile[i][e] - mean;
        tile[i][e] = d;
        vs = NM_FMA(d, d, vs);
      }
    vs += nm_shfl_xor32(vs);
    const float rstd = 1.0f / sqrtf(vs * (1.0f / ET_D) + a.eps);
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(sm_gamma + 32 * ob + 8 * q + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh_ = tile[4 * ob + q][e] * rstd;
          const float g = acc[ob][4 * q + e] * g4[e];
          tile[4 * ob + q][e] = xh_;
          acc[ob][4 * q + e] = g;
          sg += g;
          sgx = NM_FMA(g, xh_, sgx);
        }
      }
    sg += nm_shfl_xor32(sg);
    sgx += nm_shfl_xor32(sgx);
    const float mg = sg * (1.0f / ET_D), mgx = sgx * (1.0f / ET_D);
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] = rstd * ((acc[ob][4 * q + e] - mg) - tile[4 * ob + q][e] * mgx);
  }
  repack(acc, un);
  // coalesced store through this wavefront's 16 KiB of the transposition buffer (cf. the forward kernel's epilogue); `add`: a [R, 256] tensor
  // added in the store layout (dy for d_xh) or nullptr
  float* tb = tbuf + wave * 4096;
  const int rrow = lane >> 4, rpiece = lane & 15;
  auto store_rows = [&](float* __restrict__ dst, const float* __restrict__ add) {
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
          if (mm < a.R) {
            if (add) {
              const f32x4 d4 = *reinterpret_cast<const f32x4*>(add + (size_t)mm * ET_D + n0);
              v[j] = f32x4{v[j][0] + d4[0], v[j][1] + d4[1], v[j][2] + d4[2], v[j][3] + d4[3]};
            }
            *reinterpret_cast<f32x4*>(dst + (size_t)mm * ET_D + n0) = v[j];
          }
        }
      }
    }
  };
  store_rows(a.d_xh, a.dy);  // d_xh = dy + d_a (the wavefront's own 16 KiB: no barrier; LDS operations of a wavefront complete in order)
  // Everything this wavefront has in flight retires here -- the loads and stores of the epilogue above and the weight stream's requests for the
  // first K-steps of product 2 -- so the counted waits of product 2, which assume more in flight than there is, stay on the safe side.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // ---- product 2: d_att = d_a . Wo
  zero_acc(acc);
#pragma unroll
  for (int ks = 0; ks < ET_NKS; ++ks)
    kstep<1>(a.blob, 2 * ET_NKS + ks, ring, wave, lane, acc, c0, c1, __builtin_bit_cast(bf16x8, un[ks].h), __builtin_bit_cast(bf16x8, un[ks].l), [] {});
  store_rows(a.d_att, nullptr);
}

}  // namespace

extern "C" int nm_encoder_tail_bwd_bf16x3(const float* dy, const float* a_pre, const float* u_pre, const void* w2t_blob, const void* w1t_perm_blob,
                                          const void* wot_perm_blob, const float* gamma2, int rows, int dim, float eps, float* d_att, float* d_xh,
                                          nmStream_t stream) {
  NM_CHECK_ARG(dy && a_pre && u_pre && w2t_blob && w1t_perm_blob && wot_perm_blob && gamma2 && d_att && d_xh && rows > 0);
  if (dim != ET_D) return NM_ERR_UNSUPPORTED;
  TailArgs a{};
  a.dy = dy; a.a_pre = a_pre; a.u_pre = u_pre; a.blob[0] = (const char*)w2t_blob; a.blob[1] = (const char*)w1t_perm_blob;
  a.blob[2] = (const char*)wot_perm_blob; a.gamma = gamma2; a.d_att = d_att; a.d_xh = d_xh; a.R = rows; a.eps = eps;
  encoder_tail_bwd_kernel<<<(rows + ET_ROWS - 1) / ET_ROWS, 256, 0, (hipStream_t)stream>>>(a);
  return nm_launch_status();
}
