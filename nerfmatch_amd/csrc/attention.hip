// Softmax multi-head attention: the fp32 kernels and the nm_attention entry point, which also routes to the
// split-bf16 kernel of attention_v2.hip.
//
// attn32_kernel: flash-style attention for head dim 32 on the fp32 matrix cores; the (L,S,H) score tensor the
// reference materialises (415 MB at 3600^2 x 8 heads) never exists.  One wavefront owns 32 queries of one head.
//   S^T tile  = K_tile[32 keys x 32] . Q^T[32 x 32 queries]      (A = keys, B = queries; computing the TRANSPOSED
//               scores puts all keys of a query in one lane pair: row max / sum need one cross-half shuffle)
//   O^T      += V_tile^T[32 d x 32 keys] . P^T[32 keys x 32 queries]   (B = the probabilities exactly as the
//               first MFMA left them in registers: keys nrow(r, half) <-> k-step r; no LDS, no re-layout)
// K / V tiles are staged once per workgroup in LDS (see attn32_kernel) and shared by its 4 query tiles.
// attn_small_kernel: sequences <= 64 tokens (the 5x5 fine windows: 25 tokens, head dim 16): one thread per query,
// K/V of the (batch, head) in LDS, plain fp32 FMAs.
#include "attention_tile.h"
#include "internal.h"

namespace {

// Workgroup = 4 wavefronts = 128 queries of one (batch, head); every 32-key K/V tile is fetched ONCE per workgroup
// with coalesced 16-byte loads (thread t: key t/8, 16 bytes at column 4*(t%8)) and staged in a 3-slot LDS ring (rows
// padded to 36 floats so the 16-byte A-operand reads of 16 consecutive keys fall on distinct banks).
// Software pipeline per iteration t (one barrier):
//     global loads of tile t+2  ->  QK^T MFMAs of tile t+1  ||  softmax VALU of tile t  ->  PV MFMAs of tile t
// so the 16 score MFMAs of the next tile cover the softmax of the current one (one wavefront per SIMD has nothing else
// to overlap with).  Softmax runs in the exp2 domain: log2(e) is folded into the query scale and the exponentials are
// single v_exp_f32 instructions.
constexpr int KV_LD = 36;
constexpr int KV_SLOT = 2 * 32 * KV_LD;  // floats per ring slot: K tile then V tile

__global__ void __launch_bounds__(256) attn32_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                      const float* __restrict__ v, int ldq, int ldk, int ldv, int L, int S,
                                                      int H, float scale, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float sm[3 * KV_SLOT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hi = lane >> 5;
  const int qt = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;
  const int C = H * 32;
  const int qrow = qt * 32 + j;
  const int qc = qrow < L ? qrow : L - 1;
  float qreg[16];
  {  // (load16, the tail mask and store16 of attention_tile.h are written out in this kernel: as calls they changed its register allocation)
    const float qs = scale * 1.44269504088896340736f;  // scores are kept in the log2 domain
    const float* qp = q + ((size_t)b * L + qc) * ldq + h * 32 + 4 * hi;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4 t4 = *reinterpret_cast<const f32x4*>(qp + 8 * c);
#pragma unroll
      for (int t = 0; t < 4; ++t) qreg[4 * c + t] = t4[t] * qs;
    }
  }
  f32x16 o;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
  float mrun = -__builtin_inff(), lrun = 0.f;
  const float* kbase = k + (size_t)b * S * ldk + h * 32;
  const float* vbase = v + (size_t)b * S * ldv + h * 32;
  const int lrow = tid >> 3, lcol = (tid & 7) * 4;  // staging role of this thread
  const int nt = (S + 31) / 32;
  const int st_off = lrow * KV_LD + lcol;            // where this thread stages its 16 bytes (K; V at +32*KV_LD)
  const int ka_off = j * KV_LD + 4 * hi;             // A operand of QK^T: key row j
  const int va_off = 32 * KV_LD + 4 * hi * KV_LD + j;  // A operand of PV: V^T row j (feature), keys nrow(r, hi)
  auto gload = [&](int t, f32x4& kk, f32x4& vv) {
    const int key = t * 32 + lrow;
    const size_t row = (size_t)(key < S ? key : S - 1);
    kk = *reinterpret_cast<const f32x4*>(kbase + row * ldk + lcol);
    vv = *reinterpret_cast<const f32x4*>(vbase + row * ldv + lcol);
  };
  auto sstore = [&](float* slot, const f32x4& kk, const f32x4& vv) {
    *reinterpret_cast<f32x4*>(slot + st_off) = kk;
    *reinterpret_cast<f32x4*>(slot + st_off + 32 * KV_LD) = vv;
  };
  auto scores = [&](const float* slot) {
    f32x16 sc;
#pragma unroll
    for (int i = 0; i < 16; ++i) sc[i] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x4 ka = *reinterpret_cast<const f32x4*>(slot + ka_off + 8 * c);
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) sc = MFMA32(ka[tt], qreg[4 * c + tt], sc);
    }
    return sc;
  };
  f32x4 kst, vst;
  gload(0, kst, vst);
  sstore(sm, kst, vst);
  if (nt > 1) {
    gload(1, kst, vst);
    sstore(sm + KV_SLOT, kst, vst);
  }
  __syncthreads();
  f32x16 sc_next = scores(sm);
  int cur = 0;  // ring slot of tile t
  for (int t = 0; t < nt; ++t) {
    const int nxt = cur == 2 ? 0 : cur + 1, nx2 = nxt == 2 ? 0 : nxt + 1;
    f32x16 sc = sc_next;
    if (t + 2 < nt) gload(t + 2, kst, vst);
    if (t + 1 < nt) sc_next = scores(sm + nxt * KV_SLOT);
    if (t == nt - 1 && (S & 31)) {  // ragged last tile: keys >= S get zero probability
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi >= S) sc[r] = -__builtin_inff();
    }
    float mx = sc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sc[r]);
    mx = fmaxf(mx, nm_shfl_xor32(mx));
    const float mnew = fmaxf(mrun, mx);
    const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sc[r] = __builtin_amdgcn_exp2f(sc[r] - mnew);
      ps += sc[r];
    }
    ps += nm_shfl_xor32(ps);
    lrun = lrun * alpha + ps;
    mrun = mnew;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] *= alpha;
    const float* vs = sm + cur * KV_SLOT + va_off;
#pragma unroll
    for (int r = 0; r < 16; ++r) o = MFMA32(vs[nrow(r, 0) * KV_LD], sc[r], o);
    if (t + 2 < nt) sstore(sm + nx2 * KV_SLOT, kst, vst);
    __syncthreads();
    cur = nxt;
  }
  if (qrow < L) {
    const float inv = 1.0f / lrun;
    float* op = out + ((size_t)b * L + qrow) * C + h * 32 + 4 * hi;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 w4 = {o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv};
      *reinterpret_cast<f32x4*>(op + 8 * g) = w4;
    }
  }
}

// grid (H, B); block = 64 threads; thread i < L owns query i.  S <= 64, D <= 32.
template <int D>
__global__ void __launch_bounds__(64) attn_small_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                         const float* __restrict__ v, int ldq, int ldk, int ldv, int L, int S,
                                                         int H, float scale, float* __restrict__ out) {
  __shared__ float sk[64 * D], sv[64 * D];
  const int h = blockIdx.x, b = blockIdx.y, i = threadIdx.x;
  const int C = H * D;
  for (int e = i; e < S * D; e += 64) {
    const int row = e / D, d = e % D;
    sk[e] = k[((size_t)b * S + row) * ldk + h * D + d];
    sv[e] = v[((size_t)b * S + row) * ldv + h * D + d];
  }
  __syncthreads();
  if (i >= L) return;
  float qr[D], o[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    qr[d] = q[((size_t)b * L + i) * ldq + h * D + d] * scale;
    o[d] = 0.f;
  }
  // two passes like the reference (scores -> max -> exp/sum); S is tiny
  float mx = -__builtin_inff();
  for (int s = 0; s < S; ++s) {
    float dot = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) dot = NM_FMA(qr[d], sk[s * D + d], dot);
    mx = fmaxf(mx, dot);
  }
  float l = 0.f;
  for (int s = 0; s < S; ++s) {
    float dot = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) dot = NM_FMA(qr[d], sk[s * D + d], dot);
    const float p = expf(dot - mx);
    l += p;
#pragma unroll
    for (int d = 0; d < D; ++d) o[d] = NM_FMA(p, sv[s * D + d], o[d]);
  }
  const float inv = 1.0f / l;
#pragma unroll
  for (int d = 0; d < D; ++d) out[((size_t)b * L + i) * C + h * D + d] = o[d] * inv;
}

}  // namespace

extern "C" size_t nm_attention_workspace_bytes(int B, int S, int heads) {
  if (B <= 0 || S <= 0 || heads <= 0) return 0;
  return nm_internal_attn_v2_workspace(B, S, heads);
}

extern "C" int nm_attention(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, int B, int L, int S,
                            int heads, int head_dim, float scale, int flags, void* workspace, float* out, float* nlse_out,
                            nmStream_t stream) {
  const bool small = S <= 64 && L <= 64 && (head_dim == 16 || head_dim == 32);
  // the split-bf16 kernel streams pre-split operands from a workspace; the flag is ignored on the other routes
  const bool split = (flags & NM_ATTN_BF16X3) && head_dim == 32 && !small;
  if (nlse_out && !split) return NM_ERR_UNSUPPORTED;  // only the split-bf16 kernel keeps the log-sum-exp
  if (split && !workspace) return NM_ERR_WORKSPACE;
  NM_CHECK_ARG(q && k && v && out && B > 0 && L > 0 && S > 0 && heads > 0);
  const int C = heads * head_dim;
  if (ldq < C || ldk < C || ldv < C || (ldq | ldk | ldv) % 4) return NM_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (small) {
    dim3 grid(heads, B);
    if (head_dim == 16) attn_small_kernel<16><<<grid, 64, 0, s>>>(q, k, v, ldq, ldk, ldv, L, S, heads, scale, out);
    else attn_small_kernel<32><<<grid, 64, 0, s>>>(q, k, v, ldq, ldk, ldv, L, S, heads, scale, out);
    return nm_launch_status();
  }
  if (head_dim != 32) return NM_ERR_UNSUPPORTED;
  if (B > 65535 || heads > 65535) return NM_ERR_UNSUPPORTED;
  if (split) return nm_internal_attn_v2(q, k, v, ldq, ldk, ldv, B, L, S, heads, scale, workspace, out, s, nlse_out);
  dim3 grid(((L + 31) / 32 + 3) / 4, heads, B);
  attn32_kernel<<<grid, 256, 0, s>>>(q, k, v, ldq, ldk, ldv, L, S, heads, scale, out);
  return nm_launch_status();
}
