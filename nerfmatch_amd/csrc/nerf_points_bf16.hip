// Pointwise forward / backward of one NeRF MLP on the K-loop machinery of the render kernel (nerf_split_chain.h; round 4; the fine pass of the iNeRF refinement,
// nerfmatch/nerfmatch_evaluator.py:348-430 -- SURVEY.md section 8f rank 1).  The refinement needs d loss / d (ray origin, view
// direction) through the FINE network only, i.e. dX of every layer and no dW.  Both passes are pointwise over samples: the
// encodings (nm_inerf_encode) come in as rows, the compositing (nm_inerf_composite*) stays a kernel of its own, and what the
// backward needs from the forward is one BIT per activation (the ReLU gate) -- 9 x 16 bytes per sample lane instead of 8 KB of
// activations.  Arithmetic: the bf16 hi/lo split (three products, fp32 accumulate; gradients need the fp32 exponent range).
//
//   points_fwd (P = 4):  xi [n,96], xd [n,48]  ->  out4 [n,4] = (rgb logits, raw sigma),  gates [tiles][9][256] x 16 B
//       same blob and layer walk as the render kernel (nm_nerf_pack_bf16x3); gate table rows 0..7: layers 0..7 (8 bits per K-step
//       unit, gate_byte), row 8: the views layer (64 bits per lane: dword ob >> 1, bit 16 (ob & 1) + r)
//   points_bwd:  g4 [n,4] = d loss / d (logits, sigma),  gates  ->  g_xi0, g_xi5 [n,96] (layer 0 / skip connection parts), g_xd [n,48]
//       its own blob of TRANSPOSED weights (nm_nerf_pack_bwd_bf16x3), products in this order (K-steps x output blocks):
//       views^T -> xd (8 x 4), (views . feature_linear)^T -> h_7 (8 x 8: the folded matrix of the forward blob), pts 7^T, 6^T (16 x 8), pts 5^T -> IPE part (16 x 4),
//       pts 5^T, 4^T .. 1^T (16 x 8), pts 0^T -> IPE (16 x 4).  A finished product is copied out of the accumulators like in the forward
//       pass; re-packing a unit = AND with the sign-extended gate bit (v_bfe_i32 + v_and: two instructions per value, as bias + ReLU
//       were) + the hi/lo split, in the shadow of the consumer's MFMAs.
#include "nerf_split_chain.h"

namespace {
using namespace nmbf;
using nmsample::HALF_PI_F32, nmsample::frustum, nmsample::ray_consts, nmsample::lift_var, nmsample::ipe_exact, nmsample::view_row_value;  // nerf_sample.h

struct PointsArgs {
  const char* blob;
  const float* xi;   // fwd: [n,96];  bwd: unused
  const float* xd;   // fwd: [n,48]
  const float* g4;   // bwd: [n,4]
  float* out4;       // fwd: [n,4]
  float* g_xi0;      // bwd: [n,96]
  float* g_xi5;      // bwd: [n,96]
  float* g_xd;       // bwd: [n,48]
  u32x4* gates;      // [ntiles][9][256]
  int n, ntiles;
  const float* rays; // fwd, "from rays" form: [R,12]; then xi / xd are not read -- the kernel encodes its samples itself (nm_inerf_encode's formulas)
  const float* z;    //   fence posts [R, S + 1]; sample n = (ray n / Sa, interval n % Sa)
  const float* app_row;
  int S, Sa;
  // the tapped layer (the matching term of the refinement, nerfmatch_evaluator.py:420-441; round 5)
  float* feats;         // fwd: [n,256] row-major <- the tapped layer's post-ReLU activations, the rendered features
  const float* tap_w;   // bwd: [n] compositing weights and
  const float* tap_g;   //      [n / Sa rays, 256] d loss / d pt_feat: d loss / d activation (n, c) += tap_w[n] * tap_g[n / Sa][c]
  int tap;              // pts layer 0..7 that is tapped; -1: none  (behind the pointers: next to S / Sa the kernels' argument loads merge differently)
};

// Post-ReLU activations of the finished pts layer lo (raw accumulators in cx.hv) -> row `dst_row` of a row-major [n,256] matrix:
// register 4 q + e of block ob is column 32 ob + 8 q + 4 half + e (the two half-wavefronts of a sample write adjacent 16 bytes).
// Once per tile, like dump_tap (whose workspace layout only the render kernel's own reduction reads).
__device__ __forceinline__ void dump_tap_rows(int lo, const Ctx& cx, float* dst_row, int hh, bool valid) {
  const float* bl = cx.sm_small + OFF_BIAS + lo * 256 + 4 * hh;
  auto* tp = (__attribute__((address_space(1))) f32x4*)(dst_row + 4 * hh);
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(bl + ob * 32 + 8 * q);
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaxf(cx.hv[ob * 16 + 4 * q + e] + b[e], 0.f);
      if (valid) tp[ob * 8 + q * 2] = v;
    }
}

template <int P, bool RAYS>
__device__ __forceinline__ void points_fwd_body(const PointsArgs& a) {
  __shared__ __attribute__((aligned(16))) float sm[LDS_SCR];  // small block, ring, IPE operands
  float* const sm_small = sm + LDS_SMALL;
  float* const ring = sm + LDS_RING;
  float* const sm_ipe = sm + LDS_IPE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = lane & 31, hi = lane >> 5;
  const char* const blob_slots = a.blob + (size_t)SMALL_PAD * 4;
  for (int i = tid; i < SMALL / 4; i += 256) reinterpret_cast<f32x4*>(sm_small)[i] = reinterpret_cast<const f32x4*>(a.blob)[i];
#pragma unroll 1
  for (int bid = blockIdx.x; bid < a.ntiles; bid += gridDim.x) {
    __syncthreads();  // small block landed / the previous tile is through with the LDS
    const int sample = bid * TILE + wave * 32 + s;
    const size_t sc = (size_t)(sample < a.n ? sample : a.n - 1);
    ring_open<P>(blob_slots, ring, wave, lane);
    float vdir[3] = {0.f, 0.f, 0.f};  // "from rays": this sample's view direction (the views layer's extra inputs are made from it below)
    {  // the 6 IPE K-steps' B operands: this lane's 8 columns per step
      float* dst = sm_ipe + wave * (XS * 2 * 64 * 4) + lane * 4;
      if constexpr (RAYS) {
        // encode here (round 4: saves nm_inerf_encode and the 144 floats per sample it writes): nerf_sample.h's functions, the ones
        // nm_inerf_encode calls (the reference's cast_rays + PositionalEncodingMIP, render_utils.py:326-402, embedding.py:66-84), exact flavour
        const int r = (int)(sc / (size_t)a.Sa), si = (int)(sc % (size_t)a.Sa);
        const float* rp = a.rays + (size_t)r * 12;
        const float t0 = a.z[(size_t)r * (a.S + 1) + si], t1 = a.z[(size_t)r * (a.S + 1) + si + 1];
        vdir[0] = rp[8]; vdir[1] = rp[9]; vdir[2] = rp[10];
        float t_mean, t_var, r_var, dsq[3], nul[3], dnorm, mean[3], var[3];
        frustum(t0, t1, rp[11], t_mean, t_var, r_var);
        ray_consts(rp + 3, dsq, nul, dnorm);  // (dnorm unused: the compositing is another kernel)
        lift_var(t_var, r_var, dsq, nul, 0.f, var);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) mean[ax] = rp[ax] + t_mean * vdir[ax];  // (the iNeRF form of the mean: nerf_sample.h, lift_var)
        const float phl = hi ? HALF_PI_F32 : 0.f;
        park_ipe<P>(dst, [&](int idx) {
          const float scl = (float)(1 << (idx / 3));
          return ipe_exact(mean[idx % 3] * scl + phl, var[idx % 3], scl);
        });
      } else {
        const float* row = a.xi + sc * 96 + 45 * hi;  // xi is in the reference's order: this half's part (sin | shifted sin) starts at 45 half
        park_ipe<P>(dst, [&](int idx) { return row[idx]; });
      }
    }
    Ctx cx;
    cx.blob_slots = blob_slots; cx.ring = ring; cx.sm_small = sm_small; cx.tapw = nullptr;
    cx.nslots = NSLOT_FULL; cx.wave = wave; cx.lane = lane; cx.hi = hi; cx.tap = -1; cx.g = 0; cx.sig_part = 0.f;
    cx.vmax = 0.f; cx.rng = nullptr; cx.sc = 1.f; cx.tap_pref = false; cx.rgb = true; cx.tap_ring = nullptr; cx.tap_ipe = nullptr;
    cx.gptr = a.gates + (size_t)bid * 9 * 256 + tid;
    cx.gbits[0] = cx.gbits[1] = cx.gbits[2] = cx.gbits[3] = 0u;
    ring_open_wait<P>(cx);
    load_half<P>(cx.opA, ring, lane, 0);
    const float* ipe_src = sm_ipe + wave * (XS * 2 * 64 * 4) + lane * 4;
    f32x16 acc[8];
    ipe_steps<P, true>(acc, cx, ipe_src);
    finish_layer<P>(acc, 0, cx);
    const bool tapped = a.feats != nullptr;
#pragma unroll 1
    for (int l = 1; l < 8; ++l) {
      if (tapped && l - 1 == a.tap) dump_tap_rows(l - 1, cx, a.feats + sc * 256, launder(lane) >> 5, sample < a.n);
      layer_pass<P>(acc, l, cx, ipe_src);
    }
    if (tapped && a.tap == 7) dump_tap_rows(7, cx, a.feats + sc * 256, launder(lane) >> 5, sample < a.n);
    // views layer: layer 7's activations through views . feature_linear (one matrix, see fold_views in nerf_pack_bf16.hip) + this sample's xd row
    f32x16 av[4];
    views_hidden<P>(av, cx);
    cx.gptr[7 * 256] = u32x4{cx.gbits[0], cx.gbits[1], cx.gbits[2], cx.gbits[3]};  // layer 7's gates (collected by the K-loop above)
    const int hh = launder(lane) >> 5;
    {
      const float* row = a.xd + sc * 48 + 8 * hh;
      bf16x8 exh[VS], exl[VS];
#pragma unroll
      for (int e = 0; e < VS; ++e) {
        float v8[8];
        if constexpr (RAYS) {  // xd row of nm_inerf_encode: view_row_value (nerf_sample.h)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int f = 16 * e + 8 * hh + i;
            const int ax = f % 3;
            v8[i] = view_row_value(f, ax == 0 ? vdir[0] : ax == 1 ? vdir[1] : vdir[2], a.app_row);
          }
        } else {
          const f32x4 e0 = *reinterpret_cast<const f32x4*>(row + 16 * e), e1 = *reinterpret_cast<const f32x4*>(row + 16 * e + 4);
          v8[0] = e0[0]; v8[1] = e0[1]; v8[2] = e0[2]; v8[3] = e0[3]; v8[4] = e1[0]; v8[5] = e1[1]; v8[6] = e1[2]; v8[7] = e1[3];
        }
        split8_p<P>(v8, exh[e], exl[e]);
      }
      views_extras<P>(av, cx, exh, exl, RAYS && a.app_row == nullptr);  // (!RAYS: the xd rows come from memory)
    }
    const float* bv = sm_small + OFF_BVIEWS + 4 * hh;
    const float* wr = sm_small + OFF_WRGB + 4 * hh;
    float pr = 0.f, pg = 0.f, pb = 0.f;
    unsigned gv0 = 0u, gv1 = 0u;
#pragma unroll
    for (int ob = 0; ob < 4; ++ob)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(bv + ob * 32 + 8 * q);
        const f32x4 wr4 = *reinterpret_cast<const f32x4*>(wr + ob * 32 + 8 * q);
        const f32x4 wg4 = *reinterpret_cast<const f32x4*>(wr + 128 + ob * 32 + 8 * q);
        const f32x4 wb4 = *reinterpret_cast<const f32x4*>(wr + 256 + ob * 32 + 8 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float hv = __builtin_fmaxf(acc_read(av[ob][4 * q + e]) + b4[e], 0.f);
          const unsigned bit = min(__float_as_uint(hv), 1u) << (16 * (ob & 1) + 4 * q + e);  // hv >= 0: non-zero bits <=> hv > 0
          if (ob < 2) gv0 |= bit; else gv1 |= bit;
          pr = NM_FMA(hv, wr4[e], pr);
          pg = NM_FMA(hv, wg4[e], pg);
          pb = NM_FMA(hv, wb4[e], pb);
        }
      }
    cx.gptr[8 * 256] = u32x4{gv0, gv1, 0u, 0u};
    pr = (pr + nm_shfl_xor32(pr)) + sm_small[OFF_MISC + 1];
    pg = (pg + nm_shfl_xor32(pg)) + sm_small[OFF_MISC + 2];
    pb = (pb + nm_shfl_xor32(pb)) + sm_small[OFF_MISC + 3];
    const float sigma_raw = (cx.sig_part + nm_shfl_xor32(cx.sig_part)) + sm_small[OFF_MISC];
    if (hh == 0 && sample < a.n) *reinterpret_cast<f32x4*>(a.out4 + (size_t)sample * 4) = f32x4{pr, pg, pb, sigma_raw};
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// Unit u of the gradient held in cx.hv (registers 8m .. 8m+7 of block u >> 1), multiplied by its ReLU gate (GATED: byte u & 3 of
// gw[u >> 2], gate_byte's bit order) and split into bf16 hi / lo -- the operations of UnitWork (no bias), placed by the same tables.
template <bool GATED>
struct UnitWorkB {
  Ctx& cx;
  Unit& out;
  int u;
  u32x4 gw;
  float v8[8];
  float f0, f1;
  float r0[4], r1[4];
  __device__ __forceinline__ float gated(int e) const {
    float a = cx.hv[(u >> 1) * 16 + 8 * (u & 1) + e];
    if constexpr (GATED) {  // element e: bit e / 2 (e even) or 4 + e / 2 (e odd)
      const int b = 8 * (u & 3) + ((e & 1) ? 4 + (e >> 1) : (e >> 1));
      a = __int_as_float(__float_as_int(a) & __builtin_amdgcn_sbfe((int)gw[u >> 2], b, 1));
    }
    return a;
  }
  __device__ __forceinline__ void bias() {}
  __device__ __forceinline__ void ra(int j) { v8[j] = gated(j); pin(v8[j]); }
  __device__ __forceinline__ void rb(int j) { v8[4 + j] = gated(4 + j); pin(v8[4 + j]); }
  __device__ __forceinline__ void relu(int j) { ra(j); rb(j); }
  __device__ __forceinline__ void hi(int p) {
    unsigned hp = pack_bf16(v8[2 * p], v8[2 * p + 1]);
    f0 = __uint_as_float(hp << 16);
    f1 = __uint_as_float(hp & 0xffff0000u);
    pin(hp); pin(f0); pin(f1);
    out.h[p] = hp;
  }
  __device__ __forceinline__ void rem(int p) {
    r0[p] = v8[2 * p] - f0; r1[p] = v8[2 * p + 1] - f1;
    pin(r0[p]); pin(r1[p]);
  }
  __device__ __forceinline__ void lo(int p) {
    unsigned lp = pack_bf16(r0[p], r1[p]);
    pin(lp);
    out.l[p] = lp;
  }
  __device__ __forceinline__ void gates() {}
  __device__ __forceinline__ void seq(int c) { unit_seq<true>(*this, c); }
  template <bool EVEN> __device__ __forceinline__ void step8(int t) { unit_step8<EVEN, true>(*this, t); }
};
template <bool GATED>
__device__ __forceinline__ UnitWorkB<GATED> unit_work_b(int u, Ctx& cx, Unit& out, const u32x4& gw) {
  return UnitWorkB<GATED>{cx, out, u, gw, {}, 0.f, 0.f, {}, {}};
}
template <bool GATED>
__device__ __forceinline__ void make_unit0_b(Ctx& cx, const u32x4& gw) {
  UnitWorkB<GATED> w = unit_work_b<GATED>(0, cx, cx.xn, gw);
#pragma unroll
  for (int j = 0; j < 4; ++j) w.relu(j);
#pragma unroll
  for (int p = 0; p < 4; ++p) { w.hi(p); w.rem(p); }
#pragma unroll
  for (int p = 0; p < 4; ++p) w.lo(p);
}
// one product of the backward chain: NKS K-steps x NOB output blocks on the units of cx.hv (unit 0 is in cx.xn)
// (mode 3 = the arithmetic of mode 0 with the weight request that leaves M0 to the compiler: nerf_split_chain.h, owns_m0)
template <int NOB, int NKS, bool GATED>
__device__ __forceinline__ void bwd_product(f32x16 (&acc)[NOB], Ctx& cx, const u32x4& gw) {
#pragma unroll
  for (int ks = 0; ks < NKS; ks += 2) {
    {
      const Unit xc = cx.xn;
      const bf16x8 xh = __builtin_bit_cast(bf16x8, xc.h), xl = __builtin_bit_cast(bf16x8, xc.l);
      if constexpr (NOB == 8) {
        if (ks == 0) slot_step8<3, true, true>(acc, cx, xh, xl, unit_work_b<GATED>(ks + 1, cx, cx.xn, gw));
        else slot_step8<3, false, true>(acc, cx, xh, xl, unit_work_b<GATED>(ks + 1, cx, cx.xn, gw));
      } else {
        if (ks == 0) slot_step4<3, true, true>(acc, cx, xh, xl, unit_work_b<GATED>(ks + 1, cx, cx.xn, gw));
        else slot_step4<3, false, true>(acc, cx, xh, xl, unit_work_b<GATED>(ks + 1, cx, cx.xn, gw));
      }
    }
    {
      const Unit xc = cx.xn;
      const bf16x8 xh = __builtin_bit_cast(bf16x8, xc.h), xl = __builtin_bit_cast(bf16x8, xc.l);
      if constexpr (NOB == 8) {
        if (ks + 2 < NKS) slot_step8<3, false, false>(acc, cx, xh, xl, unit_work_b<GATED>(ks + 2, cx, cx.xn, gw));
        else slot_step8<3, false, false>(acc, cx, xh, xl, NoWork{});
      } else {
        if (ks + 2 < NKS) slot_step4<3, false, false>(acc, cx, xh, xl, unit_work_b<GATED>(ks + 2, cx, cx.xn, gw));
        else slot_step4<3, false, false>(acc, cx, xh, xl, NoWork{});
      }
    }
  }
}
__device__ __forceinline__ void take_acc8(const f32x16 (&acc)[8], Ctx& cx) {
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int r = 0; r < 16; ++r) cx.hv[ob * 16 + r] = acc_read(acc[ob][r]);
}
// 4-block result (output column c = 32 ob + nrow(r, half)) -> rows of a [n, ld] matrix, columns < ncol
__device__ __forceinline__ void store_acc4(const f32x16 (&av)[4], float* dst_row, int ncol, int hh, bool valid) {
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 32 * ob + 8 * q + 4 * hh;  // columns c .. c + 3 = registers 4 q .. 4 q + 3
      const f32x4 v = {acc_read(av[ob][4 * q + 0]), acc_read(av[ob][4 * q + 1]), acc_read(av[ob][4 * q + 2]), acc_read(av[ob][4 * q + 3])};
      if (valid && c + 3 < ncol) *reinterpret_cast<f32x4*>(dst_row + c) = v;
    }
}

__device__ __forceinline__ void points_bwd_body(const PointsArgs& a) {
  __shared__ __attribute__((aligned(16))) float sm[LDS_IPE];  // small block + ring
  float* const sm_small = sm + LDS_SMALL;
  float* const ring = sm + LDS_RING;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = lane & 31, hi = lane >> 5;
  const char* const blob_slots = a.blob + (size_t)SMALL_PAD * 4;
  for (int i = tid; i < SMALL / 4; i += 256) reinterpret_cast<f32x4*>(sm_small)[i] = reinterpret_cast<const f32x4*>(a.blob)[i];
#pragma unroll 1
  for (int bid = blockIdx.x; bid < a.ntiles; bid += gridDim.x) {
    __syncthreads();
    const int sample = bid * TILE + wave * 32 + s;
    const bool valid = sample < a.n;
    const size_t sc = (size_t)(valid ? sample : a.n - 1);
    ring_open<3>(blob_slots, ring, wave, lane);
    const u32x4* gt = a.gates + (size_t)bid * 9 * 256 + tid;
    const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.g4 + sc * 4);
    Ctx cx;
    cx.blob_slots = blob_slots; cx.ring = ring; cx.sm_small = sm_small; cx.tapw = nullptr;
    // (cx.g opaque: with a compile-time slot counter the fully unrolled first products had their 16 DMA source addresses precomputed
    //  at kernel entry, spilled, and reloaded -- scratch latency and a vmcnt(0) -- right behind the ring barrier of every K-step pair)
    cx.nslots = NSLOT_BWD; cx.wave = wave; cx.lane = lane; cx.hi = hi; cx.tap = -1; cx.g = launder_s(0); cx.sig_part = 0.f;
    cx.vmax = 0.f; cx.rng = nullptr; cx.sc = 1.f; cx.tap_pref = false; cx.rgb = true; cx.tap_ring = nullptr; cx.tap_ipe = nullptr; cx.gptr = nullptr;
    const int hh = launder(lane) >> 5;
    // d loss / d (views layer's post-ReLU activations) = gate . (W_rgb^T g_logit): this lane's 64 of the 128, in accumulator order
    {
      const u32x4 gv = gt[8 * 256];
      const float* wr = sm_small + OFF_WRGB + 4 * hh;
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 wr4 = *reinterpret_cast<const f32x4*>(wr + ob * 32 + 8 * q);
          const f32x4 wg4 = *reinterpret_cast<const f32x4*>(wr + 128 + ob * 32 + 8 * q);
          const f32x4 wb4 = *reinterpret_cast<const f32x4*>(wr + 256 + ob * 32 + 8 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float g = NM_FMA(wb4[e], g4[2], NM_FMA(wg4[e], g4[1], wr4[e] * g4[0]));
            const int bit = 16 * (ob & 1) + 4 * q + e;
            cx.hv[ob * 16 + 4 * q + e] = __int_as_float(__float_as_int(g) & __builtin_amdgcn_sbfe((int)gv[ob >> 1], bit, 1));
          }
        }
    }
    ring_open_wait<3>(cx);
    load_half<3>(cx.opA, ring, lane, 0);
    const u32x4 none = {0u, 0u, 0u, 0u};
    f32x16 acc[8];
    // views^T -> xd columns
    {
      f32x16 av[4];
      make_unit0_b<false>(cx, none);
      bwd_product<4, 8, false>(av, cx, none);
      store_acc4(av, a.g_xd + sc * 48, 48, hh, valid);
    }
    // (views_w[:, :256] . feature_w)^T -> layer 7's post-ReLU activations, + the density head's share
    make_unit0_b<false>(cx, none);
    bwd_product<8, 8, false>(acc, cx, none);
    take_acc8(acc, cx);
    {
      const float* wa = sm_small + OFF_WALPHA + 4 * hh;
#pragma unroll
      for (int ob = 0; ob < 8; ++ob)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 w4v = *reinterpret_cast<const f32x4*>(wa + ob * 32 + 8 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) cx.hv[ob * 16 + 4 * q + e] = NM_FMA(w4v[e], g4[3], cx.hv[ob * 16 + 4 * q + e]);
        }
    }
    // The rest of the chain as ONE loop body (a second inlined copy of the 16-step product made the allocator keep two accumulator sets
    // and spill): iteration l = 7 .. 0 consumes d loss / d (post-ReLU output of pts layer l) sitting in cx.hv, gates it with the bits of
    // the forward pass and multiplies by that layer's transposed weights.  Layers 5 and 0 first send their gated gradient through the IPE
    // columns (4 output blocks).
#pragma unroll 1
    for (int l = 7; l >= 0; --l) {
      const u32x4 gw = gt[l * 256];
      if (l == a.tap && a.tap_g) {
        // the matching term's gradient enters at the tapped layer's (post-ReLU) activations: pt_feat = sum_s w_s h_tap(s), so
        // d loss / d h_tap(n) += w_n . d loss / d pt_feat[ray]  (product, then sum: nm_inerf_ray_sums_bwd's g_feats + the residual of the GEMM chain)
        const float wn = valid ? a.tap_w[sc] : 0.f;
        const float* gr = a.tap_g + (sc / (size_t)a.Sa) * 256 + 4 * hh;
#pragma unroll
        for (int ob = 0; ob < 8; ++ob)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gr + ob * 32 + 8 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) cx.hv[ob * 16 + 4 * q + e] = __fadd_rn(cx.hv[ob * 16 + 4 * q + e], __fmul_rn(wn, g[e]));
          }
      }
      if (l == 5 || l == 0) {
        f32x16 av[4];
        make_unit0_b<true>(cx, gw);
        bwd_product<4, 16, true>(av, cx, gw);
        store_acc4(av, (l == 5 ? a.g_xi5 : a.g_xi0) + sc * 96, 96, hh, valid);
        if (l == 0) break;
      }
      make_unit0_b<true>(cx, gw);
      bwd_product<8, 16, true>(acc, cx, gw);
      take_acc8(acc, cx);
    }
  }
}

__global__ void __launch_bounds__(256, 1) nerf_points_fwd_kernel(PointsArgs a) { points_fwd_body<4, false>(a); }
__global__ void __launch_bounds__(256, 1) nerf_points_fwd_rays_kernel(PointsArgs a) { points_fwd_body<4, true>(a); }
__global__ void __launch_bounds__(256, 1) nerf_points_bwd_kernel(PointsArgs a) { points_bwd_body(a); }

}  // namespace

extern "C" size_t nm_nerf_points_gate_bytes(int n) { return (size_t)((n + TILE - 1) / TILE) * 9 * 256 * 16; }

static int points_grid(int ntiles, nmStream_t stream) {
  const int ncu = nm_stream_cus(stream);
  return ntiles < ncu ? ntiles : ncu;
}

extern "C" int nm_nerf_points_fwd_bf16x3(const void* blob, const float* xi, const float* xd, int n, float* out4, void* gates, nmStream_t stream) {
  NM_CHECK_ARG(blob && xi && xd && out4 && gates && n > 0);
  PointsArgs a = {};
  a.blob = (const char*)blob; a.xi = xi; a.xd = xd; a.out4 = out4; a.gates = (u32x4*)gates; a.n = n; a.ntiles = (n + TILE - 1) / TILE;
  a.tap = -1;
  nerf_points_fwd_kernel<<<points_grid(a.ntiles, stream), 256, 0, (hipStream_t)stream>>>(a);
  return nm_launch_status();
}

extern "C" int nm_nerf_points_bwd_bf16x3(const void* blob_bwd, const float* g4, const void* gates, int n, float* g_xi0, float* g_xi5, float* g_xd,
                                         nmStream_t stream) {
  NM_CHECK_ARG(blob_bwd && g4 && gates && g_xi0 && g_xi5 && g_xd && n > 0);
  PointsArgs a = {};
  a.blob = (const char*)blob_bwd; a.g4 = g4; a.gates = (u32x4*)const_cast<void*>(gates); a.g_xi0 = g_xi0; a.g_xi5 = g_xi5; a.g_xd = g_xd;
  a.n = n; a.ntiles = (n + TILE - 1) / TILE; a.tap = -1;
  nerf_points_bwd_kernel<<<points_grid(a.ntiles, stream), 256, 0, (hipStream_t)stream>>>(a);
  return nm_launch_status();
}

extern "C" int nm_nerf_points_fwd_rays_bf16x3(const void* blob, const float* rays, const float* z, int R, int S, int S_act, const float* app_row,
                                              int tap_layer, float* out4, void* gates, float* feats, nmStream_t stream) {
  NM_CHECK_ARG(blob && rays && z && out4 && gates && R > 0 && S > 0 && S_act > 0 && S_act <= S);
  NM_CHECK_ARG(feats ? (tap_layer >= 0 && tap_layer <= 7) : tap_layer == -1);
  PointsArgs a = {};
  a.blob = (const char*)blob; a.rays = rays; a.z = z; a.app_row = app_row; a.S = S; a.Sa = S_act; a.out4 = out4; a.gates = (u32x4*)gates;
  a.n = R * S_act; a.ntiles = (a.n + TILE - 1) / TILE; a.tap = tap_layer; a.feats = feats;
  nerf_points_fwd_rays_kernel<<<points_grid(a.ntiles, stream), 256, 0, (hipStream_t)stream>>>(a);
  return nm_launch_status();
}

extern "C" int nm_nerf_points_bwd_tap_bf16x3(const void* blob_bwd, const float* g4, const void* gates, int R, int S_act, int tap_layer,
                                             const float* tap_weights, const float* g_pt_feat, float* g_xi0, float* g_xi5, float* g_xd,
                                             nmStream_t stream) {
  NM_CHECK_ARG(blob_bwd && g4 && gates && g_xi0 && g_xi5 && g_xd && R > 0 && S_act > 0 && tap_layer >= 0 && tap_layer <= 7 && tap_weights && g_pt_feat);
  PointsArgs a = {};
  a.blob = (const char*)blob_bwd; a.g4 = g4; a.gates = (u32x4*)const_cast<void*>(gates); a.g_xi0 = g_xi0; a.g_xi5 = g_xi5; a.g_xd = g_xd;
  a.n = R * S_act; a.ntiles = (a.n + TILE - 1) / TILE; a.Sa = S_act; a.tap = tap_layer; a.tap_w = tap_weights; a.tap_g = g_pt_feat;
  nerf_points_bwd_kernel<<<points_grid(a.ntiles, stream), 256, 0, (hipStream_t)stream>>>(a);
  return nm_launch_status();
}
