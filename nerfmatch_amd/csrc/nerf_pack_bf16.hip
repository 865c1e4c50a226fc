// Host-side packing of one NeRF MLP into the weight blobs of the operand-splitting kernels (no device code): the forward blobs of
// nerf_fwd_bf16.hip / nerf_points_bf16.hip in the three arithmetic modes and the transposed blob of the pointwise backward.  A blob is the
// small-parameter block (nerf_bf16_common.h: OFF_*) followed by the weight slots in the order the kernels' K-loops consume them.
#include "nerf_bf16_common.h"
#include <stdlib.h>

namespace {
using namespace nmbf;

inline uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_to_f(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

inline uint16_t f16_bits(float f) {  // round to nearest even (the host compiler's float -> _Float16 conversion), saturating
  f = f > 65504.0f ? 65504.0f : (f < -65504.0f ? -65504.0f : f);
  const _Float16 hf = (_Float16)f;
  uint16_t bits;
  memcpy(&bits, &hf, 2);
  return bits;
}
inline float f16_to_f(uint16_t b) {
  _Float16 hf;
  memcpy(&hf, &b, 2);
  return (float)hf;
}
// w = h + l in the split modes: mode 0: bf16 hi / lo, 2: fp16 hi / lo
inline void split_hi_lo(float w, int mode, uint16_t& h, uint16_t& l) {
  if (mode == 2) {
    h = f16_bits(w);
    l = f16_bits(w - f16_to_f(h));
  } else {
    h = bf16_rne(w);
    l = bf16_rne(w - bf16_to_f(h));
  }
}

// one slot: element (obo, hl, lane, i) = split(W[32*obo + (lane&31)][col(lane>>5, i)]); col < 0 -> 0
// (fp16x1 blob: element (obo, lane, i) = fp16(W[...]) rounded to nearest even, 8 KiB per slot)
// mode 0: bf16 hi / lo, 1: single fp16, 2: fp16 hi / lo
// (sc(c): power-of-two factor of input column c -- fp16x3 operand scaling, 1 otherwise; exact in fp32)
template <typename ColFn, typename ScFn>
void pack_slot(uint16_t* slot, const float* W, int ld, int nob, ColFn col, int mode, ScFn sc) {
  for (int obo = 0; obo < nob; ++obo)
    for (int ln = 0; ln < 64; ++ln)
      for (int i = 0; i < 8; ++i) {
        const int c = col(ln >> 5, i);
        const float w = c < 0 ? 0.f : W[(size_t)(32 * obo + (ln & 31)) * ld + c] * sc(c);
        if (mode == 1) {
          slot[(obo * 64 + ln) * 8 + i] = f16_bits(w);
          continue;
        }
        uint16_t h, l;
        split_hi_lo(w, mode, h, l);
        slot[((obo * 2 + 0) * 64 + ln) * 8 + i] = h;
        slot[((obo * 2 + 1) * 64 + ln) * 8 + i] = l;
      }
}

// a slot of the paired views layer: blocks 0..3 take their columns from colA, blocks 4..7 are the SAME 128 output rows with colB
template <typename ColA, typename ColB, typename ScFn>
void pack_slot2(uint16_t* slot, const float* W, int ld, ColA colA, ColB colB, int mode, ScFn sc) {
  for (int obo = 0; obo < 8; ++obo)
    for (int ln = 0; ln < 64; ++ln)
      for (int i = 0; i < 8; ++i) {
        const int c = obo < 4 ? colA(ln >> 5, i) : colB(ln >> 5, i);
        const float w = c < 0 ? 0.f : W[(size_t)(32 * (obo & 3) + (ln & 31)) * ld + c] * sc(c);
        uint16_t h, l;
        split_hi_lo(w, mode, h, l);
        slot[((obo * 2 + 0) * 64 + ln) * 8 + i] = h;
        slot[((obo * 2 + 1) * 64 + ln) * 8 + i] = l;
      }
}

}  // namespace

extern "C" size_t nm_nerf_blob_bytes_bf16x3(void) { return BLOB_BYTES; }
extern "C" size_t nm_nerf_blob_bytes_fp16x1(void) { return BLOB_BYTES_FP16; }
extern "C" size_t nm_nerf_blob_bytes_bwd_bf16x3(void) { return BLOB_BYTES_BWD; }

// fp16x3 operand scaling (round 4).  An fp16 hi/lo pair carries 22 significant bits only while the lo part is a NORMAL fp16
// number, i.e. for |x| >~ 2^-3; below that the lo part is a subnormal with an absolute quantum of 2^-24 (U(+-1/16) weights: ~20
// bits, 2^-25 absolute each -- as much noise as the fp32 accumulation itself, scripts/fp16x3_scaling_study.py).  Powers of two
// commute with every rounding, so operands are moved into the middle of the fp16 range and the result is moved back exactly:
//   weights of layer l, input group g (hidden columns | IPE columns | direction PE | appearance):  W * 2^a(l,g), chosen HERE
//     from max|W| (-> [2^13, 2^14): constants cannot saturate);
//   inputs of layer l:  x * 2^c_l -- c_0 (IPE, |x| <= 1) and the direction PE are static (2^12); the hidden activations' c_l come from
//     the caller (act_log2: measured ranges, nm_nerf_fwd_fp16x3 status[]; NULL = 0, the unscaled activations of round 3);
//   accumulator of layer l:  2^A_l x the true pre-activation, A_l = a(l,g) + c(g) for every group g (the a's are tied by that);
//   re-packing:  fma(acc, 2^(c_{l+1} - A_l), bias * 2^c_{l+1})  (OFF_SCALE, OFF_BIAS), density head vector * 2^-c_8, rgb head: bias
//     * 2^A_9, vectors * 2^-A_9; tapped activations leave the kernel through OFF_DESCALE.
struct Fp16Scales {
  int a0 = 0, ah[10] = {0}, ax5 = 0, avd = 0, ava = 0;  // weight exponents: layer 0; hidden groups of layers 1..8 and views (9); layer 5's IPE columns; views' direction / appearance columns
  int c[12] = {0};                                      // input exponents: [0] IPE, [1..9] hidden input of layers 1..8 / views, [10] direction PE, [11] appearance
  int A[10] = {0};                                      // accumulator exponents of layers 0..8, views (9)
};
static float absmax_cols(const float* W, int rows, int ld, int c0, int c1) {
  float m = 0.f;
  for (int r = 0; r < rows; ++r)
    for (int c = c0; c < c1; ++c) m = fmaxf(m, fabsf(W[(size_t)r * ld + c]));
  return m;
}
static int weight_exp(float m) {  // a with m * 2^a in [2^13, 2^14)
  if (!(m > 0.f) || !(m < 3.0e38f)) return 0;
  int e;
  frexpf(m, &e);  // m = f * 2^e, f in [0.5, 1)
  return 14 - e;
}
// feature_linear has no activation, so  views(cat[feature_linear(h), dir, app]) = (V_h F) h + V_d dir + V_a app + (V_h f_b + v_b):
// the 128 x 256 product V_h F and the folded bias are formed here in double precision and rounded to fp32 ONCE; the kernels never
// run feature_linear as a layer (65,536 of the 607,232 multiply-adds per sample).  Layout of the result: views_w's own
// [128][283 + app] with columns 0..255 replaced, so the packing code below reads it like views_w.
struct FoldedViews {
  float* W = nullptr;  // [128][ldv]
  float b[128];
  ~FoldedViews() { free(W); }
};
static int fold_views(const nmNerfWeights* w, FoldedViews& fv) {
  const int ldv = 283 + w->app_dim;
  fv.W = (float*)malloc((size_t)128 * ldv * sizeof(float));
  if (!fv.W) return NM_ERR_ARG;
  for (int n = 0; n < 128; ++n) {
    const float* vr = w->views_w + (size_t)n * ldv;
    for (int k = 0; k < 256; ++k) {
      double acc = 0.0;
      for (int j = 0; j < 256; ++j) acc += (double)vr[j] * (double)w->feat_w[(size_t)j * 256 + k];
      fv.W[(size_t)n * ldv + k] = (float)acc;
    }
    for (int c = 256; c < ldv; ++c) fv.W[(size_t)n * ldv + c] = vr[c];
    double bb = (double)w->views_b[n];
    for (int j = 0; j < 256; ++j) bb += (double)vr[j] * (double)w->feat_b[j];
    fv.b[n] = (float)bb;
  }
  return NM_OK;
}

static int choose_fp16_scales(const nmNerfWeights* w, const float* views_folded, const int* act_log2, Fp16Scales& sc) {
  sc.c[0] = 12; sc.c[10] = 12; sc.c[11] = 0;
  if (act_log2) {
    for (int i = 0; i < 12; ++i) {
      if (act_log2[i] < -24 || act_log2[i] > 15) return NM_ERR_ARG;
      sc.c[i] = act_log2[i];
    }
    if (sc.c[0] > 15 || sc.c[10] > 15) return NM_ERR_ARG;  // |IPE|, |direction PE| <= 1 must stay below 65504
  }
  const int ldv = 283 + w->app_dim;
  sc.a0 = weight_exp(absmax_cols(w->pts_w[0], 256, 90, 0, 90));
  sc.A[0] = sc.a0 + sc.c[0];
  for (int l = 1; l < 8; ++l) {
    const float* W = w->pts_w[l];
    const int ld = l == 5 ? 346 : 256, col0 = l == 5 ? 90 : 0;
    sc.ah[l] = weight_exp(absmax_cols(W, 256, ld, col0, col0 + 256));
    sc.A[l] = sc.ah[l] + sc.c[l];
  }
  {  // layer 5: the IPE columns share the accumulator
    const int ideal = weight_exp(absmax_cols(w->pts_w[5], 256, 346, 0, 90));
    sc.ax5 = sc.A[5] - sc.c[0];
    if (sc.ax5 > ideal + 1) {  // would push the IPE columns beyond 2^15: lower the whole layer
      const int d = sc.ax5 - (ideal + 1);
      sc.ax5 -= d; sc.ah[5] -= d; sc.A[5] -= d;
    }
  }
  {  // views layer (folded): hidden = layer 7's activations, carried at 2^c[8] | direction PE | appearance
    sc.c[9] = sc.c[8];
    sc.ah[9] = weight_exp(absmax_cols(views_folded, 128, ldv, 0, 256));
    sc.A[9] = sc.ah[9] + sc.c[9];
    const int ideal_d = weight_exp(absmax_cols(views_folded, 128, ldv, 256, 283));
    const int ideal_a = w->app_dim ? weight_exp(absmax_cols(views_folded, 128, ldv, 283, ldv)) : 1 << 20;
    int d = 0;
    if (sc.A[9] - sc.c[10] > ideal_d + 1) d = sc.A[9] - sc.c[10] - (ideal_d + 1);
    if (sc.A[9] - sc.c[11] - d > ideal_a + 1) d = sc.A[9] - sc.c[11] - (ideal_a + 1);
    sc.ah[9] -= d; sc.A[9] -= d;
    sc.avd = sc.A[9] - sc.c[10];
    sc.ava = sc.A[9] - sc.c[11];
  }
  for (int i = 0; i < 10; ++i)
    if (sc.A[i] < -100 || sc.A[i] > 100) return NM_ERR_ARG;
  return NM_OK;
}

static int nerf_pack_split(const nmNerfWeights* w, void* blob_v, int fp16, const int* act_log2 = nullptr) {  // 0: bf16x3, 1: fp16x1, 2: fp16x3
  if (!w || !blob_v) return NM_ERR_ARG;
  for (int i = 0; i < 8; ++i)
    if (!w->pts_w[i] || !w->pts_b[i]) return NM_ERR_ARG;
  if (!w->alpha_w || !w->alpha_b || !w->feat_w || !w->feat_b || !w->views_w || !w->views_b || !w->rgb_w || !w->rgb_b)
    return NM_ERR_ARG;
  if (w->app_dim != 0 && w->app_dim != 16) return NM_ERR_UNSUPPORTED;
  FoldedViews fv;
  if (fold_views(w, fv) != NM_OK) return NM_ERR_ARG;
  Fp16Scales sc;  // all zero: the unscaled modes
  if (fp16 == 2) {
    const int rc = choose_fp16_scales(w, fv.W, act_log2, sc);
    if (rc != NM_OK) return rc;
  }
  auto p2 = [](int e) { return ldexpf(1.0f, e); };
  memset(blob_v, 0, fp16 == 1 ? BLOB_BYTES_FP16 : BLOB_BYTES);
  float* small = (float*)blob_v;
  // bias of layer l at the input scale of its consumer (c[l + 1]; layer 7 feeds the density head and the folded views layer);
  // row 8 of the bias table (feature_linear, before the fold) stays zero
  for (int l = 0; l < 8; ++l)
    for (int n = 0; n < 256; ++n) small[OFF_BIAS + l * 256 + n] = w->pts_b[l][n] * p2(sc.c[l + 1]);
  for (int n = 0; n < 128; ++n) small[OFF_BVIEWS + n] = fv.b[n] * p2(sc.A[9]);
  for (int n = 0; n < 256; ++n) small[OFF_WALPHA + n] = w->alpha_w[n] * p2(-sc.c[8]);
  for (int n = 0; n < 384; ++n) small[OFF_WRGB + n] = w->rgb_w[n] * p2(-sc.A[9]);
  small[OFF_MISC] = w->alpha_b[0];
  for (int c = 0; c < 3; ++c) small[OFF_MISC + 1 + c] = w->rgb_b[c];
  for (int l = 0; l < 16; ++l) small[OFF_SCALE + l] = l < 8 ? p2(sc.c[l + 1] - sc.A[l]) : 1.0f;
  for (int l = 0; l < 8; ++l) small[OFF_DESCALE + l] = p2(-sc.c[l + 1]);
  small[OFF_INSCALE + 0] = p2(sc.c[0]); small[OFF_INSCALE + 1] = p2(sc.c[10]); small[OFF_INSCALE + 2] = p2(sc.c[11]); small[OFF_INSCALE + 3] = 1.0f;

  uint16_t* slots = (uint16_t*)((char*)blob_v + (size_t)SMALL_PAD * 4);
  int g = 0;
  auto next = [&]() { return slots + (size_t)(g++) * ((fp16 == 1 ? SLOT_BYTES / 2 : SLOT_BYTES) / 2); };
  auto ipe_steps = [&](const float* W, int ld, int aexp) {
    const float f = p2(aexp);
    for (int m = 0; m < XS; ++m)
      pack_slot(next(), W, ld, 8, [&](int h, int i) { const int idx = 8 * m + i; return idx < 45 ? 45 * h + idx : -1; }, fp16, [&](int) { return f; });
  };
  auto hid_steps = [&](const float* W, int ld, int col0, int nob, int aexp) {
    const float f = p2(aexp);
    for (int ks = 0; ks < HS; ++ks)
      pack_slot(next(), W, ld, nob, [&](int h, int i) { return col0 + 32 * (ks >> 1) + nrow(8 * (ks & 1) + i, h); }, fp16, [&](int) { return f; });
  };
  for (int l = 0; l < 8; ++l) {  // kernel order: layer 0 = IPE steps; layer 5 = hidden steps, then the skip connection's IPE steps
    if (l == 0) ipe_steps(w->pts_w[0], 90, sc.a0);
    if (l != 0) hid_steps(w->pts_w[l], l == 5 ? 346 : 256, l == 5 ? 90 : 0, 8, sc.ah[l]);
    if (l == 5) ipe_steps(w->pts_w[5], 346, sc.ax5);
  }
  const int ldv = 283 + w->app_dim;
  const float fvh = p2(sc.ah[9]), fvd = p2(sc.avd), fva = p2(sc.ava);
  auto hid_col = [&](int ks, int h, int i) { return 32 * (ks >> 1) + nrow(8 * (ks & 1) + i, h); };
  auto ext_col = [&](int e, int h, int i) {
    const int f = 16 * e + 8 * h + i;
    if (f < 27) return 256 + f;
    if (f < 43 && w->app_dim) return 283 + (f - 27);
    return -1;
  };
  auto vsc = [&](int c) { return c < 256 ? fvh : c < 283 ? fvd : fva; };
  if (fp16 != 1) {
    // split modes: two K-steps of the 4-block layer per slot (slot_step4x2) -- blocks 0..3 = the layer's four output blocks for the first
    // K-step, blocks 4..7 = the same four for the second; the last extra K-step has a slot of its own (first half)
    for (int sl = 0; sl < HS / 2; ++sl)
      pack_slot2(next(), fv.W, ldv, [&](int h, int i) { return hid_col(2 * sl, h, i); }, [&](int h, int i) { return hid_col(2 * sl + 1, h, i); }, fp16, vsc);
    pack_slot2(next(), fv.W, ldv, [&](int h, int i) { return ext_col(0, h, i); }, [&](int h, int i) { return ext_col(1, h, i); }, fp16, vsc);
    pack_slot(next(), fv.W, ldv, 4, [&](int h, int i) { return ext_col(2, h, i); }, fp16, vsc);
    return g == NSLOT_FULL_PAIRED ? NM_OK : NM_ERR_ARG;
  }
  hid_steps(fv.W, ldv, 0, 4, sc.ah[9]);
  for (int e = 0; e < VS; ++e) pack_slot(next(), fv.W, ldv, 4, [&](int h, int i) { return ext_col(e, h, i); }, fp16, vsc);
  return g == NSLOT_FULL ? NM_OK : NM_ERR_ARG;
}

extern "C" int nm_nerf_pack_bf16x3(const nmNerfWeights* w, void* blob_v) { return nerf_pack_split(w, blob_v, 0); }
extern "C" int nm_nerf_pack_fp16x3(const nmNerfWeights* w, const int* act_log2, void* blob_v) { return nerf_pack_split(w, blob_v, 2, act_log2); }
extern "C" int nm_nerf_pack_fp16x1(const nmNerfWeights* w, void* blob_v) { return nerf_pack_split(w, blob_v, 1); }

// Transposed weights of one MLP in the order points_bwd_body consumes them (see the comment above PointsArgs); small block as in
// nm_nerf_pack_bf16x3 (rgb / density head vectors).
extern "C" int nm_nerf_pack_bwd_bf16x3(const nmNerfWeights* w, void* blob_v) {
  if (!w || !blob_v) return NM_ERR_ARG;
  void* tmp = malloc(BLOB_BYTES);
  if (!tmp) return NM_ERR_ARG;
  const int rc = nerf_pack_split(w, tmp, 0);
  if (rc != NM_OK) { free(tmp); return rc; }
  memset(blob_v, 0, BLOB_BYTES_BWD);
  memcpy(blob_v, tmp, (size_t)SMALL_PAD * 4);
  free(tmp);
  uint16_t* slots = (uint16_t*)((char*)blob_v + (size_t)SMALL_PAD * 4);
  int g = 0;
  auto next = [&]() { return slots + (size_t)(g++) * (SLOT_BYTES / 2); };
  const int ldv = 283 + w->app_dim;
  // product: out[o] = sum_k in[k] * Wt(o, k); rows beyond n_out are zero; nks K-steps of 16 inputs, nob blocks of 32 outputs
  auto product = [&](int n_out, int n_in, int nob, auto wt) {
    float* T = (float*)calloc((size_t)32 * nob * n_in, sizeof(float));
    for (int o = 0; o < n_out; ++o)
      for (int k = 0; k < n_in; ++k) T[(size_t)o * n_in + k] = wt(o, k);
    for (int ks = 0; ks < n_in / 16; ++ks)
      pack_slot(next(), T, n_in, nob, [&](int h, int i) { return 32 * (ks >> 1) + nrow(8 * (ks & 1) + i, h); }, 0, [](int) { return 1.0f; });
    free(T);
  };
  const int nxd = 27 + w->app_dim;
  FoldedViews fv;
  if (fold_views(w, fv) != NM_OK) return NM_ERR_ARG;
  product(nxd, 128, 4, [&](int c, int n) { return w->views_w[(size_t)n * ldv + 256 + c]; });       // views^T -> xd
  product(256, 128, 8, [&](int k, int n) { return fv.W[(size_t)n * ldv + k]; });                   // (views . feature_linear)^T -> h_7
  for (int l = 7; l >= 6; --l) product(256, 256, 8, [&](int k, int n) { return w->pts_w[l][(size_t)n * 256 + k]; });
  product(90, 256, 4, [&](int f, int n) { return w->pts_w[5][(size_t)n * 346 + f]; });            // pts 5^T -> IPE columns
  product(256, 256, 8, [&](int k, int n) { return w->pts_w[5][(size_t)n * 346 + 90 + k]; });      // pts 5^T -> hidden columns
  for (int l = 4; l >= 1; --l) product(256, 256, 8, [&](int k, int n) { return w->pts_w[l][(size_t)n * 256 + k]; });
  product(90, 256, 4, [&](int f, int n) { return w->pts_w[0][(size_t)n * 90 + f]; });             // pts 0^T -> IPE
  return g == NSLOT_BWD ? NM_OK : NM_ERR_ARG;
}
