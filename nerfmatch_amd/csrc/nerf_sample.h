// The mip-NeRF sample math, defined ONCE for every NeRF-side kernel: the conical-frustum Gaussian, its lift to a diagonal 3-D covariance,
// the integrated positional encoding, the view-direction row, the alpha / transmittance step and the compositing scan along a ray.
// Callers: nerf_fwd.hip (fp32 MFMA render), nerf_fwd_bf16.hip (split render), nerf_points_bf16.hip (pointwise forward "from rays"),
// inerf.hip (nm_inerf_encode and its backward, the per-ray compositing loops, the ray sums), nerf_train.hip (nm_nerf_train_encode),
// nerf_composite.hip (the wavefront-per-ray compositing pair), encode.hip (the constant).  Several tests require these kernels to agree BIT FOR BIT
// (tests/test_nerf_sample_math_gpu.py, test_tapped_points_kernels_vs_gemm_chain, test_wavefront_compositing_vs_per_ray_loops): they do
// because they inline the same expression trees from here -- the build uses -ffp-contract=off, so operand order and association below
// ARE the result bits.  Change a formula here and every kernel changes with it; do not re-type one at a call site.
#pragma once
#include "common.h"

namespace nmsample {

constexpr float HALF_PI_F32 = 1.57079637050628662109375f;  // fl32(0.5 * pi): the reference adds a python float to an fp32 tensor

// Opaque copy of a lane-varying int: values derived from the copy cannot be hoisted above this point.  Used so that
// cheap epilogue-only quantities (LDS addresses, view-direction encodings) are recomputed where they are needed
// instead of being kept live (= spilled to scratch) across the ~9,500 MFMAs of the MLP.
__device__ __forceinline__ int launder(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// ---- conical frustum -> Gaussian ------------------------------------------------------------------------------------------------
// Interval [t0, t1] of a cone of base radius `radius` -> mean and variance along the ray, variance across it (stable form,
// the reference's conical_frustum_to_gaussian, render_utils.py:365-374).
__device__ __forceinline__ void frustum(float t0, float t1, float radius, float& t_mean, float& t_var, float& r_var) {
  const float mu = (t0 + t1) / 2.0f, hw = (t1 - t0) / 2.0f;
  const float mu2 = mu * mu, hw2 = hw * hw, hw4 = hw2 * hw2;
  const float denom = fmaxf(1.1920928955078125e-07f, 3.0f * mu2 + hw2);
  t_mean = mu + (2.0f * mu * hw2) / denom;
  t_var = hw2 / 3.0f - (float)(4.0 / 15.0) * ((hw4 * (12.0f * mu2 - hw2)) / (denom * denom));
  r_var = (radius * radius) * ((mu2 / 4.0f + (float)(5.0 / 12.0) * hw2) - (float)(4.0 / 15.0) * hw4 / denom);
}

// Per-ray constants of the lift (render_utils.py:326-339): dsq = d^2 per axis, nul = 1 - dsq / max(1e-10, |d|^2), and dnorm = |d|
__device__ __forceinline__ void ray_consts(const float* d, float (&dsq)[3], float (&nul)[3], float& dnorm) {
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) dsq[ax] = d[ax] * d[ax];
  const float dmag = fmaxf(1e-10f, (dsq[0] + dsq[1]) + dsq[2]);
  dnorm = sqrtf((dsq[0] + dsq[1]) + dsq[2]);
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) nul[ax] = 1.0f - dsq[ax] / dmag;
}

// |d| alone (the compositing's delta = dz |d|): ray_consts' dnorm, the rest is dead code there
__device__ __forceinline__ float ray_norm(const float* d) {
  float dsq[3], nul[3], dnorm;
  ray_consts(d, dsq, nul, dnorm);
  return dnorm;
}

// Diagonal covariance of the lifted Gaussian; var_scale > 0 multiplies it (the forward kernels' option, 0 elsewhere).
// The MEAN stays with the callers on purpose: the forward kernels form d * t_mean + o from the direction rays[3:6] like the reference's
// cast_rays, the iNeRF kernels o + t_mean * v from the view direction rays[8:11], the input their backward differentiates -- two
// different inputs (equal only in the ray bundles the refinement builds), not one formula typed twice.
__device__ __forceinline__ void lift_var(float t_var, float r_var, const float (&dsq)[3], const float (&nul)[3], float var_scale, float (&var)[3]) {
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) var[ax] = t_var * dsq[ax] + r_var * nul[ax];
  if (var_scale > 0.f) {
    var[0] *= var_scale; var[1] *= var_scale; var[2] *= var_scale;
  }
}

// ---- integrated positional encoding ---------------------------------------------------------------------------------------------
// One encoding value exp(-var sc^2 / 2) sin(arg) for the scale sc = 2^i, arg = mean * sc or fl32(mean * sc + HALF_PI_F32) (formed by the
// caller: nerf_fwd.hip selects between the two, the others add a phase that is 0.f in the first half -- the same number except that
// -0 + 0.f is +0, whose encoding is a zero of the other sign).  Two flavours that differ in bits ON PURPOSE -- never mix them within one comparison:
//   ipe_exact:  expf and the fp64-reduced sine.  nerf_fwd.hip, nm_inerf_encode and the "from rays" points kernel, which are compared bit
//               for bit with each other and through the GEMM chain;
//   ipe_fast:   exp2 of the log2(e)-scaled exponent and the fp32 Cody-Waite sine sin32 (|err| <= 1e-7).  The split render kernels
//               (nerf_fwd_bf16.hip), where the 48 values per lane are exposed time in front of every tile; nm_mip_encode's arith = 1 (encode.hip) pins
//               this arithmetic against the reference: it calls sin32 and carries its OWN copy of ipe_damp_fast's expression (that
//               file's kernels are kept as they are) -- change the two together.
// fp32 sine: q = rint(x / pi), 4-term Cody-Waite reduction (q * 3.140625 is exact up to q = 2^16), odd polynomial of degree 9 (SLEEF's
// sinf coefficients).  |error| <= 1e-7 for |x| < 6.5e4 (checked against fp64 on 8e4 random arguments).
__device__ __forceinline__ float sin32(float x) {
  const float q = __builtin_rintf(x * 0.318309886183790671537767526745028724f);
  float d = __builtin_fmaf(q, -3.140625f, x);
  d = __builtin_fmaf(q, -0.0009670257568359375f, d);
  d = __builtin_fmaf(q, -6.2771141529083251953e-07f, d);
  d = __builtin_fmaf(q, -1.2154201256553420762e-10f, d);
  const float s = d * d;
  d = ((int)q & 1) ? -d : d;
  float u = 2.6083159809786593541503e-06f;
  u = __builtin_fmaf(u, s, -0.0001981069071916863322258f);
  u = __builtin_fmaf(u, s, 0.00833307858556509017944336f);
  u = __builtin_fmaf(u, s, -0.166666597127914428710938f);
  return __builtin_fmaf(s, u * d, d);
}
__device__ __forceinline__ float ipe_damp_exact(float var, float sc) { return expf(-0.5f * (var * (sc * sc))); }
__device__ __forceinline__ float ipe_damp_fast(float var, float sc) {
  return __builtin_amdgcn_exp2f((-0.5f * (var * (sc * sc))) * 1.44269504088896340736f);
}
__device__ __forceinline__ float ipe_exact(float arg, float var, float sc) { return ipe_damp_exact(var, sc) * nm_sinf(arg); }
__device__ __forceinline__ float ipe_fast(float arg, float var, float sc) { return ipe_damp_fast(var, sc) * sin32(arg); }

// ---- views-layer row ------------------------------------------------------------------------------------------------------------
// Column f of the 48-wide [direction PE | appearance] row: f = 0..11 sin(2^k v), 12..23 sin(2^k v + pi/2) (k = (f % 12) / 3), 24..26 raw v,
// 27..42 the appearance row (zeros without one), 43..47 padding.  v_ax = component f % 3 of the view direction rays[8:11].
constexpr int XI = 96;            // columns of an IPE row (90 used)
constexpr int XD = 48;            // columns of a views-layer row
constexpr int APP0 = 27, APP = 16;  // the appearance row's first column and width in it
__device__ __forceinline__ float view_row_value(int f, float v_ax, const float* app_row) {
  float v = 0.f;
  if (f < 24) {
    const float xe = v_ax * (float)(1 << ((f % 12) / 3));
    v = nm_sinf(f < 12 ? xe : xe + HALF_PI_F32);
  } else if (f < APP0) {
    v = v_ax;
  } else if (f < APP0 + APP) {
    v = app_row ? app_row[f - APP0] : 0.f;
  }
  return v;
}

// ---- the GEMM chains' input rows of one sample ----------------------------------------------------------------------------------------------
// xi [XI] = IPE (exact flavour) of the Gaussian of interval [t0, t1] of ray rp (rays row, 12 floats) with mean dir * t_mean + o | zero padding,
// xd [XD] = view_row_value.  16 threads per sample: thread i < 15 writes the six IPE columns of frequency 2^i (3 axes x {sin, sin(. + pi/2)}),
// thread 15 the view row and the padding of xi.  `dir` is the direction the MEAN reads (lift_var's comment: rays[3:6] for the training
// render, rays[8:11] for the refinement); the covariance is always that of rays[3:6].
// T: the rows' type, float or _Float16: the FINISHED fp32 value rounded once as it is stored.  The empty asm hides the value's origin from the
// compiler, which otherwise folds the conversion into the product in front of it (v_fma_mixlo_f16 rounds the exact product once): the fp16
// rows would then not be the fp32 rows rounded.
template <class T>
__device__ __forceinline__ T row_value(float v) {
  if constexpr (sizeof(T) == 2) asm volatile("" : "+v"(v));
  return (T)v;
}
template <class T>
__device__ __forceinline__ void write_sample_rows(const float* rp, const float* dir, float t0, float t1, float var_scale, const float* app_row, int i,
                                                  T* __restrict__ xi, T* __restrict__ xd) {
  if (i < 15) {
    float t_mean, t_var, r_var, dsq[3], nul[3], dnorm, var[3];
    frustum(t0, t1, rp[11], t_mean, t_var, r_var);
    ray_consts(rp + 3, dsq, nul, dnorm);
    lift_var(t_var, r_var, dsq, nul, var_scale, var);
    const float sc = (float)(1 << i);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const float mean = dir[ax] * t_mean + rp[ax];
      const float xe = mean * sc;
      xi[i * 3 + ax] = row_value<T>(ipe_exact(xe, var[ax], sc));
      xi[45 + i * 3 + ax] = row_value<T>(ipe_exact(xe + HALF_PI_F32, var[ax], sc));
    }
  } else {
#pragma unroll
    for (int f = 90; f < XI; ++f) xi[f] = (T)0.f;
    for (int c = 0; c < XD; ++c) xd[c] = row_value<T>(view_row_value(c, rp[8 + c % 3], app_row));
  }
}

// ---- alpha compositing ----------------------------------------------------------------------------------------------------------
// exp(-relu(sigma) delta), alpha = 1 - that, and the factor (1 - alpha) + 1e-10 by which a sample multiplies the transmittance behind it
__device__ __forceinline__ float attenuation(float sigma_raw, float delta) {
  const float sg = fmaxf(sigma_raw, 0.f);
  return expf(-sg * delta);
}
__device__ __forceinline__ float alpha_of(float sigma_raw, float delta) { return 1.0f - attenuation(sigma_raw, delta); }
__device__ __forceinline__ float trans_factor(float alpha) { return (1.0f - alpha) + 1e-10f; }
__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// Transmittance along the rays of one 128-sample pass of the render kernels: thread j < 128 (wavefronts 0 and 1) owns sample slot j, a
// ray owns SP = min(S, 128) consecutive slots.  Segmented inclusive product scan of u = trans_factor(alpha) over segments of min(SP, 64)
// lanes, the wavefront's last product -> totals[wave]; the CALLER's barrier (the two kernels use different ones); then the exclusive
// product in front of the lane's sample: shifted by one lane, 1 at a segment start, wavefront 0's total for wavefront 1 when a ray spans
// both, times the transmittance carried in from earlier passes of the same ray (S > 128).
constexpr int SCAN_TILE = 128;
__device__ __forceinline__ float scan_before_barrier(float u, int lane, int wave, int SP, float* totals) {
  float incl = u;
  const int seg = SP < 64 ? SP : 64;
#pragma unroll
  for (int dlt = 1; dlt < 64; dlt <<= 1) {
    const float up = __shfl_up(incl, dlt, 64);
    if (dlt < seg && (lane & (seg - 1)) >= dlt) incl *= up;
  }
  if (lane == 63) totals[wave] = incl;  // product over this wavefront's last segment (whole wave when SP >= 64)
  return incl;
}
__device__ __forceinline__ float scan_after_barrier(float incl, int lane, int wave, int SP, const float* totals, float carryT) {
  const int seg = SP < 64 ? SP : 64;
  float excl = __shfl_up(incl, 1, 64);
  if ((lane & (seg - 1)) == 0) excl = 1.f;
  if (SP == SCAN_TILE && wave == 1) excl *= totals[0];
  excl *= carryT;
  return excl;
}
// transmittance behind a whole pass (S > 128: one ray per workgroup, both wavefronts' totals)
__device__ __forceinline__ float scan_carry(float carryT, const float* totals) { return carryT * (totals[0] * totals[1]); }

// feat_comb = max: first maximum of the weights wv[0 .. n) (torch.max semantics); strict > against best_w, the best of the earlier passes
// of the ray, keeps the earliest.  Returns whether this pass holds the new best (then best_w is updated and bi is its index).
__device__ __forceinline__ bool first_max(const float* wv, int n, float& best_w, int& bi_out) {
  float bw = wv[0];
  int bi = 0;
  for (int k = 1; k < n; ++k)
    if (wv[k] > bw) { bw = wv[k]; bi = k; }
  const bool better = bw > best_w;
  if (better) best_w = bw;
  bi_out = bi;
  return better;
}

}  // namespace nmsample
