// Differentiable compositing along a ray, one WAVEFRONT per ray, for the iNeRF refinement (nerfmatch/nerfmatch_evaluator.py:394-418) and for
// NeRF scene training (volume_render_radiance_field, nerf/render_utils.py:176-230) alike: nm_nerf_composite4 / nm_nerf_composite4_bwd on the
// MLP's own output rows out4 [n, 4] = rgb logits | raw sigma (what nm_nerf_points_fwd*_bf16x3 and the GEMM chain write).  A lane takes the
// samples lane, lane + 64, ...; the transmittance is a prefix product over lanes (six shuffle steps per 64 samples, carry between chunks),
// the backward's B_s = sum_{j > s} q_j w_j a suffix sum the same way; one 16-byte load and one 16-byte store per sample.  (The
// one-thread-per-ray pair nm_inerf_composite / _bwd walks 128 dependent iterations on 75 wavefronts of a 1024-SIMD chip: 58 + 66 us per
// step at 4800 rays.)  The products / sums associate differently from a sequential loop (a scan tree): results agree to rounding.
// Options, all per launch: density noise (training), either background, S_act < S (refinement: the zero-width tail is not evaluated),
// depth / acc / weights out, d loss / d weights in, g_d = the gradient through delta = dz |d| (refinement).
#include "nerf_sample.h"

namespace {
using nmsample::ray_norm, nmsample::attenuation, nmsample::trans_factor, nmsample::sigmoid;

constexpr int MAX_CHUNKS = 16;  // of 64 samples: the backward keeps the transmittance at the start of every chunk in registers

struct Sample {
  float raw, dz, delta, ex, alpha, u;
  f32x4 o;
};
// raw = raw sigma + noise * noise_std (render_utils.py:189-194: the noise is formed first, then added); its sign is the density gate
__device__ __forceinline__ Sample sample_of(const float* __restrict__ out4, const float* __restrict__ tr, const float* __restrict__ noise,
                                            float noise_std, size_t n, int sidx, bool valid, float dn) {
  Sample c;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  c.o = valid ? *reinterpret_cast<const f32x4*>(out4 + n * 4) : zero4;
  c.raw = c.o[3];
  if (noise && valid) c.raw = c.raw + noise[n] * noise_std;
  c.dz = valid ? tr[sidx + 1] - tr[sidx] : 0.f;
  c.delta = c.dz * dn;
  c.ex = attenuation(c.raw, c.delta);
  c.alpha = valid ? 1.0f - c.ex : 0.f;  // (alpha_of's expression, from the ex the backward needs anyway)
  c.u = trans_factor(c.alpha);
  return c;
}
// inclusive prefix product over the lanes; returns it, *excl = the exclusive one (1 in lane 0)
__device__ __forceinline__ float prefix_prod(float u, int lane, float* excl) {
  float p = u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float up = __shfl_up(p, d, 64);
    if (lane >= d) p *= up;
  }
  const float e = __shfl_up(p, 1, 64);
  *excl = lane == 0 ? 1.0f : e;
  return p;
}

// AUX: depth and / or acc are wanted.  A template parameter and not a NULL check: with the sum for depth compiled in, the refinement's launch
// (neither wanted) measured 9 % slower than the kernel it replaces (profiles/r9_per_ray_refactor.log)
template <bool AUX>
__global__ void __launch_bounds__(256) composite4_kernel(const float* __restrict__ out4, const float* __restrict__ t, const float* __restrict__ rays,
                                                          const float* __restrict__ noise, float noise_std, int white_bg, int R, int S, int Sa,
                                                          float* __restrict__ rgb, float* __restrict__ depth, float* __restrict__ acc_out,
                                                          float* __restrict__ w_out) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* tr = t + (size_t)r * (S + 1);
  const float dn = ray_norm(rays + (size_t)r * 12 + 3);
  float T0 = 1.f, acc = 0.f, dep = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
  for (int base = 0; base < Sa; base += 64) {
    const int sidx = base + lane;
    const bool valid = sidx < Sa;
    const size_t n = (size_t)r * Sa + sidx;
    const Sample c = sample_of(out4, tr, noise, noise_std, n, sidx, valid, dn);
    float excl;
    const float p = prefix_prod(c.u, lane, &excl);
    const float w = c.alpha * (T0 * excl);
    if (valid) {
      if (w_out) w_out[n] = w;
      if constexpr (AUX) dep += w * (0.5f * (tr[sidx] + tr[sidx + 1]));
    }
    c0 += w * sigmoid(c.o[0]); c1 += w * sigmoid(c.o[1]); c2 += w * sigmoid(c.o[2]);
    acc += w;
    T0 *= __shfl(p, 63, 64);
  }
  acc = wave_sum(acc); c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2);
  if constexpr (AUX) dep = wave_sum(dep);
  if (lane == 0) {
    const float bg = white_bg ? 1.0f - acc : 0.f;
    rgb[(size_t)r * 3] = c0 + bg;
    rgb[(size_t)r * 3 + 1] = c1 + bg;
    rgb[(size_t)r * 3 + 2] = c2 + bg;
    if constexpr (AUX) {
      if (depth) depth[r] = dep;
      if (acc_out) acc_out[r] = acc;
    }
  }
}

// rgb = sum_s w_s (c_s - bg) + bg, w_s = alpha_s T_s, T_s = prod_{j<s} u_j, u = 1 - alpha + 1e-10:  g4 = d loss / d (rgb logits, raw sigma),
// g_d = d loss / d rays[:, 3:6] through delta = dz |d|
__global__ void __launch_bounds__(256) composite4_bwd_kernel(const float* __restrict__ out4, const float* __restrict__ t, const float* __restrict__ rays,
                                                              const float* __restrict__ noise, float noise_std, int white_bg,
                                                              const float* __restrict__ G, const float* __restrict__ g_w, int R, int S, int Sa,
                                                              float* __restrict__ g4, float* __restrict__ g_d) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* rp = rays + (size_t)r * 12;
  const float* tr = t + (size_t)r * (S + 1);
  const float dn = ray_norm(rp + 3);
  const float G0 = G[(size_t)r * 3], G1 = G[(size_t)r * 3 + 1], G2 = G[(size_t)r * 3 + 2];
  const float bg = white_bg ? 1.0f : 0.f;
  float carry[MAX_CHUNKS];  // forward sweep: the transmittance at the start of every chunk
  const int nchunk = (Sa + 63) / 64;
  {
    float T0 = 1.f;
#pragma unroll
    for (int k = 0; k < MAX_CHUNKS; ++k) {
      carry[k] = T0;
      if (k < nchunk) {
        const int sidx = k * 64 + lane;
        const Sample c = sample_of(out4, tr, noise, noise_std, (size_t)r * Sa + sidx, sidx, sidx < Sa, dn);
        float excl;
        T0 *= __shfl(prefix_prod(c.u, lane, &excl), 63, 64);
      }
    }
  }
  float Bc = 0.f, gnorm = 0.f;  // Bc = sum of q w over the chunks behind this one
#pragma unroll
  for (int k = MAX_CHUNKS - 1; k >= 0; --k) {
    if (k >= nchunk) continue;
    const int sidx = k * 64 + lane;
    const bool valid = sidx < Sa;
    const size_t n = (size_t)r * Sa + sidx;
    const Sample c = sample_of(out4, tr, noise, noise_std, n, sidx, valid, dn);
    float excl;
    prefix_prod(c.u, lane, &excl);
    const float Ts = carry[k] * excl;
    const float w = c.alpha * Ts;
    const float s0 = sigmoid(c.o[0]), s1 = sigmoid(c.o[1]), s2 = sigmoid(c.o[2]);
    float q = (G0 * (s0 - bg) + G1 * (s1 - bg)) + G2 * (s2 - bg);  // d loss / d w_s
    if (g_w && valid) q += g_w[n];
    float sfx = valid ? q * w : 0.f;  // inclusive suffix sum over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float dnv = __shfl_down(sfx, d, 64);
      if (lane + d < 64) sfx += dnv;
    }
    const float nxt = __shfl_down(sfx, 1, 64);
    const float B = Bc + (lane == 63 ? 0.f : nxt);
    const float g_alpha = q * Ts - B / c.u;
    if (valid) {
      f32x4 g;
      g[0] = G0 * w * (s0 * (1.0f - s0));
      g[1] = G1 * w * (s1 * (1.0f - s1));
      g[2] = G2 * w * (s2 * (1.0f - s2));
      g[3] = c.raw > 0.f ? g_alpha * (c.delta * c.ex) : 0.f;
      *reinterpret_cast<f32x4*>(g4 + n * 4) = g;
      gnorm += g_alpha * (fmaxf(c.raw, 0.f) * c.ex) * c.dz;
    }
    Bc += __shfl(sfx, 0, 64);
  }
  if (!g_d) return;
  gnorm = wave_sum(gnorm);
  if (lane == 0) {
    const float inv = dn > 0.f ? 1.0f / dn : 0.f;
    g_d[(size_t)r * 3] = gnorm * rp[3] * inv;
    g_d[(size_t)r * 3 + 1] = gnorm * rp[4] * inv;
    g_d[(size_t)r * 3 + 2] = gnorm * rp[5] * inv;
  }
}

}  // namespace

extern "C" int nm_nerf_composite4(const float* out4, const float* t, const float* rays, const float* noise, float noise_std, int white_bg, int R,
                                  int S, int S_act, float* rgb, float* depth, float* acc, float* weights, nmStream_t stream) {
  NM_CHECK_ARG(out4 && t && rays && rgb && R > 0 && S > 0 && S_act > 0 && S_act <= S);
  if (S_act > 64 * MAX_CHUNKS) return NM_ERR_UNSUPPORTED;
  auto kernel = depth || acc ? composite4_kernel<true> : composite4_kernel<false>;
  kernel<<<(R + 3) / 4, 256, 0, (hipStream_t)stream>>>(out4, t, rays, noise, noise_std, white_bg, R, S, S_act, rgb, depth, acc, weights);
  return nm_launch_status();
}

extern "C" int nm_nerf_composite4_bwd(const float* out4, const float* t, const float* rays, const float* noise, float noise_std, int white_bg,
                                      const float* g_rgb, const float* g_weights, int R, int S, int S_act, float* g_out4, float* g_d,
                                      nmStream_t stream) {
  NM_CHECK_ARG(out4 && t && rays && g_rgb && g_out4 && R > 0 && S > 0 && S_act > 0 && S_act <= S);
  if (S_act > 64 * MAX_CHUNKS) return NM_ERR_UNSUPPORTED;
  composite4_bwd_kernel<<<(R + 3) / 4, 256, 0, (hipStream_t)stream>>>(out4, t, rays, noise, noise_std, white_bg, g_rgb, g_weights, R, S, S_act,
                                                                      g_out4, g_d);
  return nm_launch_status();
}
