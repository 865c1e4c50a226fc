// NeRF scene training (reference: NerfRenderer.render_rays with validation=False, nerfmatch/nerf/renderer.py:182-295;
// volume_render_radiance_field, nerf/render_utils.py:176-230; t_to_s / g, render_utils.py:618-636; compute_nerf_metrics and
// lossfun_distortion, nerfmatch/utils/metrics.py:59-96, :448-465): the per-ray kernels of a training step.  The two MLPs run on the GEMM
// kernels (nm_linear*, nm_linear_wgrad*); what is here sits in front of, between and behind those chains:
//   nm_nerf_train_encode          rays, fence posts, per-ray appearance id -> the chains' input rows xi | xd (nerf_sample.h's write_sample_rows)
//   (nm_nerf_composite4(_bwd), nerf_composite.hip: the chains' output rows -> rgb, depth, acc, weights with the density noise, and back)
//   nm_nerf_distortion(_bwd)      s = t_to_s(t) with the batch-wide near / far, the mip-NeRF-360 distortion loss of (s, weights), and back
//   nm_nerf_photo_loss            the two masked MSE terms and their gradients
//   nm_nerf_app_grad              d loss / d appearance table from the chains' d loss / d xd, summed in a fixed order
// No gradient flows through t, the frustum Gaussians or the encodings (the samplers run under no_grad with stop_grad=True,
// render_utils.py:299-310, :581-597), so none of these kernels has a backward towards the rays.
#include "nerf_sample.h"

namespace {
using nmsample::XI, nmsample::XD, nmsample::APP0, nmsample::APP, nmsample::write_sample_rows;

constexpr int MAX_S = 1024;  // samples per ray of nm_nerf_distortion(_bwd): a workgroup's four rays keep u and w in LDS

__device__ __forceinline__ int clamp_id(long long id, int V) { return id < 0 ? 0 : (id >= V ? V - 1 : (int)id); }

// 16 threads per sample, write_sample_rows' roles; thread 15 also looks up the ray's appearance row.  T = float, or _Float16: the same values
// rounded once (the fp16 training walk's input rows)
template <class T>
__global__ void train_encode_kernel(const float* __restrict__ rays, const float* __restrict__ t, int R, int S, const long long* __restrict__ ray_id,
                                    const float* __restrict__ table, int V, float var_scale, T* __restrict__ xi, T* __restrict__ xd,
                                    int* __restrict__ status) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = idx >> 4;
  const int i = (int)(idx & 15);
  if (n >= (size_t)R * S) return;
  const int r = (int)(n / S), s = (int)(n % S);
  const float* rp = rays + (size_t)r * 12;
  const float* tr = t + (size_t)r * (S + 1) + s;
  const float* app_row = nullptr;
  if (table && i == 15) {
    const long long id = ray_id ? ray_id[r] : 1;  // (no ids: the reference's default id 1, renderer.py:298-299)
    if ((id < 0 || id >= V) && s == 0 && status) atomicAdd(status, 1);
    app_row = table + (size_t)clamp_id(id, V) * APP;
  }
  write_sample_rows(rp, rp + 3, tr[0], tr[1], var_scale, app_row, i, xi + n * XI, xd + n * XD);  // (cast_rays: d * t_mean + o with d = rays[3:6])
}

// ---- s = t_to_s(t, min t, max t) and the distortion loss ----------------------------------------------------------------------------------
constexpr int MM_BLOCKS = 256;  // partial (min, max) pairs of the batch-wide reduction

__global__ void __launch_bounds__(256) minmax_partial_kernel(const float* __restrict__ t, size_t total, float* __restrict__ part) {
  __shared__ float lo_s[4], hi_s[4];
  float lo = INFINITY, hi = -INFINITY;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const float v = t[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { lo_s[threadIdx.x >> 6] = lo; hi_s[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = fminf(fminf(lo_s[0], lo_s[1]), fminf(lo_s[2], lo_s[3]));
    part[2 * blockIdx.x + 1] = fmaxf(fmaxf(hi_s[0], hi_s[1]), fmaxf(hi_s[2], hi_s[3]));
  }
}

// The reference's g(x) adds its eps IN PLACE (render_utils.py:630-636), so in (g(t) - g(near)) / (g(far) - g(near)) the 0-d tensor `near`
// has had the eps added once when the numerator reads it and twice when the denominator does.  fp32 additions, as there.
__global__ void __launch_bounds__(256) t_to_s_kernel(const float* __restrict__ t, size_t total, const float* __restrict__ part, int nparts,
                                                     float* __restrict__ s) {
  float lo = INFINITY, hi = -INFINITY;
  for (int k = 0; k < nparts; ++k) {  // (every thread: 2 x 256 floats from L2, uniform addresses)
    lo = fminf(lo, part[2 * k]);
    hi = fmaxf(hi, part[2 * k + 1]);
  }
  const float eps = 1e-6f;
  const float n1 = lo + eps, n2 = n1 + eps, f1 = hi + eps;
  const float den = 1.0f / f1 - 1.0f / n2;
  const float gn = 1.0f / n1;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) s[i] = (1.0f / (t[i] + eps) - gn) / den;
}

// Per ray: inner_i = sum_j w_j |u_i - u_j| over the interval midpoints u of s (lossfun_distortion).  One wavefront per ray, u and w of the ray
// in LDS, lane = samples lane, lane + 64, ...; the sum over j is sequential in j (a fixed order).
//   forward:  loss_ray = sum_i w_i inner_i + sum_i w_i^2 (s_{i+1} - s_i) / 3
//   backward: g_w_i = scale * (2 inner_i + 2 w_i (s_{i+1} - s_i) / 3)
template <bool BWD>
__global__ void __launch_bounds__(256) distortion_kernel(const float* __restrict__ s, const float* __restrict__ w, int R, int S, float scale,
                                                          float* __restrict__ out) {
  extern __shared__ float lds[];  // 4 rays x (u[S], w[S])
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.x * 4 + wave;
  const bool live = r < R;  // (wavefront-uniform)
  float* us = lds + (size_t)wave * 2 * S;
  float* ws = us + S;
  const float* sr = s + (size_t)(live ? r : 0) * (S + 1);
  const float* wr = w + (size_t)(live ? r : 0) * S;
  for (int i = lane; i < S; i += 64) {
    us[i] = (sr[i + 1] + sr[i]) / 2.0f;
    ws[i] = wr[i];
  }
  __syncthreads();
  if (!live) return;
  float total = 0.f;
  for (int i = lane; i < S; i += 64) {
    const float ui = us[i], wi = ws[i];
    float inner = 0.f;
    for (int j = 0; j < S; ++j) inner += ws[j] * fabsf(ui - us[j]);
    const float ds = sr[i + 1] - sr[i];
    if constexpr (BWD) out[(size_t)r * S + i] = scale * (2.0f * inner + (2.0f * wi) * ds / 3.0f);
    else total += wi * inner + (wi * wi) * ds / 3.0f;
  }
  if constexpr (!BWD) {
    total = wave_sum(total);
    if (lane == 0) out[r] = total;
  }
}

// mean of v[0 .. n) in fp64, one workgroup, fixed order (thread-strided partial sums, then a tree over LDS)
__global__ void __launch_bounds__(256) mean_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
  __shared__ double red[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += (double)v[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(red[0] / (double)n);
}

// ---- photometric loss -----------------------------------------------------------------------------------------------------------------------
// acc[0] = 0.5 mean(mask (rgb_c - gt)^2), acc[1] = the same for rgb_f (means over the R x 3 elements, metrics.py:74, :80);
// g_rgb_c = coarse_weight mask (rgb_c - gt) / (3 R), g_rgb_f = mask (rgb_f - gt) / (3 R): the gradients of coarse_weight acc[0] + acc[1].
__global__ void __launch_bounds__(1024) photo_loss_kernel(const float* __restrict__ rgb_c, const float* __restrict__ rgb_f, const float* __restrict__ gt,
                                                           const float* __restrict__ mask, float coarse_weight, int R, double* __restrict__ acc,
                                                           float* __restrict__ g_c, float* __restrict__ g_f) {
  __shared__ double red[2][1024];
  const int total = R * 3;
  const float inv = 1.0f / (float)total;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < total; i += 1024) {
    const float m = mask ? mask[i / 3] : 1.0f;
    const float dc = rgb_c[i] - gt[i], df = rgb_f[i] - gt[i];
    a += (double)(m * (dc * dc));
    b += (double)(m * (df * df));
    if (g_c) g_c[i] = coarse_weight * (m * dc) * inv;
    if (g_f) g_f[i] = (m * df) * inv;
  }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] += red[1][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    acc[0] = 0.5 * red[0][0] / (double)total;
    acc[1] = 0.5 * red[1][0] / (double)total;
  }
}

// ---- appearance-table gradient ------------------------------------------------------------------------------------------------------------
// g_ray[r][c] = sum_s (g_xd_a + g_xd_b)[r * S + s][27 + c]: one wavefront per ray, lane = (row group of 4, column), rows in order, then the four
// groups in a fixed tree
__global__ void __launch_bounds__(256) app_ray_sum_kernel(const float* __restrict__ ga, const float* __restrict__ gb, int R, int S,
                                                           float* __restrict__ g_ray) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int c = lane & 15, grp = lane >> 4;
  float sum = 0.f;
  for (int s = grp; s < S; s += 4) {
    const size_t e = ((size_t)r * S + s) * XD + APP0 + c;
    float v = ga[e];
    if (gb) v += gb[e];
    sum += v;
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (grp == 0) g_ray[(size_t)r * APP + c] = sum;
}
// g_table[v][c] += sum over the rays with id v, in ray order within each of 16 strided groups, the groups in a fixed tree: one workgroup per row
__global__ void __launch_bounds__(256) app_table_kernel(const float* __restrict__ g_ray, const long long* __restrict__ ray_id, int R, int V,
                                                         float* __restrict__ g_table) {
  __shared__ float red[16][APP + 1];
  const int v = blockIdx.x, c = threadIdx.x & 15, k = threadIdx.x >> 4;
  float sum = 0.f;
  for (int r = k; r < R; r += 16)
    if (clamp_id(ray_id ? ray_id[r] : 1, V) == v) sum += g_ray[(size_t)r * APP + c];
  red[k][c] = sum;
  __syncthreads();
  for (int off = 8; off > 0; off >>= 1) {
    if (k < off) red[k][c] += red[k + off][c];
    __syncthreads();
  }
  if (k == 0) g_table[(size_t)v * APP + c] += red[0][c];
}

}  // namespace

extern "C" int nm_nerf_train_encode(const float* rays, const float* t, int R, int S, const long long* ray_id, const long long* ray_id_host,
                                    const float* table, int V, float var_scale, float* xi, float* xd, int* status, nmStream_t stream) {
  NM_CHECK_ARG(rays && t && xi && xd && R > 0 && S > 0 && (!table || V > 0) && (size_t)R * S * 16 / 256 < 0x7fffffffu);
  if (table && ray_id_host)
    for (int r = 0; r < R; ++r) NM_CHECK_ARG(ray_id_host[r] >= 0 && ray_id_host[r] < V);
  const size_t total = (size_t)R * S * 16;
  train_encode_kernel<float><<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(rays, t, R, S, ray_id, table, V, var_scale, xi, xd, status);
  return nm_launch_status();
}

extern "C" int nm_nerf_train_encode_f16(const float* rays, const float* t, int R, int S, const long long* ray_id, const long long* ray_id_host,
                                        const float* table, int V, float var_scale, void* xi, void* xd, int* status, nmStream_t stream) {
  NM_CHECK_ARG(rays && t && xi && xd && R > 0 && S > 0 && (!table || V > 0) && (size_t)R * S * 16 / 256 < 0x7fffffffu);
  if (table && ray_id_host)
    for (int r = 0; r < R; ++r) NM_CHECK_ARG(ray_id_host[r] >= 0 && ray_id_host[r] < V);
  const size_t total = (size_t)R * S * 16;
  train_encode_kernel<_Float16><<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(rays, t, R, S, ray_id, table, V, var_scale, (_Float16*)xi,
                                                                                                (_Float16*)xd, status);
  return nm_launch_status();
}

extern "C" size_t nm_nerf_distortion_workspace_bytes(void) { return (size_t)MM_BLOCKS * 2 * sizeof(float); }

extern "C" int nm_nerf_distortion(const float* t, int t_is_s, const float* weights, int R, int S, void* workspace, float* s, float* loss_ray,
                                  float* loss_mean, nmStream_t stream) {
  NM_CHECK_ARG(t && R > 0 && S > 0 && (t_is_s || (s && workspace)) && (!weights || loss_ray) && (!loss_mean || loss_ray));
  if (S > MAX_S) return NM_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)R * (S + 1);
  if (!t_is_s) {
    const int blocks = (int)(total / 1024 + 1 < (size_t)MM_BLOCKS ? total / 1024 + 1 : (size_t)MM_BLOCKS);
    minmax_partial_kernel<<<blocks, 256, 0, st>>>(t, total, (float*)workspace);
    t_to_s_kernel<<<blocks, 256, 0, st>>>(t, total, (const float*)workspace, blocks, s);
  }
  if (weights) {
    const float* sv = t_is_s ? t : s;
    distortion_kernel<false><<<(R + 3) / 4, 256, (size_t)4 * 2 * S * sizeof(float), st>>>(sv, weights, R, S, 0.f, loss_ray);
    if (loss_mean) mean_kernel<<<1, 256, 0, st>>>(loss_ray, R, loss_mean);
  }
  return nm_launch_status();
}

extern "C" int nm_nerf_distortion_bwd(const float* s, const float* weights, int R, int S, float scale, float* g_weights, nmStream_t stream) {
  NM_CHECK_ARG(s && weights && g_weights && R > 0 && S > 0);
  if (S > MAX_S) return NM_ERR_UNSUPPORTED;
  distortion_kernel<true><<<(R + 3) / 4, 256, (size_t)4 * 2 * S * sizeof(float), (hipStream_t)stream>>>(s, weights, R, S, scale / (float)R, g_weights);
  return nm_launch_status();
}

extern "C" int nm_nerf_photo_loss(const float* rgb_c, const float* rgb_f, const float* gt, const float* mask, float coarse_weight, int R, double* acc,
                                  float* g_rgb_c, float* g_rgb_f, nmStream_t stream) {
  NM_CHECK_ARG(rgb_c && rgb_f && gt && acc && R > 0 && R < (1 << 29));
  photo_loss_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(rgb_c, rgb_f, gt, mask, coarse_weight, R, acc, g_rgb_c, g_rgb_f);
  return nm_launch_status();
}

extern "C" int nm_nerf_app_grad(const float* g_xd_a, const float* g_xd_b, const long long* ray_id, int R, int S, int V, float* g_ray, float* g_table,
                                nmStream_t stream) {
  NM_CHECK_ARG(g_xd_a && g_ray && g_table && R > 0 && S > 0 && V > 0 && V <= 65535);
  hipStream_t st = (hipStream_t)stream;
  app_ray_sum_kernel<<<(R + 3) / 4, 256, 0, st>>>(g_xd_a, g_xd_b, R, S, g_ray);
  app_table_kernel<<<V, 256, 0, st>>>(g_ray, ray_id, R, V, g_table);
  return nm_launch_status();
}
