// Covisibility pair lists from a device-resident scene cache (covis_pairs.py).  Matcher training reads for every query frame the
// reference frames that see the same part of the scene (`train_pair_txt`, parsed by load_retrieval_pairs / load_topk_retrieval_pairs,
// nerfmatch/datasets/data_loading.py:94-127); the reference takes those lists from the sparse model of an SfM toolchain.  The cache
// holds the same information: pt3d [F,n,3] are every frame's rendered points in ray order -- a depth map per frame -- and cams [F,21]
// one camera row per frame (ref_bank.hip's rows).  score[i,j] = how many of frame j's masked points frame i sees is F^2 n projections:
//
//   self_depth  one thread per point: p.z of the point under its own frame's camera -- the depth map the occlusion test reads, with
//               NaN where the point's own mask is clear, so that the test is one 4-byte gather
//   scores      one workgroup per (reference frame j, tile of NM_COVIS_QUERY_TILE query cameras): the tile's camera rows are staged in
//               LDS once and read uniformly; frame j's points go through registers in blocks of COVIS_POINT_BLOCK per thread, each block
//               loaded once and tested against all cameras of the tile; a camera's count is ballot + popcount per wavefront, kept by
//               lane (camera's slot) of that wavefront; the four wavefronts' sums are combined through LDS and every score is written
//               by one thread
//   topk        one workgroup per score row: k rounds of an arg-max over the packed key (score << 32) | (F - 1 - j), each round below the
//               key of the round before it -- score descending, then index ascending, whatever the order the keys are visited in
//
// Unlike ref_bank.hip's visibility and supervision.hip there IS a depth-sign test (p.z > 0): those two reproduce a quirk of the
// reference, a pair list must not pair frames that look in opposite directions.  All counts are integers, nothing is accumulated with
// atomics and every output element has exactly one writer: two runs give the same bytes.  The build uses -ffp-contract=off; the
// projection is supervision.hip's fp32 mul / add / true-division sequence.
#include "common.h"

#include <limits.h>

namespace {

constexpr int COVIS_MAX_FRAMES = 1 << 20;
constexpr int COVIS_MAX_POINTS = 1 << 20;
constexpr int COVIS_MAX_K = 64;
constexpr int COVIS_MAX_SIDE = 8192;
constexpr long long COVIS_MAX_SCORES = 1ll << 31;
constexpr int COVIS_THREADS = 256;
constexpr int COVIS_WAVES = COVIS_THREADS / 64;
constexpr int COVIS_POINT_BLOCK = 4;  // points per thread held in registers across the tile's cameras (12 floats + 4 mask bits)
constexpr int COVIS_TILE = NM_COVIS_QUERY_TILE;
static_assert(COVIS_TILE <= 64, "a wavefront keeps the count of camera t of the tile in lane t");

// a frame id clamped into the bank (nothing read from memory can make a kernel leave the tables)
__device__ __forceinline__ int covis_frame(int f, int F) { return f < 0 ? 0 : (f >= F ? F - 1 : f); }

// p = R X + t of project_points3d (nerfmatch/utils/geometry.py:130-133) in supervision.py::_project_torch's order
__device__ __forceinline__ float covis_row(const float* Rt, float x, float y, float z) { return ((Rt[0] * x + Rt[1] * y) + Rt[2] * z) + Rt[3]; }

// floor(a / d) for 0 <= a < 2^26 and 0 < d <= 8192 with rd = 1.f / d: the fp32 estimate is within 1 of the quotient (three roundings of
// 2^-24 each on a quotient below 2^13), the remainder corrects it.  A third of the instructions of a division by a run-time divisor.
// (Restated in numpy and compared with the integer quotient at a = q d - 1, q d and q d + 1 for every d <= 8192 and q <= 8192.)
__device__ __forceinline__ int covis_div(int a, int d, float rd) {
  int q = (int)((float)a * rd);
  const int r = a - q * d;
  q += r >= d ? 1 : 0;
  q -= r < 0 ? 1 : 0;
  return q;
}

// grid (F, ceil(n / 256)): zself[f, r] = p.z of point r of frame f under camera f; with pt_mask, NaN where the point's mask is clear
__global__ void __launch_bounds__(COVIS_THREADS) covis_self_depth_kernel(const float* __restrict__ pt3d, const uint8_t* __restrict__ pt_mask,
                                                                         const float* __restrict__ cams, int n, float* __restrict__ zself) {
  const int f = blockIdx.x, r = blockIdx.y * COVIS_THREADS + threadIdx.x;
  if (r >= n) return;
  const float* Rt = cams + (size_t)f * 21 + 9;
  const size_t i = (size_t)f * n + r;
  const float pz = covis_row(Rt + 8, pt3d[i * 3], pt3d[i * 3 + 1], pt3d[i * 3 + 2]);
  zself[i] = pt_mask && !pt_mask[i] ? __builtin_nanf("") : pz;
}

// grid (F, ceil(Q / COVIS_TILE)).  DEPTH: the occlusion test against the query frame's own depth map (zself, gw x gh cells).
// A point is seen by a camera iff p.z > 0 and 0 <= x < W, 0 <= y < H for pix = K (p / p.z).  The rule also asks for a finite pix: the
// four comparisons hold for finite numbers only.  q.z = p.z / p.z is not formed: it is exactly 1 for every finite p.z > 0, where
// K[2] * 1 is K[2]; for p.z = +inf it is NaN and the point is not seen, which the test p.z < inf restates.
template <bool DEPTH>
__global__ void __launch_bounds__(COVIS_THREADS) covis_scores_kernel(const float* __restrict__ pt3d, const uint8_t* __restrict__ pt_mask,
                                                                     const float* __restrict__ cams, const int* __restrict__ rows,
                                                                     const float* __restrict__ zself, int F, int n, int Q, float img_w,
                                                                     float img_h, int W, int H, float inv_w, float inv_h, int gw, int gh,
                                                                     float depth_tol, int* __restrict__ scores) {
  __shared__ float cam[COVIS_TILE * 21];
  __shared__ int cam_frame[COVIS_TILE];
  __shared__ int wcnt[COVIS_WAVES][COVIS_TILE];
  const int j = blockIdx.x, q0 = blockIdx.y * COVIS_TILE, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = min(COVIS_TILE, Q - q0);  // cameras of this tile (>= 1 by the grid)
  for (int t = tid; t < T * 21; t += COVIS_THREADS) {
    const int s = t / 21;
    const int f = covis_frame(rows ? rows[q0 + s] : q0 + s, F);
    cam[t] = cams[(size_t)f * 21 + (t - s * 21)];
    if (t == s * 21) cam_frame[s] = f;
  }
  __syncthreads();
  const float* P = pt3d + (size_t)j * n * 3;
  const uint8_t* M = pt_mask + (size_t)j * n;
  int acc = 0;  // lane t: this wavefront's count for camera t of the tile
#pragma unroll 1
  for (int base = 0; base < n; base += COVIS_THREADS * COVIS_POINT_BLOCK) {
    float x[COVIS_POINT_BLOCK], y[COVIS_POINT_BLOCK], z[COVIS_POINT_BLOCK];
    bool m[COVIS_POINT_BLOCK];
#pragma unroll
    for (int u = 0; u < COVIS_POINT_BLOCK; ++u) {
      const int r = base + u * COVIS_THREADS + tid;
      const bool in = r < n;
      const int rr = in ? r : 0;
      x[u] = P[(size_t)rr * 3 + 0];
      y[u] = P[(size_t)rr * 3 + 1];
      z[u] = P[(size_t)rr * 3 + 2];
      m[u] = in && M[rr] != 0;
    }
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
      // the camera row once per block of points: the same LDS address in every lane.  k = diag(W / w_f, H / h_f, 1) K_f rows 0 and 1,
      // w = rows 0..2 of the world-to-camera matrix
      float k[6], w[12];
#pragma unroll
      for (int i = 0; i < 6; ++i) k[i] = cam[t * 21 + i];
#pragma unroll
      for (int i = 0; i < 12; ++i) w[i] = cam[t * 21 + 9 + i];
      const float* zq_map = DEPTH ? zself + (size_t)cam_frame[t] * n : nullptr;
      bool seen[COVIS_POINT_BLOCK];
      // straight-line code: every comparison is evaluated and the results are combined as lane masks (no short-circuit branches)
#pragma unroll
      for (int u = 0; u < COVIS_POINT_BLOCK; ++u) {
        const float px = covis_row(w, x[u], y[u], z[u]);
        const float py = covis_row(w + 4, x[u], y[u], z[u]);
        const float pz = covis_row(w + 8, x[u], y[u], z[u]);
        const float qx = px / pz, qy = py / pz;
        const float px2 = (k[0] * qx + k[1] * qy) + k[2];
        const float py2 = (k[3] * qx + k[4] * qy) + k[5];
        seen[u] = m[u] & (pz > 0.f) & (pz < __builtin_inff()) & (px2 >= 0.f) & (py2 >= 0.f) & (px2 < img_w) & (py2 < img_h);
        if (DEPTH) {
          // the cell of the truncated pixel: 0 <= xi < W and 0 <= yi < H give 0 <= cell < gw gh = n; a point that is not seen reads
          // cell 0.  One 4-byte gather per point: a cell whose own mask is clear holds NaN (nm_covis_self_depth) and fails zq > 0.
          const int xi = seen[u] ? (int)px2 : 0, yi = seen[u] ? (int)py2 : 0;
          const float zq = zq_map[min(covis_div(yi * gh, H, inv_h) * gw + covis_div(xi * gw, W, inv_w), n - 1)];
          seen[u] = seen[u] & (zq > 0.f) & (fabsf(pz - zq) <= depth_tol * zq);
        }
      }
      int c = 0;
#pragma unroll
      for (int u = 0; u < COVIS_POINT_BLOCK; ++u) c += wave_count(seen[u]);
      acc += lane == t ? c : 0;
    }
  }
  if (lane < COVIS_TILE) wcnt[wave][lane] = acc;
  __syncthreads();
  if (tid < T) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < COVIS_WAVES; ++w) s += wcnt[w][tid];
    scores[(size_t)(q0 + tid) * F + j] = s;
  }
}

// the larger key over the 64 lanes of a wavefront, in every lane
__device__ __forceinline__ long long covis_wave_max(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long other = __shfl_xor(v, o, 64);
    v = other > v ? other : v;
  }
  return v;
}

// grid (Q).  Round i takes the largest key below the key of round i - 1 among the candidates j != the row's own frame with
// score >= min_score; keys of different j differ, so k rounds list the k best by (score descending, index ascending).  The row is
// re-read every round: F * 4 bytes from L2.
__global__ void __launch_bounds__(COVIS_THREADS) covis_topk_kernel(const int* __restrict__ scores, const int* __restrict__ rows, int F, int k,
                                                                   int min_score, int* __restrict__ ids, int* __restrict__ n_pairs) {
  __shared__ long long wbest[2][COVIS_WAVES];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int self = rows ? rows[q] : q;
  const int* row = scores + (size_t)q * F;
  long long prev = LLONG_MAX;
  int found = 0;
  for (int i = 0; i < k; ++i) {
    long long best = -1;
    if (prev >= 0) {  // (uniform: prev is the same in every thread)
      for (int j = tid; j < F; j += COVIS_THREADS) {
        const int s = row[j];
        const long long key = ((long long)s << 32) | (long long)(F - 1 - j);
        if (j != self && s >= min_score && s >= 0 && key < prev && key > best) best = key;
      }
    }
    best = covis_wave_max(best);
    const int buf = i & 1;  // two buffers: the writes of round i + 1 do not meet the reads of round i, one barrier per round
    if (lane == 0) wbest[buf][wave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < COVIS_WAVES; ++w) best = wbest[buf][w] > best ? wbest[buf][w] : best;
    if (tid == 0) ids[(size_t)q * k + i] = best >= 0 ? F - 1 - (int)(best & 0xFFFFFFFFll) : -1;
    found += best >= 0 ? 1 : 0;
    prev = best;
  }
  if (tid == 0) n_pairs[q] = found;
}

}  // namespace

extern "C" int nm_covis_self_depth(const float* pt3d, const uint8_t* pt_mask, const float* cams, int F, int n, float* zself, nmStream_t stream) {
  NM_CHECK_ARG(pt3d && cams && zself && F > 0 && n > 0);
  if (F > COVIS_MAX_FRAMES || n > COVIS_MAX_POINTS) return NM_ERR_UNSUPPORTED;
  covis_self_depth_kernel<<<dim3(F, (n + COVIS_THREADS - 1) / COVIS_THREADS), COVIS_THREADS, 0, (hipStream_t)stream>>>(pt3d, pt_mask, cams, n, zself);
  return nm_launch_status();
}

extern "C" int nm_covis_scores(const float* pt3d, const uint8_t* pt_mask, const float* cams, const int* rows, const float* zself, int F, int n,
                               int Q, int img_w, int img_h, int gw, int gh, float depth_tol, int* scores, nmStream_t stream) {
  NM_CHECK_ARG(pt3d && pt_mask && cams && scores && F > 0 && n > 0 && Q > 0 && img_w > 0 && img_h > 0);
  if (zself) {
    NM_CHECK_ARG(gw > 0 && gh > 0 && (long long)gw * gh == (long long)n && depth_tol >= 0.f && depth_tol < __builtin_inff());
  } else {
    NM_CHECK_ARG(gw == 0 && gh == 0);
  }
  if (F > COVIS_MAX_FRAMES || n > COVIS_MAX_POINTS || Q > COVIS_MAX_FRAMES || (long long)Q * F > COVIS_MAX_SCORES || img_w > COVIS_MAX_SIDE ||
      img_h > COVIS_MAX_SIDE || gw > COVIS_MAX_SIDE || gh > COVIS_MAX_SIDE)
    return NM_ERR_UNSUPPORTED;
  const dim3 grid(F, (Q + COVIS_TILE - 1) / COVIS_TILE);  // (Q <= 2^20: at most 32768 tiles)
  if (zself)
    covis_scores_kernel<true><<<grid, COVIS_THREADS, 0, (hipStream_t)stream>>>(pt3d, pt_mask, cams, rows, zself, F, n, Q, (float)img_w,
                                                                                (float)img_h, img_w, img_h, 1.f / (float)img_w, 1.f / (float)img_h, gw, gh, depth_tol,
                                                                                scores);
  else
    covis_scores_kernel<false><<<grid, COVIS_THREADS, 0, (hipStream_t)stream>>>(pt3d, pt_mask, cams, rows, nullptr, F, n, Q, (float)img_w,
                                                                                 (float)img_h, img_w, img_h, 0.f, 0.f, 0, 0, 0.f, scores);
  return nm_launch_status();
}

extern "C" int nm_covis_topk(const int* scores, const int* rows, int Q, int F, int k, int min_score, int* ids, int* n_pairs, nmStream_t stream) {
  NM_CHECK_ARG(scores && ids && n_pairs && Q > 0 && F > 0 && k > 0);
  if (k > COVIS_MAX_K || F > COVIS_MAX_FRAMES || (long long)Q * F > COVIS_MAX_SCORES) return NM_ERR_UNSUPPORTED;
  covis_topk_kernel<<<Q, COVIS_THREADS, 0, (hipStream_t)stream>>>(scores, rows, F, k, min_score, ids, n_pairs);
  return nm_launch_status();
}
