// Coarse match supervision on the device: the projections of a batch's 3-D points into the query image, the coarse cell every point falls
// into, the dense ground-truth match matrix and its (b, i, j) index triple in torch.where order.  Replaces the numpy code of the reference's
// dataset classes (nerfmatch/datasets/nerfmatch_dataset.py:302-353 and :553-583 with project_points3d, nerfmatch/utils/geometry.py:119-136),
// which builds a float32 M x N matrix per pair on the host and copies it to the device.
//
// Every point projects into at most one cell, so the (B, M, N) matrix has at most one 1 per column and is a function of the N-vector
// gt_cell: the dense output is a zero fill plus one byte store per valid point, and the sorted triple comes from a counting sort of N
// entries per batch element instead of a scan of M * N bytes.
//
// Two quirks of the reference are reproduced:
//   - a cell is visible iff min(cx, cy) > 0 && cx < W / ds && cy < H / ds: the strict `> 0` excludes cell row 0 and cell column 0;
//   - there is no depth test: a point BEHIND the camera whose (flipped) projection lands in the image counts as visible.
// Where the reference is undefined (p.z == 0, a projection that is not finite: floor(nan).astype(int64)) the point is invisible.
// The build uses -ffp-contract=off: the projection is the plain fp32 mul / add / true-division sequence written below.
#include "common.h"

#include <limits.h>

namespace {

constexpr int SUP_MAX_CELLS = 6400;  // cells of the per-batch-element LDS histogram (2 x 25 KiB); 640 x 640 px at ds = 8
constexpr int SUP_SORT_THREADS = 1024;

__device__ __forceinline__ bool fallback_valid(const int* __restrict__ fallback, int b, int M, int N) {
  if (!fallback) return false;
  const int i = fallback[2 * b], j = fallback[2 * b + 1];
  return i >= 0 && i < M && j >= 0 && j < N;
}

// a. one thread per (b, j); blockIdx.y = b, so a wavefront never straddles two batch elements.
//    p = R X + t, q = p / p.z, pix = K q  (geometry.py:130-133); c = floor(pix / ds); cell id / visibility / masks (nerfmatch_dataset.py:329-345).
//    gt_cell == nullptr: projection only.  raw_counts (may be nullptr): += valid points of batch element b (one atomic per wavefront).
__global__ void __launch_bounds__(256) project_classify_kernel(const float* __restrict__ pt3d, const float* __restrict__ Kmat,
                                                                const float* __restrict__ w2c, const uint8_t* __restrict__ pt_mask,
                                                                const uint8_t* __restrict__ im_mask, int M, int N, int H, int W, int ds,
                                                                float* __restrict__ pt2d_proj, int* __restrict__ gt_cell,
                                                                uint8_t* __restrict__ conf_gt, int* __restrict__ raw_counts) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  bool valid = false;
  if (j < N) {
    const float* Rt = w2c + (size_t)b * 12;
    const float* Kb = Kmat + (size_t)b * 9;
    const size_t n = (size_t)b * N + j;
    const float x = pt3d[3 * n], y = pt3d[3 * n + 1], z = pt3d[3 * n + 2];
    const float px = ((Rt[0] * x + Rt[1] * y) + Rt[2] * z) + Rt[3];
    const float py = ((Rt[4] * x + Rt[5] * y) + Rt[6] * z) + Rt[7];
    const float pz = ((Rt[8] * x + Rt[9] * y) + Rt[10] * z) + Rt[11];
    const float qx = px / pz, qy = py / pz, qz = pz / pz;
    const float u = (Kb[0] * qx + Kb[1] * qy) + Kb[2] * qz;
    const float v = (Kb[3] * qx + Kb[4] * qy) + Kb[5] * qz;
    pt2d_proj[2 * n] = u;
    pt2d_proj[2 * n + 1] = v;
    if (gt_cell) {
      const int Wc = W / ds, Hc = H / ds;
      const float cxf = floorf(u / (float)ds), cyf = floorf(v / (float)ds);
      // (compared as floats before the conversion: |c| beyond the int range is invisible either way)
      const bool visible = pz != 0.f && __builtin_isfinite(u) && __builtin_isfinite(v) && cxf > 0.f && cyf > 0.f && cxf < (float)Wc && cyf < (float)Hc;
      int cell = -1;
      if (visible) {
        const int i = min(max((int)cxf + (int)cyf * Wc, 0), M - 1);
        valid = (!pt_mask || pt_mask[n]) && (!im_mask || im_mask[(size_t)b * M + i]);
        if (valid) {
          cell = i;
          if (conf_gt) conf_gt[((size_t)b * M + i) * N + j] = 1;
        }
      }
      gt_cell[n] = cell;
    }
  }
  if (raw_counts) {
    const int k = __popcll(__ballot(valid));
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(raw_counts + b, k);
  }
}

// c. + d. one workgroup per batch element b: counting sort of its valid points by cell, ordered by j inside a cell.
//   1. histogram of the cells in LDS (integer atomics: the sums do not depend on the order);
//   2. exclusive scan -> first slot of every cell;
//   3. the points of a cell are dropped into the cell's slots of `tmp` in ANY order (an LDS cursor per cell);
//   4. every entry finds its rank among the entries of its cell (the number of smaller j) and is written to
//      (offset of b) + (first slot of the cell) + rank: the result depends on the SET of entries only -- the same bytes on every run.
// The offset of b = the (fallback-adjusted) counts of the batch elements before it, from project_classify_kernel's raw_counts.
// An empty element takes row b of `fallback` (i, j) as its only entry, in the triple and in the dense matrix; a row outside
// [0, M) x [0, N) is ignored.
__global__ void __launch_bounds__(SUP_SORT_THREADS) sort_triple_kernel(const int* __restrict__ gt_cell, const int* __restrict__ raw_counts,
                                                                        const int* __restrict__ fallback, int M, int N, uint8_t* __restrict__ conf_gt,
                                                                        int* __restrict__ tmp_all, int64_t* __restrict__ b_ids,
                                                                        int64_t* __restrict__ i_ids, int64_t* __restrict__ j_ids, int* __restrict__ counts) {
  __shared__ int hist[SUP_MAX_CELLS];
  __shared__ int cursor[SUP_MAX_CELLS];  // first slot of the cell, advanced to its end by step 3
  __shared__ int wsum[SUP_SORT_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* cell = gt_cell + (size_t)b * N;
  int* tmp = tmp_all + (size_t)b * N;
  int off = 0;
  for (int bb = 0; bb < b; ++bb) {
    const int c = raw_counts[bb];
    off += (c == 0 && fallback_valid(fallback, bb, M, N)) ? 1 : c;
  }
  const int total = raw_counts[b];
  if (total == 0) {  // (uniform over the workgroup)
    const bool fb = fallback_valid(fallback, b, M, N);
    if (tid == 0) {
      counts[b] = fb ? 1 : 0;
      if (fb) {
        const int i = fallback[2 * b], j = fallback[2 * b + 1];
        b_ids[off] = b;
        i_ids[off] = i;
        j_ids[off] = j;
        if (conf_gt) conf_gt[((size_t)b * M + i) * N + j] = 1;
      }
    }
    return;
  }
  for (int c = tid; c < M; c += SUP_SORT_THREADS) hist[c] = 0;
  __syncthreads();
  for (int j = tid; j < N; j += SUP_SORT_THREADS) {
    const int c = cell[j];
    if (c >= 0) atomicAdd(&hist[c], 1);
  }
  __syncthreads();
  // exclusive scan: thread t owns the `per` consecutive cells from t * per
  const int per = (M + SUP_SORT_THREADS - 1) / SUP_SORT_THREADS;
  const int c0 = min(tid * per, M), c1 = min(c0 + per, M);
  int s = 0;
  for (int c = c0; c < c1; ++c) s += hist[c];
  int incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int run = incl - s;
  for (int w = 0; w < wave; ++w) run += wsum[w];
  for (int c = c0; c < c1; ++c) {
    cursor[c] = run;
    run += hist[c];
  }
  __syncthreads();
  for (int j = tid; j < N; j += SUP_SORT_THREADS) {
    const int c = cell[j];
    if (c >= 0) tmp[atomicAdd(&cursor[c], 1)] = j;  // slot < total <= N
  }
  __syncthreads();  // (tmp is global memory written and read by this workgroup only)
  for (int k = tid; k < total; k += SUP_SORT_THREADS) {
    const int j = tmp[k], c = cell[j];
    const int end = cursor[c], beg = end - hist[c];
    int rank = 0;
    for (int t = beg; t < end; ++t) rank += tmp[t] < j;
    const size_t pos = (size_t)off + beg + rank;
    b_ids[pos] = b;
    i_ids[pos] = c;
    j_ids[pos] = j;
  }
  if (tid == 0) counts[b] = total;
}

}  // namespace

extern "C" size_t nm_gt_supervision_workspace_bytes(int B, int M, int N) {
  (void)M;
  if (B <= 0 || N <= 0) return 0;
  return ((size_t)B * N + (size_t)B) * sizeof(int);  // unordered slots of the counting sort + the raw counts
}

extern "C" int nm_gt_supervision(const float* pt3d, const float* K, const float* w2c, const uint8_t* pt_mask, const uint8_t* im_mask,
                                 const int* fallback, int B, int M, int N, int H, int W, int ds, float* pt2d_proj, int* gt_cell, uint8_t* conf_gt,
                                 int64_t* b_ids, int64_t* i_ids, int64_t* j_ids, int* counts, void* workspace, size_t workspace_bytes,
                                 nmStream_t stream) {
  NM_CHECK_ARG(pt3d && K && w2c && pt2d_proj && B > 0 && N > 0 && B <= 65535 && (size_t)B * N <= (size_t)INT_MAX);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((N + 255) / 256, B);
  if (!gt_cell) {  // projection only
    NM_CHECK_ARG(!conf_gt && !b_ids && !i_ids && !j_ids && !counts && !fallback);
    project_classify_kernel<<<grid, 256, 0, s>>>(pt3d, K, w2c, nullptr, nullptr, 0, N, 0, 0, 1, pt2d_proj, nullptr, nullptr, nullptr);
    return nm_launch_status();
  }
  NM_CHECK_ARG(M > 0 && H > 0 && W > 0 && ds > 0);
  const bool triple = b_ids || i_ids || j_ids || counts;
  if (triple) NM_CHECK_ARG(b_ids && i_ids && j_ids && counts);
  NM_CHECK_ARG(!fallback || triple);
  if (W % ds || H % ds) return NM_ERR_UNSUPPORTED;
  if (triple && M > SUP_MAX_CELLS) return NM_ERR_UNSUPPORTED;
  int* tmp = nullptr;
  int* raw_counts = nullptr;
  if (triple) {
    if (!workspace || workspace_bytes < nm_gt_supervision_workspace_bytes(B, M, N)) return NM_ERR_WORKSPACE;
    tmp = static_cast<int*>(workspace);
    raw_counts = tmp + (size_t)B * N;
    if (hipMemsetAsync(raw_counts, 0, (size_t)B * sizeof(int), s) != hipSuccess) { (void)hipGetLastError(); return NM_ERR_LAUNCH; }
  }
  if (conf_gt && hipMemsetAsync(conf_gt, 0, (size_t)B * M * N, s) != hipSuccess) { (void)hipGetLastError(); return NM_ERR_LAUNCH; }
  project_classify_kernel<<<grid, 256, 0, s>>>(pt3d, K, w2c, pt_mask, im_mask, M, N, H, W, ds, pt2d_proj, gt_cell, conf_gt, raw_counts);
  if (triple) sort_triple_kernel<<<B, SUP_SORT_THREADS, 0, s>>>(gt_cell, raw_counts, fallback, M, N, conf_gt, tmp, b_ids, i_ids, j_ids, counts);
  return nm_launch_status();
}
