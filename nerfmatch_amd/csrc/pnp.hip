// Batched PnP-RANSAC on the device: the 2D-3D matches of Q queries -> Q world-to-camera poses, in three launches.
//   a. hypotheses: one thread per (query, hypothesis): four sample indices from a counter-based hash, a P3P minimal solve of the first
//      three in fp64 (Lambda Twist, Persson & Nordberg, ECCV 2018: the cubic of the pencil D1 + g D2, the degenerate conic split into two
//      lines by the adjugate method, a quadratic per line, Gauss-Newton on the three distance constraints), the root that reprojects the
//      fourth point best; stored as the 3 x 4 matrix K [R | t] in fp32 (all NaN = no hypothesis).
//   b. scoring, the hot path (Q x n_hyps x n reprojections): a workgroup owns 64 hypotheses of one query in LDS and streams that query's
//      points, one per lane; every lane tests its point against each hypothesis (all lanes read the same LDS words: a broadcast) and the
//      wavefront's count comes from ballot + popcount.  Lane h of a wavefront carries hypothesis h's running count.  Counts are integers:
//      the LDS atomics that merge the wavefronts and the 64-bit atomicMax that picks the winner, key = (count << 32) | (0xFFFFFFFF - h),
//      give the same value in any order.
//   c. refinement: one workgroup per query, `refine_iters` Levenberg-Marquardt steps in fp64 from the winning hypothesis.  Every step
//      re-evaluates the inlier set under the current pose; the 6 x 6 normal equations are summed thread-strided over the query's own
//      matches (thread t takes matches t, t + 256, ... of the query), reduced by a fixed xor butterfly per wavefront and a fixed
//      left-to-right sum over the four wavefronts, and solved by Cholesky in thread 0.
// Nothing depends on the query's position in the batch, on the other queries or on the order in which workgroups run: a query gives the
// same bits alone and inside any batch.
// The build uses -ffp-contract=off: the fp32 reprojection of (b) is the FMA chain written below, the fp64 code is plain mul / add.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int PNP_HB = 64;               // hypotheses per scoring workgroup = lanes of a wavefront
constexpr int PNP_SCORE_THREADS = 1024;  // 16 wavefronts stream the points of the query
constexpr int PNP_REFINE_THREADS = 256;
constexpr int PNP_REFINE_WAVES = PNP_REFINE_THREADS / 64;
constexpr int PNP_NSUM = 29;             // 21 (upper triangle of J^T J) + 6 (J^T r) + cost + count
constexpr int PNP_MAX_ATTEMPTS = 64;
constexpr int PNP_GN_ITERS = 5;
constexpr double PNP_AREA_FLOOR = 1e-8;  // sin^2 of the angle at x1 of the sample triangle below which there is no hypothesis
constexpr double PNP_LAMBDA0 = 1e-3, PNP_LAMBDA_MIN = 1e-9, PNP_LAMBDA_MAX = 1e9;

__device__ __forceinline__ uint32_t pnp_hash4(uint32_t seed, uint32_t h, uint32_t slot, uint32_t attempt) {  // nm_mix32: common.h
  uint32_t v = nm_mix32(seed ^ 0x9E3779B9u);
  v = nm_mix32(v + h);
  v = nm_mix32(v + slot);
  return nm_mix32(v + attempt);
}

// the range of query q in the match arrays, clamped to [0, K]: whatever `offsets` holds, no access leaves the arrays
__device__ __forceinline__ void pnp_range(const int* __restrict__ offsets, int q, int K, int& beg, int& n) {
  beg = min(max(offsets[q], 0), K);
  n = min(max(offsets[q + 1], beg), K) - beg;
}

struct PnpCam {
  double fx, sk, cx, fy, cy;
};
__device__ __forceinline__ PnpCam pnp_cam(const float* __restrict__ Kq) {
  return PnpCam{(double)Kq[0], (double)Kq[1], (double)Kq[2], (double)Kq[4], (double)Kq[5]};
}

// adjugate and determinant of a symmetric 3 x 3 matrix, packed (00, 01, 02, 11, 12, 22)
__device__ __forceinline__ void pnp_adj_sym(const double A[6], double out[6]) {
  const double a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5];
  out[0] = d * f - e * e;
  out[1] = c * e - b * f;
  out[2] = b * e - c * d;
  out[3] = a * f - c * c;
  out[4] = b * c - a * e;
  out[5] = a * d - b * b;
}
__device__ __forceinline__ double pnp_dot_sym(const double A[6], const double B[6]) {
  return (A[0] * B[0] + A[3] * B[3] + A[5] * B[5]) + 2.0 * (A[1] * B[1] + A[2] * B[2] + A[4] * B[4]);
}
__device__ __forceinline__ void pnp_cross(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double pnp_dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// a. -------------------------------------------------------------------------------------------------------------------------------
// P3P of (y, x)[0..2] (y: unit bearings), the root chosen by (u4, v4, x4).  Returns false if there is none.  Rt: row-major [R | t].
__device__ bool pnp_p3p(const double y[3][3], const double x[3][3], const double x4[3], double u4, double v4, const PnpCam& cam, double Rt[12]) {
  double d12[3], d13[3], d23[3], cr[3];
  for (int k = 0; k < 3; ++k) {
    d12[k] = x[0][k] - x[1][k];
    d13[k] = x[0][k] - x[2][k];
    d23[k] = x[1][k] - x[2][k];
  }
  const double a12 = pnp_dot3(d12, d12), a13 = pnp_dot3(d13, d13), a23 = pnp_dot3(d23, d23);
  pnp_cross(d12, d13, cr);
  if (!(pnp_dot3(cr, cr) > PNP_AREA_FLOOR * a12 * a13)) return false;
  const double b12 = pnp_dot3(y[0], y[1]), b13 = pnp_dot3(y[0], y[2]), b23 = pnp_dot3(y[1], y[2]);
  // the two quadrics L^T D L = 0 in the depths L = (l1, l2, l3)
  const double D1[6] = {a23, -a23 * b12, 0.0, a23 - a12, a12 * b23, -a12};
  const double D2[6] = {a23, 0.0, -a23 * b13, -a13, a13 * b23, a23 - a13};
  double A1[6], A2[6];
  pnp_adj_sym(D1, A1);
  pnp_adj_sym(D2, A2);
  // det(D1 + g D2) = c0 + c1 g + c2 g^2 + c3 g^3
  const double c0 = D1[0] * A1[0] + D1[1] * A1[1] + D1[2] * A1[2], c3 = D2[0] * A2[0] + D2[1] * A2[1] + D2[2] * A2[2];
  const double c1 = pnp_dot_sym(A1, D2), c2 = pnp_dot_sym(D1, A2);
  const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
  const double q = (a * a - 3.0 * b) / 9.0, r = (2.0 * a * a * a - 9.0 * a * b + 27.0 * c) / 54.0;
  const double disc = r * r - q * q * q;
  double g;
  if (disc < 0.0) {  // three real roots: the smallest
    const double th = acos(fmax(-1.0, fmin(1.0, r / sqrt(q * q * q))));
    g = -2.0 * sqrt(q) * cos(th / 3.0) - a / 3.0;
  } else {
    const double A = -copysign(cbrt(fabs(r) + sqrt(disc)), r);
    g = A + (A != 0.0 ? q / A : 0.0) - a / 3.0;
  }
  for (int it = 0; it < 2; ++it) {  // Newton polish
    const double f = ((g + a) * g + b) * g + c, fp = (3.0 * g + 2.0 * a) * g + b;
    if (fp != 0.0) g -= f / fp;
  }
  if (!isfinite(g)) return false;
  // D0 = D1 + g D2 has rank 2: two lines l, m with D0 ~ l m^T + m l^T.  -adj(D0) = p p^T with p = l x m; D0 + [p]x has rank 1.
  double D0[6], Bs[6];
  for (int k = 0; k < 6; ++k) D0[k] = D1[k] + g * D2[k];
  pnp_adj_sym(D0, Bs);
  for (int k = 0; k < 6; ++k) Bs[k] = -Bs[k];
  const double Bm[3][3] = {{Bs[0], Bs[1], Bs[2]}, {Bs[1], Bs[3], Bs[4]}, {Bs[2], Bs[4], Bs[5]}};
  int bi = 0;
  if (Bm[1][1] > Bm[bi][bi]) bi = 1;
  if (Bm[2][2] > Bm[bi][bi]) bi = 2;
  if (!(Bm[bi][bi] > 0.0)) return false;  // a pair of complex lines: no real root
  const double sp = sqrt(Bm[bi][bi]);
  const double p[3] = {Bm[0][bi] / sp, Bm[1][bi] / sp, Bm[2][bi] / sp};
  const double C[3][3] = {{D0[0], D0[1] - p[2], D0[2] + p[1]}, {D0[1] + p[2], D0[3], D0[4] - p[0]}, {D0[2] - p[1], D0[4] + p[0], D0[5]}};
  int cj = 0, ck = 0;
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 3; ++k)
      if (fabs(C[j][k]) > fabs(C[cj][ck])) { cj = j; ck = k; }
  const double lines[2][3] = {{C[cj][0], C[cj][1], C[cj][2]}, {C[0][ck], C[1][ck], C[2][ck]}};
  double X[3][3], Xi[3][3], cx12[3];  // X = [d12, d23, d12 x d23] (columns), Xi = its inverse
  pnp_cross(d12, d23, cx12);
  for (int k = 0; k < 3; ++k) {
    X[k][0] = d12[k];
    X[k][1] = d23[k];
    X[k][2] = cx12[k];
  }
  {
    const double det = X[0][0] * (X[1][1] * X[2][2] - X[1][2] * X[2][1]) - X[0][1] * (X[1][0] * X[2][2] - X[1][2] * X[2][0]) +
                       X[0][2] * (X[1][0] * X[2][1] - X[1][1] * X[2][0]);
    const double id = 1.0 / det;
    Xi[0][0] = (X[1][1] * X[2][2] - X[1][2] * X[2][1]) * id;
    Xi[0][1] = (X[0][2] * X[2][1] - X[0][1] * X[2][2]) * id;
    Xi[0][2] = (X[0][1] * X[1][2] - X[0][2] * X[1][1]) * id;
    Xi[1][0] = (X[1][2] * X[2][0] - X[1][0] * X[2][2]) * id;
    Xi[1][1] = (X[0][0] * X[2][2] - X[0][2] * X[2][0]) * id;
    Xi[1][2] = (X[0][2] * X[1][0] - X[0][0] * X[1][2]) * id;
    Xi[2][0] = (X[1][0] * X[2][1] - X[1][1] * X[2][0]) * id;
    Xi[2][1] = (X[0][1] * X[2][0] - X[0][0] * X[2][1]) * id;
    Xi[2][2] = (X[0][0] * X[1][1] - X[0][1] * X[1][0]) * id;
  }
  bool found = false;
  double best = INFINITY;
  for (int li = 0; li < 2; ++li) {
    const double* v = lines[li];
    if (v[0] == 0.0) continue;
    const double w0 = -v[1] / v[0], w1 = -v[2] / v[0];  // l1 = w0 l2 + w1 l3
    const double qa = a23 * w1 * w1 - a12;
    const double qb = a23 * (2.0 * w0 * w1 - 2.0 * b12 * w1) + 2.0 * a12 * b23;
    const double qc = a23 * (w0 * w0 - 2.0 * b12 * w0 + 1.0) - a12;
    const double dq = qb * qb - 4.0 * qa * qc;
    if (!(dq >= 0.0)) continue;
    const double qq = -0.5 * (qb + copysign(sqrt(dq), qb));
    const double taus[2] = {qq / qa, qc / qq};
    for (int ti = 0; ti < 2; ++ti) {
      const double tau = taus[ti];  // l3 / l2
      if (!(isfinite(tau) && tau > 0.0)) continue;
      double l2 = sqrt(a23 / (tau * (tau - 2.0 * b23) + 1.0));
      double l1 = (w0 + w1 * tau) * l2, l3 = tau * l2;
      if (!(l1 > 0.0)) continue;
      for (int it = 0; it < PNP_GN_ITERS; ++it) {
        const double r1 = l1 * l1 + l2 * l2 - 2.0 * b12 * l1 * l2 - a12, r2 = l1 * l1 + l3 * l3 - 2.0 * b13 * l1 * l3 - a13,
                     r3 = l2 * l2 + l3 * l3 - 2.0 * b23 * l2 * l3 - a23;
        const double j00 = 2.0 * l1 - 2.0 * b12 * l2, j01 = 2.0 * l2 - 2.0 * b12 * l1, j10 = 2.0 * l1 - 2.0 * b13 * l3,
                     j12 = 2.0 * l3 - 2.0 * b13 * l1, j21 = 2.0 * l2 - 2.0 * b23 * l3, j22 = 2.0 * l3 - 2.0 * b23 * l2;
        // J = [j00 j01 0; j10 0 j12; 0 j21 j22]
        const double det = -j00 * j12 * j21 - j01 * j10 * j22;
        if (det == 0.0) break;
        const double id = 1.0 / det;
        l1 -= (-j12 * j21 * r1 - j01 * j22 * r2 + j01 * j12 * r3) * id;
        l2 -= (-j10 * j22 * r1 + j00 * j22 * r2 - j00 * j12 * r3) * id;
        l3 -= (j10 * j21 * r1 - j00 * j21 * r2 - j01 * j10 * r3) * id;
      }
      if (!(isfinite(l1) && isfinite(l2) && isfinite(l3) && l1 > 0.0 && l2 > 0.0 && l3 > 0.0)) continue;
      double e1[3], e2[3], e3[3], R[3][3], t[3];
      for (int k = 0; k < 3; ++k) {
        e1[k] = l1 * y[0][k] - l2 * y[1][k];
        e2[k] = l2 * y[1][k] - l3 * y[2][k];
      }
      pnp_cross(e1, e2, e3);
      for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) R[i][k] = e1[i] * Xi[0][k] + e2[i] * Xi[1][k] + e3[i] * Xi[2][k];
      for (int i = 0; i < 3; ++i) t[i] = l1 * y[0][i] - pnp_dot3(R[i], x[0]);
      const double px = pnp_dot3(R[0], x4) + t[0], py = pnp_dot3(R[1], x4) + t[1], pz = pnp_dot3(R[2], x4) + t[2];
      if (!(pz > 0.0)) continue;
      const double xn = px / pz, yn = py / pz;
      const double du = cam.fx * xn + cam.sk * yn + cam.cx - u4, dv = cam.fy * yn + cam.cy - v4;
      const double err = du * du + dv * dv;
      if (err < best) {
        best = err;
        found = true;
        for (int i = 0; i < 3; ++i) {
          Rt[4 * i] = R[i][0];
          Rt[4 * i + 1] = R[i][1];
          Rt[4 * i + 2] = R[i][2];
          Rt[4 * i + 3] = t[i];
        }
      }
    }
  }
  return found;
}

__global__ void __launch_bounds__(PNP_HB) pnp_hypotheses_kernel(const float* __restrict__ pt2d, const float* __restrict__ pt3d,
                                                                 const int* __restrict__ offsets, const float* __restrict__ Kmat, int K,
                                                                 int n_hyps, uint32_t seed, float half, float* __restrict__ hyp_P) {
  const int q = blockIdx.y, h = blockIdx.x * PNP_HB + threadIdx.x;
  int beg, n;
  pnp_range(offsets, q, K, beg, n);
  float P[12];
  for (int k = 0; k < 12; ++k) P[k] = __builtin_nanf("");
  if (n >= 4) {
    int idx[4];
    for (int slot = 0; slot < 4; ++slot) {
      int attempt = 0, i;
      for (;;) {
        bool dup;
        if (attempt >= PNP_MAX_ATTEMPTS) {  // the smallest unused index
          for (i = 0;; ++i) {
            dup = false;
            for (int s = 0; s < slot; ++s) dup |= idx[s] == i;
            if (!dup) break;
          }
          break;
        }
        i = (int)(pnp_hash4(seed, (uint32_t)h, (uint32_t)slot, (uint32_t)attempt) % (uint32_t)n);
        dup = false;
        for (int s = 0; s < slot; ++s) dup |= idx[s] == i;
        if (!dup) break;
        ++attempt;
      }
      idx[slot] = i;
    }
    const PnpCam cam = pnp_cam(Kmat + (size_t)q * 9);
    double y[3][3], x[4][3], u4 = 0.0, v4 = 0.0;
    for (int s = 0; s < 4; ++s) {
      const size_t m = (size_t)beg + idx[s];
      const double u = (double)(pt2d[2 * m] + half), v = (double)(pt2d[2 * m + 1] + half);
      for (int k = 0; k < 3; ++k) x[s][k] = (double)pt3d[3 * m + k];
      if (s < 3) {
        const double yn = (v - cam.cy) / cam.fy, xn = (u - cam.cx - cam.sk * yn) / cam.fx;
        const double nrm = sqrt(xn * xn + yn * yn + 1.0);
        y[s][0] = xn / nrm;
        y[s][1] = yn / nrm;
        y[s][2] = 1.0 / nrm;
      } else {
        u4 = u;
        v4 = v;
      }
    }
    double Rt[12];
    if (pnp_p3p(y, x, x[3], u4, v4, cam, Rt)) {
      bool finite = true;
      for (int k = 0; k < 4; ++k) {
        P[k] = (float)(cam.fx * Rt[k] + cam.sk * Rt[4 + k] + cam.cx * Rt[8 + k]);
        P[4 + k] = (float)(cam.fy * Rt[4 + k] + cam.cy * Rt[8 + k]);
        P[8 + k] = (float)Rt[8 + k];
        finite = finite && __builtin_isfinite(P[k]) && __builtin_isfinite(P[4 + k]) && __builtin_isfinite(P[8 + k]);
      }
      if (!finite)
        for (int k = 0; k < 12; ++k) P[k] = __builtin_nanf("");
    }
  }
  float* out = hyp_P + ((size_t)q * n_hyps + h) * 12;
  for (int k = 0; k < 12; ++k) out[k] = P[k];
}

// b. -------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PNP_SCORE_THREADS) pnp_score_kernel(const float* __restrict__ pt2d, const float* __restrict__ pt3d,
                                                                       const int* __restrict__ offsets, const float* __restrict__ hyp_P, int K,
                                                                       int n_hyps, float thr2, float half, int* __restrict__ hyp_count,
                                                                       unsigned long long* __restrict__ best_key) {
  __shared__ float sP[PNP_HB * 12];
  __shared__ int sCnt[PNP_HB];
  const int q = blockIdx.y, h0 = blockIdx.x * PNP_HB, tid = threadIdx.x, lane = tid & 63;
  int beg, n;
  pnp_range(offsets, q, K, beg, n);
  if (tid < PNP_HB * 12) sP[tid] = hyp_P[((size_t)q * n_hyps + h0) * 12 + tid];
  if (tid < PNP_HB) sCnt[tid] = 0;
  __syncthreads();
  int mine = 0;  // lane h: inliers of hypothesis h0 + h among the points this wavefront has seen
  for (int base = 0; base < n; base += PNP_SCORE_THREADS) {
    const int i = base + tid;
    const bool valid = i < n;
    const size_t m = (size_t)beg + (valid ? i : 0);  // (n > 0 here: beg is a match of the query)
    const float u = pt2d[2 * m] + half, v = pt2d[2 * m + 1] + half;
    const float X = pt3d[3 * m], Y = pt3d[3 * m + 1], Z = pt3d[3 * m + 2];
#pragma unroll 8
    for (int h = 0; h < PNP_HB; ++h) {
      const float* P = sP + h * 12;
      const float a = NM_FMA(P[0], X, NM_FMA(P[1], Y, NM_FMA(P[2], Z, P[3])));
      const float b = NM_FMA(P[4], X, NM_FMA(P[5], Y, NM_FMA(P[6], Z, P[7])));
      const float w = NM_FMA(P[8], X, NM_FMA(P[9], Y, NM_FMA(P[10], Z, P[11])));
      const float r = 1.0f / w;
      const float du = NM_FMA(a, r, -u), dv = NM_FMA(b, r, -v);
      const float e2 = NM_FMA(du, du, dv * dv);
      const int c = wave_count(valid && w > 0.f && e2 <= thr2);  // (a NaN hypothesis compares false: it scores 0)
      if (lane == h) mine += c;
    }
  }
  if (mine) atomicAdd(&sCnt[lane], mine);
  __syncthreads();
  if (tid < PNP_HB) {
    const int cnt = sCnt[tid];
    hyp_count[(size_t)q * n_hyps + h0 + tid] = cnt;
    atomicMax(best_key + q, ((unsigned long long)(uint32_t)cnt << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(h0 + tid)));
  }
}

// c. -------------------------------------------------------------------------------------------------------------------------------
struct PnpPose {
  double R[9], t[3];
};

// residual of one match under a pose; returns whether it is an inlier
__device__ __forceinline__ bool pnp_residual(const PnpPose& p, const PnpCam& cam, double X, double Y, double Z, double u, double v, double thr2,
                                             double Xc[3], double& iz, double& xn, double& yn, double& ru, double& rv, double& e2) {
  Xc[0] = p.R[0] * X + p.R[1] * Y + p.R[2] * Z + p.t[0];
  Xc[1] = p.R[3] * X + p.R[4] * Y + p.R[5] * Z + p.t[1];
  Xc[2] = p.R[6] * X + p.R[7] * Y + p.R[8] * Z + p.t[2];
  iz = 1.0 / Xc[2];
  xn = Xc[0] * iz;
  yn = Xc[1] * iz;
  ru = cam.fx * xn + cam.sk * yn + cam.cx - u;
  rv = cam.fy * yn + cam.cy - v;
  e2 = ru * ru + rv * rv;
  return Xc[2] > 0.0 && e2 <= thr2;
}

// sums of nv per-thread values over the workgroup, in a fixed order: xor butterfly inside a wavefront (a + b == b + a, so every lane holds
// the same bits), then wavefront 0 + 1 + 2 + 3 left to right.  The totals are left in sTot.
__device__ __forceinline__ void pnp_block_sum(double* v, int nv, double (*sRed)[PNP_NSUM], double* sTot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = 0; k < nv; ++k) {
    double s = v[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) sRed[wave][k] = s;
  }
  __syncthreads();
  if (tid < nv) {
    double s = sRed[0][tid];
    for (int w = 1; w < PNP_REFINE_WAVES; ++w) s += sRed[w][tid];
    sTot[tid] = s;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(PNP_REFINE_THREADS) pnp_refine_kernel(const float* __restrict__ pt2d, const float* __restrict__ pt3d,
                                                                         const int* __restrict__ offsets, const float* __restrict__ Kmat,
                                                                         const float* __restrict__ hyp_P,
                                                                         const unsigned long long* __restrict__ best_key, int K, int n_hyps,
                                                                         double thr2, float half, int refine_iters, float* __restrict__ pose,
                                                                         int* __restrict__ n_inliers, uint8_t* __restrict__ inlier_mask) {
  __shared__ double sRed[PNP_REFINE_WAVES][PNP_NSUM];
  __shared__ double sTot[PNP_NSUM];
  __shared__ double sCand[12];
  __shared__ int sOk;
  const int q = blockIdx.x, tid = threadIdx.x;
  int beg, n;
  pnp_range(offsets, q, K, beg, n);
  const unsigned long long key = best_key[q];
  const int win_count = (int)(key >> 32), win = (int)(0xFFFFFFFFu - (uint32_t)key);
  const PnpCam cam = pnp_cam(Kmat + (size_t)q * 9);
  PnpPose cur;
  bool have = n >= 4 && win_count >= 4 && win < n_hyps;
  if (have) {  // [R | t] = K^-1 P, the rows of R made orthonormal (Gram-Schmidt: row 0, row 1, their cross product)
    const float* P = hyp_P + ((size_t)q * n_hyps + win) * 12;
    double m0[4], m1[4], m2[4];
    for (int k = 0; k < 4; ++k) {
      m2[k] = (double)P[8 + k];
      m1[k] = ((double)P[4 + k] - cam.cy * m2[k]) / cam.fy;
      m0[k] = ((double)P[k] - cam.sk * m1[k] - cam.cx * m2[k]) / cam.fx;
    }
    const double n0 = sqrt(pnp_dot3(m0, m0));
    double r0[3], r1[3], r2[3];
    for (int k = 0; k < 3; ++k) r0[k] = m0[k] / n0;
    const double d01 = pnp_dot3(r0, m1);
    for (int k = 0; k < 3; ++k) r1[k] = m1[k] - d01 * r0[k];
    const double n1 = sqrt(pnp_dot3(r1, r1));
    for (int k = 0; k < 3; ++k) r1[k] = r1[k] / n1;
    pnp_cross(r0, r1, r2);
    for (int k = 0; k < 3; ++k) {
      cur.R[k] = r0[k];
      cur.R[3 + k] = r1[k];
      cur.R[6 + k] = r2[k];
    }
    cur.t[0] = m0[3];
    cur.t[1] = m1[3];
    cur.t[2] = m2[3];
    for (int k = 0; k < 9; ++k) have = have && isfinite(cur.R[k]);
    for (int k = 0; k < 3; ++k) have = have && isfinite(cur.t[k]);
  }
  if (!have) {  // (uniform over the workgroup) no pose: identity, the winner's count (< 4, or 0), an empty mask
    if (tid == 0) {
      for (int k = 0; k < 12; ++k) pose[(size_t)q * 12 + k] = (k % 5 == 0) ? 1.f : 0.f;
      n_inliers[q] = (n >= 4 && win_count < 4) ? win_count : 0;
    }
    return;  // (the mask was zero-filled on the stream)
  }
  double lambda = PNP_LAMBDA0;
  for (int it = 0; it < refine_iters; ++it) {
    // pass A: the inlier set S of the current pose and its normal equations
    double acc[PNP_NSUM];
    for (int k = 0; k < PNP_NSUM; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += PNP_REFINE_THREADS) {
      const size_t m = (size_t)beg + i;
      const double u = (double)(pt2d[2 * m] + half), v = (double)(pt2d[2 * m + 1] + half);
      const double X = (double)pt3d[3 * m], Y = (double)pt3d[3 * m + 1], Z = (double)pt3d[3 * m + 2];
      double Xc[3], iz, xn, yn, ru, rv, e2;
      if (!pnp_residual(cur, cam, X, Y, Z, u, v, thr2, Xc, iz, xn, yn, ru, rv, e2)) continue;
      const double du[3] = {cam.fx * iz, cam.sk * iz, -(cam.fx * xn + cam.sk * yn) * iz};  // d u / d X_c
      const double dv[3] = {0.0, cam.fy * iz, -cam.fy * yn * iz};
      double Ju[6], Jv[6];  // X_c <- exp(w) X_c + t': d X_c = w x X_c + t'  ->  d/dw = X_c x (row), d/dt' = row
      pnp_cross(Xc, du, Ju);
      pnp_cross(Xc, dv, Jv);
      for (int k = 0; k < 3; ++k) {
        Ju[3 + k] = du[k];
        Jv[3 + k] = dv[k];
      }
      int s = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) acc[s++] += Ju[a] * Ju[b] + Jv[a] * Jv[b];
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[21 + a] += Ju[a] * ru + Jv[a] * rv;
      acc[27] += e2;
      acc[28] += 1.0;
    }
    pnp_block_sum(acc, PNP_NSUM, sRed, sTot);
    const double cost = sTot[27], cnt = sTot[28];
    if (tid == 0) {  // (H + lambda diag H) d = -g by Cholesky; the candidate pose
      double A[6][6], g[6], d[6];
      int s = 0;
      for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
          A[a][b] = A[b][a] = sTot[s];
          ++s;
        }
      for (int a = 0; a < 6; ++a) {
        g[a] = -sTot[21 + a];
        A[a][a] += lambda * A[a][a];
      }
      bool ok = cnt >= 3.0;
      for (int j = 0; j < 6 && ok; ++j) {  // A = L L^T, L in the lower triangle
        double sdiag = A[j][j];
        for (int k = 0; k < j; ++k) sdiag -= A[j][k] * A[j][k];
        if (!(sdiag > 0.0) || !isfinite(sdiag)) {
          ok = false;
          break;
        }
        const double ljj = sqrt(sdiag);
        A[j][j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
          double sv = A[i][j];
          for (int k = 0; k < j; ++k) sv -= A[i][k] * A[j][k];
          A[i][j] = sv / ljj;
        }
      }
      if (ok) {
        for (int i = 0; i < 6; ++i) {
          double sv = g[i];
          for (int k = 0; k < i; ++k) sv -= A[i][k] * d[k];
          d[i] = sv / A[i][i];
        }
        for (int i = 5; i >= 0; --i) {
          double sv = d[i];
          for (int k = i + 1; k < 6; ++k) sv -= A[k][i] * d[k];
          d[i] = sv / A[i][i];
        }
        for (int i = 0; i < 6; ++i) ok = ok && isfinite(d[i]);
      }
      if (ok) {  // E = exp([w]x) (Rodrigues), R' = E R, t' = E t + t'
        const double wx = d[0], wy = d[1], wz = d[2];
        const double th2 = wx * wx + wy * wy + wz * wz;
        double ca, cb;
        if (th2 < 1e-8) {
          ca = 1.0 - th2 / 6.0;
          cb = 0.5 - th2 / 24.0;
        } else {
          const double th = sqrt(th2);
          ca = sin(th) / th;
          cb = (1.0 - cos(th)) / th2;
        }
        const double W[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
        double E[9];
        for (int i = 0; i < 3; ++i)
          for (int k = 0; k < 3; ++k) {
            const double w2 = W[3 * i] * W[k] + W[3 * i + 1] * W[3 + k] + W[3 * i + 2] * W[6 + k];
            E[3 * i + k] = (i == k ? 1.0 : 0.0) + ca * W[3 * i + k] + cb * w2;
          }
        for (int i = 0; i < 3; ++i) {
          for (int k = 0; k < 3; ++k) sCand[4 * i + k] = E[3 * i] * cur.R[k] + E[3 * i + 1] * cur.R[3 + k] + E[3 * i + 2] * cur.R[6 + k];
          sCand[4 * i + 3] = E[3 * i] * cur.t[0] + E[3 * i + 1] * cur.t[1] + E[3 * i + 2] * cur.t[2] + d[3 + i];
        }
      }
      sOk = ok ? 1 : 0;
    }
    __syncthreads();
    bool accept = sOk != 0;  // (uniform)
    PnpPose cand;
    if (accept) {
      for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) cand.R[3 * i + k] = sCand[4 * i + k];
        cand.t[i] = sCand[4 * i + 3];
      }
      // pass B: the candidate's inlier count, and the cost of S under it (a member of S behind the camera: no acceptance)
      double accB[3] = {0.0, 0.0, 0.0};
      for (int i = tid; i < n; i += PNP_REFINE_THREADS) {
        const size_t m = (size_t)beg + i;
        const double u = (double)(pt2d[2 * m] + half), v = (double)(pt2d[2 * m + 1] + half);
        const double X = (double)pt3d[3 * m], Y = (double)pt3d[3 * m + 1], Z = (double)pt3d[3 * m + 2];
        double Xc[3], iz, xn, yn, ru, rv, e2, XcN[3], e2N;
        const bool inS = pnp_residual(cur, cam, X, Y, Z, u, v, thr2, Xc, iz, xn, yn, ru, rv, e2);
        const bool inN = pnp_residual(cand, cam, X, Y, Z, u, v, thr2, XcN, iz, xn, yn, ru, rv, e2N);
        if (inN) accB[0] += 1.0;
        if (inS) {
          if (XcN[2] > 0.0) accB[1] += e2N;
          else accB[2] += 1.0;
        }
      }
      pnp_block_sum(accB, 3, sRed, sTot);
      accept = sTot[0] >= cnt && sTot[2] == 0.0 && sTot[1] < cost;
    }
    __syncthreads();  // (sTot / sCand are rewritten by the next step)
    if (accept) {
      cur = cand;
      lambda = fmax(lambda / 10.0, PNP_LAMBDA_MIN);
    } else {
      lambda = fmin(lambda * 10.0, PNP_LAMBDA_MAX);
    }
  }
  // the final inlier set
  double fin[1] = {0.0};
  for (int i = tid; i < n; i += PNP_REFINE_THREADS) {
    const size_t m = (size_t)beg + i;
    const double u = (double)(pt2d[2 * m] + half), v = (double)(pt2d[2 * m + 1] + half);
    double Xc[3], iz, xn, yn, ru, rv, e2;
    const bool in = pnp_residual(cur, cam, (double)pt3d[3 * m], (double)pt3d[3 * m + 1], (double)pt3d[3 * m + 2], u, v, thr2, Xc, iz, xn, yn, ru, rv, e2);
    if (inlier_mask) inlier_mask[m] = in ? 1 : 0;
    fin[0] += in ? 1.0 : 0.0;
  }
  pnp_block_sum(fin, 1, sRed, sTot);
  if (sTot[0] < 4.0) {  // (uniform) the refined pose keeps fewer than 4 inliers in the fp64 recount: no pose, as the header promises
    if (inlier_mask)
      for (int i = tid; i < n; i += PNP_REFINE_THREADS) inlier_mask[(size_t)beg + i] = 0;  // (each thread clears what it wrote itself)
    if (tid == 0) {
      for (int k = 0; k < 12; ++k) pose[(size_t)q * 12 + k] = (k % 5 == 0) ? 1.f : 0.f;
      n_inliers[q] = (int)sTot[0];
    }
    return;
  }
  if (tid == 0) {
    n_inliers[q] = (int)sTot[0];
    for (int i = 0; i < 3; ++i) {
      for (int k = 0; k < 3; ++k) pose[(size_t)q * 12 + 4 * i + k] = (float)cur.R[3 * i + k];
      pose[(size_t)q * 12 + 4 * i + 3] = (float)cur.t[i];
    }
  }
}

}  // namespace

extern "C" size_t nm_pnp_ransac_workspace_bytes(int Q, int n_hyps) {
  if (Q <= 0 || n_hyps <= 0) return 0;
  return (size_t)Q * sizeof(unsigned long long) + (size_t)Q * n_hyps * (12 * sizeof(float) + sizeof(int));
}

extern "C" int nm_pnp_ransac(const float* pt2d, const float* pt3d, const int* offsets, const int* offsets_host, const float* Kmat, int Q, int K,
                             float thr_px, int n_hyps, int refine_iters, uint32_t seed, int add_half_px, float* pose, int* n_inliers,
                             uint8_t* inlier_mask, float* hyp_pose, int* hyp_count, void* workspace, size_t workspace_bytes,
                             nmStream_t stream) {
  NM_CHECK_ARG(offsets && Kmat && pose && n_inliers && Q > 0 && Q <= 65535 && K >= 0);
  NM_CHECK_ARG((pt2d && pt3d) || K == 0);
  NM_CHECK_ARG(thr_px > 0.f && thr_px < INFINITY && refine_iters >= 0);
  NM_CHECK_ARG(n_hyps >= PNP_HB && n_hyps <= 4096 && n_hyps % PNP_HB == 0);
  if (offsets_host) {  // the host's copy of the offsets, when the caller has one: checked before anything is enqueued
    NM_CHECK_ARG(offsets_host[0] >= 0 && offsets_host[Q] <= K);
    for (int q = 0; q < Q; ++q) NM_CHECK_ARG(offsets_host[q] <= offsets_host[q + 1]);
  }
  if (!workspace || workspace_bytes < nm_pnp_ransac_workspace_bytes(Q, n_hyps)) return NM_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* best_key = static_cast<unsigned long long*>(workspace);
  float* ws_P = reinterpret_cast<float*>(best_key + Q);
  int* ws_count = reinterpret_cast<int*>(ws_P + (size_t)Q * n_hyps * 12);
  float* P = hyp_pose ? hyp_pose : ws_P;
  int* counts = hyp_count ? hyp_count : ws_count;
  const float half = add_half_px ? 0.5f : 0.f;
  if (hipMemsetAsync(best_key, 0, (size_t)Q * sizeof(unsigned long long), s) != hipSuccess) { (void)hipGetLastError(); return NM_ERR_LAUNCH; }
  if (inlier_mask && K > 0 && hipMemsetAsync(inlier_mask, 0, (size_t)K, s) != hipSuccess) { (void)hipGetLastError(); return NM_ERR_LAUNCH; }
  const dim3 grid(n_hyps / PNP_HB, Q);
  pnp_hypotheses_kernel<<<grid, PNP_HB, 0, s>>>(pt2d, pt3d, offsets, Kmat, K, n_hyps, seed, half, P);
  pnp_score_kernel<<<grid, PNP_SCORE_THREADS, 0, s>>>(pt2d, pt3d, offsets, P, K, n_hyps, thr_px * thr_px, half, counts, best_key);
  pnp_refine_kernel<<<Q, PNP_REFINE_THREADS, 0, s>>>(pt2d, pt3d, offsets, Kmat, P, best_key, K, n_hyps, (double)thr_px * (double)thr_px, half,
                                                     refine_iters, pose, n_inliers, inlier_mask);
  return nm_launch_status();
}
