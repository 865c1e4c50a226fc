// The per-pixel expressions of a ray row, defined once for the localisation grid (rays.hip: nm_raygen*) and the training ray bank
// (ray_bank.hip: nm_raybank_*): camera-to-world direction, unit-sphere discriminant, far plane and cone radius.  Two kernels that call
// these on the same pixel of the same camera produce the same bits (the build uses -ffp-contract=off; every fma is explicit).
// Reference: get_ray_dirs / get_rays_c2w (nerfmatch/nerf/render_utils.py:23-41), rays_intersect_sphere (nerf/scene_utils.py:101-120),
// prepare_rays_data (render_utils.py:81-104).
#pragma once
#include "common.h"

struct RayGenPose {  // inverse intrinsics (row-major 3x3) and rows 0..2 of the normalised camera-to-world matrix
  float kinv[9];
  float c2w[12];
};

// dirs . R^T with dirs = [px, py, 1] . Kinv^T: INTEGER pixel coordinates, no half-pixel shift (render_utils.py:26-28, :38)
__device__ __forceinline__ void world_dir(const RayGenPose& a, int px, int py, float (&wd)[3]) {
  const float x = (float)px, y = (float)py;
  float cam[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) cam[j] = NM_FMA(1.0f, a.kinv[3 * j + 2], NM_FMA(y, a.kinv[3 * j + 1], x * a.kinv[3 * j]));
#pragma unroll
  for (int j = 0; j < 3; ++j)
    wd[j] = NM_FMA(cam[2], a.c2w[4 * j + 2], NM_FMA(cam[1], a.c2w[4 * j + 1], cam[0] * a.c2w[4 * j]));
}

__device__ __forceinline__ void unit_dir(const float (&wd)[3], float (&v)[3]) {
  const float n = sqrtf(wd[0] * wd[0] + wd[1] * wd[1] + wd[2] * wd[2]);
#pragma unroll
  for (int j = 0; j < 3; ++j) v[j] = wd[j] / n;
}

__device__ __forceinline__ void view_dir(const RayGenPose& a, int px, int py, float (&v)[3]) {
  float wd[3];
  world_dir(a, px, py, wd);
  unit_dir(wd, v);
}

// o + t v against the unit sphere: disc = (o.v)^2 + (1 - o.o) v.v; the frame is usable iff disc >= 0 for EVERY pixel
struct RaySphere {
  float od, dd, disc;
};
__device__ __forceinline__ RaySphere ray_sphere(const float (&o)[3], float oo, const float (&v)[3]) {
  RaySphere s;
  s.od = o[0] * v[0] + o[1] * v[1] + o[2] * v[2];
  s.dd = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  s.disc = s.od * s.od + (1.0f - oo) * s.dd;
  return s;
}
__device__ __forceinline__ float ray_far_plane(const RaySphere& s) { return (sqrtf(s.disc) - s.od) / s.dd; }

// distance between the directions of two image-row neighbours, x 2 / sqrt(12) (render_utils.py:93-99)
__device__ __forceinline__ float cone_radius(const float (&d)[3], const float (&dn)[3]) {
  const float e0 = d[0] - dn[0], e1 = d[1] - dn[1], e2 = d[2] - dn[2];
  const float step = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
  return step * 2.0f / 3.4641016151377544f;
}
