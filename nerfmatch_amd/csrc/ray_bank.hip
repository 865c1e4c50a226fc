// Training ray batches from GPU-resident frames (nerf/ray_bank.py).  The reference expands every pixel of every training frame into a
// 16-float row on the CPU, keeps the whole table in host memory and copies each step's rows to the device
// (NerfBaseDataset.process_train_data / load_sample, nerfmatch/datasets/nerfbase.py:255-321, :351-385).  Here the frames stay on the device
// as uint8 with one 21-float camera row each, and one launch per step turns "positions p0 .. p0 + n of epoch e" into the batch:
// ~60 flops per ray, 3 + 84 (L2-shared per frame) + 4 bytes read, 48 + 12 + 8 (+ 4) bytes written.  The per-pixel expressions are
// those of nm_raygen (ray_pixel.h).
#include "common.h"
#include "perm.h"
#include "ray_pixel.h"
#include <limits.h>

namespace {

constexpr int RB_ROUNDS = NM_PERM_ROUNDS;  // Feistel rounds of the epoch permutation (perm.h)

struct RayBankArgs {
  const uint8_t* images;       // [F,H,W,3]
  const uint8_t* masks;        // [F,H,W] or NULL
  const float* cams;           // [F,21]: Kinv (9) | rows 0..2 of c2w (12)
  const int* flags;            // [F]: 1 = far plane 1 for every ray of the frame
  const long long* ts_table;   // [F]
  const long long* ids;        // [n] or NULL (NULL: the permutation)
  const long long* valid;      // [n_src] or NULL
  long long n_src, total;      // size of the index space the ids / the permutation live in; F*H*W
  long long pos0, pos_stride;
  uint32_t keys[RB_ROUNDS];
  int half_bits;
  int H, W, n, norm_ray_dir;
  float near_plane;
  float* rays;
  float* rgbs;
  long long* ts;
  float* mask_out;
  int* bad;
};

__device__ __forceinline__ void load_pose(const float* __restrict__ cams, long long f, RayGenPose& pz) {
  const float* c = cams + f * 21;
#pragma unroll
  for (int i = 0; i < 9; ++i) pz.kinv[i] = c[i];
#pragma unroll
  for (int i = 0; i < 12; ++i) pz.c2w[i] = c[9 + i];
}

// One thread per pixel of frame f0 + blockIdx.y: the frame's flag is raised when ANY pixel's discriminant is not >= 0 (one atomic per
// wavefront that sees one, as raygen_pixels_kernel does).
__global__ void __launch_bounds__(256) raybank_flags_kernel(const float* __restrict__ cams, int f0, int H, int W, int* __restrict__ flags) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, f = f0 + blockIdx.y;
  const bool inside = idx < H * W;
  RayGenPose pz;
  load_pose(cams, f, pz);
  const int xx = inside ? idx % W : 0, yy = inside ? idx / W : 0;
  const float o[3] = {pz.c2w[3], pz.c2w[7], pz.c2w[11]};
  const float oo = o[0] * o[0] + o[1] * o[1] + o[2] * o[2];
  float v[3];
  view_dir(pz, xx, yy, v);
  const bool bad = inside && !(ray_sphere(o, oo, v).disc >= 0.0f);
  if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flags + f, 1);
}

__global__ void __launch_bounds__(256) raybank_gather_kernel(RayBankArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  bool bad = false;
  long long j;
  if (a.ids) {
    j = a.ids[i];
  } else {
    long long pos = a.pos0 + (long long)i * a.pos_stride;
    if (pos < 0 || pos >= a.n_src) {  // (a start point outside [0, n_src) need not lie on a cycle that enters it)
      bad = true;
      pos = pos < 0 ? 0 : a.n_src - 1;
    }
    // cycle walking: the walk from a point below n_src stays on that point's own cycle, which contains it -- it terminates
    j = (long long)nm_perm_walk((unsigned long long)pos, (unsigned long long)a.n_src, a.keys, a.half_bits);
  }
  if (j < 0 || j >= a.n_src) {
    bad = true;
    j = j < 0 ? 0 : a.n_src - 1;
  }
  long long g = a.valid ? a.valid[j] : j;
  if (g < 0 || g >= a.total) {
    bad = true;
    g = g < 0 ? 0 : a.total - 1;
  }
  if (bad) atomicAdd(a.bad, 1);
  const long long hw = (long long)a.H * a.W;
  const long long f = g / hw;
  const int rem = (int)(g - f * hw);
  const int py = rem / a.W, px = rem - py * a.W;

  RayGenPose pz;
  load_pose(a.cams, f, pz);
  const float o[3] = {pz.c2w[3], pz.c2w[7], pz.c2w[11]};
  const float oo = o[0] * o[0] + o[1] * o[1] + o[2] * o[2];
  float wd[3], v[3];
  world_dir(pz, px, py, wd);
  unit_dir(wd, v);
  // the far plane always comes from the unit directions (nerfbase.py:287-290); 1 for every ray of a flagged frame
  const float far_plane = a.flags[f] ? 1.0f : ray_far_plane(ray_sphere(o, oo, v));
  // cone radius: distance to the neighbour one image row below; the last row takes the value of row H-3 (`dx[-2:-1]`,
  // render_utils.py:94-95), i.e. |d(x, H-3) - d(x, H-2)|
  const bool last = py + 1 >= a.H;
  const int ya = last ? a.H - 3 : py;
  float wa[3], wb[3], da[3], db[3];
  world_dir(pz, px, ya, wa);
  world_dir(pz, px, ya + 1, wb);
  float radius;
  float d[3];
  if (a.norm_ray_dir) {
    unit_dir(wa, da);
    unit_dir(wb, db);
    radius = cone_radius(da, db);
    d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
  } else {
    radius = cone_radius(wa, wb);
    d[0] = wd[0]; d[1] = wd[1]; d[2] = wd[2];
  }
  f32x4* r = reinterpret_cast<f32x4*>(a.rays + (size_t)i * 12);  // 48-byte rows: 16-byte aligned when the base is
  r[0] = f32x4{o[0], o[1], o[2], d[0]};
  r[1] = f32x4{d[1], d[2], a.near_plane, far_plane};
  r[2] = f32x4{v[0], v[1], v[2], radius};

  const uint8_t* px8 = a.images + (size_t)g * 3;
  float* c = a.rgbs + (size_t)i * 3;
  c[0] = (float)px8[0] / 255.0f;  // a true division: to_tensor's `.div(255)` (x * (1/255) differs for 126 of the 256 codes)
  c[1] = (float)px8[1] / 255.0f;
  c[2] = (float)px8[2] / 255.0f;
  a.ts[i] = a.ts_table[f];
  if (a.mask_out) a.mask_out[i] = a.masks[g] >= 128 ? 0.0f : 1.0f;  // 1 - round(m / 255) (nerfbase.py:226-228)
}

}  // namespace

extern "C" int nm_raybank_frame_flags(const float* cams, int F, int H, int W, int* flags, nmStream_t stream) {
  NM_CHECK_ARG(cams && flags && F > 0 && H > 0 && W > 0 && (long long)H * W <= INT_MAX - 256);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(flags, 0, (size_t)F * sizeof(int), s) != hipSuccess) return NM_ERR_LAUNCH;
  constexpr int MAXY = 32768;  // frames per launch (grid y)
  for (int f0 = 0; f0 < F; f0 += MAXY) {
    const int nf = F - f0 < MAXY ? F - f0 : MAXY;
    raybank_flags_kernel<<<dim3((H * W + 255) / 256, nf), 256, 0, s>>>(cams, f0, H, W, flags);
  }
  return nm_launch_status();
}

extern "C" int nm_raybank_gather(const uint8_t* images, const uint8_t* masks, const float* cams, const int* flags, const long long* ts_table,
                                 int F, int H, int W, const long long* ids, const long long* valid, long long n_src,
                                 const uint32_t* perm_keys_host, int perm_half_bits, long long pos0, long long pos_stride, int n,
                                 int norm_ray_dir, float near_plane, float* rays, float* rgbs, long long* ts, float* mask, int* bad,
                                 nmStream_t stream) {
  NM_CHECK_ARG(images && cams && flags && ts_table && rays && rgbs && ts && bad && F > 0 && H >= 3 && W > 0 && n > 0 && n_src > 0);
  NM_CHECK_ARG((long long)H * W <= INT_MAX && (masks || !mask));
  NM_CHECK_ARG(((uintptr_t)rays & 15) == 0);
  const long long total = (long long)F * H * W;
  NM_CHECK_ARG(n_src <= total && (valid || n_src == total));
  RayBankArgs a;
  if (!ids) {
    // the permutation's domain 2^(2 half_bits) must cover n_src (cycle walking) and the halves must fit the 32-bit round function
    NM_CHECK_ARG(perm_keys_host && perm_half_bits >= 0 && perm_half_bits <= 20 && (1ll << (2 * perm_half_bits)) >= n_src);
    NM_CHECK_ARG(pos_stride >= 0 && pos0 >= 0 && pos0 < n_src && pos0 + (long long)(n - 1) * pos_stride < n_src);
    for (int k = 0; k < RB_ROUNDS; ++k) a.keys[k] = perm_keys_host[k];
  } else {
    for (int k = 0; k < RB_ROUNDS; ++k) a.keys[k] = 0;
  }
  a.images = images; a.masks = masks; a.cams = cams; a.flags = flags; a.ts_table = ts_table;
  a.ids = ids; a.valid = valid; a.n_src = n_src; a.total = total; a.pos0 = pos0; a.pos_stride = pos_stride;
  a.half_bits = perm_half_bits; a.H = H; a.W = W; a.n = n; a.norm_ray_dir = norm_ray_dir; a.near_plane = near_plane;
  a.rays = rays; a.rgbs = rgbs; a.ts = ts; a.mask_out = mask; a.bad = bad;
  raybank_gather_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(a);
  return nm_launch_status();
}
