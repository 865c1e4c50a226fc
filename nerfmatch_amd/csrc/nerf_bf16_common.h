// Shared by the files of the operand-splitting NeRF MLP kernels (nerf_split_chain.h and the render / pointwise kernels built on it,
// nerf_pack_bf16.hip): blob / LDS constants, the kernel argument block, small device helpers (the split-bf16 vocabulary itself -- vector
// types, split8, pack_bf16, nrow, MFMA_BF16 -- is bf16x3.h).
#pragma once
#include "bf16x3.h"
#include "nerf_sample.h"
#include <string.h>

namespace nmbf {
using nmsample::launder;  // (one definition for every NeRF kernel: nerf_sample.h)
using nmsample::sin32;

constexpr int TILE = 128;
constexpr int SLOT_BYTES = 16384;
constexpr int SLOT_FLOATS = SLOT_BYTES / 4;
constexpr int NRING = 4;
constexpr int WS_WORKGROUPS = 512;  // upper bound of the persistent grid (one workgroup per CU); sizes the workspace
constexpr int XS = 6;    // K-steps of the 90(->96)-d IPE input
constexpr int HS = 16;   // K-steps of a 256-d hidden input
constexpr int VS = 3;    // K-steps of the 43(->48)-d [direction PE | appearance] input of the views layer
constexpr int NSLOT_NORGB = XS + 4 * HS + (XS + HS) + 2 * HS;       // layers 0..7          = 124
constexpr int NSLOT_FULL = NSLOT_NORGB + (HS + VS);                  // + views (feature_linear folded in) = 143

// small-parameter block (fp32), same layout as nerf_fwd.hip
constexpr int OFF_BIAS = 0, OFF_BVIEWS = 2304, OFF_WALPHA = 2432, OFF_WRGB = 2688, OFF_MISC = 3072;
// Round 4, fp16x3 only (the other modes carry ones): power-of-two operand scaling chosen at pack time (nm_nerf_pack_fp16x3).
//   OFF_SCALE   [16]  s_l, l = 0..8: the finished layer l is re-packed as fma(acc, s_l, bias'_l) -- s_l = 2^(c_{l+1} - A_l) takes the
//                     accumulator from its scale A_l (weight scale + input scale) to the input scale c_{l+1} of the next layer,
//                     bias'_l = bias_l * 2^c_{l+1} (stored in OFF_BIAS); exact: a power of two commutes with every rounding
//   OFF_DESCALE [8]   2^-c_{l+1}: back to true units, applied once per ray to the weight that multiplies the tapped activations
//   OFF_INSCALE [4]   2^c of the kernel-made inputs: IPE, direction PE, appearance row, (pad)
constexpr int OFF_SCALE = 3088, OFF_DESCALE = 3104, OFF_INSCALE = 3112, SMALL = 3120;
constexpr int NRANGE = 10;  // range telemetry slots: re-packed output of layers 0..8, views-layer extra inputs
constexpr int SMALL_PAD = 4096;  // floats reserved in the blob / LDS (16 KiB)
// zero slots behind the last one, for the run-ahead of the weight stream: a slot is requested ring_ahead (4) K-steps before its use and
// the stream simply runs on past a tile's last slot (the 2w experiment, which read the same blob, is in scripts/variants/)
constexpr int NSLOT_PAD = 4;
constexpr size_t BLOB_BYTES = (size_t)SMALL_PAD * 4 + (size_t)(NSLOT_FULL + NSLOT_PAD) * SLOT_BYTES;
constexpr int NSLOT_FULL_PAIRED = NSLOT_NORGB + HS / 2 + 2;  // 134: split modes -- eight paired hidden slots of the views layer, extras 0 | 1, extra 2
constexpr size_t BLOB_BYTES_FP16 = (size_t)SMALL_PAD * 4 + (size_t)(NSLOT_FULL + 8) * (SLOT_BYTES / 2);  // fp16x1: 8 >= ring_ahead<1>() + 1 slots of padding
constexpr int NSLOT_BWD = 8 + 8 + 16 * 9;  // 160: the transposed products of the pointwise backward (nerf_points_bf16.hip)
constexpr size_t BLOB_BYTES_BWD = (size_t)SMALL_PAD * 4 + (size_t)(NSLOT_BWD + NSLOT_PAD) * SLOT_BYTES;

// LDS map (floats)
constexpr int LDS_SMALL = 0;
constexpr int LDS_RING = SMALL_PAD;
constexpr int LDS_IPE = LDS_RING + NRING * SLOT_FLOATS;        // [4 waves][XS][2][64][4 floats]
constexpr int LDS_SCR = LDS_IPE + 4 * XS * 2 * 64 * 4;          // per-sample scratch, see below
constexpr int LDS_FEAT = LDS_SCR + TILE * 12 + 32;              // [4 waves][256] partial feature sums
constexpr int LDS_EX = LDS_FEAT + 4 * 256;                     // [4 ray slots][48] views-layer extra inputs
constexpr int LDS_LEFT = LDS_EX + 4 * 48;                     // leftover list: [128] ray index, [128] transmittance
constexpr int LDS_RNG = LDS_LEFT + 2 * TILE;                   // [NRANGE][256] per-thread running maxima of the re-packed |values| (bits)
constexpr int LDS_TOTAL = LDS_RNG + NRANGE * 256;

struct NerfArgs {
  const char* blob;
  const float* rays;
  const float* t;
  const float* app_row;
  float* weights;
  float* feat;
  float* pts;
  float* rgb;
  float* depth;
  float* acc;
  float* raw;
  float* sfeat;
  float* ws;  // [gridDim.x][4 wavefronts][32][64 lanes][4]: tapped activations of the tile in flight (fp32)
  int R, S, tap, white_bg, flags, ntiles;
  int Sa;    // samples per ray evaluated by the regular tiles (= S, or S/2 with NM_NERF_ZERO_TAIL)
  int left;  // 1: sample Sa of every ray is evaluated by "leftover" passes, samples > Sa have zero width (weight 0)
  int ntiles_full;       // tile count of the full evaluation (Sa = S)
  const int* tail_viol;  // device flag raised by nm_resample when the zero-width premise does NOT hold: evaluate everything
  float var_scale;
  int* status;  // fp16x3: device int32[16] or NULL -- [0] |= 1 when an operand reached the fp16 limit, [1 + k] = max bits of range slot k
};

// -DNM_TRACE: profiling build only -- the `raw` output becomes a [grid][32] table of s_memtime stamps of wavefront 0
#ifndef NM_TRACE
#define NM_TRACE 0
#endif

// (launder: nerf_sample.h)  The same for a wavefront-uniform value that must stay in an SGPR
__device__ __forceinline__ int launder_s(int v) {
  asm volatile("" : "+s"(v));
  return v;
}

#if NM_TRACE
#define TRACE(i)                                                                                               \
  do {                                                                                                         \
    if (a.raw && threadIdx.x == 0) reinterpret_cast<unsigned long long*>(a.raw)[bid * 32 + (i)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define TRACE(i) do { } while (0)
#endif

// Element of a finished accumulator: one 32-bit cross-class copy (v_accvgpr_read_b32) at the point of use.  Without the
// opaque asm the compiler copies whole 16-register tuples around (and through scratch when it runs out of registers).
__device__ __forceinline__ float acc_read(float av) {
  asm volatile("" : "+v"(av));
  return av;
}

// Opaque identity: keeps a value (and the instructions that made it) in the basic block and at the position it was
// written -- without it LLVM sinks the re-packing arithmetic out of the MFMA stream into the block of its first use.
template <class T>
__device__ __forceinline__ void pin(T& v) {
  asm volatile("" : "+v"(v));
}

}  // namespace nmbf
