// Fused per-ray NeRF evaluation on the 16-bit matrix cores with operand splitting ("bf16x3" / "fp16x3"; "fp16x1").
//
// Round 3: the split exists in two number formats.  bf16 hi/lo parts carry 16 mantissa bits together (error of a product
// ~2^-16.5): enough for the smooth random-weight fixtures (features 3e-7 from fp32), NOT enough for a trained-like scene --
// densities of +-1e4 come out 0.25 off and the compositing weights 7e-4 (tests/golden/nerf_surface_r512_s128.npz).  fp16
// hi/lo parts carry 22 bits (11 + 11; below 2^-14 the lo part is a subnormal with an ABSOLUTE quantum of 2^-24, which is all
// a sum of products needs): the same three MFMAs per product (v_mfma_f32_32x32x16_f16 runs at the bf16 rate), the same
// re-packing cost, fp32-class results (density error 0.01 on that fixture, the fp32 MFMA kernel: 0.013).  fp16x3 is the
// default parity arithmetic (NerfRenderer.precision); operands beyond +-65504 saturate (v_med3), they do not overflow.
//
// Same computation and outputs as nerf_fwd.hip; what changes is
// the arithmetic of the layer products: every fp32 operand x is split into two bf16 values x = hi + lo (16 mantissa
// bits together) and each product is evaluated as  w_hi*x_hi + w_hi*x_lo + w_lo*x_hi  with three
// v_mfma_f32_32x32x16_bf16 (fp32 accumulation).  The dropped lo*lo term is 2^-16 relative; measured against the fp32
// oracle the rendered features differ by < 1e-6 (tolerance 1e-4) -- see DESIGN.md section 3.1b.  Three bf16 MFMAs
// cost 3/16 of the fp32 MFMA they replace.
//
// Structure (persistent workgroups, one per CU; a tile = 4 wavefronts x 32 samples, one wavefront per SIMD):
//   * activations stay in registers between layers: the MFMA result layout (lane = sample + 32*half, register r <->
//     neuron (r&3)+8*(r>>2)+4*half) maps 8 consecutive registers of a lane onto the 8 K-slots of one 32x32x16 step, so
//     re-packing into (hi, lo) bf16 B operands is lane-local (bias, relu, cvt, subtract, cvt);
//   * cross-layer software pipeline: a finished layer is moved out of the accumulators (AGPRs -> 128 VGPR scalars) and
//     re-packed one K-step "unit" at a time INSIDE the K-loop of the layer that consumes it, at most 5 VALU instructions
//     behind an MFMA (pinned with sched_barriers and opaque asm; which gap carries what: the table at UnitWork), so that only
//     the 128 accumulator reads and unit 0 are exposed per layer;
//   * weights are pre-split and pre-ordered on the host into 16 KiB "slots" = one K-step for all 8 output blocks,
//     streamed by all 4 wavefronts with global_load_lds (LDS DMA, no VGPRs) into a 4-slot LDS ring: two slots in use, two
//     in flight, ONE s_barrier + s_waitcnt vmcnt per TWO slots (ring_acquire_two; the barrier's skew was the largest single
//     overhead of a K-step in the cycle trace); every wavefront then reads its A operands with conflict-free ds_read_b128
//     (the ring layout is lane-linear, exactly what the DMA writes);
//   * the tapped activations (feature output) are parked in an L2-resident workspace (32 x 1 KiB stores per wavefront)
//     until the compositing weights are known, then reduced over the 32 samples of a wavefront with DPP adds -- except for a tap on
//     layer 7 in a pass with colour heads (the coarse pass of the renderer): the densities exist before the views layer, so the
//     weights are formed there and w * h7 is reduced straight from the registers that hold layer 7 (tap7_early: no round trip);
//   * the integrated positional encoding is evaluated once per 128-sample chunk (each lane the 48 values of its wavefront
//     half, fp32 sine with a 4-term Cody-Waite reduction of the exact argument 2^i x) and parked in LDS as ready-made
//     B operands for layers 0 and 5.
// This file: the render kernel (tile prologue, tap round trip, compositing and reductions) and its entry points.  The K-loop machinery
// it shares with the pointwise kernels of nerf_points_bf16.hip is nerf_split_chain.h; the host-side blob packing is nerf_pack_bf16.hip.
#include "nerf_split_chain.h"

namespace {
using namespace nmbf;
// the sample math shared with the fp32 and iNeRF kernels (nerf_sample.h)
using nmsample::HALF_PI_F32, nmsample::SCAN_TILE, nmsample::frustum, nmsample::ray_consts, nmsample::lift_var, nmsample::ipe_fast, nmsample::view_row_value;
using nmsample::alpha_of, nmsample::trans_factor, nmsample::sigmoid, nmsample::scan_before_barrier, nmsample::scan_after_barrier, nmsample::scan_carry;
using nmsample::first_max;
static_assert(TILE == SCAN_TILE, "the compositing scan of nerf_sample.h spans two wavefronts");

// Start the read-back of this wavefront's 32 tapped rows: LDS-DMA into the weight ring and the IPE region (nobody needs them before the
// next tile), the last four rows into registers.  Called when the tile's last K-loop is over; between here and the reduction that
// consumes the rows lie the density / colour heads and the compositing -- barriers there wait for LDS only (NM_EPI_BARRIER).
// Two calls per tile (PART 0: the ring rows, right after the last K-loop; PART 1: the IPE rows, behind the head that follows): 28 KiB per
// wavefront in one burst outruns the CU's miss queue and the wavefront sits in ISSUE for most of the latency it wanted to hide (A/B on
// one box, 4 x 4800 x 64 with all heads: one burst -0.9 % of a launch, two -1.6 ... -2.2 %, three -1.1 %: profiles/r4_ab_tap_prefetch.log).
// OWN: the kernel owns M0 (nerf_split_chain.h, dma_slot) -- it is set and not handed back.
template <int PART, bool OWN>
__device__ __forceinline__ void tap_prefetch(Ctx& cx) {
  // (the caller has waited for this wavefront's last operand reads of the ring: NM_MLP_DONE_WAIT)
  if constexpr (PART == 0) __builtin_amdgcn_s_barrier();  // everybody else is through with the ring as well
  const char* src = reinterpret_cast<const char*>(cx.tapw);
  // (inline asm, not __builtin_amdgcn_global_load_lds: the compiler cannot tell these LDS writes from the head vectors / scratch the
  //  colour heads and the compositing read -- one __shared__ array -- and would put a vmcnt(0) in front of their first ds_read; the one
  //  wait these rows need is the explicit one in front of the reduction)
#pragma unroll
  for (int q = (PART == 0 ? 0 : 4); q < (PART == 0 ? 4 : 7); ++q) {
    const char* sp = src + q * 4096;
    const float* dp = q < 4 ? cx.tap_ring + q * 1024 : cx.tap_ipe + (q - 4) * 1024;
    const unsigned lds = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(const __attribute__((address_space(3))) float*)dp);
    if constexpr (OWN) {
      asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off\n\tglobal_load_lds_dwordx4 %1, off offset:1024\n\t"
                   "global_load_lds_dwordx4 %1, off offset:2048\n\tglobal_load_lds_dwordx4 %1, off offset:3072"
                   :: "s"(lds), "v"(sp) : "memory");
      continue;
    }
    unsigned m0_saved;  // (a kernel with a builtin LDS-DMA: M0 belongs to the compiler and is handed back as found)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %2, off\n\tglobal_load_lds_dwordx4 %2, off offset:1024\n\t"
                 "global_load_lds_dwordx4 %2, off offset:2048\n\tglobal_load_lds_dwordx4 %2, off offset:3072\n\ts_mov_b32 m0, %0"
                 : "=&s"(m0_saved) : "s"(lds), "v"(sp) : "memory");
  }
}

// Sums over the 32 lanes of each half wavefront of 32 rows of four values (v[4 row + e]), "reduce-scatter": every step pairs two rows,
// adds across a lane distance (16, 8, 4, 2, 1) and keeps one row of the pair on either side, so the number of live values halves each time
// -- 64 + 32 + 16 + 8 + 4 outputs at 2-3 instructions each plus nothing for the lanes that used to idle, against 5 DPP adds for each of
// the 128 values when every row is reduced on its own (nm_half_sum_dpp8).  Lane L ends up with the four sums of row L & 31.
//   distance 16: v_permlane16_swap (gfx950) exchanges odd rows of one register with even rows of the other, then one add;
//   distance 8 / 4: v_add_dpp row_mirror / row_half_mirror, two instructions per output with complementary bank masks writing one register;
//   distance 2 / 1: quad_perm adds of both rows and a select on the lane bit.
// (summation order differs from nm_half_sum_dpp8's tree: results agree to rounding)
__device__ __forceinline__ void dpp_pairs8(float (&o)[8], const float (&x)[8], const float (&y)[8], bool eight) {
  // o = lanes whose bank bit is clear: x + x[mirror partner]; set: y + y[partner]
  if (eight)
    asm("s_nop 1\n"
        "v_add_f32_dpp %0, %8, %8 row_mirror row_mask:0xf bank_mask:0x3\n\tv_add_f32_dpp %1, %9, %9 row_mirror row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %2, %10, %10 row_mirror row_mask:0xf bank_mask:0x3\n\tv_add_f32_dpp %3, %11, %11 row_mirror row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %4, %12, %12 row_mirror row_mask:0xf bank_mask:0x3\n\tv_add_f32_dpp %5, %13, %13 row_mirror row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %6, %14, %14 row_mirror row_mask:0xf bank_mask:0x3\n\tv_add_f32_dpp %7, %15, %15 row_mirror row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %0, %16, %16 row_mirror row_mask:0xf bank_mask:0xc\n\tv_add_f32_dpp %1, %17, %17 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %2, %18, %18 row_mirror row_mask:0xf bank_mask:0xc\n\tv_add_f32_dpp %3, %19, %19 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %4, %20, %20 row_mirror row_mask:0xf bank_mask:0xc\n\tv_add_f32_dpp %5, %21, %21 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %6, %22, %22 row_mirror row_mask:0xf bank_mask:0xc\n\tv_add_f32_dpp %7, %23, %23 row_mirror row_mask:0xf bank_mask:0xc"
        : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
        : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]),
          "v"(y[0]), "v"(y[1]), "v"(y[2]), "v"(y[3]), "v"(y[4]), "v"(y[5]), "v"(y[6]), "v"(y[7]));
  else
    asm("s_nop 1\n"
        "v_add_f32_dpp %0, %8, %8 row_half_mirror row_mask:0xf bank_mask:0x5\n\tv_add_f32_dpp %1, %9, %9 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %2, %10, %10 row_half_mirror row_mask:0xf bank_mask:0x5\n\tv_add_f32_dpp %3, %11, %11 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %4, %12, %12 row_half_mirror row_mask:0xf bank_mask:0x5\n\tv_add_f32_dpp %5, %13, %13 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %6, %14, %14 row_half_mirror row_mask:0xf bank_mask:0x5\n\tv_add_f32_dpp %7, %15, %15 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %0, %16, %16 row_half_mirror row_mask:0xf bank_mask:0xa\n\tv_add_f32_dpp %1, %17, %17 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %2, %18, %18 row_half_mirror row_mask:0xf bank_mask:0xa\n\tv_add_f32_dpp %3, %19, %19 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %4, %20, %20 row_half_mirror row_mask:0xf bank_mask:0xa\n\tv_add_f32_dpp %5, %21, %21 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %6, %22, %22 row_half_mirror row_mask:0xf bank_mask:0xa\n\tv_add_f32_dpp %7, %23, %23 row_half_mirror row_mask:0xf bank_mask:0xa"
        : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
        : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]),
          "v"(y[0]), "v"(y[1]), "v"(y[2]), "v"(y[3]), "v"(y[4]), "v"(y[5]), "v"(y[6]), "v"(y[7]));
}
template <int XOR>
__device__ __forceinline__ void quad_add8(float (&v)[8]) {  // v[i] += v[i] of lane ^ XOR (1 or 2), in place, all lanes
  if (XOR == 1)
    asm("s_nop 1\n"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %3, %3, %3 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %4, %4, %4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %5, %5, %5 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %6, %6, %6 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %7, %7, %7 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
        : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
  else
    asm("s_nop 1\n"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %3, %3, %3 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %4, %4, %4 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %5, %5, %5 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %6, %6, %6 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32_dpp %7, %7, %7 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
        : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
}
// distance 16 for one value of row c (x) and one of row c + 16 (y)
__device__ __forceinline__ float reduce_scatter_step16(float x, float y) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// distances 8 .. 1, from s1[i] = reduce_scatter_step16(v[i], v[64 + i]): rows 0..15 | (lanes 16..31 of the half: rows 16..31)
__device__ __forceinline__ f32x4 reduce_scatter_16pairs(const float (&s1)[64], int lane) {
  float s2[32];  // 8 rows
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    float o[8], x[8], y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { x[i] = s1[8 * b + i]; y[i] = s1[32 + 8 * b + i]; }
    dpp_pairs8(o, x, y, true);
#pragma unroll
    for (int i = 0; i < 8; ++i) s2[8 * b + i] = o[i];
  }
  float s3[16];  // 4 rows
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    float o[8], x[8], y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { x[i] = s2[8 * b + i]; y[i] = s2[16 + 8 * b + i]; }
    dpp_pairs8(o, x, y, false);
#pragma unroll
    for (int i = 0; i < 8; ++i) s3[8 * b + i] = o[i];
  }
  float lo8[8], hi8[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { lo8[i] = s3[i]; hi8[i] = s3[8 + i]; }
  quad_add8<2>(lo8); quad_add8<2>(hi8);
  float s4[8];  // 2 rows
#pragma unroll
  for (int i = 0; i < 8; ++i) s4[i] = (lane & 2) ? hi8[i] : lo8[i];
  float t8[8] = {s4[0], s4[1], s4[2], s4[3], s4[4], s4[5], s4[6], s4[7]};
  quad_add8<1>(t8);
  return (lane & 1) ? f32x4{t8[4], t8[5], t8[6], t8[7]} : f32x4{t8[0], t8[1], t8[2], t8[3]};
}
__device__ __forceinline__ f32x4 reduce_scatter_32rows(float (&v)[128], int lane) {
  float s1[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) s1[i] = reduce_scatter_step16(v[i], v[64 + i]);
  return reduce_scatter_16pairs(s1, lane);
}

// Barriers of the tile's epilogue between tap_prefetch and the feature reduction: they order LDS traffic only (per-sample scratch), so they
// wait for LDS only -- a __syncthreads() is also a memory fence and would sit out the read-back that is meant to overlap this phase.
// End of the tile's last K-loop, on EVERY path into the epilogue: vmcnt(0) lgkmcnt(0) through the BUILTIN -- (a) this wavefront's last
// operand reads of the ring have returned; (b) the compiler sees its own LDS-DMA of the weight stream (the run-ahead into the blob's
// padding) retired; otherwise it keeps "an LDS write may be pending" on its books and puts a vmcnt(0) of its own in front of the next
// ds_read of the epilogue, which would then wait for the rows tap_prefetch requests right behind this.
#define NM_MLP_DONE_WAIT() __builtin_amdgcn_s_waitcnt(0x0070)
#define NM_EPI_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
// TAP7: the launch may composite a tap on layer 7 early (tap7_early below; decided per tile at run time).  The fp16x3 kernel exists in both
// forms and the host picks (nerf_fwd_split): without TAP7 no tile needs its densities in front of the views layer, so the views K-loop
// adds up the density head as it re-packs layer 7 (DENS; dens_open in nerf_split_chain.h) and alpha_head goes.  Two kernels, not two
// K-loops behind a branch in one: with both in one kernel the register allocator spilled 148 VGPRs.
template <int P, bool TAP7 = true>
__device__ __forceinline__ void nerf_fwd_body(const NerfArgs& a) {
  constexpr bool DENS = P == 2 && !TAP7;
  __shared__ __attribute__((aligned(16))) float sm[LDS_TOTAL];
  float* const sm_small = sm + LDS_SMALL;
  float* const ring = sm + LDS_RING;
  float* const sm_ipe = sm + LDS_IPE;
  float* const sm_sigma = sm + LDS_SCR;       // [128]
  float* const sm_rgb = sm_sigma + TILE;      // [3][128]
  float* const sm_t0 = sm_rgb + 3 * TILE;
  float* const sm_t1 = sm_t0 + TILE;
  float* const sm_mean = sm_t1 + TILE;        // [3][128]
  float* const sm_dn = sm_mean + 3 * TILE;
  float* const sm_w = sm_dn + TILE;
  float* const sm_misc = sm_w + TILE;         // [32]
  float* const sm_part = sm_misc + 32;        // [4 half wavefronts][8] partial per-ray sums (the scratch block has 128 floats to spare;
                                              // not over sm_feat: with a tap composited early the feature partials are there first)
  float* const sm_feat = sm + LDS_FEAT;       // [4][256]
  float* const sm_ex = sm + LDS_EX;           // [nr][48]
  int* const sm_lray = reinterpret_cast<int*>(sm + LDS_LEFT);  // [128] rays whose sample Sa is still to be evaluated
  float* const sm_lT = sm + LDS_LEFT + TILE;                   // [128] their transmittance after the first Sa samples
  unsigned* const sm_rng = reinterpret_cast<unsigned*>(sm + LDS_RNG);  // [NRANGE][256] range telemetry (fp16x3)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = lane & 31, hi = lane >> 5;
  // the zero-tail decision is taken HERE, from the flag nm_resample left on the device (no promise by the caller)
  const bool tail_ok = a.left && !(a.tail_viol && *a.tail_viol != 0);
  const int S = a.S, R = a.R;                // S: row length of t / weights
  const int Sa = tail_ok ? a.Sa : S;         // samples evaluated by the regular tiles
  const int left = tail_ok ? 1 : 0;
  const int ntiles = tail_ok ? a.ntiles : a.ntiles_full;
  const int SP = Sa < TILE ? Sa : TILE;
  const int nr = TILE / SP;
  const int nchunks = (Sa + TILE - 1) / TILE;
  const bool need_rgb = !(a.flags & NM_NERF_SKIP_RGB);
  const bool feat_max = (a.flags & NM_NERF_FEAT_MAX) != 0;
  const bool need_tap = (a.feat != nullptr) || (a.sfeat != nullptr);
  const int tap = (a.tap < 0 || a.tap > 7) ? 7 : a.tap;
  const int nslots = need_rgb ? NSLOT_FULL : NSLOT_NORGB;
  const char* const blob_slots = a.blob + (size_t)SMALL_PAD * 4;

  for (int i = tid; i < SMALL / 4; i += 256) reinterpret_cast<f32x4*>(sm_small)[i] = reinterpret_cast<const f32x4*>(a.blob)[i];
  if constexpr (P == 2) {
#pragma unroll
    for (int k = 0; k < NRANGE; ++k) sm_rng[k * 256 + tid] = 0u;
  }

  // persistent workgroups: one per CU (the LDS footprint allows no more), tiles dealt round robin.
  // NM_NERF_ZERO_TAIL: a regular tile evaluates samples 0..Sa-1 of its rays and queues (ray, transmittance) for the one
  // remaining non-degenerate sample (index Sa); whenever 128 of them have piled up, and at the end, a "leftover" pass
  // runs the same network over 128 queued samples (one per lane, each of a different ray) and adds their contribution
  // to the outputs of rays this workgroup has already written.
  int nleft = 0;  // queued leftovers (uniform)
  int bid = blockIdx.x;
#pragma unroll 1
  for (;;) {
  bool lo_pass = false;
  if (left && (nleft > TILE - 4 || (bid >= ntiles && nleft > 0))) lo_pass = true;
  else if (bid >= ntiles) break;
  const int nent = lo_pass ? nleft : 0;
  TRACE(0);
  // extra inputs of the views layer, one value per thread (they depend on the ray only): column f of view_row_value's row (nerf_sample.h)
  if (need_rgb && !lo_pass && tid < nr * 48) {
    const int r2 = tid / 48, f = tid % 48;
    const int ray2 = bid * nr + r2;
    const float* rq = a.rays + (size_t)(ray2 < R ? ray2 : R - 1) * 12 + 8;
    float v = view_row_value(f, rq[f % 3], a.app_row);
    if constexpr (P == 2) {  // (straight from the blob: sm_small may not have landed yet in the first tile)
      v *= reinterpret_cast<const float*>(a.blob)[OFF_INSCALE + (f < 27 ? 1 : 2)];
      __hip_atomic_fetch_max(sm_rng + 9 * 256 + tid, __float_as_uint(fabsf(v)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    sm_ex[tid] = v;
  }
  __syncthreads();  // biases are read before the first ring barrier
  TRACE(1);

  const int js = wave * 32 + s;
  const int rl = js / SP;
  // regular tile: lane's ray = slot js / SP of the tile; leftover pass: lane js owns queue entry js (idle lanes redo entry 0)
  const int ray = lo_pass ? (js < nent ? sm_lray[js] : R) : bid * nr + rl;
  const int rc = lo_pass ? sm_lray[js < nent ? js : 0] : (ray < R ? ray : R - 1);
  const float* rp = a.rays + (size_t)rc * 12;
  const float o0 = rp[0], o1 = rp[1], o2 = rp[2], d0 = rp[3], d1 = rp[4], d2 = rp[5], radius = rp[11];
  float dsq[3], nul[3], dnorm;
  ray_consts(rp + 3, dsq, nul, dnorm);

  float red_acc = 0.f;
  float carryT = 1.f;
  float best_w = -1.f;
  float feat_run = 0.f;  // thread t: running feature channel t of the (single) ray when S > 128

  const int nch = lo_pass ? 1 : nchunks;
  for (int chunk = 0; chunk < nch; ++chunk) {
    const int sidx = lo_pass ? Sa : chunk * TILE + (js % SP);
    const float t0 = a.t[(size_t)rc * (S + 1) + sidx];
    const float t1 = a.t[(size_t)rc * (S + 1) + sidx + 1];
    float t_mean, t_var, r_var;
    frustum(t0, t1, radius, t_mean, t_var, r_var);
    float mean[3] = {d0 * t_mean + o0, d1 * t_mean + o1, d2 * t_mean + o2};
    float var[3];
    lift_var(t_var, r_var, dsq, nul, a.var_scale, var);
    if (hi == 0) {
      sm_t0[js] = t0; sm_t1[js] = t1;
      sm_mean[js] = mean[0]; sm_mean[TILE + js] = mean[1]; sm_mean[2 * TILE + js] = mean[2];
      sm_dn[js] = dnorm;
    }

    // start the weight stream
    ring_open<P>(blob_slots, ring, wave, lane);

    // ---- integrated positional encoding -> B operands of the 6 IPE K-steps, parked in LDS -------------------------
    // K-slot (step m, half h, i) <-> encoding index f = 45 h + 8 m + i of the reference's order (8 m + i < 45; the last three slots of step 5
    // are padding), f = part*45 + scale*3 + axis  (part 0: sin(2^scale x), part 1: sin(2^scale x + pi/2)): the two halves of a wavefront
    // evaluate the SAME (scale, axis) and differ in the phase only, so scale, axis and the exponential's constant are compile-time per
    // value and nothing is selected on the lane's half (round 4: with f = 16 m + 8 h + i the compiler turned the per-half selects into
    // run-time integer arithmetic on f -- 43 instructions per value, 28 now; nerf_pack_split permutes the weight columns to match).
    // Every lane evaluates only the 48 encodings its wavefront half feeds to the MFMAs, directly in fp32: the argument
    // 2^scale * x is exact, sin32 (4-term Cody-Waite + degree-9 polynomial, |err| <= 1e-7 for |arg| < 6.5e4) replaces the
    // earlier fp64 angle-doubling recurrence (which both halves had to run over all 90 values), and the second half of
    // the encoding takes sin(fl32(arg + fl32(pi/2))) literally like the reference (x + 0.f is x; -0 becomes +0, its sine a zero either way).
    {
      const float ipe_scale = sm_small[OFF_INSCALE];
      const float phl = hi ? HALF_PI_F32 : 0.f;
      park_ipe<P>(sm_ipe + wave * (XS * 2 * 64 * 4) + lane * 4, [&](int idx) {  // (idx: compile time)
        const int ax = idx % 3;
        const float sc = (float)(1 << (idx / 3));
        float v = ipe_fast(mean[ax] * sc + phl, var[ax], sc);
        if constexpr (P == 2) v *= ipe_scale;  // 2^c_ipe (|v| <= 1: no saturation possible for c_ipe <= 15)
        return v;
      });
    }

    TRACE(2);
    // ---- 8 pts layers + views layer (feature_linear folded in at pack time), software pipelined across layers ----------
    // The finished layer is moved out of the accumulators (finish_layer: AGPRs -> cx.hv, plus unit 0) and re-packed one
    // K-step unit at a time INSIDE the K-loop of the layer that consumes it: unit u+1 (bias, relu, hi/lo split = ~40 VALU
    // instructions) is computed in the shadow of the MFMAs of K-step u (UnitWork and its per-gap schedule, slot_step8).
    Ctx cx;
    cx.blob_slots = blob_slots; cx.ring = ring; cx.sm_small = sm_small;
    cx.tapw = reinterpret_cast<f32x4*>(a.ws) + ((size_t)blockIdx.x * 4 + wave) * 32 * 64 + lane;
    cx.nslots = nslots; cx.wave = wave; cx.lane = lane; cx.hi = hi; cx.tap = need_tap ? tap : -1; cx.g = 0; cx.sig_part = 0.f;
    cx.vmax = 0.f; cx.rng = sm_rng + tid; cx.sc = 1.f;
    // A tap on layer 7 in a regular tile with colour heads is composited at the end of layer 7, from registers (tap7_early); the
    // per-sample feature output (a debug output) and the leftover pass keep the workspace path.
    const bool early = TAP7 && need_rgb && !lo_pass && tap == 7 && a.feat && !a.sfeat;
    cx.tap_pref = need_tap && !lo_pass && !early; cx.rgb = need_rgb;
    cx.tap_ring = ring + wave * SLOT_FLOATS; cx.tap_ipe = sm_ipe + wave * (XS * 2 * 64 * 4);
    if constexpr (is_split<P>()) {
      ring_open_wait<P>(cx);
    } else {
      ring_acquire<P>(blob_slots, 0, nslots, ring, wave, lane);
    }
    load_half<P>(cx.opA, ring, lane, 0);
    if constexpr (P == 1) load_half<1>(cx.opB, ring, lane, 1);
    const float* ipe_src = sm_ipe + wave * (XS * 2 * 64 * 4) + lane * 4;

    // ---- alpha compositing (nerf_sample.h: the expressions nerf_fwd.hip inlines too), in pieces: a tap on layer 7 needs the weights before
    // the views layer ----------
    // Piece 1, behind a barrier that follows the densities into sm_sigma: alpha, transmittance scan, weights -> sm_w, the leftover queue,
    // the transmittance carried into the next chunk.  ONE copy of these expressions: the epilogue calls it, or tap7_early does.
    auto composite_weights = [&]() __attribute__((always_inline)) {
      const int tid2 = launder(threadIdx.x), lane2 = tid2 & 63, wave2 = tid2 >> 6;
      float alpha = 0.f, incl = 1.f;
      if (tid2 < TILE) {
        alpha = alpha_of(sm_sigma[tid2], (sm_t1[tid2] - sm_t0[tid2]) * sm_dn[tid2]);
        incl = scan_before_barrier(trans_factor(alpha), lane2, wave2, SP, sm_misc);
      }
      NM_EPI_BARRIER();
      if (tid2 < TILE) {
        const float excl = scan_after_barrier(incl, lane2, wave2, SP, sm_misc, carryT);
        sm_w[tid2] = alpha * excl;
        const int r2 = tid2 / SP, ray2 = bid * nr + r2;
        if (left && chunk == nchunks - 1 && ray2 < R && tid2 % SP == SP - 1) {
          // (zero-width tail) sample Sa is queued with the transmittance in front of it
          sm_lray[nleft + r2] = ray2;
          sm_lT[nleft + r2] = excl * trans_factor(alpha);
        }
      }
      if (nchunks > 1) carryT = scan_carry(carryT, sm_misc);
    };
    // Piece 2, once the colours are in sm_rgb: the per-sample outputs and the per-ray sums, step 1 (weights from sm_w: own write or a
    // barrier ago)
    auto composite_sums = [&]() __attribute__((always_inline)) {
      const int tid2 = launder(threadIdx.x);
      if (tid2 < TILE) {
        const float wgt = sm_w[tid2];
        const int r2 = tid2 / SP, ray2 = bid * nr + r2;
        if (ray2 < R) {
          const int s2 = chunk * TILE + tid2 % SP;
          a.weights[(size_t)ray2 * S + s2] = wgt;
          if (left && chunk == nchunks - 1) {
            // the zero-width tail carries weight exactly 0
            for (int k = Sa + 1 + tid2 % SP; k < S; k += SP) a.weights[(size_t)ray2 * S + k] = 0.f;
          }
          if (a.raw && !NM_TRACE) {
            f32x4 rv = {sm_rgb[tid2], sm_rgb[TILE + tid2], sm_rgb[2 * TILE + tid2], sm_sigma[tid2]};
            *reinterpret_cast<f32x4*>(a.raw + ((size_t)ray2 * S + s2) * 4) = rv;
          }
        }
        // w * {1, rgb, t_mid, mean} reduced over each 32-sample half wavefront
        float pq[8] = {wgt, wgt * sm_rgb[tid2], wgt * sm_rgb[TILE + tid2], wgt * sm_rgb[2 * TILE + tid2],
                       wgt * (0.5f * (sm_t0[tid2] + sm_t1[tid2])), wgt * sm_mean[tid2], wgt * sm_mean[TILE + tid2],
                       wgt * sm_mean[2 * TILE + tid2]};
        nm_half_sum_dpp8(pq);  // valid in lanes 16..31 / 48..63
        if ((tid2 & 31) == 16) {
          *reinterpret_cast<f32x4*>(sm_part + (tid2 >> 5) * 8) = f32x4{pq[0], pq[1], pq[2], pq[3]};
          *reinterpret_cast<f32x4*>(sm_part + (tid2 >> 5) * 8 + 4) = f32x4{pq[4], pq[5], pq[6], pq[7]};
        }
      }
    };
    // feat_comb max, a barrier behind sm_w: the max-weight sample of each ray slot (over all chunks so far: best_w) -> sm_misc[8 + slot],
    // and its mean as the point output
    auto pick_best = [&]() __attribute__((always_inline)) {
      const int tid2 = launder(threadIdx.x);
      if (tid2 < 8 * nr) {
        const int q = tid2 & 7, r2 = tid2 >> 3;
        const float* wv = sm_w + r2 * SP;
        int bi;
        const bool better = first_max(wv, SP, best_w, bi);
        if (q == 0) sm_misc[8 + r2] = better ? __int_as_float(r2 * SP + bi) : __int_as_float(-1);
        if (q >= 5 && better) red_acc = sm_mean[(q - 5) * TILE + r2 * SP + bi];
      }
    };
    // Tap on layer 7 with colour heads, called by layer_pass right behind the density head (cx.sig_part), in front of the views layer:
    // layer 7 is still in this wavefront's registers (c.hv) and every sample's raw density is one shuffle away, so the weights are formed
    // now and sum_s w_s h7_s is taken from c.hv -- the 32 x 1 KiB per wavefront neither go to the workspace nor come back (5 GB each way per
    // 4 x 4800 x 64 launch).  Same values, same multiplication order and same reduction as the workspace path; the eight accumulator blocks
    // are free here (finish_layer moved them out), which is what the 128 products live in.
    auto tap7_early = [&](Ctx& c) __attribute__((always_inline)) {
      const int t2 = launder(threadIdx.x), jl = (t2 >> 6) * 32 + (t2 & 31), hl = (t2 >> 5) & 1;
      const float sigma_raw = (c.sig_part + nm_shfl_xor32(c.sig_part)) + sm_small[OFF_MISC];  // (the epilogue stores the same value again)
      if (hl == 0) sm_sigma[jl] = sigma_raw;
      NM_EPI_BARRIER();  // (LDS only, like the epilogue's: the weight stream of the views layer stays in flight)
      composite_weights();
      NM_EPI_BARRIER();
      if (feat_max) {
        pick_best();
        NM_EPI_BARRIER();
      }
      const float desc = sm_small[OFF_DESCALE + 7];  // back to true units (1 unless fp16x3): folded into the weight
      const float wj = sm_w[jl] * desc;
      const int best = feat_max ? __float_as_int(sm_misc[8 + jl / SP]) : -2;
      const float mult = feat_max ? (jl == best ? desc : 0.f) : wj;  // (one multiplier per lane: see the workspace path below)
      const float* bl = sm_small + OFF_BIAS + 7 * 256 + 4 * hl;
      const float s7 = sm_small[OFF_SCALE + 7];
      // row cq = 4 block + quad holds c.hv[4 cq ..], as dump_tap lays the workspace out; rows cq and cq + 16 are made together and go
      // through the first reduction step at once, so that 64 values are live beside c.hv and not 128
      float s1[64];
#pragma unroll
      for (int cq = 0; cq < HS; ++cq) {
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(bl + (cq >> 2) * 32 + 8 * (cq & 3));
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(bl + (4 + (cq >> 2)) * 32 + 8 * (cq & 3));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = mult * __builtin_fmaxf(__builtin_fmaf(c.hv[4 * cq + e], s7, b0[e]), 0.f);
          const float y = mult * __builtin_fmaxf(__builtin_fmaf(c.hv[64 + 4 * cq + e], s7, b1[e]), 0.f);
          s1[4 * cq + e] = reduce_scatter_step16(x, y);
        }
      }
      const f32x4 sum4 = reduce_scatter_16pairs(s1, jl);
      const int r = jl & 31;
      float* prow = sm_feat + (jl >> 5) * 256 + 4 * hl;  // partial sums of this wavefront: read by the epilogue's cross-wavefront add
      *reinterpret_cast<f32x4*>(prow + (r >> 2) * 32 + 16 * ((r >> 1) & 1) + 8 * (r & 1)) = sum4;
    };
    const Tap7InRegisters<decltype(tap7_early)> tap7{early, tap7_early};
    f32x16 acc[8];
    ipe_steps<P, true>(acc, cx, ipe_src);  // layer 0
    finish_layer<P>(acc, 0, cx);
    TRACE(3);
#pragma unroll 1
    for (int l = 1; l < 8; ++l) {
      layer_pass<P, DENS>(acc, l, cx, ipe_src, tap7);
      TRACE(3 + l);
    }
    float c_r = 0.f, c_g = 0.f, c_b = 0.f;
    if (!need_rgb) {
      if (cx.tap == 7) dump_tap(7, cx);  // (in front of the wait: its stores are retired before the rows are asked back)
      NM_MLP_DONE_WAIT();
      if (cx.tap_pref) tap_prefetch<0, owns_m0<P>()>(cx);
      alpha_head(cx);
      if (cx.tap_pref) tap_prefetch<1, owns_m0<P>()>(cx);
    } else {
      // ---- views layer + rgb head.  Input: layer 7's activations (cx.hv, bias + relu like any pts layer) through the PRODUCT
      // views_w[:, :256] . feature_w that nerf_pack_split forms (feature_linear is linear: one 128 x 256 map instead of a 256 x 256
      // layer followed by a 128 x 256 one), then the direction / appearance columns ------------------------------------------
      const int hh = launder(lane) >> 5;
      const float* exr = sm_ex + launder(rl) * 48 + 8 * hh;  // K-slot (step e, half h, i) <-> extra input 16 e + 8 h + i
      f32x16 av[4];
      if constexpr (DENS) {
        views_hidden<P, true>(av, cx);
        dens_close(cx);
      } else views_hidden<P>(av, cx);
      fold_range<P>(cx, 7);  // (layer 7's output is re-packed by the views layer's K-loop)
      bf16x8 exh[VS], exl[VS];
#pragma unroll
      for (int e = 0; e < VS; ++e) {
        float v8[8];
        if (!lo_pass) {
          const f32x4 e0 = *reinterpret_cast<const f32x4*>(exr + 16 * e), e1 = *reinterpret_cast<const f32x4*>(exr + 16 * e + 4);
          v8[0] = e0[0]; v8[1] = e0[1]; v8[2] = e0[2]; v8[3] = e0[3]; v8[4] = e1[0]; v8[5] = e1[1]; v8[6] = e1[2]; v8[7] = e1[3];
        } else {
          // leftover pass: every lane has its own ray, so the per-slot table does not apply; the same view_row_value, in registers
          const float* rq = a.rays + (size_t)launder(rc) * 12 + 8;
          const float vd0 = rq[0], vd1 = rq[1], vd2 = rq[2];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int f = 16 * e + 8 * hh + i;
            const int ax = f % 3;
            float v = view_row_value(f, ax == 0 ? vd0 : ax == 1 ? vd1 : vd2, a.app_row);
            if constexpr (P == 2) v *= sm_small[OFF_INSCALE + (f < 27 ? 1 : 2)];
            v8[i] = v;
          }
        }
        if constexpr (is_split<P>()) split8_p<P>(v8, exh[e], exl[e]);
        else exh[e] = exl[e] = pack8_f16(v8);
      }
      views_extras<P>(av, cx, exh, exl, a.app_row == nullptr);
      TRACE(11);
      NM_MLP_DONE_WAIT();
      if (cx.tap_pref) tap_prefetch<0, owns_m0<P>()>(cx);
      const float* bv = sm_small + OFF_BVIEWS + 4 * hh;
      const float* wr = sm_small + OFF_WRGB + 4 * hh;
      float pr = 0.f, pg = 0.f, pb = 0.f;
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(bv + ob * 32 + 8 * q);
          const f32x4 wr4 = *reinterpret_cast<const f32x4*>(wr + ob * 32 + 8 * q);
          const f32x4 wg4 = *reinterpret_cast<const f32x4*>(wr + 128 + ob * 32 + 8 * q);
          const f32x4 wb4 = *reinterpret_cast<const f32x4*>(wr + 256 + ob * 32 + 8 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float hv = __builtin_fmaxf(acc_read(av[ob][4 * q + e]) + b4[e], 0.f);
            pr = NM_FMA(hv, wr4[e], pr);
            pg = NM_FMA(hv, wg4[e], pg);
            pb = NM_FMA(hv, wb4[e], pb);
          }
        }
      }
      pr = (pr + nm_shfl_xor32(pr)) + sm_small[OFF_MISC + 1];
      pg = (pg + nm_shfl_xor32(pg)) + sm_small[OFF_MISC + 2];
      pb = (pb + nm_shfl_xor32(pb)) + sm_small[OFF_MISC + 3];
      c_r = sigmoid(pr);
      c_g = sigmoid(pg);
      c_b = sigmoid(pb);
      if (cx.tap_pref) tap_prefetch<1, owns_m0<P>()>(cx);
    }
    const float sigma_raw = (cx.sig_part + nm_shfl_xor32(cx.sig_part)) + sm_small[OFF_MISC];
    TRACE(12);
    {
      const int jsw = launder(js);
      if ((launder(lane) >> 5) == 0) {
        sm_sigma[jsw] = sigma_raw;
        sm_rgb[jsw] = c_r; sm_rgb[TILE + jsw] = c_g; sm_rgb[2 * TILE + jsw] = c_b;
      }
    }
    NM_EPI_BARRIER();
    TRACE(13);
    const int tid2 = launder(threadIdx.x), lane2 = tid2 & 63, wave2 = tid2 >> 6;

    if (lo_pass) {
      // ---- leftover pass: lane tid2 < nent is sample Sa of ray sm_lray[tid2]; its weight is alpha * T(first Sa samples) and
      // its contributions are ADDED (atomics: they execute at L2, where this workgroup's earlier plain stores are)
      if (tid2 < nent) {
        const int ray2 = sm_lray[tid2];
        const float wgt = alpha_of(sm_sigma[tid2], (sm_t1[tid2] - sm_t0[tid2]) * sm_dn[tid2]) * sm_lT[tid2];
        sm_w[tid2] = wgt;
        a.weights[(size_t)ray2 * S + Sa] = wgt;
        if (a.acc) atomicAdd(a.acc + ray2, wgt);
        if (a.rgb && need_rgb) {
#pragma unroll
          for (int c = 0; c < 3; ++c) atomicAdd(a.rgb + (size_t)ray2 * 3 + c, a.white_bg ? wgt * sm_rgb[c * TILE + tid2] - wgt : wgt * sm_rgb[c * TILE + tid2]);
        }
        if (a.depth) atomicAdd(a.depth + ray2, wgt * (0.5f * (sm_t0[tid2] + sm_t1[tid2])));
        if (a.pts) {
#pragma unroll
          for (int c = 0; c < 3; ++c) atomicAdd(a.pts + (size_t)ray2 * 3 + c, wgt * sm_mean[c * TILE + tid2]);
        }
      }
      __syncthreads();
      if (need_tap) {
        const int jl = launder(js), hl = launder(lane) >> 5;
        const f32x4* tw = reinterpret_cast<const f32x4*>(a.ws) + ((size_t)blockIdx.x * 4 + wave2) * 32 * 64 + lane2;
        if (jl < nent) {
          const int ray2 = sm_lray[jl];
          const float desc = sm_small[OFF_DESCALE + tap];  // (workspace values carry the next layer's input scale)
          const float wj = sm_w[jl] * desc;
#pragma unroll 4
          for (int ks = 0; ks < HS; ++ks) {
            const f32x4 ta = tw[(2 * ks) * 64], tb = tw[(2 * ks + 1) * 64];
            const int n0 = (ks >> 1) * 32 + 16 * (ks & 1) + 4 * hl;  // neurons n0 .. n0+3 and n0+8 .. n0+11
            if (a.sfeat) {
              float* dsf = a.sfeat + ((size_t)ray2 * S + Sa) * 256 + n0;
              *reinterpret_cast<f32x4*>(dsf) = ta * desc;
              *reinterpret_cast<f32x4*>(dsf + 8) = tb * desc;
            }
            if (a.feat) {
              float* df = a.feat + (size_t)ray2 * 256 + n0;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                atomicAdd(df + e, wj * ta[e]);
                atomicAdd(df + 8 + e, wj * tb[e]);
              }
            }
          }
        }
      }
      __syncthreads();
      break;  // (the chunk loop; a leftover pass has a single chunk)
    }

    if (!early) composite_weights();
    composite_sums();
    NM_EPI_BARRIER();

    // ---- per-ray sums, step 2: combine the SP/32 half wavefronts of each ray ------------------------------------------
    if (tid2 < 8 * nr) {
      const int q = tid2 & 7, r2 = tid2 >> 3;
      if (!feat_max || q < 5) {
        float sum = 0.f;
        for (int hw = r2 * (SP / 32); hw < (r2 + 1) * (SP / 32); ++hw) sum += sm_part[hw * 8 + q];
        red_acc += sum;
      }
    }
    if (feat_max && !early) {
      pick_best();
      NM_EPI_BARRIER();
    }

    TRACE(14);
    // ---- feature output: weighted sum over the 32 samples of this wavefront, read back from the workspace --------------
    // (tap7_early has done this at the end of layer 7 when `early`; what follows the barrier below is common to both)
    if (need_tap && !early) {
      const int jl = launder(js), hl = launder(lane) >> 5;
      f32x4 tapv[2 * HS];
      {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's DMA rows have landed (nobody else reads them)
        // the four rows that did not fit: ordinary loads, issued now, used by the last two units (their latency sits behind the DPP work
        // of the first fourteen).  Not earlier: a compiler-tracked load in flight turns every wait on the way here into a wait for the DMA.
        f32x4 tail[4];
        {
          const f32x4* tw = reinterpret_cast<const f32x4*>(a.ws) + ((size_t)blockIdx.x * 4 + (launder(threadIdx.x) >> 6)) * 32 * 64 + (launder(threadIdx.x) & 63);
#pragma unroll
          for (int i = 0; i < 4; ++i) tail[i] = tw[(28 + i) * 64];
        }
        const float* lr = ring + (launder(threadIdx.x) >> 6) * SLOT_FLOATS + (launder(threadIdx.x) & 63) * 4;
        const float* li = sm_ipe + (launder(threadIdx.x) >> 6) * (XS * 2 * 64 * 4) + (launder(threadIdx.x) & 63) * 4;
#pragma unroll
        for (int c = 0; c < 2 * HS; ++c)
          tapv[c] = c < 16 ? *reinterpret_cast<const f32x4*>(lr + c * 256) : c < 28 ? *reinterpret_cast<const f32x4*>(li + (c - 16) * 256) : tail[c - 28];
      }
      const float desc = sm_small[OFF_DESCALE + tap];             // back to true units (1 unless fp16x3): folded into the weight
      const float wj = sm_w[jl] * desc;
      const int rsel = jl / SP;                                   // ray slot of this lane's sample
      const int best = feat_max ? __float_as_int(sm_misc[8 + rsel]) : -2;
      float* prow = sm_feat + (jl >> 5) * 256 + 4 * hl;           // partial sums of this wavefront
      if (a.sfeat && ray < R) {
#pragma unroll
        for (int ks = 0; ks < HS; ++ks) {
          const f32x4 ta = tapv[2 * ks], tb = tapv[2 * ks + 1];
          float* dsf = a.sfeat + ((size_t)ray * S + sidx) * 256 + (ks >> 1) * 32 + 16 * (ks & 1) + 4 * hl;
          *reinterpret_cast<f32x4*>(dsf) = ta * desc;
          *reinterpret_cast<f32x4*>(dsf + 8) = tb * desc;
        }
      }
      if (a.feat) {
        float wv[128];
        // one multiplier per lane (the sample's weight; feat_comb max: the descale for the selected sample, 0 for the others -- the tapped
        // activations are finite and >= 0, so 0 * v is the 0.f the select produced): a run-time select per VALUE cost 270 v_cndmask here
        const float mult = feat_max ? (jl == best ? desc : 0.f) : wj;
#pragma unroll
        for (int c = 0; c < 2 * HS; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) wv[4 * c + e] = mult * tapv[c][e];
        const f32x4 sum4 = reduce_scatter_32rows(wv, jl);
        // lane (half hl, r = jl & 31) holds row r: K-step unit r >> 1, second quad if r & 1 -> neurons 32 (r >> 2) + 16 ((r >> 1) & 1) + 8 (r & 1) + 4 hl + 0..3
        const int r = jl & 31;
        *reinterpret_cast<f32x4*>(prow + (r >> 2) * 32 + 16 * ((r >> 1) & 1) + 8 * (r & 1)) = sum4;
      }
    }
    TRACE(15);
    __syncthreads();
    TRACE(16);
    if (a.feat) {
      // combine the wavefronts of each ray: SP samples = SP/32 wavefronts
      const int wpr = SP / 32;  // wavefronts per ray slot (1, 2 or 4)
      for (int r2 = 0; r2 < nr; ++r2) {
        float f = 0.f;
        bool any = !feat_max;
        if (feat_max) {
          const int best = __float_as_int(sm_misc[8 + r2]);
          any = best >= 0;
        }
        for (int w2 = 0; w2 < wpr; ++w2) f += sm_feat[(r2 * wpr + w2) * 256 + tid2];
        const int ray2 = bid * nr + r2;
        if (nchunks > 1) {
          if (feat_max) { if (any) feat_run = f; }
          else feat_run += f;
          f = feat_run;
        }
        if (ray2 < R && chunk == nchunks - 1 && (any || nchunks > 1)) a.feat[(size_t)ray2 * 256 + tid2] = f;
      }
    }
    __syncthreads();
  }

  if (lo_pass) {
    nleft = 0;
    continue;
  }
  if (tid < 8 * nr) {
    const int q = tid & 7, r2 = tid >> 3, ray2 = bid * nr + r2;
    const float accv = __shfl(red_acc, lane & ~7, 64);
    if (ray2 < R) {
      if (q == 0) { if (a.acc) a.acc[ray2] = red_acc; }
      else if (q <= 3) { if (a.rgb && need_rgb) a.rgb[(size_t)ray2 * 3 + (q - 1)] = a.white_bg ? red_acc + (1.0f - accv) : red_acc; }
      else if (q == 4) { if (a.depth) a.depth[ray2] = red_acc; }
      else { if (a.pts) a.pts[(size_t)ray2 * 3 + (q - 5)] = red_acc; }
    }
  }
  TRACE(17);
  if (left) nleft += (R - bid * nr) < nr ? (R - bid * nr) : nr;
  bid += gridDim.x;
  }  // tile loop
  if constexpr (P == 2) {
    // range telemetry / saturation flag: once per workgroup lifetime.  A re-packed value AT the fp16 limit (v_med3 clamps there)
    // means some operand of this launch was saturated: status[0] |= 1, which the caller turns into a re-run on the fp32 kernel
    // (nm_nerf_fwd_guarded reads the flag on the device) -- the fp16x3 path never returns silently clamped results.
    __syncthreads();
    if (a.status && tid < NRANGE) {
      unsigned m = 0u;
      for (int i = 0; i < 256; ++i) m = max(m, sm_rng[tid * 256 + ((i + 32 * tid) & 255)]);
      if (m) atomicMax(reinterpret_cast<unsigned*>(a.status) + 1 + tid, m);
      if (m >= __float_as_uint(F16_MAX)) atomicOr(a.status, 1);
    }
  }
}

__global__ void __launch_bounds__(256, 1) nerf_fwd_bf16x3_kernel(NerfArgs a) { nerf_fwd_body<0>(a); }
__global__ void __launch_bounds__(256, 1) nerf_fwd_fp16x1_kernel(NerfArgs a) { nerf_fwd_body<1>(a); }
__global__ void __launch_bounds__(256, 1) nerf_fwd_fp16x3_kernel(NerfArgs a) { nerf_fwd_body<2, false>(a); }
__global__ void __launch_bounds__(256, 1) nerf_fwd_fp16x3_tap7_kernel(NerfArgs a) { nerf_fwd_body<2, true>(a); }

}  // namespace

extern "C" size_t nm_nerf_workspace_bytes_bf16x3(void) { return (size_t)WS_WORKGROUPS * TILE * 256 * sizeof(float); }

static int nerf_fwd_split(int mode, const void* blob, const float* rays, const float* t, const float* app_row, int R, int S, int tap_layer,
                          int white_bg, float var_scale, int flags, float* weights, float* feat, float* pts, float* rgb, float* depth,
                          float* acc, float* raw, float* sample_feat, void* workspace, const int* zero_tail_violation, nmStream_t stream,
                          int* status = nullptr) {
  NM_CHECK_ARG(blob && rays && t && weights && R > 0 && S > 0);
  if (!(S == 32 || S == 64 || (S % 128) == 0)) return NM_ERR_UNSUPPORTED;
  if (tap_layer > 7) return NM_ERR_ARG;
  if ((feat || sample_feat) && !workspace) return NM_ERR_WORKSPACE;
  NerfArgs a;
  a.ws = (float*)workspace;
  a.blob = (const char*)blob; a.rays = rays; a.t = t; a.app_row = app_row;
  a.weights = weights; a.feat = feat; a.pts = pts; a.rgb = rgb; a.depth = depth; a.acc = acc; a.raw = raw; a.sfeat = sample_feat;
  a.R = R; a.S = S; a.tap = tap_layer; a.white_bg = white_bg; a.flags = flags; a.var_scale = var_scale;
  a.status = status;
  // NM_NERF_ZERO_TAIL: samples 0 .. S/2 are evaluated (S/2 by the regular tiles, sample S/2 by leftover passes)
  // (S/2 must itself be a supported row length: 32, 64, 128 or a multiple of 128)
  const bool zero_tail = (flags & NM_NERF_ZERO_TAIL) && (S == 64 || S == 128 || (S >= 256 && S % 256 == 0)) && !raw && !sample_feat &&
                         !(flags & NM_NERF_FEAT_MAX);
  a.Sa = zero_tail ? S / 2 : S;
  a.left = zero_tail ? 1 : 0;
  const int SP = a.Sa < TILE ? a.Sa : TILE, nr = TILE / SP;
  a.ntiles = (R + nr - 1) / nr;
  const int SPf = S < TILE ? S : TILE, nrf = TILE / SPf;
  a.ntiles_full = (R + nrf - 1) / nrf;
  a.tail_viol = zero_tail ? zero_tail_violation : nullptr;
  const int ncu = nm_stream_cus(stream);  // (a CU-partitioned stream runs one workgroup per CU of its partition)
  const int grid = a.ntiles < ncu ? a.ntiles : (ncu < WS_WORKGROUPS ? ncu : WS_WORKGROUPS);
  // (the two-wavefronts-per-SIMD experiment of round 2, 12 % slower, lives in scripts/variants/ now: DESIGN.md section 3.1c)
  if (mode == 1) nerf_fwd_fp16x1_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
  else if (mode == 2) {
    // (the condition of `early` in nerf_fwd_body, without its per-tile part)
    const bool tap7_early = !(flags & NM_NERF_SKIP_RGB) && (tap_layer < 0 || tap_layer == 7) && feat && !sample_feat;
    if (tap7_early) nerf_fwd_fp16x3_tap7_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
    else nerf_fwd_fp16x3_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
  }
  else nerf_fwd_bf16x3_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
  return nm_launch_status();
}

extern "C" int nm_nerf_fwd_bf16x3(const void* blob, const float* rays, const float* t, const float* app_row, int R, int S,
                                  int tap_layer, int white_bg, float var_scale, int flags, float* weights, float* feat, float* pts,
                                  float* rgb, float* depth, float* acc, float* raw, float* sample_feat, void* workspace,
                                  const int* zero_tail_violation, nmStream_t stream) {
  return nerf_fwd_split(0, blob, rays, t, app_row, R, S, tap_layer, white_bg, var_scale, flags, weights, feat, pts, rgb, depth, acc, raw,
                        sample_feat, workspace, zero_tail_violation, stream);
}

extern "C" int nm_nerf_fwd_fp16x1(const void* blob, const float* rays, const float* t, const float* app_row, int R, int S,
                                  int tap_layer, int white_bg, float var_scale, int flags, float* weights, float* feat, float* pts,
                                  float* rgb, float* depth, float* acc, float* raw, float* sample_feat, void* workspace,
                                  const int* zero_tail_violation, nmStream_t stream) {
  return nerf_fwd_split(1, blob, rays, t, app_row, R, S, tap_layer, white_bg, var_scale, flags, weights, feat, pts, rgb, depth, acc, raw,
                        sample_feat, workspace, zero_tail_violation, stream);
}

extern "C" int nm_nerf_fwd_fp16x3(const void* blob, const float* rays, const float* t, const float* app_row, int R, int S,
                                  int tap_layer, int white_bg, float var_scale, int flags, float* weights, float* feat, float* pts,
                                  float* rgb, float* depth, float* acc, float* raw, float* sample_feat, void* workspace,
                                  const int* zero_tail_violation, int* status, nmStream_t stream) {
  return nerf_fwd_split(2, blob, rays, t, app_row, R, S, tap_layer, white_bg, var_scale, flags, weights, feat, pts, rgb, depth, acc, raw,
                        sample_feat, workspace, zero_tail_violation, stream, status);
}
