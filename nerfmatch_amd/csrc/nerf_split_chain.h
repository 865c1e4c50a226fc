// The K-loop machinery of the operand-splitting NeRF MLP kernels ("bf16x3" / "fp16x3" / "fp16x1"): everything the bodies of both
// kernel files call -- nerf_fwd_bf16.hip (the fused per-ray render, whose header comment describes the structure) and
// nerf_points_bf16.hip (the pointwise forward / backward pair of the iNeRF refinement).  Mode traits, the LDS ring of weight slots and
// its barrier protocol, the loop-carried state (Ctx), the re-packing of a finished layer in the shadow of its consumer's MFMAs
// (UnitWork), the K-steps (slot_step8 / 4 / 4x2) and the layer walk built from them (ipe_steps, layer_pass, views_*).
// Everything here is __forceinline__: the two files compile to the device code they had as one translation unit.
#pragma once
#include "nerf_bf16_common.h"

namespace nmbf {

// Arithmetic mode P of the layer products (template parameter of everything below):
//   P = 0  "bf16x3": operands split into bf16 hi / lo parts, three MFMAs per product block (16 KiB weight slots: hi and lo)
//   P = 2  "fp16x3": the same with fp16 hi / lo parts (22 instead of 16 mantissa bits; saturating at the fp16 range)
//   P = 1  "fp16x1": operands rounded once to fp16, ONE MFMA per product block (8 KiB slots) -- opt-in throughput mode of
//                    the lean render's coarse pass: DESIGN.md section 3.1d
//   P = 4  bf16x3 + the ReLU gates of every layer recorded as bits (the pointwise forward of the iNeRF refinement, nerf_points_bf16.hip)
//   P = 3  bf16x3 of the pointwise backward: the arithmetic of P = 0 with the weight request of rounds 7-10 (see owns_m0)
// Operands are carried as 16-byte vectors typed bf16x8 in all modes; P = 1, 2 reinterpret them as 8 x fp16.
template <int P> constexpr bool is_bf16() { return P == 0 || P == 3 || P == 4; }
template <int P> constexpr bool has_gates() { return P == 4; }
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
template <int P>
__device__ __forceinline__ f32x16 mfma_p(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  if constexpr (is_bf16<P>()) return MFMA_BF16(a, b, c);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <int P> constexpr bool is_split() { return P != 1; }  // hi / lo operand pairs, three products
template <int P> constexpr int slot_bytes() { return is_split<P>() ? SLOT_BYTES : SLOT_BYTES / 2; }
template <int P> constexpr int slot_floats() { return slot_bytes<P>() / 4; }
// ring geometry: the same 64 KiB hold 4 slots of 16 KiB or 8 of 8 KiB; a slot is requested `ring_ahead` K-steps before its use
// (fp16x1: a K-step is 8 MFMAs, ~300 cycles -- two steps ahead would be less than the L2 -> LDS latency)
template <int P> constexpr int ring_slots() { return is_split<P>() ? NRING : 2 * NRING; }
template <int P> constexpr int ring_ahead() { return is_split<P>() ? 4 : 6; }
constexpr float F16_MAX = 65504.0f;
// x = hi + lo with hi, lo fp16 (round to nearest even), x clamped to the fp16 range first
__device__ __forceinline__ void split8_f16(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
  f16x8 h8, l8;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float c = __builtin_amdgcn_fmed3f(v[i], -F16_MAX, F16_MAX);
    const _Float16 h = (_Float16)c;
    h8[i] = h;
    l8[i] = (_Float16)(c - (float)h);
  }
  hi = __builtin_bit_cast(bf16x8, h8);
  lo = __builtin_bit_cast(bf16x8, l8);
}
template <int P>
__device__ __forceinline__ void split8_p(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
  if constexpr (is_bf16<P>()) split8(v, hi, lo);
  else split8_f16(v, hi, lo);
}
template <int P>
__device__ __forceinline__ float* ring_slot(float* ring, int g) { return ring + (g & (ring_slots<P>() - 1)) * slot_floats<P>(); }
__device__ __forceinline__ unsigned pack_f16(float a, float b) {  // v_cvt_pk_f16_f32 (round to nearest even, two values)
  const f16x2 h = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ bf16x8 pack8_f16(const float (&v)[8]) {
  const u32x4 r = {pack_f16(v[0], v[1]), pack_f16(v[2], v[3]), pack_f16(v[4], v[5]), pack_f16(v[6], v[7])};
  return __builtin_bit_cast(bf16x8, r);
}
// Parks the B operands of the 6 IPE K-steps of one wavefront in LDS (dst: the lane's 16 bytes of the wavefront's block).  K-slot (step m,
// half h, i) holds encoding 45 h + idx, idx = 8 m + i < 45 (the last three slots of step 5 are padding); value(idx) yields this lane's
// value -- idx is a compile-time constant after unrolling.  Split modes store hi and lo operands, fp16x1 the one rounded operand.
template <int P, class F>
__device__ __forceinline__ void park_ipe(float* dst, F value) {
#pragma unroll
  for (int m = 0; m < XS; ++m) {
    float v8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = 8 * m + i;
      if (idx < 45) v8[i] = value(idx);
      else v8[i] = 0.f;
    }
    if constexpr (is_split<P>()) {
      bf16x8 h8, l8;
      split8_p<P>(v8, h8, l8);
      *reinterpret_cast<u32x4*>(dst + (m * 2 + 0) * 256) = __builtin_bit_cast(u32x4, h8);
      *reinterpret_cast<u32x4*>(dst + (m * 2 + 1) * 256) = __builtin_bit_cast(u32x4, l8);
    } else {
      *reinterpret_cast<u32x4*>(dst + m * 256) = __builtin_bit_cast(u32x4, pack8_f16(v8));
    }
  }
}

// The 4 pieces share ONE global address and ONE M0 (LDS base) and differ only in the instruction's immediate offset,
// which the hardware adds on both sides -- measured 31 instead of 58 cycles of issue per piece beside the MFMAs.
// Address = uniform slot base (SGPR pair) + one 32-bit per-lane offset: no 64-bit VGPR arithmetic per slot.
// Who owns M0: a kernel of the split modes issues EVERY LDS-DMA as inline asm (here, ring_request, the render kernel's tap_prefetch), so the
// compiler emits no instruction of its own that reads or writes M0 in it and the asm sets M0 without handing it back (M0 is reserved: a
// clobber of it is not honoured, which is why a kernel that keeps one builtin LDS-DMA -- fp16x1 -- keeps the builtin everywhere and the
// save / restore around its asm pieces).  `scripts/kstep_gaps.py --m0` lists what touches M0 in a kernel; tests/test_nerf_m0_cpu.py runs it.
// The pointwise backward (P = 3) stays as it was as well: with the running request state of ring_arm its register allocation, which has no
// VGPR to spare, went to scratch (651 VGPR spills).
template <int P> constexpr bool owns_m0() { return is_split<P>() && P != 3; }
template <int P>
__device__ __forceinline__ void dma_slot(const char* blob_slots, int g, float* ring, int wave, int lane) {
  const unsigned voff = (unsigned)(wave * (slot_bytes<P>() / 4) + lane * 16);
  const char* base = blob_slots + (size_t)g * slot_bytes<P>();  // uniform
  if constexpr (owns_m0<P>()) {
    const float* q = ring_slot<P>(ring, g) + wave * (slot_floats<P>() / 4);
    const unsigned lds = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(const __attribute__((address_space(3))) float*)q);
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\t"
                 "global_load_lds_dwordx4 %1, %2 offset:2048\n\tglobal_load_lds_dwordx4 %1, %2 offset:3072"
                 :: "s"(lds), "v"(voff), "s"(base) : "memory");
    return;
  }
  const auto* src = (const __attribute__((address_space(1))) void*)(base + voff);
  auto* dst = (__attribute__((address_space(3))) void*)(ring_slot<P>(ring, g) + wave * (slot_floats<P>() / 4));
  __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
  __builtin_amdgcn_global_load_lds(src, dst, 16, 1024, 0);
  if constexpr (is_split<P>()) {
    __builtin_amdgcn_global_load_lds(src, dst, 16, 2048, 0);
    __builtin_amdgcn_global_load_lds(src, dst, 16, 3072, 0);
  }
}

// Ring protocol for slot g (identical sequence in all 4 wavefronts):
//   wait until this wavefront's DMA pieces of slot g have landed (at most the 4 instructions of slot g+1 may remain
//   in flight), barrier (=> every wavefront's pieces landed AND everybody finished reading slot g-1... g-2), then
//   start the DMA of slot g+2 into the ring position that slot g-2 occupied.
template <int P>
__device__ __forceinline__ void ring_acquire(const char* blob_slots, int g, int nslots, float* ring, int wave, int lane) {
  if constexpr (is_split<P>()) {
    NM_WAIT_VMCNT(4);  // (slot g+1 is always in flight: the stream runs on into the blob's padding)
  } else {
    // Branch free: the stream simply runs on past the tile's last slot (the blob is padded by ring_ahead slots), so slots
    // g+1 .. g+5 are ALWAYS in flight here, 2 DMA instructions per wavefront each.  (A first version that counted the
    // remaining slots cost ten scalar branches per K-step -- as much as the 8 MFMAs.)
    NM_WAIT_VMCNT(10);
  }
  __builtin_amdgcn_s_barrier();
  if constexpr (is_split<P>()) dma_slot<P>(blob_slots, g + ring_ahead<P>(), ring, wave, lane);
  // (fp16x1: this form only opens a tile -- slot 0 landed, slots 1..5 in flight, nothing new requested; inside the stream
  //  ring_acquire_pair does the work for two K-steps at once)
}

// Split modes, NM_RING_PAIRS: ONE barrier per two K-steps.  The s_memtime trace with the barrier compiled out
// (scripts/trace_nerf.py on the -DNM_ABL=2 build of scripts/variants/nerf_study_switches_r6.patch) put the per-K-step barrier at 196 of a K-step's 1150 cycles -- more than the weight DMA
// (81), the operand reads (160) or the re-packing (143): four wavefronts on four SIMDs re-synchronised every 24 MFMAs pay the
// slowest one's stalls every time.  Called in the middle of every ODD K-step g (8-block layers; at the start of it in the views
// layer): slots g+1 and g+2 -- requested one K-step ago, in the first half of K-step g-1 (ring_request) -- must have landed (this
// wavefront's pieces: vmcnt(0); everybody's: the barrier).  Behind it the ring positions of slots g-1 and g are free for good: their
// last reads (the second-half operands of slot g, fetched in the first half of K-step g) every wavefront issued before it arrived
// here.  The 4-slot ring suffices: two slots in use, two in flight.
__device__ __forceinline__ void ring_acquire_two() {
  // lgkmcnt(0): this wavefront's own reads of slot g (issued 8 MFMAs ago) have RETURNED before it signals the barrier -- the DMA
  // another wavefront issues behind the barrier overwrites that ring position
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// fp16x3: an LDS wait the COMPILER sees, placed where every outstanding ds_read was issued several MFMAs ago (it costs nothing there).
// The compiler's own waits in these K-loops are all lgkmcnt(0), put in front of the first MFMA that needs a register it has not waited
// for yet -- without this one that is an MFMA one or two gaps behind FRESH operand reads, whose whole LDS latency it then sits out
// (hipcc -S of the parent: a wait right behind the B reads of first-half gaps 0, 1 of every odd K-step and behind the bias reads of
// every views-layer half).  With the reads of the next K-step's A operands retired here, its waits fall in front of a half's first
// MFMA, where everything pending is old.  (simm16: vmcnt 63, expcnt 7, lgkmcnt 0)
template <int P>
__device__ __forceinline__ void lds_retire() {
  if constexpr (P == 2) __builtin_amdgcn_s_waitcnt(0xC07F);
}

// fp16x1, called in every EVEN K-step g: slots g+1 and g+2 have landed when at most the 6 DMA instructions of slots g+3..g+5
// remain in flight; one barrier for both; then slots g+6 and g+7 are requested into the ring positions of slots g-2 and g-1
// (every wavefront is past their MFMAs).  Halves the barriers / counted waits per MFMA of a stream whose K-step is 8 MFMAs.
__device__ __forceinline__ void ring_acquire_pair(const char* blob_slots, int g, float* ring, int wave, int lane) {
  NM_WAIT_VMCNT(6);
  __builtin_amdgcn_s_barrier();
  dma_slot<1>(blob_slots, g + 6, ring, wave, lane);
  dma_slot<1>(blob_slots, g + 7, ring, wave, lane);
}

// A operands of half a slot: 4 output blocks x (hi, lo) = 8 x 16 bytes per lane.
struct OpHalf {
  bf16x8 h[4], l[4];
};

template <int P>
__device__ __forceinline__ void load_half(OpHalf& d, const float* slot, int lane, int p) {
  const u32x4* s4 = reinterpret_cast<const u32x4*>(slot) + lane;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    if constexpr (is_split<P>()) {
      d.h[o] = __builtin_bit_cast(bf16x8, s4[((4 * p + o) * 2 + 0) * 64]);
      d.l[o] = __builtin_bit_cast(bf16x8, s4[((4 * p + o) * 2 + 1) * 64]);
    } else {
      d.h[o] = __builtin_bit_cast(bf16x8, s4[(4 * p + o) * 64]);
    }
  }
}

// Loop-carried state of the layer pipeline (all per wavefront; Unit = the B operands of one K-step: bf16x3.h)
struct Ctx {
  const char* blob_slots;
  float* ring;
  const float* sm_small;
  f32x4* tapw;      // this lane's column of the workspace
  // NM_TAP_PREFETCH: read-back of the tile's tapped activations (32 rows of 1 KiB per wavefront; the workspace of the 32 CUs of an XCD
  // is as large as their L2, so the rows come back over the fabric: 6.6 k cycles when the reduction asks for them itself)
  bool tap_pref;    // this tile reads its tap back (a feature output is wanted, regular tile)
  bool rgb;         // the pass has colour heads (the views K-loop is the tile's last; else layer 7's)
  float* tap_ring;  // landing zones of this wavefront, both free once the tile's last K-loop is over: ring slot `wave` (rows 0..15)
  float* tap_ipe;   //   and its IPE operand region (rows 16..27); rows 28..31 are loaded by the reduction itself, behind its first 14 units
  int nslots, wave, lane, hi;
  int tap;          // layer whose activations are tapped (-1: none)
  int g;            // next weight slot
  unsigned dma_voff;  // split modes, ring_request: this lane's byte offset inside a slot (its wavefront's quarter + 16 lane) and
  unsigned dma_lds;   //   (P = 3) the LDS byte address of its wavefront's quarter of ring position 0 (uniform: an SGPR); set by ring_open_wait
  // owns_m0: the running state of the weight request, all uniform (SGPRs), set by ring_open_wait and stepped by ring_arm:
  unsigned long long dma_p, dma_q;  // global address of the second / the first slot of the request being issued (before ring_arm: dma_p = the
                                    //   last slot requested so far)
  unsigned dma_m, dma_s;            // LDS byte address of this wavefront's quarter of the request's first ring position (0 or 2), and the
                                    //   sum of the two (the position steps and wraps as m = s - m)
  OpHalf opA;       // A operands of the next half slot, fetched one half slot ahead
  OpHalf opB;       // fp16x1: blocks 4-7 of the next slot (the whole slot is fetched one K-step ahead there)
  f32x4 hb0, hb1;   // split modes: biases of unit 0 of the layer being finished, read by its last K-step (AccTake) for finish_layer
  Unit xn;          // B operands of the next hidden K-step
  float sig_part;   // this lane's partial dot product of the density head
  float dp[4];      // fp16x3, density head accumulated in the views K-loop (UnitWork<2, true>): the four partial sums of alpha_head,
  float dv[3], dw[3];  //   and the three terms a unit hands to the next one
  f32x4 nb0, nb1;   // fp16x3: the biases of the NEXT unit to be made, read by the unit in front of it (UnitWork::bias_next; unit 1's by finish_layer)
  float sc;         // fp16x3: s_l of the finished layer in cx.hv (OFF_SCALE), wavefront-uniform -> lives in an SGPR: the re-packing fma
                    // has two VGPR sources like the add it replaces
  float vmax;       // fp16x3: running max |re-packed value| of the layer being consumed (range telemetry / saturation flag)
  unsigned* rng;    // this thread's column of the [NRANGE][256] LDS table
  u32x4* gptr;       // P = 4: this thread's cell of the gate table of the tile in flight, [layer][256 threads] x 16 bytes
  unsigned gbits[4]; // P = 4: ReLU gates of the layer being re-packed, 8 bits per unit (bit k < 4: element 2k, bit 4 + k: element 2k + 1)
  float hv[128];    // finished layer (raw accumulators, before bias/relu), lane local: hv[16 block + register]
};

// Split modes: every EVEN K-step g requests slots g+2 and g+3 into the ring positions of slots g-2 and g-1, which the barrier of K-step
// g-1 freed -- one of the eight pieces behind each of eight MFMAs that carry little else (8-block layers: the tail of the first half;
// views layer: MFMAs 4..11), and not as a burst right behind that barrier: eight pieces back to back were ~250 cycles in which this SIMD
// issued no MFMA, paid by all four wavefronts together because the barrier had just re-aligned them.  The barrier of K-step g+1
// (ring_acquire_two: vmcnt(0)) retires them, a K-step of ~1100 cycles after the request against 250-400 of L2-warm landing time.  A
// tile opens with slots 0 and 1 (ring_open); past its last slot the stream runs on into the blob's padding, branch free.
// Piece j & 3 of slot g + 2 + (j >> 2): the same address, M0 and immediate offsets as dma_slot's four.  Inline asm like tap_prefetch
// (nerf_fwd_bf16.hip): the compiler cannot tell these LDS writes from the operands the next ds_read fetches
// and may wait vmcnt(0) in front of it; and the address is the uniform slot base in an SGPR pair plus the lane's 32-bit offset -- no
// 64-bit VGPR pair kept alive beside the accumulators (the pointwise backward has none to spare).  One asm statement per piece and no
// sched_barrier of its own where a work piece shares the gap: the K-loops' bodies are close to the size up to which `#pragma unroll`
// unrolls fully, and a loop left rolled indexes cx.hv at run time -- Ctx in scratch.
// Round 11: a DMA gap holds the piece and nothing else.  A scalar instruction takes an issue turn like a VALU one (scripts/ubench/fillers.hip:
// six per gap hide behind an MFMA, ten do not; ten beside a piece cost 50 cycles), and through round 10 the first piece of a slot had the
// 64-bit `blob_slots + slot * 16 KiB`, the ring position from `g` and the M0 save / set / restore beside it, 9-11 scalar instructions.  Now
// the request's addresses are running state (Ctx::dma_p, dma_q, dma_m), stepped by ring_arm in two gaps in FRONT of the request's first piece
// that carry no DMA (three scalar instructions each), M0 is set there once for the first slot, and the second slot's ring position -- always
// the next one: a request is an (even, odd) pair of slots -- is one s_add on M0 behind the first slot's last piece.  The requests of a tile
// are consecutive pairs of slots starting with (2, 3), so the state needs no slot number: ring_open_wait resets it where cx.g is reset.
template <int P>
__device__ __forceinline__ void ring_arm(Ctx& cx, int stage) {
  if constexpr (!owns_m0<P>()) return;
  if (stage == 0) {
    cx.dma_q = cx.dma_p + (unsigned)slot_bytes<P>();
    cx.dma_m = cx.dma_s - cx.dma_m;
    asm volatile("" : "+s"(cx.dma_q), "+s"(cx.dma_m));  // (made here, not where the pieces use them)
  } else {
    cx.dma_p = cx.dma_q + (unsigned)slot_bytes<P>();
    asm volatile("s_mov_b32 m0, %1" : "+s"(cx.dma_p) : "s"(cx.dma_m));
  }
}
// (g: the even K-step the request belongs to -- used by the form that does not own M0 only, which makes every piece's addresses from it and
//  hands M0 back as found)
template <int P>
__device__ __forceinline__ void ring_request(const Ctx& cx, int g, int j) {
  static_assert(slot_bytes<P>() == 0x4000 || !is_split<P>(), "the M0 step behind piece 3 is one slot");
  if constexpr (!owns_m0<P>()) {
    const int slot = g + 2 + (j >> 2);
    const char* base = cx.blob_slots + (size_t)slot * slot_bytes<P>();  // uniform
    const unsigned lds = cx.dma_lds + (unsigned)(slot & (ring_slots<P>() - 1)) * slot_bytes<P>();
    unsigned m0_saved;
#define NM_DMA_PIECE(OFS)                                                                                                        \
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %2, %3 offset:" #OFS "\n\ts_mov_b32 m0, %0" \
               : "=&s"(m0_saved) : "s"(lds), "v"(cx.dma_voff), "s"(base) : "memory")
    switch (j & 3) {  // (a compile-time constant after unrolling)
      case 0: NM_DMA_PIECE(0); break;
      case 1: NM_DMA_PIECE(1024); break;
      case 2: NM_DMA_PIECE(2048); break;
      default: NM_DMA_PIECE(3072); break;
    }
#undef NM_DMA_PIECE
    return;
  }
#define NM_DMA_PIECE(OFS, BASE) asm volatile("global_load_lds_dwordx4 %0, %1 offset:" #OFS :: "v"(cx.dma_voff), "s"(BASE) : "memory")
  switch (j) {  // (a compile-time constant after unrolling)
    case 0: NM_DMA_PIECE(0, cx.dma_q); break;
    case 1: NM_DMA_PIECE(1024, cx.dma_q); break;
    case 2: NM_DMA_PIECE(2048, cx.dma_q); break;
    case 3:  // (+ M0 to the second slot's ring position)
      asm volatile("global_load_lds_dwordx4 %0, %1 offset:3072\n\ts_add_u32 m0, m0, 0x4000" :: "v"(cx.dma_voff), "s"(cx.dma_q) : "memory", "scc");
      break;
    case 4: NM_DMA_PIECE(0, cx.dma_p); break;
    case 5: NM_DMA_PIECE(1024, cx.dma_p); break;
    case 6: NM_DMA_PIECE(2048, cx.dma_p); break;
    default: NM_DMA_PIECE(3072, cx.dma_p); break;
  }
#undef NM_DMA_PIECE
}
// fp16x3, 8-block layers (slot_step8<.., RQE = true>): the ring positions an even K-step g fills are free as soon as the barrier in the
// middle of odd K-step g-1 has passed, and that K-step's second-half gaps 5-10 carry nothing in this mode.  So pieces 0..5 go there, one
// per gap, and pieces 6, 7 into first-half gaps 4, 5 of K-step g: the youngest piece is asked for ~31 MFMAs in front of the barrier that
// waits for it instead of 24, the oldest ~43 instead of 32.  Same pieces, same barrier.  Only for a pair (odd g-1, even g) inside one
// K-loop: a layer's last K-step fills those gaps with AccTake, and a tile's first K-step has no predecessor -- the K-step behind either
// keeps all eight pieces; the views layer's seq() leaves no empty gaps either.  The bf16 modes use second-half gaps 5-10 for the re-packing.
template <int P> constexpr bool request_early() { return P == 2; }
// Opens a tile's weight stream: the slots K-step 0 does not request itself
template <int P>
__device__ __forceinline__ void ring_open(const char* blob_slots, float* ring, int wave, int lane) {
#pragma unroll
  for (int g0 = 0; g0 < (is_split<P>() ? 2 : ring_ahead<P>()); ++g0) dma_slot<P>(blob_slots, g0, ring, wave, lane);
}
// ... and waits for them (split modes), everybody's pieces: barrier
template <int P>
__device__ __forceinline__ void ring_open_wait(Ctx& cx) {
  cx.dma_voff = (unsigned)(cx.wave * (slot_bytes<P>() / 4) + cx.lane * 16);
  const float* q = cx.ring + cx.wave * (slot_floats<P>() / 4);
  const unsigned lds0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(const __attribute__((address_space(3))) float*)q);
  if constexpr (owns_m0<P>()) {
    // the first request is slots (2, 3) into ring positions (2, 3): ring_arm steps from "slot 1 requested last, position 0"
    cx.dma_m = lds0; cx.dma_s = 2u * lds0 + 2u * (unsigned)slot_bytes<P>();
    cx.dma_p = (unsigned long long)(size_t)(cx.blob_slots + slot_bytes<P>());
    cx.dma_q = cx.dma_p;
  } else {
    cx.dma_lds = lds0;
  }
  NM_WAIT_VMCNT(0);
  __builtin_amdgcn_s_barrier();
}

// 8 gate bits of one unit from its four packed hi words (two bf16 halves each): bit k = low half of word k non-zero, bit 4 + k = high half
__device__ __forceinline__ unsigned gate_byte(const u32x4& h) {
  // v_pk_min_u16 against (1, 1): 0 / 1 per half.  (Inline asm on scalars: the vector-typed __builtin_elementwise_min on a bit-cast
  // element of the ext-vector came out reading word 0 four times -- scripts/ubench/gate_byte.hip.)
  const unsigned w0 = h[0], w1 = h[1], w2 = h[2], w3 = h[3];
  unsigned m0, m1, m2, m3;
  const unsigned one = 0x00010001u;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(m0) : "v"(w0), "v"(one));
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(m1) : "v"(w1), "v"(one));
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(m2) : "v"(w2), "v"(one));
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(m3) : "v"(w3), "v"(one));
  const unsigned t = m0 | (m1 << 1) | (m2 << 2) | (m3 << 3);
  return (t & 0xfu) | ((t >> 12) & 0xf0u);
}

// Unit u of the finished layer lo held in cx.hv: registers 8m .. 8m+7 (m = u & 1) of output block u >> 1, i.e. neurons
// 32 (u>>1) + 16 m + 4 half + {0..3, 8..11}  ->  + bias, relu, hi/lo split.
// Cut into operations of 1..5 VALU instructions which the K-steps place in the gaps behind their MFMAs by the tables below
// ("Per-gap schedule"), pinned with sched_barriers, so that the re-packing runs in the shadow of the matrix pipe.  Branch free on
// purpose: the operations must stay inside the MFMAs' basic block.  The operations of a unit (split modes; element pairs p = 0..3):
//   bias()          the two bias reads (LDS), >= 2 gaps in front of the first ra / rb / relu
//   ra(j), rb(j)    element j / element 4 + j: bias, relu (fp16x3: input scale, clamp; rb also folds both into the running maximum);
//   relu(j)         = both in one gap
//   hi(p)           packed hi halves of elements 2p, 2p+1 (bf16 modes: + their fp32 values f0, f1 -- ONE pair of registers, so rem(p) comes
//                   before hi(p + 1))
//   rem(p), lo(p)   the two remainders v - hi, and their packed rounding.  The compiler pads one wait state between an inline-asm result and
//                   its first reader (it assumes a partial-register write), so hi -> rem -> lo of a pair sit in three DIFFERENT gaps: the MFMA
//                   between them is the wait state (in one gap they cost two s_nop, 8 cycles of issue, per pair)
//   gates()         P = 4: the unit's gate byte from its four hi words
// ---- Per-gap schedule ---------------------------------------------------------------------------------------------------------------
// One wavefront per SIMD: an MFMA holds vector issue for 8 of its 32 cycles, so what sits in the gap behind it hides while its issue costs
// stay within 24 cycles (VALU / s_nop 4 each, two ds_read_b128 <= 3, an LDS-DMA piece 31-60).  Every gap is therefore one of
//   (a) one DMA piece and nothing else   (b) <= 2 ds_read_b128 + <= 3 VALU   (c) <= 5 VALU (an s_nop counts as one; so does a
// scalar ALU instruction -- round 11: ring_arm's three, in front of an even K-step's pieces in first-half gaps 2, 3 or, request_early, in the
// odd K-step's first-half gap 5 and second-half gap 4, are not in the table below);
// scripts/kstep_gaps.py prints what the compiler made of it (profiles/r8_kstep_gaps_*.log).  8-block K-step (slot_step8), gap k = behind
// MFMA k of the half; B = operands of blocks 4-7 of this slot, A' = operands of blocks 0-3 of the next slot:
//   gap        | odd K-step, fp16x3       | odd, bf16 modes    | even K-step, fp16x3      | even, bf16 modes
//   first  0-3 | 2 B reads each           | the same           | 2 B reads each           | the same
//   first  4   | bias                     | bias               | DMA piece 0              | the same
//   first  5   | -                        | -                  | DMA piece 1              |
//   first  6-9 | relu(0) .. relu(3)       | the same           | DMA pieces 2-5           |
//   first  10  | hi(0..3)                 | hi(0)              | DMA piece 6              |
//   first  11  | rem(0) rem(1)            | rem(0)             | DMA piece 7              |
//   (odd: s_waitcnt vmcnt(0) lgkmcnt(0), s_barrier)
//   second 0   | lo(0) lo(1) rem(2)       | hi(1)              | bias                     | bias
//   second 1   | 2 A' reads, rem(3)       | 2 A', rem(1)       | 2 A' reads               | 2 A'
//   second 2   | 2 A' reads, lo(2)        | 2 A', lo(0) lo(1)  | 2 A' reads, ra(0)        | the same
//   second 3   | 2 A' reads, lo(3)        | 2 A'               | 2 A' reads, rb(0)        | the same
//   second 4   | 2 A' reads               | 2 A'               | 2 A' reads, ra(1)        | the same
//   second 5   | -                        | hi(2)              | rb(1) ra(2)              | the same
//   second 6   | -                        | rem(2)             | rb(2) ra(3)              | the same
//   second 7   | -                        | hi(3) lo(2)        | rb(3) hi(0)              | the same
//   second 8   | -                        | rem(3)             | hi(1) hi(2) hi(3) rem(0) | rem(0) hi(1)
//   second 9   | -                        | lo(3)              | lo(0) rem(1) rem(2)      | rem(1) hi(2)
//   second 10  | -                        | (P = 4: gates)     | lo(1) lo(2) rem(3)       | rem(2) hi(3)
//   second 11  | -                        | -                  | lo(3)                    | rem(3) lo(0..3) (P = 4: + gates)
// fp16x3 reads a unit's biases one unit ahead (UnitWork::bias_next: second-half gap 11, views layer gap 11 of the half, behind lds_retire), so
// "bias" in its columns is a register copy and gap 11 carries two reads.
// fp16x3, K-steps 1 .. 14 of a hidden K-loop and 1 .. 4 of an IPE group (request_early): the odd K-step's second-half gaps 5-10 carry DMA
// pieces 0-5 of the NEXT even K-step's request, whose first-half gaps 4, 5 keep pieces 6, 7 and whose gaps 6-11 are empty; an IPE K-step
// also fetches the next one's two B operands (IpeFetch: first-half gap 6 / 4, the group's first K-step second-half gap 5).  Views layer,
// fp16x3 without an early tap: seq() with the density head's terms (UnitWork::dens_seq) -- gap 0 holds four reads and nothing else.
// The last B read has 8 MFMAs in front of the second half, the last A' read 7 in front of the next K-step; the A' reads of an odd K-step
// stay behind its barrier.  The second half of an even K-step is the "compact sequence" seq(0..11) (unit_seq), which the views layer's
// forms use as well.  Gaps that stay over the budget, and why:
//   * bf16 modes, even K-steps, second half 7-11 (6 VALU each; P = 4: + the ~10 of the gate byte in the last): hi is four instructions
//     there (no mixed-precision FMA reads the packed half: two conversions, a shift and a mask), and 44 VALU do not fit into the 45 issue
//     slots behind the bias reads in whole operations.  P = 4, odd K-steps: the gate byte is one operation of ~10 in an otherwise empty gap.
//   * (through round 10: the IPE K-steps of layer 0, DMA gaps 4 and 8, two v_readlane each -- the slot address came back from an SGPR spilled
//     to a VGPR lane.  With the request's addresses as running state the reload is the tile's first ring_arm's, in first-half gap 2.)
//   * a layer's last K-step (AccTake): nothing; the 17 accumulator reads that do not fit go to the head of finish_layer, where they run
//     while the K-loop's last MFMAs drain.
//   * views layer, even positions (slot_step4x2 / slot_step4): two units per 24 MFMAs (72 VALU, 20 ds_read) and 8 DMA pieces are more than
//     24 gaps hold under (a)-(c) -- the DMA pieces share gaps 4..11 of the first half with seq(); five such K-steps per tile.
template <bool BF, class W> __device__ __forceinline__ void unit_seq(W& w, int c);
template <bool EVEN, bool BF, class W> __device__ __forceinline__ void unit_step8(W& w, int t);
// DENS (fp16x3, the views layer's units of layer 7): the unit also adds its eight terms to the density head's dot product (dens_seq)
template <int P, bool DENS = false>
struct UnitWork {
  Ctx& cx;
  Unit& out;
  int u, lo_;
  float floor_v;
  f32x4 b0, b1;
  float sc;  // fp16x3: s_lo (OFF_SCALE)
  float v8[8];
  float f0, f1;              // bf16 modes: fp32 values of the current pair's hi halves
  float r0[4], r1[4];        // remainders of pair p, rem(p) -> lo(p)
  f32x4 wa0, wa1;            // DENS: the density vector's entries of elements 0..3 / 4..7
  // DENS: p_j += v8[j] w[j], then p_j += v8[4 + j] w'[j], units ascending -- alpha_head's own order of summation, so cx.sig_part keeps its
  // bits (v8 is med3(fma(hv, s, b), 0, F16_MAX) where alpha_head takes max(.., 0): the same value unless the launch raises the saturation
  // flag and is redone in fp32).  In the compact sequence: the two reads in gap 0; one term where a gap has an issue slot left
  // and its input was pinned in an EARLIER gap (no wait state), no two terms of one p_j in a gap; the last three terms do not fit and are
  // handed to the next unit's gap 1 (cx.dv, cx.dw), the last unit's to DensTail.  Volatile asm: placed where written, like rem().
  __device__ __forceinline__ static void dens_fma(float& p, float v, float w) { asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(p) : "v"(v), "v"(w)); }
  __device__ __forceinline__ void dens_seq(int c) {
    if constexpr (DENS) {
      switch (c) {
        case 0: {
          const float* wl = cx.sm_small + OFF_WALPHA + (u >> 1) * 32 + 16 * (u & 1) + 4 * cx.hi;
          wa0 = *reinterpret_cast<const f32x4*>(wl); wa1 = *reinterpret_cast<const f32x4*>(wl + 8);
        } break;
        case 1:  // (the previous unit's last three)
          dens_fma(cx.dp[1], cx.dv[0], cx.dw[0]); dens_fma(cx.dp[2], cx.dv[1], cx.dw[1]); dens_fma(cx.dp[3], cx.dv[2], cx.dw[2]);
          break;
        case 7: dens_fma(cx.dp[0], v8[0], wa0[0]); break;  // (first use of the two reads: the operand reads of gaps 1-4 are old by now)
        case 10: dens_fma(cx.dp[0], v8[4], wa1[0]); break;
        case 11:
          dens_fma(cx.dp[1], v8[1], wa0[1]); dens_fma(cx.dp[2], v8[2], wa0[2]); dens_fma(cx.dp[3], v8[3], wa0[3]);
          cx.dv[0] = v8[5]; cx.dw[0] = wa1[1]; cx.dv[1] = v8[6]; cx.dw[1] = wa1[2]; cx.dv[2] = v8[7]; cx.dw[2] = wa1[3];
          break;
        default: break;
      }
    }
  }
  __device__ __forceinline__ void bias() {
    if constexpr (P == 2) {  // (read a unit ahead: bias_next)
      b0 = cx.nb0; b1 = cx.nb1;
      return;
    }
    const int ob = u >> 1, m = u & 1;
    const float* bl = cx.sm_small + OFF_BIAS + lo_ * 256 + ob * 32 + 16 * m + 4 * cx.hi;
    b0 = *reinterpret_cast<const f32x4*>(bl); b1 = *reinterpret_cast<const f32x4*>(bl + 8);
  }
  // fp16x3: the two bias reads of unit u + 1, in the LAST gap of the half that makes unit u, behind lds_retire.  Read in the unit's own
  // first gap they were first used two gaps on, and the compiler's wait there (always lgkmcnt(0)) also sat out the operand reads issued
  // in between.  From here they are several MFMAs old at the next wait the compiler places (in front of a half's first MFMA).
  __device__ __forceinline__ void bias_next() {
    if constexpr (P == 2) {
      if (u + 1 < HS) {
        const int ob = (u + 1) >> 1, m = (u + 1) & 1;
        const float* bl = cx.sm_small + OFF_BIAS + lo_ * 256 + ob * 32 + 16 * m + 4 * cx.hi;
        cx.nb0 = *reinterpret_cast<const f32x4*>(bl); cx.nb1 = *reinterpret_cast<const f32x4*>(bl + 8);
      }
    }
  }
  // element e = j or 4 + j of the unit: accumulator + bias (fp16x3: accumulator x next layer's input scale + bias, exact), relu
  __device__ __forceinline__ float act(int e, float b) const {
    const float h = cx.hv[(u >> 1) * 16 + 8 * (u & 1) + e];
    if constexpr (is_bf16<P>()) return __builtin_fmaxf(h + b, floor_v);
    else if constexpr (P == 1) return __builtin_amdgcn_fmed3f(h + b, floor_v, F16_MAX);  // fp16 operands: the same instruction count with
                                     // v_med3_f32 -- an activation beyond the fp16 range saturates instead of turning into infinity
    else return __builtin_amdgcn_fmed3f(__builtin_fmaf(h, sc, b), floor_v, F16_MAX);
  }
  // fp16x3: the running maximum of what is about to become fp16 is kept: a value AT the limit raises the saturation flag at the end of
  // the kernel (status[0]) -- never a silent clamp
  __device__ __forceinline__ void range(int j) {
    if constexpr (P == 2) asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(cx.vmax) : "v"(v8[j]), "v"(v8[4 + j]));
  }
  __device__ __forceinline__ void ra(int j) { v8[j] = act(j, b0[j]); pin(v8[j]); }
  __device__ __forceinline__ void rb(int j) { v8[4 + j] = act(4 + j, b1[j]); range(j); pin(v8[4 + j]); }
  __device__ __forceinline__ void relu(int j) {  // (the maximum reads both values before either is pinned: no wait state)
    v8[j] = act(j, b0[j]); v8[4 + j] = act(4 + j, b1[j]);
    range(j);
    pin(v8[j]); pin(v8[4 + j]);
  }
  __device__ __forceinline__ void hi(int p) {
    unsigned hp;
    if constexpr (is_bf16<P>()) {
      hp = pack_bf16(v8[2 * p], v8[2 * p + 1]);
      f0 = __uint_as_float(hp << 16);
      f1 = __uint_as_float(hp & 0xffff0000u);
    } else {
      // fp16 parts: lo = v - hi comes straight from the PACKED hi register with v_fma_mix_f32 (an fp16 half as a source of an fp32 FMA:
      // hi * -1 + v, exact) in rem(p) -- no fp32 copy of hi is made -- and needs 12 bits at most, rounded to nearest by
      // v_cvt_pk_f16_f32: 22 significant bits (below 2^-14, where fp16 is subnormal, the absolute quantum 2^-24 bounds the error).
      hp = pack_f16(v8[2 * p], v8[2 * p + 1]);  // (round to nearest: |lo| <= 2^-12 |v|; the remainder is exact for either rounding)
    }
    pin(hp);
    if constexpr (is_bf16<P>()) { pin(f0); pin(f1); }
    out.h[p] = hp;
  }
  __device__ __forceinline__ void rem(int p) {
    if constexpr (is_bf16<P>()) {
      r0[p] = v8[2 * p] - f0; r1[p] = v8[2 * p + 1] - f1;
      pin(r0[p]); pin(r1[p]);
    } else {  // (volatile instead of a pin behind them: a pin would read an inline-asm result in the same gap -- one s_nop each)
      asm volatile("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r0[p]) : "v"(out.h[p]), "v"(v8[2 * p]));
      asm volatile("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1[p]) : "v"(out.h[p]), "v"(v8[2 * p + 1]));
    }
  }
  __device__ __forceinline__ void lo(int p) {
    unsigned lp = is_bf16<P>() ? pack_bf16(r0[p], r1[p]) : pack_f16(r0[p], r1[p]);
    pin(lp);
    out.l[p] = lp;
  }
  __device__ __forceinline__ void gates() {
    if constexpr (has_gates<P>()) {  // all four hi words of the unit exist: value > 0 <=> its bf16 hi half is non-zero (after the ReLU nothing is negative)
      const unsigned t = gate_byte(out.h);
      cx.gbits[u >> 2] |= t << (8 * (u & 3));
    }
  }
  __device__ __forceinline__ void seq(int c) {
    unit_seq<is_bf16<P>()>(*this, c); dens_seq(c);
    if (c == 11) bias_next();
  }
  template <bool EVEN> __device__ __forceinline__ void step8(int t) {
    unit_step8<EVEN, is_bf16<P>()>(*this, t);
    if (t == 23) bias_next();
  }
  // fp16x1 (slot_step8_one / slot_step4_one) and finish_layer: the unit in 12 pieces, in order
  __device__ __forceinline__ void prefetch() { bias(); }
  __device__ __forceinline__ void operator()(int j) {
    if (j < 4) relu(j);
    else if constexpr (P == 1) {  // pieces 4..7: pair p = j - 4 rounded to fp16 and packed (pieces 8..11: nothing)
      if (j < 8) {
        unsigned hp = pack_f16(v8[2 * (j - 4)], v8[2 * (j - 4) + 1]);
        pin(hp);
        out.h[j - 4] = hp;
      }
    } else if (!(j & 1)) hi((j - 4) >> 1);
    else {
      rem((j - 5) >> 1); lo((j - 5) >> 1);
      if (j == 11) gates();
    }
  }
};
// The compact sequence: a whole unit in 12 consecutive gaps of which gaps 1..4 also carry two operand reads each (<= 3 VALU there).
// BF: the bf16 forms (hi = 3 instructions, one f0 / f1 pair).
template <bool BF, class W>
__device__ __forceinline__ void unit_seq(W& w, int c) {
  switch (c) {  // (a compile-time constant after unrolling)
    case 0: w.bias(); break;
    case 2: w.ra(0); break;
    case 3: w.rb(0); break;
    case 4: w.ra(1); break;
    case 5: w.rb(1); w.ra(2); break;
    case 6: w.rb(2); w.ra(3); break;
    case 7: w.rb(3); w.hi(0); break;
    case 8: if constexpr (BF) { w.rem(0); w.hi(1); } else { w.hi(1); w.hi(2); w.hi(3); w.rem(0); } break;
    case 9: if constexpr (BF) { w.rem(1); w.hi(2); } else { w.lo(0); w.rem(1); w.rem(2); } break;
    case 10: if constexpr (BF) { w.rem(2); w.hi(3); } else { w.lo(1); w.lo(2); w.rem(3); } break;
    case 11: if constexpr (BF) { w.rem(3); w.lo(0); w.lo(1); w.lo(2); w.lo(3); w.gates(); } else { w.lo(3); } break;
    default: break;
  }
}
// Gap t of an 8-block K-step (0..11: first half, 12..23: second half): the table above
template <bool EVEN, bool BF, class W>
__device__ __forceinline__ void unit_step8(W& w, int t) {
  if constexpr (EVEN) {
    if (t >= 12) unit_seq<BF>(w, t - 12);
  } else {
    switch (t) {
      case 4: w.bias(); break;
      case 6: case 7: case 8: case 9: w.relu(t - 6); break;
      case 10: if constexpr (BF) { w.hi(0); } else { w.hi(0); w.hi(1); w.hi(2); w.hi(3); } break;
      case 11: if constexpr (BF) { w.rem(0); } else { w.rem(0); w.rem(1); } break;
      case 12: if constexpr (BF) { w.hi(1); } else { w.lo(0); w.lo(1); w.rem(2); } break;
      case 13: w.rem(BF ? 1 : 3); break;
      case 14: if constexpr (BF) { w.lo(0); w.lo(1); } else { w.lo(2); } break;
      case 15: if constexpr (!BF) { w.lo(3); } break;
      case 17: if constexpr (BF) { w.hi(2); } break;
      case 18: if constexpr (BF) { w.rem(2); } break;
      case 19: if constexpr (BF) { w.hi(3); w.lo(2); } break;
      case 20: if constexpr (BF) { w.rem(3); } break;
      case 21: if constexpr (BF) { w.lo(3); } break;
      case 22: if constexpr (BF) { w.gates(); } break;
      default: break;
    }
  }
}
// fp16x3: the consumer of layer `slot`'s output has made all its units -- fold the running maximum into this thread's LDS cell
// (ds_max_u32 without return: fire and forget; the values are >= 0, so the bit patterns order like the floats)
template <int P>
__device__ __forceinline__ void fold_range(Ctx& cx, int slot) {
  if constexpr (P == 2) {
    // (inline asm: for a ds_ instruction it can see, the compiler first waits vmcnt(0) -- the weight stream's LDS-DMA "may write LDS" --
    //  i.e. for the two slots requested half a K-step ago, at the end of EVERY layer's K-loop.  An LDS atomic without return needs no wait;
    //  LDS operations complete in order, so one more in flight only makes the compiler's own lgkmcnt waits conservative.)
    const unsigned addr = (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned*)(cx.rng + slot * 256);
    asm volatile("ds_max_u32 %0, %1" :: "v"(addr), "v"(__float_as_uint(cx.vmax)) : "memory");
    cx.vmax = 0.f;
  }
}
struct NoWork {
  __device__ __forceinline__ void prefetch() {}
  __device__ __forceinline__ void operator()(int) {}
  __device__ __forceinline__ void seq(int) {}
  template <bool EVEN> __device__ __forceinline__ void step8(int) {}
};
// fp16x3, the work of an IPE K-step (ipe_steps): the B operands of IPE K-step m (hi, lo: two LDS reads) in gap T of an 8-block K-step
template <int T>
struct IpeFetch {
  const float* src;
  int m;
  bf16x8& ph;
  bf16x8& pl;
  template <bool EVEN> __device__ __forceinline__ void step8(int t) {
    if (t != T) return;
    ph = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(src + (m * 2 + 0) * 256));
    pl = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(src + (m * 2 + 1) * 256));
  }
};
// The work of the LAST K-step of layer l (which re-packs nothing: all 16 units of the previous layer exist, cx.hv is dead): blocks 0..3 of the
// layer being finished are final once that K-step's first half is through, so their accumulator reads (v_accvgpr_read) go behind the MFMAs
// of its second half instead of in front of the next layer.  Split modes: as many per gap as the per-gap schedule allows (take_n; gap 0 one less: the compiler pads the first read behind the MFMAs with an s_nop), 47 of the
// 64 -- the rest opens finish_layer, where it runs while the last MFMAs drain -- and in second-half gap 10 the two bias reads of the next
// layer's unit 0, which finish_layer would otherwise wait for with nothing to cover their LDS latency.
constexpr int take_n(int s) { return s == 0 ? 4 : s == 1 ? 2 : s <= 4 ? 3 : s == 10 ? 2 : 5; }  // (gaps 1..4: + operand reads; 10: + bias reads and their address)
constexpr int take_before(int s) {
  int n = 0;
  for (int k = 0; k < s; ++k) n += take_n(k);
  return n;
}
constexpr int TAKE_HIDDEN = take_before(12);
__device__ __forceinline__ const float* unit0_bias(const Ctx& cx, int l) { return cx.sm_small + OFF_BIAS + l * 256 + 4 * cx.hi; }
template <int P>
struct AccTake {
  const f32x16 (&acc)[8];
  Ctx& cx;
  int l;
  __device__ __forceinline__ void prefetch() {}
  __device__ __forceinline__ void operator()(int j) {  // fp16x1: 8 pieces of 8
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = 8 * j + k;
      if (i < 64) cx.hv[i] = acc_read(acc[i >> 4][i & 15]);
    }
  }
  __device__ __forceinline__ void seq(int) {}
  template <bool EVEN> __device__ __forceinline__ void step8(int t) {
    if (t < 12) return;
    const int s = t - 12;
#pragma unroll
    for (int k = 0; k < take_n(s); ++k) {
      const int i = take_before(s) + k;
      cx.hv[i] = acc_read(acc[i >> 4][i & 15]);
    }
    if (s == 10) {
      const float* bl = unit0_bias(cx, l);
      cx.hb0 = *reinterpret_cast<const f32x4*>(bl); cx.hb1 = *reinterpret_cast<const f32x4*>(bl + 8);
    }
  }
};
template <int P, bool DENS = false>
__device__ __forceinline__ UnitWork<P, DENS> unit_work(int u, int lo, Ctx& cx, Unit& out) {
  return UnitWork<P, DENS>{cx, out, u, lo, lo < 8 ? 0.f : (!is_bf16<P>() ? -F16_MAX : -__builtin_inff()), {}, {}, cx.sc, {}, 0.f, 0.f, {}, {}, {}, {}};
}

// End of layer l: move the rest of the accumulators out of the AGPRs (the next layer starts from C = 0 in the same registers) and
// make unit 0.  The only part of the re-packing that is not hidden behind MFMAs (~80 + ~40 VALU instructions).
template <int P>
__device__ __forceinline__ void finish_layer(const f32x16 (&acc)[8], int l, Ctx& cx) {
  if constexpr (is_split<P>()) {
#pragma unroll
    for (int i = TAKE_HIDDEN; i < 64; ++i) cx.hv[i] = acc_read(acc[i >> 4][i & 15]);  // (what AccTake left of blocks 0..3)
  }
#pragma unroll
  for (int ob = 4; ob < 8; ++ob)  // (blocks 0..3: AccTake, in the shadow of the layer's last K-step)
#pragma unroll
    for (int r = 0; r < 16; ++r) cx.hv[ob * 16 + r] = acc_read(acc[ob][r]);
  if constexpr (P == 2)
    cx.sc = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, cx.sm_small[OFF_SCALE + l])));
  UnitWork<P> w = unit_work<P>(0, l, cx, cx.xn);
  if constexpr (P == 2) {  // unit 1's biases for K-step 0 of the layer's consumer (UnitWork::bias_next reads the others)
    const float* bl = unit0_bias(cx, l) + 16;
    cx.nb0 = *reinterpret_cast<const f32x4*>(bl); cx.nb1 = *reinterpret_cast<const f32x4*>(bl + 8);
  }
  if constexpr (is_split<P>()) {  // (hi, rem and lo of a pair apart: see UnitWork)
    w.b0 = cx.hb0; w.b1 = cx.hb1;  // (read by AccTake)
#pragma unroll
    for (int j = 0; j < 4; ++j) w.relu(j);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      w.hi(p);
      if constexpr (is_bf16<P>()) w.rem(p);  // (one f0 / f1 pair)
    }
    if constexpr (!is_bf16<P>()) {
#pragma unroll
      for (int p = 0; p < 4; ++p) w.rem(p);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) w.lo(p);
    w.gates();
  } else {
    w.prefetch();
#pragma unroll
    for (int j = 0; j < 12; ++j) w(j);
  }
}

// Density head on the finished layer 7: sigma partial = relu(h7) . w_alpha over this lane's 128 neurons.  Once per tile,
// not hidden behind MFMAs (~2k cycles).
// (fp16x3: bias and density vector are stored pre-scaled -- relu(fma(acc, s_7, b'_7)) = 2^c_8 relu(h_7), w'_alpha = 2^-c_8 w_alpha)
__device__ __forceinline__ void alpha_head(Ctx& cx) {
  const float* bl = cx.sm_small + OFF_BIAS + 7 * 256 + 4 * cx.hi;
  const float* wa = cx.sm_small + OFF_WALPHA + 4 * cx.hi;
  const float s7 = cx.sm_small[OFF_SCALE + 7];  // (1 in the other modes: fma(x, 1, b) == x + b)
  float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(bl + ob * 32 + 8 * q);
      const f32x4 w4v = *reinterpret_cast<const f32x4*>(wa + ob * 32 + 8 * q);
      p0 = NM_FMA(__builtin_fmaxf(__builtin_fmaf(cx.hv[ob * 16 + 4 * q + 0], s7, b[0]), 0.f), w4v[0], p0);
      p1 = NM_FMA(__builtin_fmaxf(__builtin_fmaf(cx.hv[ob * 16 + 4 * q + 1], s7, b[1]), 0.f), w4v[1], p1);
      p2 = NM_FMA(__builtin_fmaxf(__builtin_fmaf(cx.hv[ob * 16 + 4 * q + 2], s7, b[2]), 0.f), w4v[2], p2);
      p3 = NM_FMA(__builtin_fmaxf(__builtin_fmaf(cx.hv[ob * 16 + 4 * q + 3], s7, b[3]), 0.f), w4v[3], p3);
    }
  cx.sig_part = (p0 + p1) + (p2 + p3);
}

// fp16x3, a pass with colour heads whose tap is not composited in front of the views layer: the views K-loop re-packs layer 7 unit by
// unit, i.e. makes relu(fma(hv, s_7, b_7)) a second time -- its units add their terms to the dot product as they go (UnitWork<2, true>)
// and alpha_head's 128 x 3 VALU + 64 LDS reads with the matrix pipe idle go.  dens_open: unit 0's terms (finish_layer made unit 0; its
// last three are handed on like every unit's); DensTail: the last unit's three, in the empty second half of the last hidden slot;
// dens_close: alpha_head's final sum.
__device__ __forceinline__ void dens_open(Ctx& cx) {
  const float* bl = cx.sm_small + OFF_BIAS + 7 * 256 + 4 * cx.hi;
  const float* wa = cx.sm_small + OFF_WALPHA + 4 * cx.hi;
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(bl), b1 = *reinterpret_cast<const f32x4*>(bl + 8);
  const f32x4 w0 = *reinterpret_cast<const f32x4*>(wa), w1 = *reinterpret_cast<const f32x4*>(wa + 8);
  float v[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = __builtin_fmaxf(__builtin_fmaf(cx.hv[j], cx.sc, b0[j]), 0.f);
    v[4 + j] = __builtin_fmaxf(__builtin_fmaf(cx.hv[4 + j], cx.sc, b1[j]), 0.f);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) cx.dp[j] = NM_FMA(v[j], w0[j], 0.f);
  cx.dp[0] = NM_FMA(v[4], w1[0], cx.dp[0]);
#pragma unroll
  for (int j = 0; j < 3; ++j) { cx.dv[j] = v[5 + j]; cx.dw[j] = w1[1 + j]; }
}
struct DensTail {
  Ctx& cx;
  __device__ __forceinline__ void seq(int c) {
    if (c == 1) {
#pragma unroll
      for (int j = 0; j < 3; ++j) UnitWork<2, true>::dens_fma(cx.dp[1 + j], cx.dv[j], cx.dw[j]);
    }
  }
};
__device__ __forceinline__ void dens_close(Ctx& cx) { cx.sig_part = (cx.dp[0] + cx.dp[1]) + (cx.dp[2] + cx.dp[3]); }

// Tapped activations (fp32, after bias and relu) of the finished layer lo -> L2-resident workspace, 1 KiB per store.
// Once per tile and not hidden behind MFMAs (~2k cycles).
__device__ __forceinline__ void dump_tap(int lo, Ctx& cx) {
  const float* bl = cx.sm_small + OFF_BIAS + lo * 256 + 4 * cx.hi;
  const float sl = cx.sm_small[OFF_SCALE + lo];  // (fp16x3: the workspace holds 2^c_{lo+1} x the activations; OFF_DESCALE undoes it per ray)
  auto* tp = (__attribute__((address_space(1))) f32x4*)cx.tapw;  // (global_store, not flat_store: a pending FLAT access makes every later ds_read wait for vmcnt)
#pragma unroll
  for (int ob = 0; ob < 8; ++ob) {
    f32x4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(bl + ob * 32 + 8 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[q][e] = __builtin_fmaxf(__builtin_fmaf(cx.hv[ob * 16 + 4 * q + e], sl, b[e]), 0.f);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) tp[q * 64] = v[q];  // immediate offsets 0, 1, 2, 3 KiB
    tp += 256;
    pin(tp);  // one running pointer instead of 32 precomputed addresses
  }
}

// fp16x1 form of the K-step: 8 MFMAs whose A operands (all 8 blocks of slot g) were fetched during the PREVIOUS K-step, so
// no MFMA waits for LDS, and everything else a K-step has to issue -- the ring barrier of slot g+1 with the DMA of a later
// slot, the 8 operand reads of slot g+1, the bias reads and the 8 pieces of re-packing work -- sits BETWEEN the MFMAs, a
// few instructions behind each (with 8 MFMAs per K-step instead of 24 there is no second half to hide them behind; a first
// version that issued barrier and reads up front ran at 640 cycles per K-step against 256 of MFMA time).
// (past the last slot the fetched operands are stale ring contents nobody uses)
__device__ __forceinline__ bf16x8 load_op1(const float* slot, int lane, int blk) {
  return __builtin_bit_cast(bf16x8, (reinterpret_cast<const u32x4*>(slot) + lane)[blk * 64]);
}
#define NM_SB __builtin_amdgcn_sched_barrier(0)
template <bool FIRST, bool ACQ, class Work>
__device__ __forceinline__ void slot_step8_one(f32x16 (&acc)[8], Ctx& cx, const bf16x8& x, Work work) {
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int g = cx.g;
  const OpHalf A = cx.opA, B = cx.opB;
  const float* nxt = ring_slot<1>(cx.ring, g + 1);
  acc[0] = mfma_p<1>(A.h[0], x, FIRST ? zero : acc[0]); NM_SB;
  if constexpr (ACQ) ring_acquire_pair(cx.blob_slots, g, cx.ring, cx.wave, cx.lane);
  NM_SB;
  acc[1] = mfma_p<1>(A.h[1], x, FIRST ? zero : acc[1]); NM_SB;
  cx.opA.h[0] = load_op1(nxt, cx.lane, 0); cx.opA.h[1] = load_op1(nxt, cx.lane, 1); work.prefetch(); NM_SB;
  acc[2] = mfma_p<1>(A.h[2], x, FIRST ? zero : acc[2]); NM_SB;
  cx.opA.h[2] = load_op1(nxt, cx.lane, 2); cx.opA.h[3] = load_op1(nxt, cx.lane, 3); NM_SB;
  acc[3] = mfma_p<1>(A.h[3], x, FIRST ? zero : acc[3]); NM_SB;
  cx.opB.h[0] = load_op1(nxt, cx.lane, 4); cx.opB.h[1] = load_op1(nxt, cx.lane, 5); NM_SB;
  acc[4] = mfma_p<1>(B.h[0], x, FIRST ? zero : acc[4]); NM_SB;
  cx.opB.h[2] = load_op1(nxt, cx.lane, 6); cx.opB.h[3] = load_op1(nxt, cx.lane, 7); NM_SB;
  acc[5] = mfma_p<1>(B.h[1], x, FIRST ? zero : acc[5]); NM_SB;
  work(0); work(1); NM_SB;  // (first use of the bias reads: the LDS wait in front of it has two more MFMAs of cover)
  acc[6] = mfma_p<1>(B.h[2], x, FIRST ? zero : acc[6]); NM_SB;
  work(2); work(3); work(4); NM_SB;
  acc[7] = mfma_p<1>(B.h[3], x, FIRST ? zero : acc[7]); NM_SB;
  work(5); work(6); work(7); NM_SB;
  cx.g = g + 1;
}

// One operand pair (hi, lo) of output block 4 p + o of a slot: the two ds_read_b128 a gap carries
template <int P>
__device__ __forceinline__ void load_pair(OpHalf& d, const float* slot, int lane, int p, int o) {
  const u32x4* s4 = reinterpret_cast<const u32x4*>(slot) + lane;
  d.h[o] = __builtin_bit_cast(bf16x8, s4[((4 * p + o) * 2 + 0) * 64]);
  d.l[o] = __builtin_bit_cast(bf16x8, s4[((4 * p + o) * 2 + 1) * 64]);
}
// MFMA k = 0..11 of a half slot on four blocks: w_hi*x_hi (FIRST: from C = 0), w_hi*x_lo, w_lo*x_hi -- four blocks each
template <int P, bool FIRST>
__device__ __forceinline__ f32x16 mfma_k(int k, const OpHalf& a, const bf16x8& xh, const bf16x8& xl, const f32x16& c) {
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (k < 4) return mfma_p<P>(a.h[k], xh, FIRST ? zero : c);
  if (k < 8) return mfma_p<P>(a.h[k & 3], xl, c);
  return mfma_p<P>(a.l[k & 3], xh, c);
}

// One K-step (slot cx.g) of an 8-block layer, software pipelined over half slots: 12 MFMAs on blocks 0-3 with the A operands fetched
// during the previous K-step, 12 on blocks 4-7 with the B operands fetched during the first half; odd position: the ring barrier of slots
// g+1, g+2 between the halves.  What else a K-step issues -- 16 operand reads, the 8 DMA pieces of an even position's weight request and
// `work`, VALU work independent of this slot (the re-packing of the next K-step's B operands, or AccTake) -- sits in the 24 gaps behind the
// MFMAs by the per-gap schedule (table at UnitWork): operand reads two per gap, B in gaps 0-3 of the first half, the next slot's A in gaps
// 1-4 of the second; the DMA pieces alone in gaps 4-11 of the first half; work.step8<EVEN>(t) says what the work does in gap t.
// (EVEN: the K-step's position in the weight stream is even -- every layer holds an even number of K-steps, so the callers know)
// (the next slot's operands are read unconditionally: past the last slot they are stale ring contents nobody uses)
template <int P, bool FIRST, bool EVEN, bool RQE = false, class Work>
__device__ __forceinline__ void slot_step8(f32x16 (&acc)[8], Ctx& cx, const bf16x8& xh, const bf16x8& xl, Work work) {
  if constexpr (P == 1) {
    slot_step8_one<FIRST, EVEN>(acc, cx, xh, work);
    return;
  }
  const int g = cx.g;
  const OpHalf A = cx.opA;
  OpHalf B;
  const float* cur = cx.ring + (g & (NRING - 1)) * SLOT_FLOATS;
  const float* nxt = cx.ring + ((g + 1) & (NRING - 1)) * SLOT_FLOATS;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    acc[k & 3] = mfma_k<P, FIRST>(k, A, xh, xl, acc[k & 3]);
    __builtin_amdgcn_sched_barrier(0);
    if (k < 4) load_pair<P>(B, cur, cx.lane, 1, k);
    if constexpr (EVEN && !RQE) {
      if (k == 2 || k == 3) ring_arm<P>(cx, k - 2);
      if (k >= 4) ring_request<P>(cx, g, k - 4);
    }
    if constexpr (EVEN && RQE) {  // (pieces 0..5: the previous K-step, behind its barrier)
      if (k == 4 || k == 5) ring_request<P>(cx, g, k + 2);
    }
    if constexpr (!EVEN && RQE) {  // (the next K-step's request: its addresses, in a gap this mode leaves empty)
      if (k == 5) ring_arm<P>(cx, 0);
    }
    work.template step8<EVEN>(k);
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (!EVEN) {
    ring_acquire_two();
    __builtin_amdgcn_sched_barrier(0);  // (the second half's first MFMA stays behind the barrier)
  }
  // from here to the end of the K-step: ONE basic block (the work must not be separated from its MFMAs)
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    acc[4 + (k & 3)] = mfma_k<P, FIRST>(k, B, xh, xl, acc[4 + (k & 3)]);
    __builtin_amdgcn_sched_barrier(0);
    if (k >= 1 && k <= 4) load_pair<P>(cx.opA, nxt, cx.lane, 0, k - 1);
    if constexpr (!EVEN && RQE) {
      if (k == 4) ring_arm<P>(cx, 1);
      if (k >= 5 && k <= 10) ring_request<P>(cx, g + 1, k - 5);
    }
    if (k == 11) lds_retire<P>();  // (the next slot's A operands: read in gaps 1-4; in front of the work: its bias_next reads stay in flight)
    work.template step8<EVEN>(12 + k);
    __builtin_amdgcn_sched_barrier(0);
  }
  cx.g = g + 1;
}

// Same for the 4-block views layer (a slot is a single half).
template <bool FIRST, bool ACQ, class Work>
__device__ __forceinline__ void slot_step4_one(f32x16 (&acc)[4], Ctx& cx, const bf16x8& x, Work work) {
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int g = cx.g;
  const OpHalf C = cx.opA;
  const float* nxt = ring_slot<1>(cx.ring, g + 1);
  acc[0] = mfma_p<1>(C.h[0], x, FIRST ? zero : acc[0]); NM_SB;
  if constexpr (ACQ) ring_acquire_pair(cx.blob_slots, g, cx.ring, cx.wave, cx.lane);
  NM_SB;
  acc[1] = mfma_p<1>(C.h[1], x, FIRST ? zero : acc[1]); NM_SB;
#pragma unroll
  for (int o = 0; o < 4; ++o) cx.opA.h[o] = load_op1(nxt, cx.lane, o);
  work.prefetch(); NM_SB;
  acc[2] = mfma_p<1>(C.h[2], x, FIRST ? zero : acc[2]); NM_SB;
  work(0); work(1); work(2); work(3); NM_SB;
  acc[3] = mfma_p<1>(C.h[3], x, FIRST ? zero : acc[3]); NM_SB;
  work(4); work(5); work(6); work(7); NM_SB;
  cx.g = g + 1;
}

// Split modes: 12 MFMAs, the work as the compact sequence (seq(k) in gap k), the next slot's operands two per gap in gaps 1-4, an even
// position's DMA pieces in gaps 4-11 next to the work (over the per-gap budget: see the table at UnitWork).
template <int P, bool FIRST, bool EVEN, class Work>
__device__ __forceinline__ void slot_step4(f32x16 (&acc)[4], Ctx& cx, const bf16x8& xh, const bf16x8& xl, Work work) {
  if constexpr (P == 1) {
    slot_step4_one<FIRST, EVEN>(acc, cx, xh, work);
    return;
  }
  const int g = cx.g;
  const OpHalf C = cx.opA;
  const float* nxt = cx.ring + ((g + 1) & (NRING - 1)) * SLOT_FLOATS;
  if constexpr (!EVEN) ring_acquire_two();
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    acc[k & 3] = mfma_k<P, FIRST>(k, C, xh, xl, acc[k & 3]);
    __builtin_amdgcn_sched_barrier(0);
    if (k >= 1 && k <= 4) load_pair<P>(cx.opA, nxt, cx.lane, 0, k - 1);
    if constexpr (EVEN) {
      if (k == 2 || k == 3) ring_arm<P>(cx, k - 2);
      if (k >= 4) ring_request<P>(cx, g, k - 4);
    }
    work.seq(k);
    __builtin_amdgcn_sched_barrier(0);
  }
  cx.g = g + 1;
}

// Split modes, NM_VIEWS_PAIRS: TWO K-steps of the 4-block views layer per weight slot (half 0: the four output blocks of K-step 2s, half 1:
// those of K-step 2s + 1) -- the shape of slot_step8 with both halves accumulating into the same four blocks: one ring barrier, one DMA of a
// FULL slot and one counted wait per 24 MFMAs instead of per 12 (a single 4-block K-step runs at 67 cycles per MFMA against the 8-block
// layers' 46: its fixed cost does not hide behind 12 MFMAs).  w0 makes the unit the SECOND half consumes (u1, ready behind this slot's
// 12th MFMA), w1 the first unit of the next slot (cx.xn).
// Each half is a compact sequence, seq(k) in gap k, with its operand reads (first half: this slot's second K-step, second half: the next
// slot) two per gap in gaps 1-4; u1 is complete in gap 11 of the first half.  Even positions: the DMA pieces in gaps 4-11 of the first half,
// next to w0 (over the per-gap budget: see the table at UnitWork; they stay in gaps that carry VALU work only but for the first, where a
// piece was measured cheapest).
template <int P, bool FIRST, bool EVEN, class W0, class W1>
__device__ __forceinline__ void slot_step4x2(f32x16 (&av)[4], Ctx& cx, const bf16x8& x0h, const bf16x8& x0l, Unit& u1, W0 w0, W1 w1) {
  const int g = cx.g;
  const OpHalf A = cx.opA;
  OpHalf B;
  const float* cur = cx.ring + (g & (NRING - 1)) * SLOT_FLOATS;
  const float* nxt = cx.ring + ((g + 1) & (NRING - 1)) * SLOT_FLOATS;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    av[k & 3] = mfma_k<P, FIRST>(k, A, x0h, x0l, av[k & 3]);
    __builtin_amdgcn_sched_barrier(0);
    if (k >= 1 && k <= 4) load_pair<P>(B, cur, cx.lane, 1, k - 1);  // the second K-step's operands
    if constexpr (EVEN) {  // (ring_arm: gap 0 holds reads only, gap 2 the fewest VALU of gaps 1-3)
      if (k == 0 || k == 2) ring_arm<P>(cx, k >> 1);
      if (k >= 4) ring_request<P>(cx, g, k - 4);
    }
    if (k == 11) lds_retire<P>();  // (the second K-step's operands: read in gaps 1-4)
    w0.seq(k);
    __builtin_amdgcn_sched_barrier(0);
  }
  // (all reads of this slot are issued: the barrier below frees its ring position for the K-step after next)
  if constexpr (!EVEN) {
    ring_acquire_two();
    __builtin_amdgcn_sched_barrier(0);
  }
  const bf16x8 x1h = __builtin_bit_cast(bf16x8, u1.h), x1l = __builtin_bit_cast(bf16x8, u1.l);
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    av[k & 3] = mfma_k<P, false>(k, B, x1h, x1l, av[k & 3]);
    __builtin_amdgcn_sched_barrier(0);
    if (k >= 1 && k <= 4) load_pair<P>(cx.opA, nxt, cx.lane, 0, k - 1);
    if (k == 11) lds_retire<P>();
    w1.seq(k);
    __builtin_amdgcn_sched_barrier(0);
  }
  cx.g = g + 1;
}

// The hidden part of the views layer: layer 7's sixteen units (unit 0 in cx.xn) against the folded 128 x 256 matrix
// (DENS: fp16x3 only, the density head rides along -- see dens_open)
template <int P, bool DENS = false>
__device__ __forceinline__ void views_hidden(f32x16 (&av)[4], Ctx& cx) {
  static_assert(!DENS || P == 2, "the density head accumulates in the views K-loop in fp16x3 only");
  if constexpr (is_split<P>()) {
#pragma unroll
    for (int sl = 0; sl < HS / 2; ++sl) {
      const Unit x0 = cx.xn;
      Unit u1;
      const bf16x8 x0h = __builtin_bit_cast(bf16x8, x0.h), x0l = __builtin_bit_cast(bf16x8, x0.l);
      // (NSLOT_NORGB is even: slot sl of the views layer sits at an even stream position iff sl is even)
      if (sl == 0) slot_step4x2<P, true, true>(av, cx, x0h, x0l, u1, unit_work<P, DENS>(1, 7, cx, u1), unit_work<P, DENS>(2, 7, cx, cx.xn));
      else if (sl + 1 == HS / 2) {
        if constexpr (DENS) slot_step4x2<P, false, false>(av, cx, x0h, x0l, u1, unit_work<P, DENS>(2 * sl + 1, 7, cx, u1), DensTail{cx});
        else slot_step4x2<P, false, false>(av, cx, x0h, x0l, u1, unit_work<P>(2 * sl + 1, 7, cx, u1), NoWork{});
      } else if (sl & 1) slot_step4x2<P, false, false>(av, cx, x0h, x0l, u1, unit_work<P, DENS>(2 * sl + 1, 7, cx, u1), unit_work<P, DENS>(2 * sl + 2, 7, cx, cx.xn));
      else slot_step4x2<P, false, true>(av, cx, x0h, x0l, u1, unit_work<P, DENS>(2 * sl + 1, 7, cx, u1), unit_work<P, DENS>(2 * sl + 2, 7, cx, cx.xn));
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < HS; ks += 2) {
      {
        const Unit xc = cx.xn;
        if (ks == 0) slot_step4<P, true, true>(av, cx, __builtin_bit_cast(bf16x8, xc.h), __builtin_bit_cast(bf16x8, xc.l), unit_work<P>(ks + 1, 7, cx, cx.xn));
        else slot_step4<P, false, true>(av, cx, __builtin_bit_cast(bf16x8, xc.h), __builtin_bit_cast(bf16x8, xc.l), unit_work<P>(ks + 1, 7, cx, cx.xn));
      }
      {
        const Unit xc = cx.xn;
        if (ks + 2 < HS) slot_step4<P, false, false>(av, cx, __builtin_bit_cast(bf16x8, xc.h), __builtin_bit_cast(bf16x8, xc.l), unit_work<P>(ks + 2, 7, cx, cx.xn));
        else slot_step4<P, false, false>(av, cx, __builtin_bit_cast(bf16x8, xc.h), __builtin_bit_cast(bf16x8, xc.l), NoWork{});
      }
    }
  }
}
// The three extra K-steps (direction encoding, appearance row, padding): split modes with NM_VIEWS_PAIRS -- the first two share a slot.
// no_app (wavefront-uniform: the launch has no appearance row): inputs 32..47 are all zero, and the third K-step, which would add exact
// zeros, is left out with its barrier -- it is the tile's last, so nothing behind it counts stream positions (cx.g starts over).
template <int P>
__device__ __forceinline__ void views_extras(f32x16 (&av)[4], Ctx& cx, const bf16x8 (&eh)[VS], const bf16x8 (&el)[VS], bool no_app) {
  if constexpr (is_split<P>()) {
    Unit u1;
    u1.h = __builtin_bit_cast(u32x4, eh[1]); u1.l = __builtin_bit_cast(u32x4, el[1]);
    slot_step4x2<P, false, true>(av, cx, eh[0], el[0], u1, NoWork{}, NoWork{});   // stream position NSLOT_NORGB + 8: even
    if (!no_app) slot_step4<P, false, false>(av, cx, eh[2], el[2], NoWork{});     // a single half slot at an odd position
  } else {
    slot_step4<P, false, true>(av, cx, eh[0], el[0], NoWork{});  // (the views layer's extra K-steps sit at positions 16, 17, 18)
    slot_step4<P, false, false>(av, cx, eh[1], el[1], NoWork{});
    if (!no_app) slot_step4<P, false, true>(av, cx, eh[2], el[2], NoWork{});
  }
}

// IPE K-steps of layers 0 (FIRST: they open the layer) and 5 (skip connection, after the hidden K-steps)
// (l: the layer they close, 0 or 5)
template <int P, bool FIRST>
__device__ __forceinline__ void ipe_steps(f32x16 (&acc)[8], Ctx& cx, const float* ipe_src, int l = FIRST ? 0 : 5) {
  auto operand = [&](int m, bf16x8& ph, bf16x8& pl) {
    // (fp16x1: one operand per K-step, at [m][64 lanes][4 floats] of the same LDS region)
    ph = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(ipe_src + (is_split<P>() ? (m * 2 + 0) : m) * 256));
    pl = ph;
    if constexpr (is_split<P>()) pl = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(ipe_src + (m * 2 + 1) * 256));
  };
  if constexpr (P == 2) {
    // fp16x3: K-step m + 1's pair is fetched in an empty gap of K-step m (IpeFetch), not in front of its first MFMA, where the LDS latency
    // was exposed twelve times per tile; only the group's first pair is read up front.  (cx.hv is dead here: the registers are free.)
    bf16x8 ph, pl, qh, ql;
    operand(0, ph, pl);
#pragma unroll
    for (int m = 0; m < XS; m += 2) {
      // (gaps: the first K-step of the group carries its eight DMA pieces in the first half, the others pieces 6, 7 in gaps 4, 5)
      if (m == 0) slot_step8<P, FIRST, true>(acc, cx, ph, pl, IpeFetch<17>{ipe_src, m + 1, qh, ql});
      else slot_step8<P, false, true, true>(acc, cx, ph, pl, IpeFetch<6>{ipe_src, m + 1, qh, ql});
      if (m + 2 == XS) slot_step8<P, false, false>(acc, cx, qh, ql, AccTake<P>{acc, cx, l});  // (the IPE steps close layers 0 and 5)
      else slot_step8<P, false, false, true>(acc, cx, qh, ql, IpeFetch<4>{ipe_src, m + 2, ph, pl});
    }
    return;
  }
#pragma unroll
  for (int m = 0; m < XS; m += 2) {  // (XS is even; pairs so that the position parity is a template argument)
    bf16x8 ph, pl;
    operand(m, ph, pl);
    if (m == 0) slot_step8<P, FIRST, true>(acc, cx, ph, pl, NoWork{});
    else slot_step8<P, false, true>(acc, cx, ph, pl, NoWork{});
    operand(m + 1, ph, pl);
    if (m + 2 == XS) slot_step8<P, false, false>(acc, cx, ph, pl, AccTake<P>{acc, cx, l});  // (the IPE steps close layers 0 and 5)
    else slot_step8<P, false, false>(acc, cx, ph, pl, NoWork{});
  }
}

// What a pass with colour heads does with a tap on layer 7, whose activations (cx.hv) the views layer is about to consume:
//   Tap7Workspace: parks them in the workspace (dump_tap) until the epilogue knows the compositing weights;
//   Tap7InRegisters{on, fn}: when `on`, calls fn(cx) right behind the density head instead -- the render kernel forms the weights there
//     (every sample's density exists one shuffle later) and reduces w * h7 straight from cx.hv: no store, no read-back.
struct Tap7Workspace {
  static constexpr bool on = false;
  __device__ __forceinline__ void fn(Ctx&) const {}
};
template <class F>
struct Tap7InRegisters {
  bool on;
  F fn;
};

// One pts layer (l = 1..7): unit ks+1 of the finished layer l-1 (in cx.hv) is made in the shadow of K-step ks.
// (feature_linear is no layer of this kernel: it has no activation, so nerf_pack_split multiplies it into the views layer.)
// (DENS: the caller's views K-loop accumulates the density head -- views_hidden<2, true> -- and this layer only opens the sum)
template <int P, bool DENS = false, class Tap7 = Tap7Workspace>
__device__ __forceinline__ void layer_pass(f32x16 (&acc)[8], int l, Ctx& cx, const float* ipe_src, const Tap7& tap7 = Tap7()) {
  if (l - 1 == cx.tap) dump_tap(l - 1, cx);
#pragma unroll
  for (int ks = 0; ks < HS; ks += 2) {  // (pairs: the parity of a K-step's position in the stream is a template argument)
    {
      const Unit xc = cx.xn;
      if (ks == 0) slot_step8<P, true, true>(acc, cx, __builtin_bit_cast(bf16x8, xc.h), __builtin_bit_cast(bf16x8, xc.l), unit_work<P>(ks + 1, l - 1, cx, cx.xn));
      else slot_step8<P, false, true, request_early<P>()>(acc, cx, __builtin_bit_cast(bf16x8, xc.h), __builtin_bit_cast(bf16x8, xc.l), unit_work<P>(ks + 1, l - 1, cx, cx.xn));
    }
    {
      const Unit xc = cx.xn;
      if (ks + 2 < HS) slot_step8<P, false, false, request_early<P>()>(acc, cx, __builtin_bit_cast(bf16x8, xc.h), __builtin_bit_cast(bf16x8, xc.l), unit_work<P>(ks + 2, l - 1, cx, cx.xn));
      // (every layer, no branch in the MFMA stream: in layer 5 the skip connection's IPE steps still follow, what is taken here is
      //  overwritten by their own AccTake)
      else slot_step8<P, false, false>(acc, cx, __builtin_bit_cast(bf16x8, xc.h), __builtin_bit_cast(bf16x8, xc.l), AccTake<P>{acc, cx, l});
    }
  }
  fold_range<P>(cx, l - 1);  // (all 16 units of layer l-1's output exist now)
  if constexpr (has_gates<P>()) {
    cx.gptr[(l - 1) * 256] = u32x4{cx.gbits[0], cx.gbits[1], cx.gbits[2], cx.gbits[3]};
    cx.gbits[0] = cx.gbits[1] = cx.gbits[2] = cx.gbits[3] = 0u;
  }
  if (l == 5) ipe_steps<P, false>(acc, cx, ipe_src);
  finish_layer<P>(acc, l, cx);
  if (l == 7) {  // the last pts layer: tap / density head read it from cx.hv (inside the layer loop's body: after the loop, next to the
                 // views K-loop, the register allocator spilled ~150 registers per tile)
    // (a pass without colour heads has no K-loop behind this point: it does the same after the layer loop, behind tap_prefetch)
    if (cx.rgb) {
      if (cx.tap == 7 && !tap7.on) dump_tap(7, cx);
      if constexpr (DENS) dens_open(cx);
      else alpha_head(cx);
      if (tap7.on) tap7.fn(cx);  // (here and not behind the loop for the same reason; the eight accumulator blocks are free at this point)
    }
  }
}

}  // namespace nmbf
