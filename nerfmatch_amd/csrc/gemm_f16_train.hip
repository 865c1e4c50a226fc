// The GEMMs of the fp16 mixed-precision NeRF training walk (nerf/train_render.py): fp16 operands, ONE product per K-step on
// v_mfma_f32_32x32x16_f16, fp32 accumulation.
//
// nm_linear_chain_f16 -- the chain GEMM, forward layers and dX products alike.  It is gemm_f16.hip's structure (8 KiB slots of a blob in
//   nm_linear_pack_f16's order streamed through the LDS ring one slot ahead, x rows as 16-byte fp16 pieces that already are B operands,
//   result lane = row / register = feature, transposed through the idle ring and written as row segments) with
//     * a second (x2, blob2) source: the K loop runs over the slots of both blobs, y = x . w^T + x2 . w2^T (the layers with a concatenated
//       input: no fp32 `pre` tensor is written or read);
//     * the epilogue  y = alpha * [gate > 0] * (relu?(acc) + residual)  with fp16 residual and gate rows (the saved activation of the layer
//       the gradient passes), applied to the fp32 accumulator whose start value is the bias;
//     * fp16 output rounded once (nearest even, no saturation; a stored value that is not finite while the fp32 value it was rounded from was
//       is counted into `overflow`) or fp32 output (the 8-wide heads, the appearance columns of d loss / d xd: never counted);
//     * a one-block form for N <= 32 (the heads): a quarter of the MFMAs and accumulators of the 128-column tile.
//   A row's result does not depend on M or on the row's place in its tile (column j of an MFMA is a function of column j of its B operand).
// nm_linear_pack_t_f16 -- the blob of w^T straight from the stored (K, N) tensor, like nm_linear_pack_t_bf16x3.
//
// nm_linear_wgrad_f16 -- dw[N,K] (+)= alpha * dy^T . x and db[N] (+)= alpha * column sums of dy.  Both operands are summed over the ROW index
//   of row-major fp16 tensors, so an MFMA operand is a column of 8 consecutive rows: row tiles of dy and x (64 rows x 128 columns) are staged
//   into LDS in 16-byte pieces -- the image of 8-row x 32-column subtiles of 512 bytes with the chunk index XOR-ed by (row >> 2) & 3, on which
//   the 32x32x16 operand's transposed reads are conflict free: a 32-lane half covers 4 rows x 64 bytes = 256 contiguous bytes -- and read back
//   with ds_read_b64_tr_b16.  That read needs EXEC all ones: the workgroup is 256 threads, the grid holds no surplus workgroup, and there
//   is no lane-dependent branch around the reads; rows past the slice's end and columns past N / K are ZEROS in the image (padded, not masked).
//   A workgroup owns a slice of rows (nm_linear_wgrad_f16_slice_rows) and one 128 x 128 tile of dw (wave = 32 rows of dw x 4 blocks; N <= 32:
//   32 x 128, wave = one block) and writes its partial to the workspace; a second kernel adds the slices' partials IN SLICE ORDER and applies
//   alpha: two runs give the same bits.  The column sums of dy ride in the staging registers (fp16 -> fp32 is exact), reduced in a fixed order.
#include "common.h"

namespace {

constexpr int CH_ROWS = 128;          // rows per workgroup
constexpr int CH_COLS = 128;          // output features per workgroup (4 blocks of 32)
constexpr int CH_KSLOT = 32;          // K per slot
constexpr int CH_SLOT_BYTES = 8192;   // 2 K-steps x 4 blocks x 64 lanes x 16 bytes (nm_linear_pack_f16's slot)
constexpr int CH_SLOT_FLOATS = CH_SLOT_BYTES / 4;
constexpr int CH_RING = 4;

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct ChainArgs {
  const _Float16* x;
  const char* blob;
  const _Float16* x2;
  const char* blob2;
  const float* bias;
  const _Float16* res;
  const _Float16* gate;
  void* y;
  int* overflow;
  float alpha;
  int M, N, K, K2, nks, nks2;
};

struct XRowC {
  u32x4 a, b;
};

// NB: 32-column blocks of the tile that are computed (4, or 1 when N <= 32); OUT16: fp16 output; RELU on the accumulator
template <int NB, bool OUT16, bool RELU>
__global__ void __launch_bounds__(256, 4) chain_f16_kernel(ChainArgs a) {
  __shared__ __attribute__((aligned(16))) float ring[CH_RING * CH_SLOT_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hi = lane >> 5;
  const int chunks = (a.N + CH_COLS - 1) / CH_COLS;
  const int g = blockIdx.x >> 3, chunk = g % chunks, row_tile = 8 * (g / chunks) + (blockIdx.x & 7);
  if (row_tile * CH_ROWS >= a.M) return;  // (whole workgroup: the row tiles are padded to a multiple of 8)
  const int m = row_tile * CH_ROWS + wave * 32 + r;
  const int mc = m < a.M ? m : a.M - 1;
  const int nks = a.nks, nkt = a.nks + a.nks2;
  const char* slots = a.blob + (size_t)chunk * nks * CH_SLOT_BYTES;
  const char* slots2 = a.nks2 ? a.blob2 + (size_t)chunk * a.nks2 * CH_SLOT_BYTES : slots;
  const _Float16* xrow = a.x + (size_t)mc * a.K;
  const _Float16* xrow2 = a.nks2 ? a.x2 + (size_t)mc * a.K2 : xrow;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  // step s of the K loop reads slot s of the first source, or slot s - nks of the second (a wavefront-uniform choice)
  auto dma = [&](int s) {
    const char* p = s < nks ? slots + (size_t)s * CH_SLOT_BYTES : slots2 + (size_t)(s - nks) * CH_SLOT_BYTES;
    const unsigned voff = (unsigned)(wave * 2048 + lane * 16);
    const auto* src = (const __attribute__((address_space(1))) void*)(p + voff);
    auto* dst = (__attribute__((address_space(3))) void*)(ring + (s & (CH_RING - 1)) * CH_SLOT_FLOATS + wave * 512);
    __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds(src, dst, 16, 1024, 0);
  };
  // an 8-wide piece is inside the row or entirely outside (K, K2 multiples of 8): one from outside is loaded at the row's first bytes and
  // replaced by zeros where it is consumed (gemm_f16.hip)
  auto xload = [&](int s) {
    XRowC v;
    const bool second = s >= nks;
    const _Float16* row = second ? xrow2 : xrow;
    const int Kc = second ? a.K2 : a.K, k = CH_KSLOT * (second ? s - nks : s) + 16 * hi;
    v.a = *reinterpret_cast<const u32x4*>(row + (k < Kc ? k : 0));
    v.b = *reinterpret_cast<const u32x4*>(row + (k + 8 < Kc ? k + 8 : 0));
    return v;
  };
  f32x16 acc[NB];
#pragma unroll
  for (int ob = 0; ob < NB; ++ob)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n0 = chunk * CH_COLS + 4 * hi + 32 * ob + 8 * q;
      f32x4 b = {0.f, 0.f, 0.f, 0.f};
      if (a.bias && n0 < a.N) b = *reinterpret_cast<const f32x4*>(a.bias + n0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[ob][4 * q + e] = b[e];
    }

  // one step = one slot: full wait + barrier, the requests of slot s + 1, the products of slot s (gemm_f16.hip's `step`)
  auto step = [&](int s, XRowC& xc, XRowC& xn) {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0); expcnt / lgkmcnt: no wait
    __builtin_amdgcn_s_barrier();
    if (s + 1 < nkt) {
      dma(s + 1);
      xn = xload(s + 1);
    }
    const bool second = s >= nks;
    const int Kc = second ? a.K2 : a.K, k = CH_KSLOT * (second ? s - nks : s) + 16 * hi;
    const f16x8 xa = __builtin_bit_cast(f16x8, k < Kc ? xc.a : zero4), xb = __builtin_bit_cast(f16x8, k + 8 < Kc ? xc.b : zero4);
    const u32x4* s4 = reinterpret_cast<const u32x4*>(ring + (s & (CH_RING - 1)) * CH_SLOT_FLOATS) + lane;
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {
      const f16x8 wa = __builtin_bit_cast(f16x8, s4[ob * 64]);
      const f16x8 wb = __builtin_bit_cast(f16x8, s4[(4 + ob) * 64]);
      acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa, xa, acc[ob], 0, 0, 0);
      acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wb, xb, acc[ob], 0, 0, 0);
    }
  };
  dma(0);
  XRowC xA = xload(0), xB = {zero4, zero4};
  for (int s = 0; s < nkt; s += 2) {
    step(s, xA, xB);
    if (s + 1 < nkt) step(s + 1, xB, xA);
  }

  // ---- epilogue: this wavefront's 8 KiB of the ring as the transposition buffer (32 rows x 16 pieces of 16 bytes, XOR-swizzled), 64 columns
  // at a time
  __builtin_amdgcn_s_barrier();
  float* tb = ring + wave * 2048;
  const int m0 = row_tile * CH_ROWS + wave * 32, n_chunk = chunk * CH_COLS;
  const int rrow = lane >> 4, rpiece = lane & 15;  // read side: row 4 i + rrow, piece rpiece
  constexpr int HALVES = NB == 4 ? 2 : 1, OBL = NB == 4 ? 2 : 1;
  int events = 0;
#pragma unroll
  for (int h = 0; h < HALVES; ++h) {
#pragma unroll
    for (int obl = 0; obl < OBL; ++obl)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ob = 2 * h + obl;
        f32x4 v = {acc[ob][4 * q], acc[ob][4 * q + 1], acc[ob][4 * q + 2], acc[ob][4 * q + 3]};
        if (RELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];  // (a NaN passes through the comparison)
        }
        const int p = obl * 8 + 2 * q + hi;
        *reinterpret_cast<f32x4*>(tb + r * 64 + ((p ^ (r & 15)) << 2)) = v;
      }
    const int n0 = n_chunk + 64 * h + 4 * rpiece;
    if (n0 < a.N && (NB == 4 || rpiece < 8)) {  // N a multiple of 8, n0 of 4: a piece is inside or outside
#pragma unroll
      for (int ib = 0; ib < 8; ++ib) {  // 4 rows at a time (8 or 16 in flight cost the fp16 kernels register spills at 4 wavefronts per SIMD)
        const int row = 4 * ib + rrow, mm = m0 + row;
        const size_t at = (size_t)(mm < a.M ? mm : a.M - 1) * a.N + n0;
        f16x4 rs, gt;
        if (a.res) rs = *reinterpret_cast<const f16x4*>(a.res + at);
        if (a.gate) gt = *reinterpret_cast<const f16x4*>(a.gate + at);
        f32x4 o = *reinterpret_cast<const f32x4*>(tb + row * 64 + ((rpiece ^ (row & 15)) << 2));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (a.res) o[e] = o[e] + (float)rs[e];
          if (a.gate) o[e] = gt[e] > (_Float16)0 ? o[e] : 0.f;
          o[e] = a.alpha * o[e];
        }
        if (OUT16) {
          f16x4 h4;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            h4[e] = (_Float16)o[e];
            events += (mm < a.M && f16_overflowed(o[e], h4[e])) ? 1 : 0;
          }
          if (mm < a.M) *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(a.y) + (size_t)mm * a.N + n0) = h4;
        } else {
          if (mm < a.M) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.y) + (size_t)mm * a.N + n0) = o;
        }
      }
    }
  }
  if (OUT16 && events && a.overflow) atomicAdd(a.overflow, events);
}

// blob element (chunk, s, j, ob, lane, i) = fp16(w[32 s + 16 (lane >> 5) + 8 j + i][128 chunk + 32 ob + (lane & 31)]) of the stored w (K, N):
// nm_linear_pack_f16's blob of w^T
__global__ void linear_pack_t_f16_kernel(const float* __restrict__ w, int N, int K, int nks, _Float16* __restrict__ blob, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int i = idx & 7, lane = (idx >> 3) & 63, ob = (idx >> 9) & 3, j = (idx >> 11) & 1;
  const size_t slot = idx >> 12;
  const int s = slot % nks, chunk = slot / nks;
  const int n = 128 * chunk + 32 * ob + (lane & 31), k = CH_KSLOT * s + 16 * (lane >> 5) + 8 * j + i;
  blob[idx] = (_Float16)((n < N && k < K) ? w[(size_t)k * N + n] : 0.f);
}

template <int NB>
void launch_chain(const ChainArgs& a, bool out16, bool relu, unsigned grid, hipStream_t s) {
  if (out16 && relu) chain_f16_kernel<NB, true, true><<<grid, 256, 0, s>>>(a);
  else if (out16) chain_f16_kernel<NB, true, false><<<grid, 256, 0, s>>>(a);
  else if (relu) chain_f16_kernel<NB, false, true><<<grid, 256, 0, s>>>(a);
  else chain_f16_kernel<NB, false, false><<<grid, 256, 0, s>>>(a);
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------------------
constexpr int WG_ROWS = 64;           // rows per stage (and the granule of a slice)
constexpr int WG_TILE = 128;          // columns of dy / of x per workgroup
constexpr int WG_MAX_SLICES = 256;    // slices of M at most: the partials of a 256 x 256 gradient then take 64 MiB

typedef short i16x4 __attribute__((ext_vector_type(4)));

// byte offset of 16-byte chunk `ch` of row `row` in the image of 8-row x 32-column subtiles, SUB subtiles per 8-row group
template <int SUB>
__device__ __forceinline__ int img_off(int row, int ch) {
  return 512 * SUB * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}

__device__ __forceinline__ i16x4 read_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(p));
}

// the 32x32x16 operand of rows r16 .. r16 + 15, columns 32 cb .. + 31 of an image: lane (half, column l & 31) gets rows r16 + 8 half .. + 7
template <int SUB>
__device__ __forceinline__ f16x8 operand_tr(const char* img, int r16, int cb, int lane) {
  const int half = lane >> 5, g1 = (lane >> 4) & 1, q = (lane >> 2) & 3, p = lane & 3;
  const int row = r16 + 8 * half + q, ch = 4 * cb + 2 * g1 + (p >> 1);
  const i16x4 lo = read_tr(img + img_off<SUB>(row, ch) + 8 * (p & 1));
  const i16x4 hi = read_tr(img + img_off<SUB>(row + 4, ch) + 8 * (p & 1));
  typedef short i16x8 __attribute__((ext_vector_type(8)));
  const i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(f16x8, v);
}

// DCH: 16-byte chunks per staged row of dy.  16: a 128-wide tile of dy, wavefront w = rows 32 w .. + 31 of the dw tile x 4 column blocks;
// 4 (N <= 32): a 32-wide tile, wavefront w = column block w.
template <int DCH>
__global__ void __launch_bounds__(256, 2) wgrad_f16_kernel(const _Float16* __restrict__ dy, const _Float16* __restrict__ x, int M, int N, int K,
                                                            int slice_rows, float* __restrict__ part_w, float* __restrict__ part_b) {
  constexpr int KB = DCH == 16 ? 4 : 1, DSUB = DCH / 4, DP = DCH / 4, DROWS = 256 / DCH;
  constexpr int DY_BYTES = WG_ROWS * DCH * 16, X_BYTES = WG_ROWS * 256;
  __shared__ __attribute__((aligned(16))) char lds[DY_BYTES + X_BYTES];
  char* dimg = lds;
  char* ximg = lds + DY_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ktiles = (K + WG_TILE - 1) / WG_TILE;
  const int slice = blockIdx.x, nt = blockIdx.y / ktiles, kt = blockIdx.y % ktiles;
  const int n_base = nt * DCH * 8, k_base = kt * WG_TILE;
  const int m_lo = slice * slice_rows, m_hi = min(M, m_lo + slice_rows);  // (m_lo < M: the grid holds no surplus slice)
  const int stages = (m_hi - m_lo + WG_ROWS - 1) / WG_ROWS;
  const int dch = tid % DCH, drow = tid / DCH, xch = tid & 15, xrow = tid >> 4;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  u32x4 dreg[DP], xreg[4];
  // every load is issued, at the tensor's first bytes when the piece lies outside, and replaced by zeros when it is written to LDS
  auto load = [&](int st) {
#pragma unroll
    for (int u = 0; u < DP; ++u) {
      const int mm = m_lo + st * WG_ROWS + drow + DROWS * u, col = n_base + 8 * dch;
      dreg[u] = *reinterpret_cast<const u32x4*>(dy + ((mm < m_hi && col < N) ? (size_t)mm * N + col : 0));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int mm = m_lo + st * WG_ROWS + xrow + 16 * u, col = k_base + 8 * xch;
      xreg[u] = *reinterpret_cast<const u32x4*>(x + ((mm < m_hi && col < K) ? (size_t)mm * K + col : 0));
    }
  };
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto store = [&](int st) {
#pragma unroll
    for (int u = 0; u < DP; ++u) {
      const int row = drow + DROWS * u, mm = m_lo + st * WG_ROWS + row, col = n_base + 8 * dch;
      const u32x4 v = (mm < m_hi && col < N) ? dreg[u] : zero4;
      *reinterpret_cast<u32x4*>(dimg + img_off<DSUB>(row, dch)) = v;
      const f16x8 h = __builtin_bit_cast(f16x8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) bsum[e] += (float)h[e];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = xrow + 16 * u, mm = m_lo + st * WG_ROWS + row, col = k_base + 8 * xch;
      *reinterpret_cast<u32x4*>(ximg + img_off<4>(row, xch)) = (mm < m_hi && col < K) ? xreg[u] : zero4;
    }
  };
  f32x16 acc[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[kb][e] = 0.f;

  load(0);
  for (int st = 0; st < stages; ++st) {
    __syncthreads();  // nobody reads the previous stage's image any more
    store(st);
    __syncthreads();
    if (st + 1 < stages) load(st + 1);  // in flight while this stage's products run
#pragma unroll
    for (int r16 = 0; r16 < WG_ROWS; r16 += 16) {
      const f16x8 av = operand_tr<DSUB>(dimg, r16, KB == 4 ? wave : 0, lane);
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const f16x8 bv = operand_tr<4>(ximg, r16, KB == 4 ? kb : wave, lane);
        acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv, acc[kb], 0, 0, 0);
      }
    }
  }
  // partial of this slice: register e of a lane = dw[n_base + 32 nb + nrow(e, half)][k_base + 32 cb + (lane & 31)]
  float* pw = part_w + (size_t)slice * N * K;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const int nb = KB == 4 ? wave : 0, cb = KB == 4 ? kb : wave;
    const int k = k_base + 32 * cb + (lane & 31);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int n = n_base + 32 * nb + nrow(e, lane >> 5);
      if (n < N && k < K) pw[(size_t)n * K + k] = acc[kb][e];
    }
  }
  // column sums of dy: this thread's 8 columns over its rows -> LDS -> one thread per column adds the DROWS row groups in order
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int e = 0; e < 8; ++e) red[drow * (DCH * 8) + dch * 8 + e] = bsum[e];
  __syncthreads();
  if (tid < DCH * 8 && kt == 0 && part_b && n_base + tid < N) {
    float s = 0.f;
    for (int gI = 0; gI < DROWS; ++gI) s += red[gI * (DCH * 8) + tid];
    part_b[(size_t)slice * N + n_base + tid] = s;
  }
}

// out[i] (+)= alpha * (partial 0 + partial 1 + ... in slice order)
__global__ void wgrad_f16_reduce_kernel(const float* __restrict__ part, int slices, size_t count, float alpha, int accumulate, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float s = 0.f;
  for (int k = 0; k < slices; ++k) s += part[(size_t)k * count + i];
  s = alpha * s;
  out[i] = accumulate ? out[i] + s : s;
}

// g4 (n,4) fp32 -> the two padded operand rows of the backward chain: g_logit (n,8) = fp16(scale g4[:, :3]) | 0, g_sig (n,8) = fp16(scale g4[:, 3]) | 0
__global__ void g4_split_f16_kernel(const float* __restrict__ g4, size_t n, float scale, _Float16* __restrict__ g_logit, _Float16* __restrict__ g_sig,
                                    int* __restrict__ overflow) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  int events = 0;
  if (i < n) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g4 + 4 * i);
    f16x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = a;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float sv = scale * v[e];
      const _Float16 h = (_Float16)sv;
      events += f16_overflowed(sv, h) ? 1 : 0;
      if (e < 3) a[e] = h;
      else b[0] = h;
    }
    *reinterpret_cast<f16x8*>(g_logit + 8 * i) = a;
    *reinterpret_cast<f16x8*>(g_sig + 8 * i) = b;
  }
  if (events && overflow) atomicAdd(overflow, events);
}

int wgrad_slices(int M, int* slice_rows) {
  const int granules = (M + WG_ROWS - 1) / WG_ROWS;
  const int per = (granules + WG_MAX_SLICES - 1) / WG_MAX_SLICES;
  *slice_rows = WG_ROWS * (per > 0 ? per : 1);
  return (M + *slice_rows - 1) / *slice_rows;
}

}  // namespace

extern "C" int nm_linear_pack_t_f16(const float* w, int N, int K, void* blob, nmStream_t stream) {
  NM_CHECK_ARG(w && blob && N > 0 && K > 0);
  const int nks = (K + CH_KSLOT - 1) / CH_KSLOT;
  const size_t total = (size_t)((N + CH_COLS - 1) / CH_COLS) * nks * (CH_SLOT_BYTES / 2);
  linear_pack_t_f16_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, N, K, nks, (_Float16*)blob, total);
  return nm_launch_status();
}

extern "C" int nm_linear_chain_f16(const void* x, const void* blob, int K, const void* x2, const void* blob2, int K2, const float* bias,
                                   const void* residual, const void* gate, float alpha, int relu, int M, int N, int out_f16, void* y,
                                   int* overflow, nmStream_t stream) {
  NM_CHECK_ARG(x && blob && y && x != y && M > 0 && N > 0 && K > 0 && (out_f16 == 0 || out_f16 == 1) && (relu == 0 || relu == 1));
  NM_CHECK_ARG((x2 != nullptr) == (blob2 != nullptr) && (x2 ? K2 > 0 : K2 == 0) && x2 != y && residual != y && gate != y);
  NM_CHECK_ARG(al16(x) && al16(blob) && al16(x2) && al16(blob2) && al16(y) && al16(bias) && al16(residual) && al16(gate));
  if (K % 8 != 0 || K2 % 8 != 0 || N % 8 != 0) return NM_ERR_UNSUPPORTED;
  ChainArgs a{};
  a.x = (const _Float16*)x; a.blob = (const char*)blob; a.x2 = (const _Float16*)x2; a.blob2 = (const char*)blob2; a.bias = bias;
  a.res = (const _Float16*)residual; a.gate = (const _Float16*)gate; a.y = y; a.overflow = overflow; a.alpha = alpha;
  a.M = M; a.N = N; a.K = K; a.K2 = K2; a.nks = (K + CH_KSLOT - 1) / CH_KSLOT; a.nks2 = x2 ? (K2 + CH_KSLOT - 1) / CH_KSLOT : 0;
  const int row_tiles = (M + CH_ROWS - 1) / CH_ROWS, chunks = (N + CH_COLS - 1) / CH_COLS;
  const unsigned grid = (unsigned)(((row_tiles + 7) / 8) * 8 * chunks);
  if (N <= 32) launch_chain<1>(a, out_f16 != 0, relu != 0, grid, (hipStream_t)stream);
  else launch_chain<4>(a, out_f16 != 0, relu != 0, grid, (hipStream_t)stream);
  return nm_launch_status();
}

extern "C" int nm_linear_wgrad_f16_slice_rows(int M) {
  int rows = 0;
  wgrad_slices(M > 0 ? M : 1, &rows);
  return rows;
}

extern "C" size_t nm_linear_wgrad_f16_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  int rows = 0;
  return (size_t)wgrad_slices(M, &rows) * ((size_t)N * K + N) * sizeof(float);
}

extern "C" int nm_linear_wgrad_f16(const void* dy, const void* x, int M, int N, int K, float alpha, int accumulate, float* dw, float* db,
                                   void* workspace, size_t workspace_bytes, nmStream_t stream) {
  NM_CHECK_ARG(dy && x && dw && M > 0 && N > 0 && K > 0 && (accumulate == 0 || accumulate == 1));
  if (N % 8 != 0 || K % 8 != 0 || !al16(dy) || !al16(x) || !al16(dw)) return NM_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < nm_linear_wgrad_f16_workspace_bytes(M, N, K)) return NM_ERR_WORKSPACE;
  int rows = 0;
  const int slices = wgrad_slices(M, &rows);
  float* part_w = (float*)workspace;
  float* part_b = part_w + (size_t)slices * N * K;
  hipStream_t s = (hipStream_t)stream;
  const int ktiles = (K + WG_TILE - 1) / WG_TILE;
  if (N <= 32)
    wgrad_f16_kernel<4><<<dim3(slices, ktiles), 256, 0, s>>>((const _Float16*)dy, (const _Float16*)x, M, N, K, rows, part_w, db ? part_b : nullptr);
  else
    wgrad_f16_kernel<16><<<dim3(slices, ((N + 127) / 128) * ktiles), 256, 0, s>>>((const _Float16*)dy, (const _Float16*)x, M, N, K, rows, part_w,
                                                                                 db ? part_b : nullptr);
  const size_t nw = (size_t)N * K;
  wgrad_f16_reduce_kernel<<<(unsigned)((nw + 255) / 256), 256, 0, s>>>(part_w, slices, nw, alpha, accumulate, dw);
  if (db) wgrad_f16_reduce_kernel<<<(unsigned)((N + 255) / 256), 256, 0, s>>>(part_b, slices, (size_t)N, alpha, accumulate, db);
  return nm_launch_status();
}

extern "C" int nm_nerf_g4_split_f16(const float* g4, size_t n, float scale, void* g_logit, void* g_sig, int* overflow, nmStream_t stream) {
  NM_CHECK_ARG(g4 && g_logit && g_sig && n > 0 && n / 256 < 0x7fffffffu && al16(g4) && al16(g_logit) && al16(g_sig));
  g4_split_f16_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(g4, n, scale, (_Float16*)g_logit, (_Float16*)g_sig, overflow);
  return nm_launch_status();
}
