// The split-bf16 vocabulary of the matrix-core kernels: every fp32 operand is two bf16 values (x = hi + lo) and a product is
// w_hi x_hi + w_hi x_lo + w_lo x_hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (gemm_bf16.hip has the error budget).
// Vector types, the hi / lo split, the re-packing of the accumulator layout (nrow, common.h), the 8 KiB weight-slot DMA, the fast exact-erf GELU.
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// x = hi + lo with hi, lo bf16 (round to nearest even): 16 bits of mantissa survive.
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const __bf16 h = (__bf16)v[i];
    hi[i] = h;
    lo[i] = (__bf16)(v[i] - (float)h);
  }
}

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {  // v_cvt_pk_bf16_f32 (round to nearest even)
  return __builtin_bit_cast(unsigned, bf16x2{(__bf16)a, (__bf16)b});
}

// B operands (hi, lo) of one K-step: 8 bf16 each, as 4 packed pairs
struct Unit {
  u32x4 h, l;
};

// values v[ob][r] (accumulator layout, NB blocks of 32 features) -> the 2 NB K-step operands of the next product, whose weights are
// packed in the matching K order (nm_linear_pack_perm_bf16x3): unit 2 ob + m = registers 8m .. 8m+7 of block ob
template <int NB>
__device__ __forceinline__ void repack(const f32x16 (&v)[NB], Unit (&u)[2 * NB]) {
#pragma unroll
  for (int ob = 0; ob < NB; ++ob)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      unsigned h4[4], l4[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const float x0 = v[ob][8 * m + 2 * p], x1 = v[ob][8 * m + 2 * p + 1];
        const unsigned hp = pack_bf16(x0, x1);
        h4[p] = hp;
        l4[p] = pack_bf16(x0 - __uint_as_float(hp << 16), x1 - __uint_as_float(hp & 0xffff0000u));
      }
      u[2 * ob + m].h = u32x4{h4[0], h4[1], h4[2], h4[3]};
      u[2 * ob + m].l = u32x4{l4[0], l4[1], l4[2], l4[3]};
    }
}

// Slot g of a stream of 8 KiB weight slots (4 blocks x (hi, lo) x 64 lanes x 16 bytes: one 16-wide K-step of a 128-row chunk) -> position
// g % RING of an LDS ring, by LDS DMA.  Two 1 KiB pieces per wavefront: one address / one M0, told apart by the immediate offset.
constexpr int NM_SLOT8K_BYTES = 8192;
template <int RING>
__device__ __forceinline__ void dma_slot_8k(const char* slots, int g, float* ring, int wave, int lane) {
  static_assert((RING & (RING - 1)) == 0, "ring positions: a power of two");
  const unsigned voff = (unsigned)(wave * 2048 + lane * 16);
  const char* base = slots + (size_t)g * NM_SLOT8K_BYTES;
  const auto* src = (const __attribute__((address_space(1))) void*)(base + voff);
  auto* dst = (__attribute__((address_space(3))) void*)(ring + (g & (RING - 1)) * (NM_SLOT8K_BYTES / 4) + wave * 512);
  __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
  __builtin_amdgcn_global_load_lds(src, dst, 16, 1024, 0);
}

// exact-erf GELU with erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7: below fp32 resolution of 1 + erf for the values that
// matter; one v_rcp + one v_exp + 7 FMA-class instructions instead of the ~50 of erff -- in the chained kernels 64 to 128 activations
// per lane sit between two products with nothing to overlap them).  NOT the arithmetic of gemm.hip / gemm_bf16.hip, which call erff.
__device__ __forceinline__ float gelu_erf(float v) {
  const float x = fabsf(v) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(NM_FMA(0.3275911f, x, 1.0f));
  float p = NM_FMA(1.061405429f, t, -1.453152027f);
  p = NM_FMA(p, t, 1.421413741f);
  p = NM_FMA(p, t, -0.284496736f);
  p = NM_FMA(p, t, 0.254829592f);
  const float e = 1.0f - (p * t) * __builtin_amdgcn_exp2f(-(x * x) * 1.44269504088896340736f);
  return 0.5f * v * (1.0f + copysignf(e, v));
}
