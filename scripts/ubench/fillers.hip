// What does one wavefront per SIMD hide behind a v_mfma_f32_32x32x16_f16?  Cycles per MFMA for streams of 24 MFMAs on 8
// accumulators (the NeRF K-step's shape) with different fillers per gap.  Build: hipcc --offload-arch=gfx950 -O3 fillers.hip -o fillers
#include <hip/hip_runtime.h>
#include <cstdio>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)
#define SB __builtin_amdgcn_sched_barrier(0)

// MODE 0: bare MFMAs.  1: + 4 independent VALU per gap.  2: + 4 VALU in two dependent pairs (add -> med3).  3: + chain of 4 dependent
// VALU.  4: + 1 ds_read_b128 per gap (consumed a K-step later).  5: mode 2 + 1 ds_read_b128 per gap.  6: mode 5 + one s_barrier
// per 24 MFMAs.  7: mode 0 + one s_barrier per 24.  8: 6 VALU per gap, independent.  9: 8 VALU per gap, independent.
template <int MODE>
__global__ void __launch_bounds__(256, 1) k(float* out, int iters, unsigned long long* cyc) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < 16384; i += 256) lds[i] = 1e-3f * (i & 255);
  __syncthreads();
  f32x16 acc[8];
  for (int b = 0; b < 8; ++b)
    for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
  u32x4 opq[8];
  for (int b = 0; b < 8; ++b) opq[b] = u32x4{0x3c003c00u + lane, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u + b};
  f16x8 x = __builtin_bit_cast(f16x8, opq[0]);
  float v[8];
  for (int i = 0; i < 8; ++i) v[i] = 0.5f + lane * 1e-3f + i;
  const float cmax = 65504.f;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int m = 0; m < 24; ++m) {
      const int b = m & 7;
      acc[b] = MFMA(__builtin_bit_cast(f16x8, opq[b]), x, acc[b]);
      SB;
      if (MODE == 1 || MODE == 8 || MODE == 9) {
        const int n = MODE == 1 ? 4 : (MODE == 8 ? 6 : 8);
#pragma unroll
        for (int i = 0; i < n; ++i) { v[i] = v[i] * 1.0001f + 0.5f; asm volatile("" : "+v"(v[i])); }
      }
      if (MODE == 2 || MODE == 5 || MODE == 6) {
        float a0 = v[0] + v[2], a1 = v[1] + v[3];
        asm volatile("" : "+v"(a0), "+v"(a1));
        v[0] = __builtin_amdgcn_fmed3f(a0, 0.f, cmax); v[1] = __builtin_amdgcn_fmed3f(a1, 0.f, cmax);
        asm volatile("" : "+v"(v[0]), "+v"(v[1]));
      }
      if (MODE == 3) {
        float a0 = v[0] + v[2];
        asm volatile("" : "+v"(a0));
        a0 = __builtin_amdgcn_fmed3f(a0, 0.f, cmax);
        asm volatile("" : "+v"(a0));
        a0 = a0 * 1.0001f;
        asm volatile("" : "+v"(a0));
        v[0] = a0 + 0.25f;
        asm volatile("" : "+v"(v[0]));
      }
      if (MODE == 4 || MODE == 5 || MODE == 6) {
        opq[(b + 4) & 7] = reinterpret_cast<const u32x4*>(lds)[((m * 64) & 1023) + lane];
      }
      SB;
      if ((MODE == 6 || MODE == 7) && m == 11) { __builtin_amdgcn_s_barrier(); SB; }
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
  float r = 0.f;
  for (int b = 0; b < 8; ++b)
    for (int i = 0; i < 16; ++i) r += acc[b][i];
  for (int i = 0; i < 8; ++i) r += v[i];
  out[blockIdx.x * 256 + threadIdx.x] = r;
}

// Round 11: what does a SCALAR instruction cost in an MFMA gap, alone and beside an LDS-DMA piece?  The K-step's shape: 48 MFMAs per
// iteration, the eight 1 KiB pieces of a weight request (two slots of four pieces: one address / M0 each, told apart by the immediate
// offset) in gaps 4..11, every other gap empty unless the arm fills it; the pieces are waited for one iteration (~1500 cycles) later,
// as the ring barrier does.  The source is the same 64 KiB for all workgroups (L2 warm, like the weight blob).
//   SALU = k: k independent s_add_i32 in EVERY gap, no DMA (k = 0 is the bare stream).
//   DMA = 1: the pieces, M0 set once per slot in the empty gap in front of its first piece; + MOV s_mov_b32 beside every piece.
//   DMA = 2: the pieces with M0 saved, set and restored around each (the form the kernels used through round 10).
template <int SALU, int DMA, int MOV>
__global__ void __launch_bounds__(256, 1) ks(float* out, const char* src, int iters, unsigned long long* cyc) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x16 acc[8];
  for (int b = 0; b < 8; ++b)
    for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
  u32x4 opq[8];
  for (int b = 0; b < 8; ++b) opq[b] = u32x4{0x3c003c00u + lane, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u + b};
  const f16x8 x = __builtin_bit_cast(f16x8, opq[0]);
  int sv[10];
  for (int i = 0; i < 10; ++i) sv[i] = __builtin_amdgcn_readfirstlane(iters + i);
  // this wavefront's quarter (4 KiB) of two 16 KiB ring positions; piece = 64 lanes x 16 bytes at M0 + immediate offset
  const unsigned voff = (unsigned)(wave * 4096 + lane * 16);
  const unsigned lds0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(const __attribute__((address_space(3))) float*)(lds + wave * 1024));
  const unsigned lds1 = lds0 + 16384u;
  const char* src1 = src + 16384;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int m = 0; m < 48; ++m) {
      const int b = m & 7;
      acc[b] = MFMA(__builtin_bit_cast(f16x8, opq[b]), x, acc[b]);
      SB;
#pragma unroll
      for (int i = 0; i < SALU; ++i) asm volatile("s_add_i32 %0, %0, 1" : "+s"(sv[i]));
      if (DMA == 1 && (m == 3 || m == 7)) asm volatile("s_mov_b32 m0, %0" :: "s"(m == 3 ? lds0 : lds1));
      if (DMA && m >= 4 && m < 12) {
        const unsigned l = m < 8 ? lds0 : lds1;
        const char* s = m < 8 ? src : src1;
        unsigned saved;
#define PIECE(OFS)                                                                                                                    \
  if (DMA == 1) asm volatile("global_load_lds_dwordx4 %0, %1 offset:" #OFS :: "v"(voff), "s"(s) : "memory");                          \
  else asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %2, %3 offset:" #OFS "\n\ts_mov_b32 m0, %0"      \
                    : "=&s"(saved) : "s"(l), "v"(voff), "s"(s) : "memory")
        switch (m & 3) {
          case 0: PIECE(0); break;
          case 1: PIECE(1024); break;
          case 2: PIECE(2048); break;
          default: PIECE(3072); break;
        }
#undef PIECE
#pragma unroll
        for (int i = 0; i < MOV; ++i) asm volatile("s_mov_b32 %0, 7" : "=s"(sv[i]));
      }
      SB;
    }
    if (DMA) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // (the previous iteration's pieces)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
  float r = 0.f;
  for (int b = 0; b < 8; ++b)
    for (int i = 0; i < 16; ++i) r += acc[b][i];
  for (int i = 0; i < 10; ++i) r += (float)sv[i];
  __syncthreads();
  out[blockIdx.x * 256 + threadIdx.x] = r + lds[threadIdx.x];
}

template <int SALU, int DMA, int MOV>
double run_s(float* out, const char* src, unsigned long long* cyc, const char* name, double bare) {
  const int iters = 1000;
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  ks<SALU, DMA, MOV><<<256, 256, 65536>>>(out, src, iters, cyc);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  for (int i = 0; i < 3; ++i) ks<SALU, DMA, MOV><<<256, 256, 65536>>>(out, src, iters, cyc);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  ms /= 3;
  unsigned long long h[256];
  hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);
  double c = 0;
  for (int i = 0; i < 256; ++i) c += (double)h[i];
  c /= 256;
  const double per48 = c / iters;
  printf("%-66s %7.3f ms  %5.1f shader cycles/MFMA (s_memtime)  %7.1f per 48 MFMAs", name, ms, per48 / 48.0, per48);
  if (bare > 0) printf("  %+6.1f per %s", (per48 - bare) / (DMA ? 8.0 : 48.0), DMA ? "DMA gap" : "gap");
  printf("  clock %.2f GHz  (%s)\n", c / (ms * 1e6), hipGetErrorString(hipGetLastError()));
  return per48;
}

template <int MODE>
void run(float* out, unsigned long long* cyc, const char* name) {
  const int iters = 2000;
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  k<MODE><<<256, 256, 65536>>>(out, iters, cyc);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  for (int i = 0; i < 3; ++i) k<MODE><<<256, 256, 65536>>>(out, iters, cyc);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  ms /= 3;
  unsigned long long h[256];
  hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);
  double c = 0;
  for (int i = 0; i < 256; ++i) c += (double)h[i];
  c /= 256;
  printf("%-66s %7.3f ms  %5.1f shader cycles/MFMA (s_memtime)  clock %.2f GHz  (%s)\n", name, ms, c / (iters * 24.0), c / (ms * 1e6),
         hipGetErrorString(hipGetLastError()));
}

int main() {
  float* out;
  unsigned long long* cyc;
  hipMalloc(&out, 256 * 256 * 4);
  hipMalloc(&cyc, 256 * 8);
  run<0>(out, cyc, "0: bare MFMAs, 8 accumulators");
  run<1>(out, cyc, "1: + 4 independent VALU per gap");
  run<8>(out, cyc, "8: + 6 independent VALU per gap");
  run<9>(out, cyc, "9: + 8 independent VALU per gap");
  run<2>(out, cyc, "2: + 4 VALU per gap in two dependent pairs");
  run<3>(out, cyc, "3: + a chain of 4 dependent VALU per gap");
  run<4>(out, cyc, "4: + 1 ds_read_b128 per gap");
  run<5>(out, cyc, "5: + two dependent VALU pairs + 1 ds_read_b128 per gap");
  run<6>(out, cyc, "6: as 5 + one s_barrier per 24 MFMAs");
  run<7>(out, cyc, "7: bare + one s_barrier per 24 MFMAs");
  char* src;
  hipMalloc(&src, 65536);
  hipMemset(src, 0, 65536);
  const double bare = run_s<0, 0, 0>(out, src, cyc, "s0: bare MFMAs, 48 per iteration", 0.);
  run_s<3, 0, 0>(out, src, cyc, "s3: + 3 independent SALU per gap", bare);
  run_s<6, 0, 0>(out, src, cyc, "s6: + 6 independent SALU per gap", bare);
  run_s<10, 0, 0>(out, src, cyc, "s10: + 10 independent SALU per gap", bare);
  run_s<0, 1, 0>(out, src, cyc, "d0: 8 DMA pieces per 48 MFMAs, alone in their gaps", bare);
  run_s<0, 1, 1>(out, src, cyc, "d1: + 1 s_mov beside each piece", bare);
  run_s<0, 1, 3>(out, src, cyc, "d3: + 3 s_mov beside each piece", bare);
  run_s<0, 1, 10>(out, src, cyc, "d10: + 10 s_mov beside each piece", bare);
  run_s<0, 2, 0>(out, src, cyc, "dm: pieces with the M0 save / set / restore triple", bare);
  run_s<0, 0, 0>(out, src, cyc, "s0: bare MFMAs again", bare);
  return 0;
}
