// Reference point sets of a matcher batch from a device-resident scene cache (ref_bank.py).  The reference reads the cached renders of a
// query's top-k retrieved frames from disk, stacks k * n rows of 3 + D floats, projects all of them into each of the k cameras, runs a
// sequential co-visibility rule over the views, compacts, draws sample_pts rows by a randperm and copies the result to the device
// (NeRFMatchMultiPair.load_ref_pts, nerfmatch/datasets/nerfmatch_dataset.py:441-518; load_frame_3d, datasets/data_loading.py:36-80).
// Here the cache lives on the device -- pt3d [F,n,3], pt_feat [F,n,D], pt_mask [F,n], one 21-float camera row per frame -- and three
// launches make a batch's sets in place:
//
//   visibility  one thread per (query, candidate): k projections, one 32-bit word (bit j: inside image j)        (:480-498)
//   select      one workgroup per query: the k sequential union / intersection decisions, then the ordered list of the visible candidates
//               and their number Nv                                                                              (:499-506)
//   gather      one wavefront per output row: row q is candidate list[perm(q mod Nv)]                            (:509-516)
//
// Candidate c = s * n + r is row r of the frame in slot s of the query's id row.  `visible` is never stored: after rounds 0 .. j it is a
// function of the candidate's word w and the decision bits d alone.  A round changes a candidate only when its bit equals the decision
// (union with bit 1 sets it, intersection with bit 0 clears it), so the value is the bit of the LAST round i <= j with w_i == d_i, and
// true when there is none -- two bit operations and a count-leading-zeros, for every k <= 32, with neither a bitmap in LDS nor a spare
// bit in the word.  Every round re-reads the words (k * n * 4 bytes per query: they stay in L2).
//
// All counts are integers and every output element has exactly one writer: two runs give the same bits.  The build uses
// -ffp-contract=off; the projection is supervision.hip's fp32 mul / add / true-division sequence.
#include "common.h"
#include "perm.h"

#include <limits.h>

namespace {

constexpr int REF_MAX_K = 32;             // views per query: one bit each in a 32-bit word
constexpr int REF_MAX_CAND = 1 << 20;     // k * n
constexpr int REF_MAX_ROWS = 1 << 20;     // sample_pts
constexpr int REF_MAX_D = 1024;
constexpr int REF_SELECT_THREADS = 1024;  // the chunk of the compaction's scan
constexpr int REF_SELECT_WAVES = REF_SELECT_THREADS / 64;
constexpr int REF_SELECT_UNROLL = 8;      // chunks whose words are loaded together when they are streamed
constexpr int REF_SELECT_GROUP = 64;      // chunks per scan: 64 x 16 wavefront counts, one per thread

// a frame id clamped into the bank (an id outside it is counted by the gather kernel)
__device__ __forceinline__ long long clamp_frame(long long f, int F) { return f < 0 ? 0 : (f >= F ? F - 1 : f); }

// `visible` of a candidate with word w after the rounds 0 .. rounds-1 with decision bits dec (1 = the union was taken)
__device__ __forceinline__ bool visible_after(uint32_t w, uint32_t dec, int rounds) {
  const uint32_t m = rounds >= 32 ? 0xFFFFFFFFu : ((1u << rounds) - 1u);
  const uint32_t decisive = ~(w ^ dec) & m;
  if (!decisive) return true;
  return (w >> (31 - __clz(decisive))) & 1u;
}

// one chunk of a wavefront in the compaction: its number of visible candidates to *count; its visible candidates to first[rank among them]
__device__ __forceinline__ void count_chunk(bool vis, int* count, int lane) {
  const int n_vis = wave_count(vis);
  if (lane == 0) *count = n_vis;
}
__device__ __forceinline__ void place_chunk(bool vis, int c, int* first, int lane) {
  const unsigned long long ballot = __ballot(vis);
  if (vis) first[__popcll(ballot & ((1ull << lane) - 1ull))] = c;
}

// grid (ceil(k n / 256), B).  The k camera rows of the query are staged in LDS once per block; every lane reads the same address.
__global__ void __launch_bounds__(256) refbank_visibility_kernel(const float* __restrict__ pt3d, const float* __restrict__ cams,
                                                                  const long long* __restrict__ ref_ids, int F, int n, int k, float img_w,
                                                                  float img_h, uint32_t* __restrict__ words) {
  __shared__ float cam[REF_MAX_K * 21];
  const int b = blockIdx.y, N = k * n;
  const long long* ids = ref_ids + (size_t)b * k;
  for (int t = threadIdx.x; t < k * 21; t += 256) {
    const int s = t / 21;
    cam[t] = cams[(size_t)clamp_frame(ids[s], F) * 21 + (t - s * 21)];
  }
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int s = c / n, r = c - s * n;
  const float* X = pt3d + ((size_t)clamp_frame(ids[s], F) * n + r) * 3;
  const float x = X[0], y = X[1], z = X[2];
  uint32_t w = 0;
  for (int j = 0; j < k; ++j) {
    const float* Kc = cam + j * 21;  // diag(W / w_f, H / h_f, 1) K_f, row-major
    const float* Rt = Kc + 9;        // rows 0..2 of the world-to-camera matrix
    // p = R X + t, q = p / p.z, pix = K q  (project_points3d, nerfmatch/utils/geometry.py:130-133; supervision.py::_project_torch's order)
    const float px = ((Rt[0] * x + Rt[1] * y) + Rt[2] * z) + Rt[3];
    const float py = ((Rt[4] * x + Rt[5] * y) + Rt[6] * z) + Rt[7];
    const float pz = ((Rt[8] * x + Rt[9] * y) + Rt[10] * z) + Rt[11];
    const float qx = px / pz, qy = py / pz, qz = pz / pz;
    const float u = (Kc[0] * qx + Kc[1] * qy) + Kc[2] * qz;
    const float v = (Kc[3] * qx + Kc[4] * qy) + Kc[5] * qz;
    // (rpt2d >= 0).all(-1) & (rpt2d < WH).all(-1), :498 -- no depth test; a NaN or an infinity fails a comparison, as in torch
    if (u >= 0.f && v >= 0.f && u < img_w && v < img_h) w |= 1u << j;
  }
  words[(size_t)b * N + c] = w;
}

// One workgroup per query.  Round j counts I = |visible & bit_j| and U = |visible | bit_j| over all candidates (ballot + popcount per
// wavefront, the wavefronts' sums through LDS); V = |visible| is carried: N before round 0, then U or I.  The union is taken when
// 3 I < V (`intersect.sum() < visible.sum() / 3`, :502).  V >= 1 throughout: an intersection is only taken with 3 I >= V >= 1.
// Then the visible candidates in ascending order, in groups of 64 chunks of 1024 candidates: every wavefront's ballot count of every
// chunk goes to LDS (1024 counts in candidate order), one exclusive scan over them -- a thread per count -- gives each wavefront its
// first slot, a running carry chains the groups.  list[Nv .. N) = -1.
// Every pass streams the words from L2, eight chunks' loads in flight together.  The kernel is bound by its integer work on ONE compute
// unit per query (about 14 instructions per candidate and round), not by these loads: a variant that held the words in registers across
// the rounds was measured and was not faster.
__global__ void __launch_bounds__(REF_SELECT_THREADS) refbank_select_kernel(const uint32_t* __restrict__ words_all, int k, int N,
                                                                             int* __restrict__ list_all, int* __restrict__ n_visible,
                                                                             int* __restrict__ decisions) {
  __shared__ int wI[2][REF_SELECT_WAVES];
  __shared__ int wU[2][REF_SELECT_WAVES];
  __shared__ int cnt[REF_SELECT_GROUP * REF_SELECT_WAVES];  // per (chunk, wavefront) of a group: the count, then its exclusive prefix
  __shared__ int wsum[REF_SELECT_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* words = words_all + (size_t)b * N;
  int* list = list_all + (size_t)b * N;
  uint32_t dec = 0;
  int V = N;
  for (int j = 0; j < k; ++j) {
    int cI = 0, cU = 0;  // (the same value in every lane of the wavefront)
#pragma unroll 1
    for (int base = 0; base < N; base += REF_SELECT_UNROLL * REF_SELECT_THREADS) {
      uint32_t w[REF_SELECT_UNROLL];  // the loads of eight chunks are in flight together
#pragma unroll
      for (int u = 0; u < REF_SELECT_UNROLL; ++u) {
        const int c = base + u * REF_SELECT_THREADS + tid;
        w[u] = c < N ? words[c] : 0u;
      }
#pragma unroll
      for (int u = 0; u < REF_SELECT_UNROLL; ++u) {
        const bool in = base + u * REF_SELECT_THREADS + tid < N;
        const bool vis = in && visible_after(w[u], dec, j), bit = in && ((w[u] >> j) & 1u);
        cI += wave_count(vis && bit);
        cU += wave_count(vis || bit);
      }
    }
    const int buf = j & 1;  // two buffers: the writes of round j + 1 do not meet the reads of round j, one barrier per round
    if (lane == 0) {
      wI[buf][wave] = cI;
      wU[buf][wave] = cU;
    }
    __syncthreads();
    int I = 0, U = 0;
#pragma unroll
    for (int w = 0; w < REF_SELECT_WAVES; ++w) {
      I += wI[buf][w];
      U += wU[buf][w];
    }
    const bool take_union = 3 * I < V;  // (3 I <= 3 * 2^20: no overflow)
    V = take_union ? U : I;
    dec |= (take_union ? 1u : 0u) << j;
  }
  int carry = 0;
  for (int g0 = 0; g0 < N; g0 += REF_SELECT_GROUP * REF_SELECT_THREADS) {
    // 1. the wavefronts' counts of the group's 64 chunks, in candidate order (chunks past N count 0)
#pragma unroll 1
    for (int u0 = 0; u0 < REF_SELECT_GROUP; u0 += REF_SELECT_UNROLL) {
      uint32_t w[REF_SELECT_UNROLL];
#pragma unroll
      for (int u = 0; u < REF_SELECT_UNROLL; ++u) {
        const int c = g0 + (u0 + u) * REF_SELECT_THREADS + tid;
        w[u] = c < N ? words[c] : 0u;
      }
#pragma unroll
      for (int u = 0; u < REF_SELECT_UNROLL; ++u)
        count_chunk(g0 + (u0 + u) * REF_SELECT_THREADS + tid < N && visible_after(w[u], dec, k), cnt + (u0 + u) * REF_SELECT_WAVES + wave, lane);
    }
    __syncthreads();
    // 2. exclusive scan of the 1024 counts, one per thread: shuffles inside the wavefront, the wavefronts' sums through LDS
    const int mine = cnt[tid];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = incl - mine, total = 0;
#pragma unroll
    for (int w = 0; w < REF_SELECT_WAVES; ++w) {
      const int s = wsum[w];
      before += w < wave ? s : 0;
      total += s;
    }
    cnt[tid] = before;  // (its own entry: no other thread reads cnt[tid] before the barrier)
    __syncthreads();
    // 3. every visible candidate to (carry) + (first slot of its wavefront's chunk) + (visible lanes below it): slot < carry + total <= N
#pragma unroll 1
    for (int u0 = 0; u0 < REF_SELECT_GROUP; u0 += REF_SELECT_UNROLL) {
      uint32_t w[REF_SELECT_UNROLL];
#pragma unroll
      for (int u = 0; u < REF_SELECT_UNROLL; ++u) {
        const int c = g0 + (u0 + u) * REF_SELECT_THREADS + tid;
        w[u] = c < N ? words[c] : 0u;
      }
#pragma unroll
      for (int u = 0; u < REF_SELECT_UNROLL; ++u) {
        const int c = g0 + (u0 + u) * REF_SELECT_THREADS + tid;
        place_chunk(c < N && visible_after(w[u], dec, k), c, list + carry + cnt[(u0 + u) * REF_SELECT_WAVES + wave], lane);
      }
    }
    carry += total;
    __syncthreads();  // the next group rewrites cnt and wsum
  }
  for (int i = carry + tid; i < N; i += REF_SELECT_THREADS) list[i] = -1;
  if (tid == 0) {
    n_visible[b] = carry;
    decisions[b] = (int)dec;
  }
}

// grid (ceil(P / 4), B), four wavefronts per block, one output row each.  list == NULL: row q is candidate q (the stacked layout, P = k n).
// Otherwise row q is candidate list[perm(q mod Nv)] with perm the bank permutation of [0, Nv) under the query's round keys; its width comes
// from Nv here, on the device: 2 half_bits = the smallest even number of bits with 2^bits >= Nv (ray_bank.perm_params).
__global__ void __launch_bounds__(256) refbank_gather_kernel(const float* __restrict__ pt3d, const float* __restrict__ pt_feat,
                                                              const uint8_t* __restrict__ pt_mask, const long long* __restrict__ ref_ids, int F,
                                                              int n, int D, int k, const int* __restrict__ list_all,
                                                              const int* __restrict__ n_visible, const uint32_t* __restrict__ perm_keys, int P,
                                                              float* __restrict__ out_pt3d, float* __restrict__ out_feat,
                                                              uint8_t* __restrict__ out_mask, int* __restrict__ bad) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = k * n;
  const long long* ids = ref_ids + (size_t)b * k;
  if (blockIdx.x == 0 && wave == 0) {  // the query's k frame ids are checked once per launch (k <= 32 lanes)
    const bool out = lane < k && (ids[lane] < 0 || ids[lane] >= F);
    const int cnt = wave_count(out);
    if (lane == 0 && cnt) atomicAdd(bad, cnt);
  }
  const int q = blockIdx.x * 4 + wave;
  if (q >= P) return;
  int c = q;
  if (list_all) {
    const int Nv = min(max(n_visible[b], 1), N);
    const int bits = Nv > 1 ? 32 - __clz(Nv - 1) : 0, hb = (bits + 1) >> 1;
    uint32_t keys[NM_PERM_ROUNDS];
#pragma unroll
    for (int i = 0; i < NM_PERM_ROUNDS; ++i) keys[i] = perm_keys[b * NM_PERM_ROUNDS + i];
    const int slot = (int)nm_perm_walk((unsigned long long)(q % Nv), (unsigned long long)Nv, keys, hb);
    c = list_all[(size_t)b * N + slot];
  }
  c = min(max(c, 0), N - 1);  // (nothing read from memory can make the kernel leave the tables)
  const int s = c / n, r = c - s * n;
  const size_t src = (size_t)clamp_frame(ids[s], F) * n + r, dst = (size_t)b * P + q;
  const f32x4* fs = reinterpret_cast<const f32x4*>(pt_feat + src * D);  // D % 4 == 0 and 16-byte aligned bases: aligned rows
  f32x4* fd = reinterpret_cast<f32x4*>(out_feat + dst * D);
  for (int i = lane; i < D / 4; i += 64) fd[i] = fs[i];
  if (lane < 3) out_pt3d[dst * 3 + lane] = pt3d[src * 3 + lane];
  if (lane == 3) out_mask[dst] = pt_mask[src];
}

}  // namespace

extern "C" int nm_refbank_visibility(const float* pt3d, const float* cams, const long long* ref_ids, int F, int n, int B, int k, int img_w,
                                     int img_h, uint32_t* words, nmStream_t stream) {
  NM_CHECK_ARG(pt3d && cams && ref_ids && words && F > 0 && n > 0 && B > 0 && B <= 65535 && k > 0 && img_w > 0 && img_h > 0);
  if (k > REF_MAX_K || (long long)k * n > REF_MAX_CAND) return NM_ERR_UNSUPPORTED;
  const int N = k * n;
  refbank_visibility_kernel<<<dim3((N + 255) / 256, B), 256, 0, (hipStream_t)stream>>>(pt3d, cams, ref_ids, F, n, k, (float)img_w, (float)img_h,
                                                                                        words);
  return nm_launch_status();
}

extern "C" int nm_refbank_select(const uint32_t* words, int B, int k, int N, int* list, int* n_visible, int* decisions, nmStream_t stream) {
  NM_CHECK_ARG(words && list && n_visible && decisions && B > 0 && k > 0 && N > 0);
  if (k > REF_MAX_K || N > REF_MAX_CAND) return NM_ERR_UNSUPPORTED;
  refbank_select_kernel<<<B, REF_SELECT_THREADS, 0, (hipStream_t)stream>>>(words, k, N, list, n_visible, decisions);
  return nm_launch_status();
}

extern "C" int nm_refbank_gather(const float* pt3d, const float* pt_feat, const uint8_t* pt_mask, const long long* ref_ids, int F, int n, int D,
                                 int B, int k, const int* list, const int* n_visible, const uint32_t* perm_keys, int P, float* out_pt3d,
                                 float* out_feat, uint8_t* out_mask, int* bad, nmStream_t stream) {
  NM_CHECK_ARG(pt3d && pt_feat && pt_mask && ref_ids && out_pt3d && out_feat && out_mask && bad);
  NM_CHECK_ARG(F > 0 && n > 0 && D > 0 && B > 0 && B <= 65535 && k > 0 && P > 0);
  NM_CHECK_ARG(list ? (n_visible && perm_keys) : (long long)P == (long long)k * n);
  NM_CHECK_ARG((((uintptr_t)pt_feat | (uintptr_t)out_feat) & 15) == 0);
  if (D % 4 || D > REF_MAX_D || k > REF_MAX_K || (long long)k * n > REF_MAX_CAND || P > REF_MAX_ROWS) return NM_ERR_UNSUPPORTED;
  refbank_gather_kernel<<<dim3((P + 3) / 4, B), 256, 0, (hipStream_t)stream>>>(pt3d, pt_feat, pt_mask, ref_ids, F, n, D, k, list, n_visible,
                                                                                perm_keys, P, out_pt3d, out_feat, out_mask, bad);
  return nm_launch_status();
}
