// The keyed permutation of [0, n) that the banks draw their orders from (nerf/ray_bank.py::epoch_ids states it in torch): a balanced
// Feistel network over 2 * half_bits bits whose round function is nm_mix32, re-applied while the value is >= n (cycle walking).
// Shared by ray_bank.hip (the epoch order of the training pixels) and ref_bank.hip (the draw of a query's reference points).
#pragma once
#include "common.h"

constexpr int NM_PERM_ROUNDS = 4;

// one pass of the keyed bijection of [0, 2^(2 half_bits)): (l, r) -> (r, l ^ (mix(r + key) & (2^half_bits - 1))), four rounds
__device__ __forceinline__ unsigned long long nm_feistel(unsigned long long x, const uint32_t (&keys)[NM_PERM_ROUNDS], int hb) {
  const uint32_t m = (1u << hb) - 1u;
  uint32_t l = (uint32_t)(x >> hb), r = (uint32_t)x & m;
#pragma unroll
  for (int k = 0; k < NM_PERM_ROUNDS; ++k) {
    const uint32_t t = l ^ (nm_mix32(r + keys[k]) & m);
    l = r;
    r = t;
  }
  return ((unsigned long long)l << hb) | r;
}

// cycle walking from a position below n: the walk stays on the start point's own cycle, which contains a value below n (the start point
// itself) -- it terminates.  The domain 2^(2 half_bits) must cover n.
__device__ __forceinline__ unsigned long long nm_perm_walk(unsigned long long pos, unsigned long long n, const uint32_t (&keys)[NM_PERM_ROUNDS],
                                                           int hb) {
  unsigned long long x = pos;
  do x = nm_feistel(x, keys, hb);
  while (x >= n);
  return x;
}
