// Sort keys and the LDS sort that every ordering kernel shares: the tie rules of the callers (which index wins among equal
// scores) live in how they compose a key, the order of the scores themselves lives here.
#pragma once
#include "common.h"

namespace relnet {

// Order-preserving float -> unsigned (larger value => larger key; -inf below every finite value, -0.0 below +0.0).
__device__ __forceinline__ unsigned int order_key(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long order_key(double d) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// Descending bitonic sort of keys[0, np2) in LDS by a workgroup of THREADS threads; np2 is a power of two and the caller has
// filled the tail with keys that sort last.  Preceded by the caller's barrier after the fill, ends with a barrier.
// Thread = element index: half of the threads idle in every stage.
template <int THREADS>
__device__ __forceinline__ void bitonic_sort_desc(unsigned long long* keys, int np2) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < np2; i += THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = keys[i], d = keys[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (a < d) : (a > d)) { keys[i] = d; keys[ixj] = a; }
        }
      }
      __syncthreads();
    }
}
// The same network with thread = pair (i, i | j): all threads busy in every stage.
template <int THREADS>
__device__ __forceinline__ void bitonic_sort_desc_pairs(unsigned long long* keys, int np2) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= np2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = tid; p < (np2 >> 1); p += THREADS) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), ixj = i | j;
        const unsigned long long a = keys[i], c = keys[ixj];
        const bool desc = (i & k) == 0;
        if (desc ? (a < c) : (a > c)) { keys[i] = c; keys[ixj] = a; }
      }
      __syncthreads();
    }
  }
}

}  // namespace relnet
