// counter_draw.hpp -- the counter-based generator and the three uniform picks that the BPR-style samplers share (slim_draw_kernel in
// slim_bpr.hpp, mf_draw_kernel in mf_sgd.hpp; cfgan_masks.hpp and caae_sample.hpp use the generator alone).  slim_bpr.hpp states the
// scheme in full; the number of refusals in front of a fall-back is the caller's (SLIM_ATTEMPTS).
//     mix(z): the output function of splitmix64;   word(key, stream, attempt) = mix(key ^ (stream << 32 | attempt));
//     below(w, m) = ((w >> 32) * m) >> 32          (a value in [0, m), m < 2^32)
#pragma once
#include <hip/hip_runtime.h>
#include "itemknn_rows.hpp"

namespace ganmf {

__host__ __device__ __forceinline__ unsigned long long slim_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ unsigned long long slim_word(unsigned long long key, unsigned stream, unsigned attempt) {
  return slim_mix(key ^ (((unsigned long long)stream << 32) | attempt));
}
__host__ __device__ __forceinline__ unsigned slim_below(unsigned long long w, unsigned m) {
  return (unsigned)(((w >> 32) * (unsigned long long)m) >> 32);
}
__host__ __device__ __forceinline__ unsigned long long slim_key(unsigned long long seed, unsigned long long epoch, unsigned long long index) {
  return slim_mix(slim_mix(slim_mix(seed) ^ epoch) ^ index);
}

__device__ __forceinline__ bool slim_in_profile(const int* __restrict__ items, long long a, long long b, int item) {
  const long long q = knn_lower_bound(items, a, b, item);
  return q < b && items[q] == item;
}

// stream 0: a user whose profile [*a, *b) is neither empty nor full, uniform over the eligible ones either way
__device__ __forceinline__ int slim_draw_user(unsigned long long key, unsigned attempts, const long long* __restrict__ indptr,
                                              const int* __restrict__ eligible, int n_users, int n_items, int n_eligible, long long* a,
                                              long long* b) {
  for (unsigned at = 0; at < attempts; ++at) {
    const int c = (int)slim_below(slim_word(key, 0, at), (unsigned)n_users);
    *a = indptr[c];
    *b = indptr[c + 1];
    if (*b > *a && *b - *a < n_items) return c;
  }
  const int u = eligible[slim_below(slim_word(key, 0, attempts), (unsigned)n_eligible)];
  *a = indptr[u];
  *b = indptr[u + 1];
  return u;
}

// stream 1: the position in [a, b) of a uniform item of the profile
__device__ __forceinline__ long long slim_draw_positive(unsigned long long key, long long a, long long b) {
  return a + slim_below(slim_word(key, 1, 0), (unsigned)(b - a));
}

// stream 2: a uniform item outside the (ascending) profile [a, b)
__device__ __forceinline__ int slim_draw_negative(unsigned long long key, unsigned attempts, const int* __restrict__ items, long long a,
                                                  long long b, int n_items) {
  for (unsigned at = 0; at < attempts; ++at) {
    const int c = (int)slim_below(slim_word(key, 2, at), (unsigned)n_items);
    if (!slim_in_profile(items, a, b, c)) return c;
  }
  int j = (int)slim_below(slim_word(key, 2, attempts), (unsigned)(n_items - (int)(b - a)));      // the k-th item outside the profile
  for (long long q = a; q < b && items[q] <= j; ++q) ++j;
  return j;
}

}  // namespace ganmf
