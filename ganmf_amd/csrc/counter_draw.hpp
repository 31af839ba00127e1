// counter_draw.hpp -- the counter-based generator, the three uniform picks and the one sampler kernel of the SGD trainers (slim_bpr.hpp,
// mf_sgd.hpp; lib/sgd_train.inc launches it).  cfgan_masks.hpp and caae_sample.hpp use the generator alone.
//
// Generator.  With mix() the output function of splitmix64,
//     mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
//     key = mix(mix(mix(seed) ^ epoch) ^ index);   word(stream, attempt) = mix(key ^ (stream << 32 | attempt));
//     below(w, m) = ((w >> 32) * m) >> 32          (a value in [0, m), m < 2^32)
// Sampler (draw_kernel), one thread per sample: sample g of a call has epoch epoch0 + g / per_epoch and index g % per_epoch.
//   user:     u = below(word(0, a), n_users) for a = 0, 1, ... until 0 < |profile(u)| < n_items; after DRAW_ATTEMPTS refusals
//             u = eligible[below(word(0, DRAW_ATTEMPTS), n_eligible)] (the eligible users ascending): uniform over them either way;
//   positive: i = profile(u)[below(word(1, 0), |profile(u)|)];
//   negative: j = below(word(2, a), n_items) for a = 0, 1, ... until j is not in the profile (binary search); after DRAW_ATTEMPTS
//             refusals the k-th item outside the profile, k = below(word(2, DRAW_ATTEMPTS), n_items - |profile(u)|).
//   rated = 0 (SLIM-BPR, MF-BPR): the triple (u, i, j).  rated = 1 (FunkSVD): the same user; a coin on stream 3 -- a positive iff
//   quota == 0 or double(below(word(3, 0), 2^31)) <= quota (2^31 - 1) -- then the positive pick with its stored rating, or the
//   negative pick with rating 0, as the sample's one item.
#pragma once
#include <hip/hip_runtime.h>
#include "itemknn_rows.hpp"

namespace ganmf {

__host__ __device__ __forceinline__ unsigned long long draw_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ unsigned long long draw_word(unsigned long long key, unsigned stream, unsigned attempt) {
  return draw_mix(key ^ (((unsigned long long)stream << 32) | attempt));
}
__host__ __device__ __forceinline__ unsigned draw_below(unsigned long long w, unsigned m) {
  return (unsigned)(((w >> 32) * (unsigned long long)m) >> 32);
}
__host__ __device__ __forceinline__ unsigned long long draw_key(unsigned long long seed, unsigned long long epoch, unsigned long long index) {
  return draw_mix(draw_mix(draw_mix(seed) ^ epoch) ^ index);
}

__device__ __forceinline__ bool in_profile(const int* __restrict__ items, long long a, long long b, int item) {
  const long long q = knn_lower_bound(items, a, b, item);
  return q < b && items[q] == item;
}

// stream 0: a user whose profile [*a, *b) is neither empty nor full, uniform over the eligible ones either way
__device__ __forceinline__ int draw_user(unsigned long long key, unsigned attempts, const long long* __restrict__ indptr,
                                              const int* __restrict__ eligible, int n_users, int n_items, int n_eligible, long long* a,
                                              long long* b) {
  for (unsigned at = 0; at < attempts; ++at) {
    const int c = (int)draw_below(draw_word(key, 0, at), (unsigned)n_users);
    *a = indptr[c];
    *b = indptr[c + 1];
    if (*b > *a && *b - *a < n_items) return c;
  }
  const int u = eligible[draw_below(draw_word(key, 0, attempts), (unsigned)n_eligible)];
  *a = indptr[u];
  *b = indptr[u + 1];
  return u;
}

// stream 1: the position in [a, b) of a uniform item of the profile
__device__ __forceinline__ long long draw_positive(unsigned long long key, long long a, long long b) {
  return a + draw_below(draw_word(key, 1, 0), (unsigned)(b - a));
}

// stream 2: a uniform item outside the (ascending) profile [a, b)
__device__ __forceinline__ int draw_negative(unsigned long long key, unsigned attempts, const int* __restrict__ items, long long a,
                                                  long long b, int n_items) {
  for (unsigned at = 0; at < attempts; ++at) {
    const int c = (int)draw_below(draw_word(key, 2, at), (unsigned)n_items);
    if (!in_profile(items, a, b, c)) return c;
  }
  int j = (int)draw_below(draw_word(key, 2, attempts), (unsigned)(n_items - (int)(b - a)));      // the k-th item outside the profile
  for (long long q = a; q < b && items[q] <= j; ++q) ++j;
  return j;
}

// ---- the sampler ------------------------------------------------------------------------------------------------------------------
constexpr int DRAW_THREADS = 256;
constexpr int DRAW_ATTEMPTS = 64;

struct DrawP {
  const long long* indptr;     // the profiles: users x items, items ascending without repeats inside a user
  const int* items;
  const double* ratings;       // rated: the stored value of every profile entry; else null
  const int* eligible;         // [n_eligible] the users with 0 < |profile| < n_items, ascending
  int n_users, n_items, n_eligible, rated;
  double quota;
  unsigned long long seed;
  long long epoch0, per_epoch, n;      // sample g of the call: epoch epoch0 + g / per_epoch, index g % per_epoch
  int* users;
  int* pos;
  int* neg;                    // the triple
  double* rating;              // rated
};

__global__ __launch_bounds__(DRAW_THREADS) void draw_kernel(const DrawP p) {
#pragma clang fp contract(off)
  const long long g = (long long)blockIdx.x * DRAW_THREADS + threadIdx.x;
  if (g >= p.n) return;
  const unsigned long long epoch = (unsigned long long)(p.epoch0 + g / p.per_epoch), index = (unsigned long long)(g % p.per_epoch);
  const unsigned long long key = draw_key(p.seed, epoch, index);
  long long a = 0, b = 0;
  const int u = draw_user(key, DRAW_ATTEMPTS, p.indptr, p.eligible, p.n_users, p.n_items, p.n_eligible, &a, &b);
  p.users[g] = u;
  if (!p.rated) {
    p.pos[g] = p.items[draw_positive(key, a, b)];
    p.neg[g] = draw_negative(key, DRAW_ATTEMPTS, p.items, a, b, p.n_items);
    return;
  }
  bool positive = true;
  if (p.quota != 0.0) positive = (double)draw_below(draw_word(key, 3, 0), 0x80000000u) <= p.quota * 2147483647.0;
  if (positive) {
    const long long q = draw_positive(key, a, b);
    p.pos[g] = p.items[q];
    p.rating[g] = p.ratings[q];
  } else {
    p.pos[g] = draw_negative(key, DRAW_ATTEMPTS, p.items, a, b, p.n_items);
    p.rating[g] = 0.0;
  }
}

}  // namespace ganmf
