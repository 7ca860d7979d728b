// The dropout masks of the pooling net's two sites (include/sgg.h, "Pooling
// dropout masks"): a stateless function of (seed, offset, site, i, j, col).
//   i: global row of the pooled ped; j: scene-local index of the other ped;
//   col: hidden unit k (site SGG_POOL_DROP_SITE_HIDDEN) or output column c
//   (site SGG_POOL_DROP_SITE_OUT).
//   counter (i, (j << 8) | ((col >> 4) << 2) | (col & 3), site << 8, offset),
//   output word (col >> 2) & 3: one call covers col, col + 4, col + 8, col + 12
//   -- the four hidden units one lane of the forward owns over four k-steps.
// Key, keep rule and scale: dropout_common.h.  sgan.kernels
// .pool_dropout_keep_host restates it in numpy.
#pragma once
#include "sgg_common.h"
#include "dropout_common.h"

namespace sgg {

struct PoolDropKey {
  uint32_t k0, k1, c3, thr;
  float scale;
};

__device__ __forceinline__ PoolDropKey pool_drop_key(const DropArgs& a) {
  // (the by-value words pass through readfirstlane -- they are uniform -- so that the compiler keeps them in
  // registers: it otherwise turns "by value or from rng" into one load through a selected pointer, with a.seed
  // copied to the stack for it)
  uint32_t k0 = __builtin_amdgcn_readfirstlane((uint32_t)a.seed);
  uint32_t k1 = __builtin_amdgcn_readfirstlane((uint32_t)(a.seed >> 32));
  uint32_t c3 = __builtin_amdgcn_readfirstlane(a.offset);
  if (a.rng) {
    const unsigned long long seed = a.rng[0];
    k0 = (uint32_t)seed;
    k1 = (uint32_t)(seed >> 32);
    c3 = (uint32_t)a.rng[1];
  }
  return PoolDropKey{k0, k1, c3, a.thr, a.scale};
}

// the words of (i, j) at columns col, col + 4, col + 8, col + 12 (col & 12 == 0)
__device__ __forceinline__ Philox4 pool_drop_words(const PoolDropKey& k, uint32_t site, uint32_t i, uint32_t j,
                                                   uint32_t col) {
  return philox4x32_10(i, (j << 8) | ((col >> 4) << 2) | (col & 3), site << 8, k.c3, k.k0, k.k1);
}

// scale where the word keeps, else 0
__device__ __forceinline__ float pool_drop_mul(const PoolDropKey& k, uint32_t word) {
  return word >= k.thr ? k.scale : 0.f;
}

// one element: kept?
__device__ __forceinline__ bool pool_drop_keep(const PoolDropKey& k, uint32_t site, uint32_t i, uint32_t j,
                                               uint32_t col) {
  const Philox4 x = pool_drop_words(k, site, i, j, col);
  const uint32_t r = (col >> 2) & 3;
  return (r == 0 ? x.w[0] : r == 1 ? x.w[1] : r == 2 ? x.w[2] : x.w[3]) >= k.thr;
}

// one element's factor
__device__ __forceinline__ float pool_drop_factor(const PoolDropKey& k, uint32_t site, uint32_t i, uint32_t j,
                                                  uint32_t col) {
  return pool_drop_keep(k, site, i, j, col) ? k.scale : 0.f;
}

// a 64-bit value that is the same in every lane, held in SGPRs
__device__ __forceinline__ unsigned long long wave_uniform(unsigned long long v) {
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)v);
  return ((unsigned long long)hi << 32) | (unsigned long long)lo;
}

// The hidden mask's keep bits of hidden unit `col` against the peds i0 + b, b the set bits of `need` (a
// wave-uniform set): what the backward kernels form once per (j, i tile) before walking the selected pairs.
__device__ __forceinline__ unsigned long long pool_drop_keep_bits(const PoolDropKey& k, unsigned long long need,
                                                                  uint32_t i0, uint32_t j, uint32_t col) {
  unsigned long long kp = 0ull;
  while (need) {
    const int b = __builtin_ctzll(need);
    need &= need - 1;
    kp |= (unsigned long long)pool_drop_keep(k, SGG_POOL_DROP_SITE_HIDDEN, i0 + (uint32_t)b, j, col) << b;
  }
  return kp;
}

// the entry points' dropout arguments -> DropArgs (thr / scale computed once, here)
static inline bool pool_drop_args(const char* who, float p, unsigned long long seed, unsigned offset,
                                  const unsigned long long* rng_dev, DropArgs* out) {
  if (!(p >= 0.f && p < 1.f)) {
    set_error("%s: dropout p=%g outside [0, 1)", who, (double)p);
    return false;
  }
  *out = DropArgs{seed, rng_dev, offset, SGG_POOL_DROP_SITE_HIDDEN, 0, drop_threshold(p), drop_scale(p)};
  return true;
}

}  // namespace sgg
