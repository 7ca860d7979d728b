// The dropout mask of every kernel (include/sgg.h, "Dropout masks"): a
// stateless function of (seed, offset, site, head, row, column), so a backward
// regenerates the mask its forward used and nothing is stored.
//   Philox4x32-10, key (seed & 0xffffffff, seed >> 32),
//   counter (row >> 2, col, (site << 8) | head, offset), output word row & 3;
//   keep iff word >= thr, thr = (uint32_t)((double)p * 2^32); a kept value is
//   multiplied by scale = 1 / (1 - p), a dropped one is exactly 0.
// Nothing here depends on a tile shape, an LDS layout or a grid: sgan.kernels
// .dropout_keep_host restates it in numpy.
#pragma once
#include <stdint.h>

namespace sgg {

// by-value arguments of a dropout launch; rng != NULL: {seed, offset} are read
// from those two device words instead (the low 32 bits of the second)
struct DropArgs {
  unsigned long long seed;
  const unsigned long long* rng;
  uint32_t offset, site, head0, thr;
  float scale;
};

// what a kernel keeps per (site, head): key, the two fixed counter words
struct DropKey {
  uint32_t k0, k1, c2, c3, thr;
  float scale;
};

// thr / scale of a probability p in [0, 1) (the entry points check the range)
inline uint32_t drop_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }
inline float drop_scale(float p) { return 1.0f / (1.0f - p); }

__device__ __forceinline__ DropKey drop_key(const DropArgs& a, uint32_t head) {
  unsigned long long seed = a.seed;
  uint32_t offset = a.offset;
  if (a.rng) {
    seed = a.rng[0];
    offset = (uint32_t)a.rng[1];
  }
  return DropKey{(uint32_t)seed, (uint32_t)(seed >> 32), (a.site << 8) | (a.head0 + head), offset, a.thr, a.scale};
}

struct Philox4 {
  uint32_t w[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the four words of rows 4 rq .. 4 rq + 3 at column col
__device__ __forceinline__ Philox4 drop_words(const DropKey& k, uint32_t rq, uint32_t col) {
  return philox4x32_10(rq, col, k.c2, k.c3, k.k0, k.k1);
}

// one element's word
__device__ __forceinline__ uint32_t drop_word(const DropKey& k, uint32_t row, uint32_t col) {
  const Philox4 x = drop_words(k, row >> 2, col);
  const uint32_t r = row & 3;
  return r == 0 ? x.w[0] : r == 1 ? x.w[1] : r == 2 ? x.w[2] : x.w[3];
}

}  // namespace sgg
