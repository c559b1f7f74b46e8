// What the kernels on a balloon window's bit planes share (kernels_layout.hip, kernels_fit.hip): the planes' layout in
// dynamic LDS, the load of B_b, its erosion to E_b by shifted ANDs, and the run of ones of a row that contains a column.
// Layout: nw = ceil(ww / 64) 64-bit words a row, bit x of a row is bit x & 63 of word x >> 6; plane A at words 0 ..
// max_words - 1 of the dynamic LDS, plane Q behind it.
#pragma once

#include "kernels.h"

namespace lybits {

typedef unsigned long long u64;

constexpr int LY_THREADS = 512, LY_WAVES = LY_THREADS / 64;
static_assert(CTD_LAYOUT_MAX_INSET < 64, "an erosion shift stays inside the neighbouring word");

// the middle word of three eroded by m pixels either way (m < 64): bit x stays iff bits x - m .. x + m are all set
__device__ __forceinline__ u64 hero3(u64 l, u64 mid, u64 r, int m) {
  u64 v = mid;
  for (int s = 1; s <= m; ++s) v &= ((mid << s) | (l >> (64 - s))) & ((mid >> s) | (r << (64 - s)));
  return v;
}

// B_b from `src` into plane A (the last word of a row masked to the window), eroded by m: rows A -> Q (shifts cross the word
// boundaries of a row, zeros come in at the window's sides), columns Q -> A = E_b (rows beyond the window count as zero).
// Every thread of the block calls it; behind it A holds E_b, Q is free, and the sum of the returns over the block is |E_b|.
__device__ __forceinline__ int load_eroded(u64* __restrict__ A, u64* __restrict__ Q, const u64* __restrict__ src, int ww, int wh,
                                           int nw, int m, int t) {
  const int words = nw * wh;
  const u64 last_valid = (ww & 63) ? ((1ull << (ww & 63)) - 1ull) : ~0ull;   // the window's bits of a row's last word
  for (int i = t; i < words; i += LY_THREADS) {
    const int j = i % nw;
    A[i] = j == nw - 1 ? src[i] & last_valid : src[i];
  }
  __syncthreads();
  for (int i = t; i < words; i += LY_THREADS) {
    const int j = i % nw;
    Q[i] = hero3(j > 0 ? A[i - 1] : 0ull, A[i], j + 1 < nw ? A[i + 1] : 0ull, m);
  }
  __syncthreads();
  int n_inner = 0;
  for (int i = t; i < words; i += LY_THREADS) {
    const int y = i / nw;
    u64 v = 0ull;
    if (y >= m && y + m < wh) {
      v = Q[i];
      for (int d = 1; d <= m; ++d) v &= Q[i - d * nw] & Q[i + d * nw];
    }
    A[i] = v;
    n_inner += __popcll(v);
  }
  __syncthreads();
  return n_inner;
}

// the run of ones of a row that contains column c (0 <= c < 64 nw): [x1, x2), or false where the bit is not set
__device__ __forceinline__ bool run_at(const u64* __restrict__ p, int nw, int c, int& x1, int& x2) {
  const int jc = c >> 6, b = c & 63;
  const u64 w = p[jc];
  if (!((w >> b) & 1ull)) return false;
  const u64 lo = ~w & ((1ull << b) - 1ull), hi = ~w & ~((2ull << b) - 1ull);
  int l = 64 * jc, r = 64 * jc + 64;
  if (lo) {
    l += 64 - __builtin_clzll(lo);
  } else {
    for (int j = jc - 1; j >= 0; --j) {
      const u64 v = p[j];
      if (v != ~0ull) {
        l -= __builtin_clzll(~v);
        break;
      }
      l -= 64;
    }
  }
  if (hi) {
    r = 64 * jc + __builtin_ctzll(hi);
  } else {
    for (int j = jc + 1; j < nw; ++j) {
      const u64 v = p[j];
      if (v != ~0ull) {
        r += __builtin_ctzll(~v);
        break;
      }
      r += 64;
    }
  }
  x1 = l, x2 = r;
  return true;
}

}  // namespace lybits
