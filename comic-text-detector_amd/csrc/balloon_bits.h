// What the kernels that MAKE a balloon window's bit plane share (kernels_balloon.hip, kernels_footprint.hip): the window of a
// block, the seed F_b = D_g(M & X_b) by one __ballot per 64 mask bytes and two word-shift dilations, the word-wise dilation
// itself, and the reduction of a finished plane to its ctd_balloon_row.  Layout as in layout_bits.h: nw = ceil(ww / 64) 64-bit
// words a row, bit x of a row is bit x & 63 of word x >> 6; two planes of prm.max_words words in the dynamic LDS.
#pragma once

#include "kernels.h"

namespace blbits {

typedef unsigned long long u64;

constexpr int BL_THREADS = 512, BL_WAVES = BL_THREADS / 64;
constexpr int BL_MAX_DEVICES = 64;
static_assert(CTD_BALLOON_MIN_REACH_MIN >= CTD_ERASE_MAX_GROW, "F_b lies inside the window");

// the middle word of three dilated by k pixels either way (k < 64)
__device__ __forceinline__ u64 hdil3(u64 l, u64 m, u64 r, int k) {
  u64 v = m;
  for (int s = 1; s <= k; ++s) v |= (m << s) | (l >> (64 - s)) | (m >> s) | (r << (64 - s));
  return v;
}

// the sum of the indices of the set bits of a word
__device__ __forceinline__ int bit_index_sum(u64 w) {
  return __popcll(w & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(w & 0xCCCCCCCCCCCCCCCCull) + 4 * __popcll(w & 0xF0F0F0F0F0F0F0F0ull) +
         8 * __popcll(w & 0xFF00FF00FF00FF00ull) + 16 * __popcll(w & 0xFFFF0000FFFF0000ull) + 32 * __popcll(w & 0xFFFFFFFF00000000ull);
}

// Win_b and the clipped box X_b, from the box and the page's size alone (all 0 where X_b is empty)
struct window {
  int wx1, wy1, ww, wh, bx1, by1, bx2, by2;
};

__device__ __forceinline__ window window_of(const int32_t* xyxy, int W, int H, int reach, int reach_min) {
  window w = {0, 0, 0, 0, 0, 0, 0, 0};
  w.bx1 = max(xyxy[0], 0), w.by1 = max(xyxy[1], 0), w.bx2 = min(xyxy[2], W), w.by2 = min(xyxy[3], H);
  if (w.bx1 < w.bx2 && w.by1 < w.by2) {
    const long long ex = max((long long)reach_min, ((long long)(w.bx2 - w.bx1) * reach) >> 3);
    const long long ey = max((long long)reach_min, ((long long)(w.by2 - w.by1) * reach) >> 3);
    w.wx1 = (int)max((long long)w.bx1 - ex, 0ll), w.wy1 = (int)max((long long)w.by1 - ey, 0ll);
    w.ww = (int)min((long long)w.bx2 + ex, (long long)W) - w.wx1, w.wh = (int)min((long long)w.by2 + ey, (long long)H) - w.wy1;
  }
  return w;
}

// the window's bits of a row's last word
__device__ __forceinline__ u64 last_valid_of(int ww) { return (ww & 63) ? ((1ull << (ww & 63)) - 1ull) : ~0ull; }

// src dilated by k (< 64) into src again, through tmp: rows src -> tmp (shifts cross the word boundaries of a row, the last
// word of a row masked to the window), columns tmp -> src (rows beyond the window are empty).  Every thread of the block
// calls it with src complete; behind it src is complete again, and the sum of the returns over the block is its popcount.
__device__ __forceinline__ int dilate_plane(u64* __restrict__ src, u64* __restrict__ tmp, int nw, int wh, int words, int k,
                                            u64 last_valid, int t) {
  for (int i = t; i < words; i += BL_THREADS) {
    const int y = i / nw, j = i - y * nw;
    u64 v = hdil3(j > 0 ? src[i - 1] : 0ull, src[i], j + 1 < nw ? src[i + 1] : 0ull, k);
    if (j == nw - 1) v &= last_valid;
    tmp[i] = v;
  }
  __syncthreads();
  int n = 0;
  for (int i = t; i < words; i += BL_THREADS) {
    const int y = i / nw;
    u64 v = 0ull;
    for (int yy = max(y - k, 0); yy <= min(y + k, wh - 1); ++yy) v |= tmp[i + (yy - y) * nw];
    src[i] = v;
    n += __popcll(v);
  }
  __syncthreads();
  return n;
}

// F_b into R (O is scratch): T_b = M & X_b by one __ballot per 64 mask bytes, then D_g of it.  X_b lies g or more inside the
// window except at a page edge, where D_g is clipped anyway: no halo.  The sum of the returns over the block is |F_b|.
__device__ __forceinline__ int load_seed(u64* __restrict__ O, u64* __restrict__ R, const ctd_erase_page& P, const window& w, int nw,
                                         int words, int g, int t) {
  const int lane = t & 63, wave = t >> 6;
  for (int task = wave; task < words; task += BL_WAVES) {
    const int y = task / nw, j = task - y * nw;
    const int px = w.wx1 + 64 * j + lane, py = w.wy1 + y;
    bool bit = false;
    if (py >= w.by1 && py < w.by2 && px >= w.bx1 && px < w.bx2) bit = P.mask_dev[(long long)py * P.mask_pitch + px] != 0;
    const u64 word = __ballot(bit);
    if (lane == 0) R[task] = word;
  }
  __syncthreads();
  return dilate_plane(R, O, nw, w.wh, words, g, last_valid_of(w.ww), t);
}

// what a thread gathers over the words of the finished plane it stores
struct tally {
  int area, minx, miny, maxx, maxy, flags;
  long long sx, sy;
};

__device__ __forceinline__ tally tally_none() { return {0, 0x7fffffff, 0x7fffffff, -1, -1, 0, 0ll, 0ll}; }

// word i of the plane: popcount, box, coordinate sums, contact with the window's sides
__device__ __forceinline__ void tally_word(tally& a, u64 rw, int i, int nw, const window& w) {
  if (!rw) return;
  const int y = i / nw, j = i - y * nw;
  const int n = __popcll(rw), x0 = w.wx1 + 64 * j;
  a.area += n;
  a.minx = min(a.minx, x0 + __ffsll((long long)rw) - 1), a.maxx = max(a.maxx, x0 + 63 - __clzll((long long)rw));
  a.miny = min(a.miny, w.wy1 + y), a.maxy = max(a.maxy, w.wy1 + y);
  a.sx += (long long)n * x0 + bit_index_sum(rw), a.sy += (long long)n * (w.wy1 + y);
  if (j == 0 && (rw & 1ull)) a.flags |= CTD_BALLOON_CUT_LEFT;
  if (y == 0) a.flags |= CTD_BALLOON_CUT_TOP;
  if (j == nw - 1 && ((rw >> ((w.ww - 1) & 63)) & 1ull)) a.flags |= CTD_BALLOON_CUT_RIGHT;
  if (y == w.wh - 1) a.flags |= CTD_BALLOON_CUT_BOTTOM;
}

// the threads' tallies and seed counts to one OK row: wave shuffles, one LDS step across the waves (red_i: [BL_WAVES][8],
// red_l: [BL_WAVES][2], static LDS of the caller), thread 0 writes the row with ordinary stores.  A side that is the page's
// edge reports in bits 4 .. 7; `more_flags` is ORed in as it stands.  Every thread of the block calls it.
__device__ __forceinline__ void write_row(tally a, int n_seed, int (*red_i)[8], long long (*red_l)[2], ctd_balloon_row* __restrict__ row,
                                          const window& w, int W, int H, int more_flags, int t) {
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    a.area += __shfl_down(a.area, d, 64), n_seed += __shfl_down(n_seed, d, 64);
    a.minx = min(a.minx, __shfl_down(a.minx, d, 64)), a.miny = min(a.miny, __shfl_down(a.miny, d, 64));
    a.maxx = max(a.maxx, __shfl_down(a.maxx, d, 64)), a.maxy = max(a.maxy, __shfl_down(a.maxy, d, 64));
    a.flags |= __shfl_down(a.flags, d, 64);
    a.sx += __shfl_down(a.sx, d, 64), a.sy += __shfl_down(a.sy, d, 64);
  }
  if (lane == 0) {
    red_i[wave][0] = a.area, red_i[wave][1] = n_seed, red_i[wave][2] = a.minx, red_i[wave][3] = a.miny, red_i[wave][4] = a.maxx,
    red_i[wave][5] = a.maxy, red_i[wave][6] = a.flags;
    red_l[wave][0] = a.sx, red_l[wave][1] = a.sy;
  }
  __syncthreads();
  if (t == 0) {
    for (int v = 1; v < BL_WAVES; ++v) {
      a.area += red_i[v][0], n_seed += red_i[v][1];
      a.minx = min(a.minx, red_i[v][2]), a.miny = min(a.miny, red_i[v][3]), a.maxx = max(a.maxx, red_i[v][4]),
      a.maxy = max(a.maxy, red_i[v][5]);
      a.flags |= red_i[v][6];
      a.sx += red_l[v][0], a.sy += red_l[v][1];
    }
    int f = more_flags;
    f |= (a.flags & CTD_BALLOON_CUT_LEFT) << (w.wx1 == 0 ? 4 : 0);
    f |= (a.flags & CTD_BALLOON_CUT_TOP) << (w.wy1 == 0 ? 4 : 0);
    f |= (a.flags & CTD_BALLOON_CUT_RIGHT) << (w.wx1 + w.ww == W ? 4 : 0);
    f |= (a.flags & CTD_BALLOON_CUT_BOTTOM) << (w.wy1 + w.wh == H ? 4 : 0);
    row->status = CTD_BALLOON_OK, row->area = a.area;
    row->bbox[0] = a.area ? a.minx : 0, row->bbox[1] = a.area ? a.miny : 0, row->bbox[2] = a.area ? a.maxx + 1 : 0,
    row->bbox[3] = a.area ? a.maxy + 1 : 0;
    row->flags = f, row->n_seed = n_seed, row->sum_x = a.sx, row->sum_y = a.sy;
  }
}

}  // namespace blbits
