// The tile compositor that typeset_kernel (kernels_typeset.hip), glyphs_kernel (kernels_glyphs.hip) and tilted_kernel
// (kernels_tilted.hip) share: a workgroup of TS_THREADS threads owns a TW x TH tile of one page, holds it in registers (PX
// packed pixels a thread: column t % TW, rows t / TW + LYS j) and applies coverage patches to it one after another.  The
// kernels differ in how a layer's coverage F gets into the LDS patch `cov` (patch (0, 0) is tile (-r, -r)) -- a bitmap's bytes,
// glyphs gathered from an atlas, glyphs gathered in a layer's frame and resampled; what the two glyph kernels share of that is
// glyph_walk.h's -- and from there on the rule is here, once: the outline S is the
// grey-scale dilation of F by a disk of radius r <= RMAX, taken as running horizontal maxima kept for the disk's distinct
// half-widths (at most TS_PLANES planes: 9 at r = 12) and 2 r + 1 reads down a column, and a pixel becomes
// blend(blend(P, stroke, S), fill, F).  Integers only.  Device code only.
//
// No helper holds a barrier: what each one reads and writes of LDS is stated with it, and every __syncthreads() stands in
// the kernel bodies.  The helpers take plain values and pointers, not the layer structs, which differ between the kernels.
#pragma once
#include "kernels.h"

namespace {

constexpr int TW = CTD_TYPESET_TILE_W, TH = CTD_TYPESET_TILE_H, RMAX = CTD_TYPESET_MAX_RADIUS;
constexpr int TS_THREADS = 256;
constexpr int PX = TW * TH / TS_THREADS;                   // pixels a thread
constexpr int LYS = TS_THREADS / TW;                       // rows between two pixels of a thread
constexpr int CW = TW + 2 * RMAX, CH = TH + 2 * RMAX;      // the coverage patch
static_assert(TW == 64 && TS_THREADS % TW == 0 && (TW * TH) % TS_THREADS == 0 && TH % (TS_THREADS / TW) == 0,
              "a wave is one tile row; every thread has PX pixels");

constexpr int half_width(int r, int dy) {
  int k = 0;
  while ((k + 1) * (k + 1) + dy * dy <= r * r) ++k;
  return k;
}
constexpr int distinct_half_widths(int r) {
  int n = 0;
  for (int dy = 0; dy <= r; ++dy) n += dy == 0 || half_width(r, dy) != half_width(r, dy - 1);
  return n;
}
constexpr int max_planes() {
  int n = 0;
  for (int r = 1; r <= RMAX; ++r) n = distinct_half_widths(r) > n ? distinct_half_widths(r) : n;
  return n;
}
constexpr int TS_PLANES = max_planes();

__device__ __forceinline__ int blend(int c, int k, int a) { return (c * (255 - a) + k * a + 127) / 255; }

// The tile of this workgroup (block-uniform): its row T of the tile table, its page P, its origin and its entries
// [e_begin, e_end).  false: a tile that is no tile of its page, or one without entries, does nothing.  The origin is set
// on every path: what the checks establish about it (not negative, a multiple of the tile) then reaches the address
// arithmetic of load_tile and store_tile; left unset on the early returns it does not, at a cost of registers.
__device__ __forceinline__ bool open_tile(const ctd_typeset_tile* tiles, const ctd_typeset_page* pages, int n_pages,
                                          int n_entries, ctd_typeset_tile& T, ctd_typeset_page& P, int& tx0, int& ty0,
                                          int& e_begin, int& e_end) {
  T = tiles[blockIdx.x];
  tx0 = ty0 = 0;
  if (T.page < 0 || T.page >= n_pages || T.tx < 0 || T.ty < 0) return false;
  P = pages[T.page];
  if (P.H < 1 || P.W < 1 || P.H > CTD_TYPESET_MAX_SIDE || P.W > CTD_TYPESET_MAX_SIDE) return false;
  if ((long long)T.tx * TW >= P.W || (long long)T.ty * TH >= P.H) return false;
  tx0 = T.tx * TW, ty0 = T.ty * TH;
  e_begin = min(max(T.first, 0), n_entries), e_end = min(max(tiles[blockIdx.x + 1].first, 0), n_entries);
  return e_begin < e_end;
}

// Thread t's pixels of the tile at (tx0, ty0) into pix[], one packed pixel a register, by byte loads: pages have 3-byte
// pixels at any pitch and alignment.  Beyond the page: 0.
__device__ __forceinline__ void load_tile(const ctd_typeset_page& P, int tx0, int ty0, int t, unsigned (&pix)[PX]) {
  const unsigned char* base = (const unsigned char*)P.page_dev;
  const int gx = tx0 + t % TW;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const int gy = ty0 + t / TW + j * LYS;
    pix[j] = 0;
    if (gx < P.W && gy < P.H) {
      const unsigned char* q = base + (long long)gy * P.pitch + 3 * gx;
      pix[j] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
    }
  }
}

// ... and back, once: the pixels some layer wrote (bit 24).
__device__ __forceinline__ void store_tile(const ctd_typeset_page& P, int tx0, int ty0, int t, const unsigned (&pix)[PX]) {
  unsigned char* base = (unsigned char*)P.page_dev;
  const int gx = tx0 + t % TW;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    if (pix[j] >> 24) {
      unsigned char* q = base + (long long)(ty0 + t / TW + j * LYS) * P.pitch + 3 * gx;
      q[0] = (unsigned char)pix[j], q[1] = (unsigned char)(pix[j] >> 8), q[2] = (unsigned char)(pix[j] >> 16);
    }
  }
}

// The planes of radius r >= 1, by ONE thread: slot[k], the plane of half-width k, -1 where no row of the disk has it, and
// slot_dy[|dy|], the plane of that row's half-width floor(sqrt(r^2 - dy^2)).  Writes LDS that rows_pass and blend_count read:
// the caller puts a barrier between.
__device__ __forceinline__ void slot_table(int r, signed char* slot, signed char* slot_dy) {
  for (int k = 0; k <= r; ++k) slot[k] = -1;
  int n = 0;
  for (int dy = 0; dy <= r; ++dy) {
    int k = 0;
    while ((k + 1) * (k + 1) + dy * dy <= r * r) ++k;
    if (slot[k] < 0) slot[k] = (signed char)n++;          // half-widths fall as dy grows: n <= TS_PLANES
    slot_dy[dy] = slot[k];
  }
}

// For the patch rows [row1, row2) and every tile column, the running horizontal max m_k = max F(x - k .. x + k), k = 0 .. r,
// two byte reads a step; m_k is stored to plane slot[k] where k is a half-width of the disk.  All threads, r >= 1.  Reads
// cov and slot, writes plane.
__device__ __forceinline__ void rows_pass(const unsigned char (*cov)[CW], unsigned char (*plane)[CH][TW],
                                          const signed char* slot, int r, int row1, int row2, int t) {
  for (int i = t; i < (row2 - row1) * TW; i += TS_THREADS) {
    const int py = row1 + i / TW, x = i % TW;
    const unsigned char* __restrict__ row = &cov[py][x + r];
    int m = row[0];
    if (slot[0] >= 0) plane[slot[0]][py][x] = (unsigned char)m;
    for (int k = 1; k <= r; ++k) {
      m = max(m, max((int)row[-k], (int)row[k]));
      const int s = slot[k];
      if (s >= 0) plane[s][py][x] = (unsigned char)m;
    }
  }
}

// The layer onto this thread's pixels of the active rectangle [ax1, ax2) x [ay1, ay2) (page coordinates, within the tile):
// F from cov, S(p) = max over dy of plane[slot_dy[|dy|]](px, py + dy), 2 r + 1 byte reads (r = 0: S = 0, no plane is read),
// blend(blend(P, stroke, S), fill, F) in the register; the pixels written with F > 0 and with S > 0 go wave-reduced to the
// layer's row rows[li] by atomicAdd (the table and the index, not the row's address: that is formed only in the lanes
// that add).  All threads of the workgroup.  Reads cov, plane and slot_dy.
__device__ __forceinline__ void blend_count(int r, int ax1, int ay1, int ax2, int ay2, const unsigned char (&fill)[3],
                                            const unsigned char (&stroke)[3], const unsigned char (*cov)[CW],
                                            const unsigned char (*plane)[CH][TW], const signed char* slot_dy, int tx0, int ty0,
                                            int t, unsigned (&pix)[PX], ctd_typeset_row* rows, int li) {
  const int lx = t % TW, ly = t / TW, gx = tx0 + lx;
  const int f0 = fill[0], f1 = fill[1], f2 = fill[2], s0 = stroke[0], s1 = stroke[1], s2 = stroke[2];
  int n_fill = 0, n_stroke = 0;
  if (gx >= ax1 && gx < ax2) {
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const int yy = ly + j * LYS, gy = ty0 + yy;
      if (gy < ay1 || gy >= ay2) continue;
      const int F = cov[yy + r][lx + r];
      int S = 0;
      if (r > 0) {
        S = plane[slot_dy[0]][yy + r][lx];
        for (int dy = 1; dy <= r; ++dy) {
          const int s = slot_dy[dy];
          S = max(S, max((int)plane[s][yy + r - dy][lx], (int)plane[s][yy + r + dy][lx]));
        }
      }
      const unsigned c = pix[j];
      const int c0 = blend(blend(c & 255, s0, S), f0, F);
      const int c1 = blend(blend((c >> 8) & 255, s1, S), f1, F);
      const int c2 = blend(blend((c >> 16) & 255, s2, S), f2, F);
      pix[j] = (unsigned)c0 | ((unsigned)c1 << 8) | ((unsigned)c2 << 16) | 0x1000000u;   // bit 24: written
      n_fill += F > 0, n_stroke += S > 0;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n_fill += __shfl_down(n_fill, d, 64);
    n_stroke += __shfl_down(n_stroke, d, 64);
  }
  if ((t & 63) == 0) {
    if (n_fill) atomicAdd(&rows[li].n_fill, n_fill);
    if (n_stroke) atomicAdd(&rows[li].n_stroke, n_stroke);
  }
}

}  // namespace
