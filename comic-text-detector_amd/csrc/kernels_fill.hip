// Smooth pull-push fill of a hole mask (`ctd_fill_rest`; the rule is stated in include/ctd_hip.h and restated in numpy in
// tests/fill_ref.py): pull builds a pyramid of the known pixels, push fills the hole from coarse to fine by bilinear
// upsampling.  Integers only: sums, one division by 2 n, shifts.  A level pixel is one dword, c[0] | c[1] << 8 | c[2] << 16 |
// k << 24, and 0 where k = 0.
//
// Three launches, no host step between them, whatever the pages.
//
// fill_pull_kernel, one workgroup per 64 x 64 tile of all pages: the children of a level pixel never cross an aligned tile,
// so the tile's pixels of levels 1 .. 6 (32 x 32 .. 1 x 1) are pulled in LDS and written to scratch; the tile's hole count
// goes to the per-tile table (a sum in registers and LDS, no atomics).  A level pixel beyond its level's edge has no child
// and so comes out 0 by itself.
//
// fill_page_kernel, one workgroup per page: the level-6 plane (at most 128 x 128 dwords) into dynamic LDS, levels 7 .. T
// pulled behind it, then pushed back down to level 6; the finished level-6 pixels that were unknown are written back.  The
// tile counts are summed and thread 0 writes the row.  Where T < 6 the levels T + 1 .. 6 are 1 x 1 copies of the top
// ((2 c + 1) / 2 = c upwards, (16 c + 8) >> 4 = c downwards): nothing is special about a small page.
//
// fill_push_kernel, one workgroup per tile: a tile without a hole, or of a page whose row is not OK, is a copy.  Otherwise a
// tile needs, of every coarser level, its own pixels and a halo of exactly ONE pixel (3 x 3 of level 6, 4 x 4 of level 5,
// .. 34 x 34 of level 1: 1641 dwords), loaded at coordinates clamped to the level -- which is the rule's clamp of ny and
// nx -- and pushed down in LDS, the halo pixels included; then the tile's hole pixels from level 1.  Every byte of the
// tile's `out` is written exactly once, moved as in the erase paint launch: a wave owns a row, a lane one ALIGNED dword of
// the output row segment, read from the page as one or two aligned dwords and a funnel shift.
#include <mutex>

#include "kernels.h"

namespace {

constexpr int FL_TILE = CTD_FILL_TILE;
constexpr int FL_THREADS = 256, FL_WAVES = FL_THREADS / 64;
constexpr int FL_TOP = 6;                                         // the level at which a tile is one pixel
constexpr int FL_MAX_PLANE = (CTD_FILL_MAX_SIDE >> FL_TOP) * (CTD_FILL_MAX_SIDE >> FL_TOP);   // level 6 of the largest page
// levels 7 .. 13 of the largest page: 64 x 64 + 32 x 32 + .. + 1
constexpr int FL_MAX_UPPER = 4096 + 1024 + 256 + 64 + 16 + 4 + 1;
constexpr int FL_PAGE_LDS = (FL_MAX_PLANE + FL_MAX_UPPER) * 4;
constexpr int FL_MAX_DEVICES = 64;
constexpr int FL_RPW = FL_TILE / FL_WAVES;                        // tile rows a wave owns in the push launch
constexpr int FL_CHUNK = 8;                                       // of which so many are in flight at a time
static_assert(FL_TILE == 64 && (1 << FL_TOP) == FL_TILE, "a tile row is a wave; level 6 of a tile is one pixel");
static_assert(CTD_FILL_MAX_SIDE % FL_TILE == 0 && FL_MAX_PLANE == 128 * 128, "the level-6 plane fits 64 KB");
static_assert(3 * FL_TILE / 4 + 2 <= 64, "a lane per dword of a tile row of `out`");
static_assert(FL_RPW % FL_CHUNK == 0, "whole chunks");
static_assert(sizeof(ctd_fill_page) == 56 && sizeof(ctd_fill_params) == 32 && sizeof(ctd_fill_row) == 32,
              "fill ABI sizes (fill.py dtypes)");
static_assert(offsetof(ctd_fill_page, H) == 24 && offsetof(ctd_fill_page, tile0) == 44 && offsetof(ctd_fill_page, lvl0) == 48 &&
              offsetof(ctd_fill_row, top) == 12, "fill ABI offsets");

__device__ __forceinline__ int lvl_dim(int n, int l) { return (n + (1 << l) - 1) >> l; }

// the page's level l (1 .. 6) in scratch, relative to its lvl0
__device__ __forceinline__ long long lvl_off(int H, int W, int l) {
  long long off = 0;
  for (int j = 1; j < l; ++j) off += (long long)lvl_dim(H, j) * lvl_dim(W, j);
  return off;
}

// the first level that is 1 x 1
__device__ __forceinline__ int top_level(int H, int W) {
  int l = 0;
  while (lvl_dim(H, l) > 1 || lvl_dim(W, l) > 1) ++l;
  return l;
}

// the pull of up to four children (0 where a child is unknown or beyond the level)
__device__ __forceinline__ unsigned pull4(unsigned a, unsigned b, unsigned c, unsigned d) {
  const unsigned n = (a >> 24) + (b >> 24) + (c >> 24) + (d >> 24);
  if (!n) return 0u;
  const unsigned s02 = (a & 0xff00ffu) + (b & 0xff00ffu) + (c & 0xff00ffu) + (d & 0xff00ffu);   // <= 1020 a half
  const unsigned s1 = ((a >> 8) & 255u) + ((b >> 8) & 255u) + ((c >> 8) & 255u) + ((d >> 8) & 255u);
  const unsigned n2 = 2u * n;
  const unsigned r0 = (2u * (s02 & 0xffffu) + n) / n2, r1 = (2u * s1 + n) / n2, r2 = (2u * (s02 >> 16) + n) / n2;
  return r0 | r1 << 8 | r2 << 16 | 1u << 24;
}

// the push of one pixel: weights 9, 3, 3, 1 of four finished pixels
__device__ __forceinline__ unsigned push4(unsigned a, unsigned b, unsigned c, unsigned d) {
  const unsigned s02 = 9u * (a & 0xff00ffu) + 3u * ((b & 0xff00ffu) + (c & 0xff00ffu)) + (d & 0xff00ffu) + 0x00080008u;   // <= 4088 a half
  const unsigned s1 = 9u * ((a >> 8) & 255u) + 3u * (((b >> 8) & 255u) + ((c >> 8) & 255u)) + ((d >> 8) & 255u) + 8u;
  return ((s02 >> 4) & 255u) | ((s1 >> 4) & 255u) << 8 | ((s02 >> 20) & 255u) << 16 | 1u << 24;
}

// the page of a tile: the last one whose tile0 <= tile (uniform)
__device__ __forceinline__ int page_of_tile(const ctd_fill_page* __restrict__ pages, int n_pages, int tile) {
  int lo = 0, hi = n_pages - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pages[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- pull: levels 1 .. 6 of a tile ------------------------------------------------------------------------------------

// one level of the tile from the one below it in LDS: n x n pixels from 2n x 2n; written to scratch where inside the level
template <int N>
__device__ __forceinline__ void pull_level(const unsigned* __restrict__ src, unsigned* __restrict__ dst, unsigned* __restrict__ g,
                                           int gh, int gw, int gy0, int gx0) {
  for (int i = threadIdx.x; i < N * N; i += FL_THREADS) {
    const int y = i / N, x = i - y * N;
    const unsigned* s = src + (2 * y) * (2 * N) + 2 * x;
    const unsigned v = pull4(s[0], s[1], s[2 * N], s[2 * N + 1]);
    dst[i] = v;
    if (gy0 + y < gh && gx0 + x < gw) g[(long long)(gy0 + y) * gw + gx0 + x] = v;
  }
}

__global__ __launch_bounds__(FL_THREADS) void fill_pull_kernel(const ctd_fill_page* __restrict__ pages, int n_pages,
                                                               unsigned* __restrict__ scratch) {
  __shared__ unsigned L1[32 * 32], L2[16 * 16], L3[8 * 8], L4[4 * 4], L5[2 * 2], L6[1];
  __shared__ int red[FL_WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const ctd_fill_page P = pages[page_of_tile(pages, n_pages, (int)blockIdx.x)];
  const int tiles_x = (P.W + FL_TILE - 1) / FL_TILE, tiles_y = (P.H + FL_TILE - 1) / FL_TILE;
  const int local = (int)blockIdx.x - P.tile0;
  if (local < 0 || local >= tiles_x * tiles_y) return;
  const int tyi = local / tiles_x, txi = local - tyi * tiles_x;
  const int x0 = txi * FL_TILE, y0 = tyi * FL_TILE;
  unsigned* __restrict__ lv = scratch + P.lvl0;

  // level 1 from the page: a thread four level pixels, a wave two rows of them
  int holes = 0;
  {
    const int gh = lvl_dim(P.H, 1), gw = lvl_dim(P.W, 1);
    constexpr int NR = 32 * 32 / FL_THREADS;
    // every load of the thread's 16 page pixels first, whatever the mask says: nothing waits for a mask byte
    unsigned px[NR][4], hb[NR][4];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = t + r * FL_THREADS, ly = i >> 5, lx = i & 31;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int y = y0 + 2 * ly + (q >> 1), x = x0 + 2 * lx + (q & 1);
        px[r][q] = 0u, hb[r][q] = 2u;                      // 2: beyond the page
        if (y < P.H && x < P.W) {
          const uint8_t* p = P.page_dev + (long long)y * P.pitch + 3ll * x;
          hb[r][q] = P.hole_dev[(long long)y * P.hole_pitch + x] != 0;
          px[r][q] = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | 1u << 24;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = t + r * FL_THREADS, ly = i >> 5, lx = i & 31;
      unsigned ch[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ch[q] = hb[r][q] == 0u ? px[r][q] : 0u;
        holes += hb[r][q] == 1u;
      }
      const unsigned v = pull4(ch[0], ch[1], ch[2], ch[3]);
      L1[i] = v;
      const int gy = 32 * tyi + ly, gx = 32 * txi + lx;
      if (gy < gh && gx < gw) lv[(long long)gy * gw + gx] = v;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) holes += __shfl_down(holes, d, 64);
  if (lane == 0) red[wave] = holes;
  __syncthreads();
  if (t == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < FL_WAVES; ++w) s += red[w];
    scratch[blockIdx.x] = (unsigned)s;
  }
  pull_level<16>(L1, L2, lv + lvl_off(P.H, P.W, 2), lvl_dim(P.H, 2), lvl_dim(P.W, 2), 16 * tyi, 16 * txi);
  __syncthreads();
  pull_level<8>(L2, L3, lv + lvl_off(P.H, P.W, 3), lvl_dim(P.H, 3), lvl_dim(P.W, 3), 8 * tyi, 8 * txi);
  __syncthreads();
  pull_level<4>(L3, L4, lv + lvl_off(P.H, P.W, 4), lvl_dim(P.H, 4), lvl_dim(P.W, 4), 4 * tyi, 4 * txi);
  __syncthreads();
  pull_level<2>(L4, L5, lv + lvl_off(P.H, P.W, 5), lvl_dim(P.H, 5), lvl_dim(P.W, 5), 2 * tyi, 2 * txi);
  __syncthreads();
  pull_level<1>(L5, L6, lv + lvl_off(P.H, P.W, 6), lvl_dim(P.H, 6), lvl_dim(P.W, 6), tyi, txi);
}

// ---- page: levels 7 .. T, the push down to level 6, the row ----------------------------------------------------------

// where level l (>= 6) of the page starts in the page launch's LDS
__device__ __forceinline__ int plane_off(int H, int W, int l) {
  int off = 0;
  for (int j = FL_TOP; j < l; ++j) off += lvl_dim(H, j) * lvl_dim(W, j);
  return off;
}

__global__ __launch_bounds__(FL_THREADS) void fill_page_kernel(const ctd_fill_page* __restrict__ pages,
                                                               unsigned* __restrict__ scratch, ctd_fill_row* __restrict__ rows) {
  extern __shared__ unsigned lds[];                        // level 6, then 7, .. up to the first that is 1 x 1
  __shared__ int red[FL_WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const ctd_fill_page P = pages[blockIdx.x];
  const int H = P.H, W = P.W;
  const int tiles = ((W + FL_TILE - 1) / FL_TILE) * ((H + FL_TILE - 1) / FL_TILE);
  const int T = top_level(H, W), top = max(T, FL_TOP);
  unsigned* __restrict__ g6 = scratch + P.lvl0 + lvl_off(H, W, FL_TOP);
  const int n6 = lvl_dim(H, FL_TOP) * lvl_dim(W, FL_TOP);   // = tiles

  int holes = 0;
  for (int i = t; i < tiles; i += FL_THREADS) holes += (int)scratch[P.tile0 + i];
  for (int i = t; i < n6; i += FL_THREADS) lds[i] = g6[i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) holes += __shfl_down(holes, d, 64);
  if (lane == 0) red[wave] = holes;
  __syncthreads();
  holes = 0;
#pragma unroll
  for (int w = 0; w < FL_WAVES; ++w) holes += red[w];

  // pull 7 .. top
  for (int l = FL_TOP; l < top; ++l) {
    const int h = lvl_dim(H, l), w = lvl_dim(W, l), h2 = lvl_dim(H, l + 1), w2 = lvl_dim(W, l + 1);
    const unsigned* __restrict__ src = lds + plane_off(H, W, l);
    unsigned* __restrict__ dst = lds + plane_off(H, W, l + 1);
    for (int i = t; i < h2 * w2; i += FL_THREADS) {
      const int y = i / w2, x = i - y * w2;
      const bool by = 2 * y + 1 < h, bx = 2 * x + 1 < w;
      const unsigned* s = src + (2 * y) * w + 2 * x;
      dst[i] = pull4(s[0], bx ? s[1] : 0u, by ? s[w] : 0u, (bx && by) ? s[w + 1] : 0u);
    }
    __syncthreads();
  }
  const unsigned topv = lds[plane_off(H, W, top)];
  const int status = holes == 0 ? CTD_FILL_NO_HOLE : (topv >> 24) ? CTD_FILL_OK : CTD_FILL_NO_KNOWN;
  if (t == 0) {
    ctd_fill_row* __restrict__ row = rows + blockIdx.x;
    row->status = status, row->n_hole = holes, row->levels = T;
#pragma unroll
    for (int c = 0; c < 3; ++c) row->top[c] = (uint8_t)(topv >> (8 * c));
#pragma unroll
    for (int c = 0; c < 17; ++c) row->pad_[c] = 0;
  }
  if (status != CTD_FILL_OK) return;                       // block-uniform

  // push top - 1 .. 6; the level-6 pixels that were unknown go back to scratch, finished
  for (int l = top - 1; l >= FL_TOP; --l) {
    const int h = lvl_dim(H, l), w = lvl_dim(W, l), h2 = lvl_dim(H, l + 1), w2 = lvl_dim(W, l + 1);
    unsigned* __restrict__ dst = lds + plane_off(H, W, l);
    const unsigned* __restrict__ src = lds + plane_off(H, W, l + 1);
    for (int i = t; i < h * w; i += FL_THREADS) {
      if (dst[i] >> 24) continue;
      const int y = i / w, x = i - y * w;
      const int py = y >> 1, px = x >> 1;
      const int ny = min(max(py + ((y & 1) ? 1 : -1), 0), h2 - 1), nx = min(max(px + ((x & 1) ? 1 : -1), 0), w2 - 1);
      const unsigned v = push4(src[py * w2 + px], src[py * w2 + nx], src[ny * w2 + px], src[ny * w2 + nx]);
      dst[i] = v;
      if (l == FL_TOP) g6[i] = v;
    }
    __syncthreads();
  }
}

// ---- push: levels 5 .. 0 of a tile ------------------------------------------------------------------------------------

// level l (1 .. 6) of a tile with its halo: side 2^(6 - l) + 2; the levels lie in LDS from 6 down to 1
__host__ __device__ constexpr int halo_side(int l) { return (1 << (FL_TOP - l)) + 2; }
__host__ __device__ constexpr int halo_off(int l) { return l >= FL_TOP ? 0 : halo_off(l + 1) + halo_side(l + 1) * halo_side(l + 1); }
constexpr int FL_HALO_DWORDS = halo_off(1) + halo_side(1) * halo_side(1);
static_assert(FL_HALO_DWORDS == 1641, "3^2 + 4^2 + 6^2 + 10^2 + 18^2 + 34^2");

__global__ __launch_bounds__(FL_THREADS) void fill_push_kernel(const ctd_fill_page* __restrict__ pages, int n_pages,
                                                               const unsigned* __restrict__ scratch,
                                                               const ctd_fill_row* __restrict__ rows) {
  __shared__ unsigned lv[FL_HALO_DWORDS];
  __shared__ unsigned win[FL_TILE][FL_TILE];               // c[0] | c[1] << 8 | c[2] << 16 | 1 << 24 on a hole pixel, else 0
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int pi = page_of_tile(pages, n_pages, (int)blockIdx.x);
  const ctd_fill_page P = pages[pi];
  const int tiles_x = (P.W + FL_TILE - 1) / FL_TILE, tiles_y = (P.H + FL_TILE - 1) / FL_TILE;
  const int local = (int)blockIdx.x - P.tile0;
  if (local < 0 || local >= tiles_x * tiles_y) return;
  const int tyi = local / tiles_x, txi = local - tyi * tiles_x;
  const int x0 = txi * FL_TILE, y0 = tyi * FL_TILE;
  const int tw = min(FL_TILE, P.W - x0), th = min(FL_TILE, P.H - y0);
  const bool fill = rows[pi].status == CTD_FILL_OK && scratch[blockIdx.x] != 0u;   // block-uniform

  if (fill) {
    // levels 1 .. 6 with their halo, at coordinates clamped to the level (level 6 is finished, 1 .. 5 as pulled)
    const unsigned* __restrict__ g = scratch + P.lvl0;
#pragma unroll
    for (int l = 1; l <= FL_TOP; ++l) {
      const int n = 1 << (FL_TOP - l), s = n + 2, h = lvl_dim(P.H, l), w = lvl_dim(P.W, l);
      for (int i = t; i < s * s; i += FL_THREADS) {
        const int sy = i / s, sx = i - sy * s;
        const int y = min(max(n * tyi - 1 + sy, 0), h - 1), x = min(max(n * txi - 1 + sx, 0), w - 1);
        lv[halo_off(l) + i] = g[(long long)y * w + x];
      }
      g += (long long)h * w;
    }
    __syncthreads();
    // push 5 .. 1: a slot is the level pixel at its clamped coordinate; its parents' slots hold finished pixels
#pragma unroll
    for (int l = FL_TOP - 1; l >= 1; --l) {
      const int n = 1 << (FL_TOP - l), s = n + 2, s2 = n / 2 + 2;
      const int h = lvl_dim(P.H, l), w = lvl_dim(P.W, l), h2 = lvl_dim(P.H, l + 1), w2 = lvl_dim(P.W, l + 1);
      const int oy = n * tyi - 1, ox = n * txi - 1, oy2 = (n / 2) * tyi - 1, ox2 = (n / 2) * txi - 1;
      unsigned* __restrict__ dst = lv + halo_off(l);
      const unsigned* __restrict__ src = lv + halo_off(l + 1);
      for (int i = t; i < s * s; i += FL_THREADS) {
        if (dst[i] >> 24) continue;
        const int sy = i / s, sx = i - sy * s;
        const int y = min(max(oy + sy, 0), h - 1), x = min(max(ox + sx, 0), w - 1);
        const int py = y >> 1, px = x >> 1;
        const int ny = min(max(py + ((y & 1) ? 1 : -1), 0), h2 - 1), nx = min(max(px + ((x & 1) ? 1 : -1), 0), w2 - 1);
        const int a = py - oy2, b = ny - oy2, c = px - ox2, d = nx - ox2;   // 0 .. s2 - 1
        dst[i] = push4(src[a * s2 + c], src[a * s2 + d], src[b * s2 + c], src[b * s2 + d]);
      }
      __syncthreads();
    }
    // level 0: the tile's hole pixels from level 1 (slot 0 is level-1 row 32 tyi - 1)
    {
      const int h1 = lvl_dim(P.H, 1), w1 = lvl_dim(P.W, 1);
      const int oy1 = 32 * tyi - 1, ox1 = 32 * txi - 1;
      const unsigned* __restrict__ src = lv + halo_off(1);
      constexpr int s1 = halo_side(1);
      bool hole[FL_RPW];
#pragma unroll
      for (int r = 0; r < FL_RPW; ++r) {
        const int j = wave * FL_RPW + r;
        hole[r] = j < th && lane < tw && P.hole_dev[(long long)(y0 + j) * P.hole_pitch + x0 + lane] != 0;
      }
#pragma unroll
      for (int r = 0; r < FL_RPW; ++r) {
        const int j = wave * FL_RPW + r, y = y0 + j, x = x0 + lane;
        unsigned v = 0u;
        if (hole[r]) {
          const int py = y >> 1, px = x >> 1;
          const int ny = min(max(py + ((y & 1) ? 1 : -1), 0), h1 - 1), nx = min(max(px + ((x & 1) ? 1 : -1), 0), w1 - 1);
          const int a = py - oy1, b = ny - oy1, c = px - ox1, d = nx - ox1;
          v = push4(src[a * s1 + c], src[a * s1 + d], src[b * s1 + c], src[b * s1 + d]);
        }
        win[j][lane] = v;
      }
    }
    __syncthreads();
  }

  // ---- every byte of the tile's `out`: a wave per row, a lane per aligned dword of the row's 3 * tw bytes; the loads of
  // a chunk of rows first (the inputs overlap no output, so they may fly together), then the stores
  const int nbytes = 3 * tw;
  for (int r0 = 0; r0 < FL_RPW; r0 += FL_CHUNK) {
    unsigned val[FL_CHUNK];
    int offs[FL_CHUNK], lens[FL_CHUNK];
#pragma unroll
    for (int r = 0; r < FL_CHUNK; ++r) {
      const int j = wave * FL_RPW + r0 + r, y = y0 + j;
      val[r] = 0, offs[r] = 0, lens[r] = 0;
      if (j >= th) continue;                                // wave-uniform
      const uint8_t* src = P.page_dev + (long long)y * P.pitch + 3ll * x0;
      const uintptr_t d = (uintptr_t)(P.out_dev + (long long)y * P.out_pitch + 3ll * x0);
      const int lead = (int)((4u - (unsigned)(d & 3u)) & 3u);   // bytes before the first aligned dword
      // unit 0: bytes 0 .. lead - 1; unit u >= 1: bytes lead + 4 (u - 1) .. + 3, the last one maybe short
      const int off = lane == 0 ? 0 : lead + 4 * (lane - 1);
      const int len = lane == 0 ? min(lead, nbytes) : max(min(4, nbytes - off), 0);
      offs[r] = off, lens[r] = len;
      unsigned v = 0;
      const uintptr_t s = (uintptr_t)(src + off);
      if (len == 4) {
        const unsigned sh = (unsigned)(s & 3u) * 8u;
        const unsigned* sa = (const unsigned*)(s & ~(uintptr_t)3);
        v = sa[0];
        if (sh) v = (v >> sh) | (sa[1] << (32u - sh));      // byte s + 3 lies in sa[1]: both dwords hold bytes of the row
      } else {
        for (int k = 0; k < len; ++k) v |= (unsigned)src[off + k] << (8 * k);
      }
      val[r] = v;
    }
#pragma unroll
    for (int r = 0; r < FL_CHUNK; ++r) {
      const int j = wave * FL_RPW + r0 + r, y = y0 + j;
      if (j >= th) continue;
      uint8_t* dst = P.out_dev + (long long)y * P.out_pitch + 3ll * x0;
      const int off = offs[r], len = lens[r];
      unsigned v = val[r];
      if (fill) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int o = off + k, px = o / 3, c = o - 3 * px;
          if (k < len) {
            const unsigned w = win[j][px];
            if (w >> 24) v = (v & ~(255u << (8 * k))) | ((w >> (8 * c)) & 255u) << (8 * k);
          }
        }
      }
      if (len == 4) {
        *(unsigned*)(dst + off) = v;
      } else {
        for (int k = 0; k < len; ++k) dst[off + k] = (uint8_t)(v >> (8 * k));
      }
    }
  }
}

std::once_flag g_lds_once[FL_MAX_DEVICES];
hipError_t g_lds_rc[FL_MAX_DEVICES];

}  // namespace

hipError_t launch_fill_rest(const ctd_fill_page* pages, int n_pages, int n_tiles, void* scratch, ctd_fill_row* rows,
                            hipStream_t st) {
  // the page launch asks for more dynamic LDS than the default limit: raised ONCE per device, so that concurrent callers
  // never see each other's setting
  int dev = -1;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  if (dev < 0 || dev >= FL_MAX_DEVICES) return hipErrorInvalidDevice;
  std::call_once(g_lds_once[dev], [dev] {
    g_lds_rc[dev] = hipFuncSetAttribute((const void*)fill_page_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FL_PAGE_LDS);
  });
  if (g_lds_rc[dev] != hipSuccess) return g_lds_rc[dev];
  hipLaunchKernelGGL(fill_pull_kernel, dim3(n_tiles), dim3(FL_THREADS), 0, st, pages, n_pages, (unsigned*)scratch);
  rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(fill_page_kernel, dim3(n_pages), dim3(FL_THREADS), FL_PAGE_LDS, st, pages, (unsigned*)scratch, rows);
  rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(fill_push_kernel, dim3(n_tiles), dim3(FL_THREADS), 0, st, pages, n_pages, (const unsigned*)scratch, rows);
  return hipGetLastError();
}
