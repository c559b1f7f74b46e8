// Texture fill of a hole mask by patch matching (`ctd_texture_fill`; the rule is stated in include/ctd_hip.h and restated in
// numpy in tests/texture_ref.py): a nearest-neighbour field of 7 x 7 patches found by Jacobi sweeps of propagation and random
// search, and patch voting.  Integers only: sums of squared byte differences, one hash, one division by 2 n.
//
// 1 + (n_em * n_sweep + 1) + n_em + 1 launches, no host step between them, whatever the pages.
//
// texture_prepare_kernel, one workgroup per 64 x 64 tile of all pages: the mask with a halo of 3 into LDS, the 7 x 7 "any
// hole" by a row pass and a column pass, then per pixel the class byte (hole / target / valid centre), the working image C
// into `out` (`init` on holes, the page elsewhere), 0 into field plane 0 at targets, and the tile's counts (sums in
// registers and LDS, no atomics).
//
// texture_sweep_kernel, one workgroup per tile: a tile without a target returns after reading its count.  Otherwise C of
// the tile with a halo of 3, at coordinates clamped to the page -- the rule's clamp of a target's patch --, goes into LDS
// as packed bytes, the tile's targets are compacted in LDS (ballot and prefix sums) and threads take compacted targets.  A
// target's own patch is read from LDS, source patches from `out` in global memory: the search window is local, so they hit
// L2, as aligned dwords; a row's sum of squared differences is a.a + b.b - 2 a.b in byte dot products.  A candidate's
// cost loop stops after patch rows 1, 3 and 5 once it has reached the best; replacement is strict, so that changes no
// result.  The sweep reads field plane s & 1 and writes the other.
//
// texture_vote_kernel, one workgroup per tile: a tile without a hole returns.  The field of the tile's targets and of a
// halo of 3 goes into LDS; a hole pixel gathers from the up to 49 targets whose patch covers it, seven loads in flight.  It
// reads `out` at source pixels only (known, never written) and writes hole pixels only, so it runs in place.
//
// texture_rows_kernel, one workgroup per page: the tile counts summed into the row.
#include <algorithm>
#include <string>
#include <vector>

#include "kernels.h"

namespace {

constexpr int TX_TILE = CTD_TEXTURE_TILE;
constexpr int TX_THREADS = 256, TX_WAVES = TX_THREADS / 64;
constexpr int TX_PR = CTD_TEXTURE_PATCH / 2;                      // the patch radius
constexpr int TX_SIDE = TX_TILE + 2 * TX_PR;                      // a tile with its halo
constexpr unsigned TX_HOLE = 1u, TX_TARGET = 2u, TX_VALID = 4u;   // the class byte
constexpr unsigned TX_NONE = 0xffffffffu;                         // above every cost: 49 * 3 * 255^2 < 2^24
static_assert(TX_TILE == 64 && CTD_TEXTURE_PATCH == 7, "a tile row is a wave; the patch loops");
static_assert(CTD_TEXTURE_MAX_RADIUS <= 127, "an offset is an int8");
static_assert(sizeof(ctd_texture_page) == 80 && sizeof(ctd_texture_params) == 32 && sizeof(ctd_texture_row) == 32,
              "texture ABI sizes (texture.py dtypes)");
static_assert(offsetof(ctd_texture_page, H) == 32 && offsetof(ctd_texture_page, tile0) == 56 && offsetof(ctd_texture_page, fld0) == 64 &&
              offsetof(ctd_texture_params, scratch_bytes) == 24, "texture ABI offsets");

// the page of a tile: the last one whose tile0 <= tile (uniform)
__device__ __forceinline__ int page_of_tile(const ctd_texture_page* __restrict__ pages, int n_pages, int tile) {
  int lo = 0, hi = n_pages - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pages[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the tile of this workgroup: its page and the tile's first pixel; false where the table does not hold it
__device__ __forceinline__ bool locate(const ctd_texture_page* __restrict__ pages, int n_pages, ctd_texture_page& P, int& x0, int& y0) {
  P = pages[page_of_tile(pages, n_pages, (int)blockIdx.x)];
  const int tiles_x = (P.W + TX_TILE - 1) / TX_TILE, tiles_y = (P.H + TX_TILE - 1) / TX_TILE;
  const int local = (int)blockIdx.x - P.tile0;
  if (local < 0 || local >= tiles_x * tiles_y) return false;
  const int tyi = local / tiles_x;
  y0 = tyi * TX_TILE, x0 = (local - tyi * tiles_x) * TX_TILE;
  return true;
}

// the sum of v over the workgroup, in every thread (red: TX_WAVES ints)
__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  __syncthreads();                                          // red may still be read from the sum before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < TX_WAVES; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- prepare ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(TX_THREADS) void texture_prepare_kernel(const ctd_texture_page* __restrict__ pages, int n_pages,
                                                                     uint8_t* __restrict__ scratch) {
  __shared__ uint8_t m[TX_SIDE][TX_SIDE + 2];              // 1 on a hole pixel, 0 elsewhere and beyond the page
  __shared__ uint8_t hor[TX_SIDE][TX_TILE];                // any hole in the 7 pixels of the row
  __shared__ int red[TX_WAVES];
  const int t = threadIdx.x;
  ctd_texture_page P;
  int x0, y0;
  if (!locate(pages, n_pages, P, x0, y0)) return;
  for (int i = t; i < TX_SIDE * TX_SIDE; i += TX_THREADS) {
    const int sy = i / TX_SIDE, sx = i - sy * TX_SIDE;
    const int y = y0 - TX_PR + sy, x = x0 - TX_PR + sx;
    m[sy][sx] = (y >= 0 && y < P.H && x >= 0 && x < P.W) ? (P.hole_dev[(long long)y * P.hole_pitch + x] != 0) : 0;
  }
  __syncthreads();
  for (int i = t; i < TX_SIDE * TX_TILE; i += TX_THREADS) {
    const int sy = i >> 6, lx = i & 63;
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < CTD_TEXTURE_PATCH; ++k) v |= m[sy][lx + k];
    hor[sy][lx] = (uint8_t)v;
  }
  __syncthreads();
  uint8_t* __restrict__ cls = scratch + P.cls0;
  unsigned* __restrict__ fld = (unsigned*)(scratch + P.fld0);
  int n_hole = 0, n_target = 0, n_valid = 0;
  for (int i = t; i < TX_TILE * TX_TILE; i += TX_THREADS) {
    const int ly = i >> 6, lx = i & 63, y = y0 + ly, x = x0 + lx;
    if (y >= P.H || x >= P.W) continue;
    const unsigned hole = m[ly + TX_PR][lx + TX_PR];
    unsigned any = 0;
#pragma unroll
    for (int k = 0; k < CTD_TEXTURE_PATCH; ++k) any |= hor[ly + k][lx];
    const unsigned valid = !any && y >= TX_PR && y < P.H - TX_PR && x >= TX_PR && x < P.W - TX_PR;
    const long long at = (long long)y * P.W + x;
    cls[at] = (uint8_t)(hole * TX_HOLE | any * TX_TARGET | valid * TX_VALID);
    if (any) fld[at] = 0u;                                  // the field before the initial sweep: ok = 0, offset (0, 0)
    const uint8_t* src = hole ? P.init_dev + (long long)y * P.init_pitch + 3ll * x : P.page_dev + (long long)y * P.pitch + 3ll * x;
    uint8_t* dst = P.out_dev + (long long)y * P.out_pitch + 3ll * x;
    const uint8_t c0 = src[0], c1 = src[1], c2 = src[2];
    dst[0] = c0, dst[1] = c1, dst[2] = c2;
    n_hole += (int)hole, n_target += (int)any, n_valid += (int)valid;
  }
  n_hole = block_sum(n_hole, red);
  n_target = block_sum(n_target, red);
  n_valid = block_sum(n_valid, red);
  if (t == 0) {
    int* __restrict__ cnt = (int*)scratch + 4ll * blockIdx.x;
    cnt[0] = n_hole, cnt[1] = n_target, cnt[2] = n_valid, cnt[3] = n_target;
  }
}

// ---- sweep ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned hash32(unsigned x, unsigned y, unsigned s, unsigned k, unsigned seed) {
  unsigned h = x * 0x9E3779B1u + y * 0x85EBCA77u + s * 0xC2B2AE3Du + k * 0x27D4EB2Fu + seed;
  h ^= h >> 16, h *= 0x7FEB352Du, h ^= h >> 15, h *= 0x846CA68Bu, h ^= h >> 16;
  return h;
}

__device__ __forceinline__ int draw(int x, int y, int s, int k, unsigned seed, int rho) {
  return (int)(hash32((unsigned)x, (unsigned)y, (unsigned)s, (unsigned)k, seed) % (unsigned)(2 * rho + 1)) - rho;
}

constexpr int TX_ROW_DWORDS = (3 * CTD_TEXTURE_PATCH + 3 + 3) / 4;   // 21 bytes at any alignment lie in six aligned dwords
static_assert(TX_ROW_DWORDS == 6, "a source patch row");
// the patch rows after which a cost sum is compared with the best so far (a bit a row).  The compiler sinks a row's loads
// behind the last check before it, so every check is one more memory round trip a candidate and fewer loads for a
// candidate that loses; the call measured on the record's two batches: none 1611 / 82 746 us,
// row 3 1530 / 68 397, rows 1, 3, 5 1588 / 57 788
constexpr unsigned TX_CHECK_ROWS = 0x2a;

// The staged tile in LDS: C of the tile and its halo as packed bytes, 3 a pixel, a row TX_IMG_PITCH bytes (a multiple of 4)
constexpr int TX_IMG_PITCH = (3 * TX_SIDE + 3) / 4 * 4;
static_assert(TX_IMG_PITCH == 212 && 3 * (TX_TILE - 1) / 4 * 4 + TX_ROW_DWORDS * 4 <= TX_IMG_PITCH, "the last patch's six dwords lie inside its row");

// A target's own patch: its seven rows of 21 bytes as six dwords each, bytes 21 .. 23 zero, and the rows' sums of squares
struct Own {
  unsigned a[CTD_TEXTURE_PATCH][TX_ROW_DWORDS];
  unsigned a2[CTD_TEXTURE_PATCH];
};

// 21 bytes that start `sh` / 8 bytes into the aligned dwords d[0 .. 5], as six dwords with bytes 21 .. 23 zero
__device__ __forceinline__ void align_row(const unsigned (&d)[TX_ROW_DWORDS], unsigned sh, unsigned (&w)[TX_ROW_DWORDS]) {
#pragma unroll
  for (int k = 0; k + 1 < TX_ROW_DWORDS; ++k) w[k] = __builtin_amdgcn_alignbit(d[k + 1], d[k], sh);   // {hi, lo} >> sh
  w[TX_ROW_DWORDS - 1] = (d[TX_ROW_DWORDS - 1] >> sh) & 255u;   // byte 20 alone is wanted of it
}

// the sum over the 24 bytes of two rows of a * b: six byte dot products
__device__ __forceinline__ unsigned row_dot(const unsigned (&a)[TX_ROW_DWORDS], const unsigned (&b)[TX_ROW_DWORDS]) {
  unsigned s = 0;
#pragma unroll
  for (int k = 0; k < TX_ROW_DWORDS; ++k) s = __builtin_amdgcn_udot4(a[k], b[k], s, false);
  return s;
}

__device__ __forceinline__ void load_own(Own& o, const unsigned* __restrict__ img, int ly, int lx) {
  const int at = 3 * lx;                                    // the patch's first byte in the row; TX_IMG_PITCH % 4 = 0
#pragma unroll
  for (int r = 0; r < CTD_TEXTURE_PATCH; ++r) {
    const unsigned* __restrict__ p = img + (ly + r) * (TX_IMG_PITCH / 4) + (at >> 2);
    unsigned d[TX_ROW_DWORDS];
#pragma unroll
    for (int k = 0; k < TX_ROW_DWORDS; ++k) d[k] = p[k];
    align_row(d, (unsigned)(at & 3) * 8u, o.a[r]);
    o.a2[r] = row_dot(o.a[r], o.a[r]);
  }
}

// D of a target with the patch `own` and the source patch that starts at `src`.  The 7 x 21 source bytes are fetched as 42
// ALIGNED dwords (every one of them holds a byte of the patch, so none leaves the image's rows) and shifted into place by
// the row's misalignment.  A row's sum of (a - b)^2 is a.a + b.b - 2 a.b, exact in integers, as byte dot products.  The sum
// gives up after a row of TX_CHECK_ROWS once it has reached `limit` (the value is then >= limit and wins nothing).
__device__ __forceinline__ unsigned patch_cost(const Own& own, const uint8_t* __restrict__ src, long long pitch, unsigned limit) {
  unsigned d[CTD_TEXTURE_PATCH][TX_ROW_DWORDS];
  unsigned sh[CTD_TEXTURE_PATCH];
#pragma unroll
  for (int r = 0; r < CTD_TEXTURE_PATCH; ++r) {
    const uintptr_t a = (uintptr_t)(src + r * pitch);
    const unsigned* __restrict__ p = (const unsigned*)(a & ~(uintptr_t)3);
    sh[r] = (unsigned)(a & 3u) * 8u;
#pragma unroll
    for (int k = 0; k < TX_ROW_DWORDS; ++k) d[r][k] = p[k];
  }
  unsigned c = 0;
#pragma unroll
  for (int r = 0; r < CTD_TEXTURE_PATCH; ++r) {
    unsigned w[TX_ROW_DWORDS];
    align_row(d[r], sh[r], w);
    c += own.a2[r] + row_dot(w, w) - 2u * row_dot(own.a[r], w);
    if (((TX_CHECK_ROWS >> r) & 1u) && c >= limit) break;
  }
  return c;
}

__device__ __forceinline__ int field_dy(unsigned f) { return (int)(signed char)(f & 255u); }
__device__ __forceinline__ int field_dx(unsigned f) { return (int)(signed char)((f >> 8) & 255u); }
__device__ __forceinline__ bool field_ok(unsigned f) { return ((f >> 16) & 1u) != 0; }

// the best of a target while a sweep tries candidates
struct Best {
  int dy, dx;
  unsigned cost;                                            // TX_NONE: none
};

// an admissible candidate replaces the best where its cost is strictly lower
__device__ __forceinline__ void consider(Best& b, int cy, int cx, int y, int x, int R, const ctd_texture_page& P,
                                         const uint8_t* __restrict__ cls, const Own& own) {
  if (cy < -R || cy > R || cx < -R || cx > R) return;
  const int sy = y + cy, sx = x + cx;
  if (sy < 0 || sy >= P.H || sx < 0 || sx >= P.W) return;
  if (!(cls[(long long)sy * P.W + sx] & TX_VALID)) return;  // valid: the whole source patch lies inside the page
  const unsigned c = patch_cost(own, P.out_dev + (long long)(sy - TX_PR) * P.out_pitch + 3ll * (sx - TX_PR), P.out_pitch, b.cost);
  if (c < b.cost) b.dy = cy, b.dx = cx, b.cost = c;
}

__global__ __launch_bounds__(TX_THREADS) void texture_sweep_kernel(const ctd_texture_page* __restrict__ pages, int n_pages,
                                                                   uint8_t* __restrict__ scratch, int R, int n_init, unsigned seed,
                                                                   int s) {
  __shared__ unsigned img[TX_SIDE * TX_IMG_PITCH / 4];     // C of the tile and its halo, clamped to the page: packed bytes
  __shared__ unsigned short list[TX_TILE * TX_TILE];       // the tile's targets: ly << 6 | lx
  __shared__ int rowoff[TX_TILE + 1];
  __shared__ int red[TX_WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int* __restrict__ cnt = (int*)scratch + 4ll * blockIdx.x;
  if (cnt[1] == 0) return;                                  // no target (block-uniform); prepare left cnt[3] = 0
  ctd_texture_page P;
  int x0, y0;
  if (!locate(pages, n_pages, P, x0, y0)) return;
  const uint8_t* __restrict__ cls = scratch + P.cls0;
  const long long px = (long long)P.H * P.W;
  const unsigned* __restrict__ oldf = (const unsigned*)(scratch + P.fld0) + ((s & 1) ? px : 0);
  unsigned* __restrict__ newf = (unsigned*)(scratch + P.fld0) + ((s & 1) ? 0 : px);

  for (int i = t; i < TX_SIDE * TX_SIDE; i += TX_THREADS) {
    const int sy = i / TX_SIDE, sx = i - sy * TX_SIDE;
    const int y = clampi(y0 - TX_PR + sy, 0, P.H - 1), x = clampi(x0 - TX_PR + sx, 0, P.W - 1);
    const uint8_t* p = P.out_dev + (long long)y * P.out_pitch + 3ll * x;
    uint8_t* q = (uint8_t*)img + sy * TX_IMG_PITCH + 3 * sx;
    q[0] = p[0], q[1] = p[1], q[2] = p[2];
  }
  if (t < TX_SIDE) {                                        // the bytes behind a row's last pixel: read with it, weigh nothing
    uint8_t* q = (uint8_t*)img + t * TX_IMG_PITCH + 3 * TX_SIDE;
    q[0] = 0, q[1] = 0;
  }
  // compact the targets: the count of every tile row, their prefix, then every target's slot
  for (int r = wave; r < TX_TILE; r += TX_WAVES) {
    const int y = y0 + r, x = x0 + lane;
    const bool tg = y < P.H && x < P.W && (cls[(long long)y * P.W + x] & TX_TARGET);
    const unsigned long long mask = __ballot(tg);
    if (lane == 0) rowoff[r + 1] = __popcll(mask);
  }
  __syncthreads();
  if (t == 0) {
    rowoff[0] = 0;
    for (int r = 0; r < TX_TILE; ++r) rowoff[r + 1] += rowoff[r];
  }
  __syncthreads();
  for (int r = wave; r < TX_TILE; r += TX_WAVES) {
    const int y = y0 + r, x = x0 + lane;
    const bool tg = y < P.H && x < P.W && (cls[(long long)y * P.W + x] & TX_TARGET);
    const unsigned long long mask = __ballot(tg);
    if (tg) list[rowoff[r] + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)(r << 6 | lane);
  }
  __syncthreads();
  const int n = rowoff[TX_TILE];

  int unmatched = 0;
  for (int i = t; i < n; i += TX_THREADS) {
    const int ly = list[i] >> 6, lx = list[i] & 63, y = y0 + ly, x = x0 + lx;
    Own own;                                                // the patch's first pixel: (ly + 3 - 3, lx + 3 - 3)
    load_own(own, img, ly, lx);
    const unsigned f = oldf[(long long)y * P.W + x];
    Best b = {field_dy(f), field_dx(f), TX_NONE};
    if (field_ok(f))                                        // the old entry, its cost computed anew: C has changed
      b.cost = patch_cost(own, P.out_dev + (long long)(y + b.dy - TX_PR) * P.out_pitch + 3ll * (x + b.dx - TX_PR), P.out_pitch, TX_NONE);
    if (s == 0) {
      for (int j = 0; j < n_init; ++j)
        consider(b, draw(x, y, s, 2 * j, seed, R), draw(x, y, s, 2 * j + 1, seed, R), y, x, R, P, cls, own);
    } else {
      for (int d = 1; d <= 8; d <<= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {                       // (0, -d), (0, +d), (-d, 0), (+d, 0) as (dy, dx)
          const int ny = y + (q == 2 ? -d : q == 3 ? d : 0), nx = x + (q == 0 ? -d : q == 1 ? d : 0);
          if (ny < 0 || ny >= P.H || nx < 0 || nx >= P.W) continue;
          if (!(cls[(long long)ny * P.W + nx] & TX_TARGET)) continue;
          const unsigned g = oldf[(long long)ny * P.W + nx];
          if (field_ok(g)) consider(b, field_dy(g), field_dx(g), y, x, R, P, cls, own);
        }
      }
      int j = 0;
      for (int rho = R; rho >= 1; rho >>= 1, ++j) {         // a best of none has the offset (0, 0)
        const int cy = b.dy + draw(x, y, s, 2 * j, seed, rho), cx = b.dx + draw(x, y, s, 2 * j + 1, seed, rho);
        consider(b, cy, cx, y, x, R, P, cls, own);
      }
    }
    const bool ok = b.cost != TX_NONE;
    newf[(long long)y * P.W + x] = ok ? ((unsigned)b.dy & 255u) | ((unsigned)b.dx & 255u) << 8 | 1u << 16 : 0u;
    unmatched += !ok;
  }
  unmatched = block_sum(unmatched, red);
  if (t == 0) cnt[3] = unmatched;
}

// ---- vote -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(TX_THREADS) void texture_vote_kernel(const ctd_texture_page* __restrict__ pages, int n_pages,
                                                                  uint8_t* __restrict__ scratch, int plane) {
  __shared__ unsigned fl[TX_SIDE * TX_SIDE];
  const int* __restrict__ cnt = (const int*)scratch + 4ll * blockIdx.x;
  if (cnt[0] == 0) return;                                  // no hole (block-uniform)
  ctd_texture_page P;
  int x0, y0;
  if (!locate(pages, n_pages, P, x0, y0)) return;
  const uint8_t* __restrict__ cls = scratch + P.cls0;
  const unsigned* __restrict__ fld = (const unsigned*)(scratch + P.fld0) + (plane ? (long long)P.H * P.W : 0);
  // the field of the tile's targets and of its halo, the class byte on top: 0 beyond the page and where there is no target
  for (int i = threadIdx.x; i < TX_SIDE * TX_SIDE; i += TX_THREADS) {
    const int sy = i / TX_SIDE, sx = i - sy * TX_SIDE;
    const int y = y0 - TX_PR + sy, x = x0 - TX_PR + sx;
    unsigned v = 0;
    if (y >= 0 && y < P.H && x >= 0 && x < P.W) {
      const long long at = (long long)y * P.W + x;
      const unsigned c = cls[at];
      v = c << 24;
      if (c & TX_TARGET) v |= fld[at];
    }
    fl[i] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TX_TILE * TX_TILE; i += TX_THREADS) {
    const int ly = i >> 6, lx = i & 63, y = y0 + ly, x = x0 + lx;
    if (!((fl[(ly + TX_PR) * TX_SIDE + lx + TX_PR] >> 24) & TX_HOLE)) continue;   // 0 beyond the page
    uint8_t* dst = P.out_dev + (long long)y * P.out_pitch + 3ll * x;
    unsigned s0 = 0, s1 = 0, s2 = 0, n = 0;
    for (int oy = -TX_PR; oy <= TX_PR; ++oy) {
      // the target t = p - o votes with C[t + off(t) + o] = C[p + off(t)]: t + off(t) is a valid centre, so that pixel lies
      // inside the page and is known.  No branch inside a row: the seven loads fly together; a target that does not vote
      // reads the pixel itself and adds nothing
      unsigned c0[CTD_TEXTURE_PATCH], c1[CTD_TEXTURE_PATCH], c2[CTD_TEXTURE_PATCH], okm[CTD_TEXTURE_PATCH];
#pragma unroll
      for (int k = 0; k < CTD_TEXTURE_PATCH; ++k) {
        const unsigned f = fl[(ly + TX_PR - oy) * TX_SIDE + lx + TX_PR - (k - TX_PR)];
        okm[k] = field_ok(f) ? 1u : 0u;
        const uint8_t* p = okm[k] ? P.out_dev + (long long)(y + field_dy(f)) * P.out_pitch + 3ll * (x + field_dx(f)) : dst;
        c0[k] = p[0], c1[k] = p[1], c2[k] = p[2];
      }
#pragma unroll
      for (int k = 0; k < CTD_TEXTURE_PATCH; ++k) s0 += okm[k] * c0[k], s1 += okm[k] * c1[k], s2 += okm[k] * c2[k], n += okm[k];
    }
    if (!n) continue;
    dst[0] = (uint8_t)((2u * s0 + n) / (2u * n)), dst[1] = (uint8_t)((2u * s1 + n) / (2u * n)), dst[2] = (uint8_t)((2u * s2 + n) / (2u * n));
  }
}

// ---- rows -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(TX_THREADS) void texture_rows_kernel(const ctd_texture_page* __restrict__ pages,
                                                                  const uint8_t* __restrict__ scratch, ctd_texture_row* __restrict__ rows) {
  __shared__ int red[TX_WAVES];
  const ctd_texture_page P = pages[blockIdx.x];
  const int tiles = ((P.W + TX_TILE - 1) / TX_TILE) * ((P.H + TX_TILE - 1) / TX_TILE);
  const int* __restrict__ cnt = (const int*)scratch + 4ll * P.tile0;
  int v[4] = {0, 0, 0, 0};
  for (int i = threadIdx.x; i < tiles; i += TX_THREADS) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += cnt[4 * i + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = block_sum(v[k], red);
  if (threadIdx.x == 0) {
    ctd_texture_row* __restrict__ row = rows + blockIdx.x;
    row->status = v[0] == 0 ? CTD_TEXTURE_NO_HOLE : v[2] == 0 ? CTD_TEXTURE_NO_SOURCE : CTD_TEXTURE_OK;
    row->n_hole = v[0], row->n_target = v[1], row->n_source = v[2], row->n_unmatched = v[3];
    row->pad_[0] = row->pad_[1] = row->pad_[2] = 0;
  }
}

struct Span {
  uintptr_t lo, hi;                                         // [lo, hi)
};

Span span_of(const uint8_t* p, int H, int pitch, int row_bytes) {
  return {(uintptr_t)p, (uintptr_t)p + (uintptr_t)(H - 1) * (uintptr_t)pitch + (uintptr_t)row_bytes};
}

}  // namespace

extern "C" int ctd_texture_fill(const ctd_texture_page* pages_dev, int32_t n_pages, const ctd_texture_params* params,
                                void* scratch_dev, ctd_texture_row* rows_dev, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n_pages < 0) return api_fail(CTD_ERR_INVALID, "bad sizes");
  if (n_pages == 0) return CTD_OK;
  if (!pages_dev || !params || !scratch_dev || !rows_dev) return api_fail(CTD_ERR_INVALID, "null pointer");
  const ctd_texture_params prm = *params;
  if (prm.radius < 1 || prm.radius > CTD_TEXTURE_MAX_RADIUS || prm.n_em < 1 || prm.n_em > 16 || prm.n_sweep < 1 || prm.n_sweep > 8 ||
      prm.n_init < 1 || prm.n_init > 16)
    return api_fail(CTD_ERR_INVALID, "texture: radius 1 .. " + std::to_string(CTD_TEXTURE_MAX_RADIUS) +
                                         ", n_em 1 .. 16, n_sweep 1 .. 8, n_init 1 .. 16");
  if ((uintptr_t)scratch_dev & 15u) return api_fail(CTD_ERR_INVALID, "texture: scratch_dev is 16-byte aligned");
  // the shapes decide the grid and what the kernels may touch: the table is checked here, before anything launches
  std::vector<ctd_texture_page> tab((size_t)n_pages);
  hipError_t rc = hipMemcpyAsync(tab.data(), pages_dev, tab.size() * sizeof(ctd_texture_page), hipMemcpyDefault, st);
  if (rc == hipSuccess) rc = hipStreamSynchronize(st);
  if (rc != hipSuccess) return api_fail(CTD_ERR_HIP, std::string("texture: fetching the page table: ") + hipGetErrorString(rc));
  long long tiles = 0, pixels = 0;
  for (int32_t i = 0; i < n_pages; ++i) {
    const ctd_texture_page& p = tab[(size_t)i];
    const std::string at = "texture: page " + std::to_string(i) + ": ";
    if (!p.page_dev || !p.hole_dev || !p.init_dev || !p.out_dev) return api_fail(CTD_ERR_INVALID, at + "null pointer");
    if (p.H < 1 || p.W < 1 || p.H > CTD_TEXTURE_MAX_SIDE || p.W > CTD_TEXTURE_MAX_SIDE)
      return api_fail(CTD_ERR_INVALID, at + "sides 1 .. " + std::to_string(CTD_TEXTURE_MAX_SIDE));
    if (p.pitch < 3 * p.W || p.hole_pitch < p.W || p.init_pitch < 3 * p.W || p.out_pitch < 3 * p.W)
      return api_fail(CTD_ERR_INVALID, at + "a pitch below the row size");
    if (p.tile0 != tiles) return api_fail(CTD_ERR_INVALID, at + "tile0 is the tiles of the pages before it");
    tiles += (long long)((p.W + TX_TILE - 1) / TX_TILE) * ((p.H + TX_TILE - 1) / TX_TILE);
    if (tiles > 0x7fffffffll) return api_fail(CTD_ERR_INVALID, "texture: too many tiles for one call");
    pixels += (long long)p.H * p.W;
  }
  if (prm.n_tiles != tiles) return api_fail(CTD_ERR_INVALID, "texture: n_tiles is the tiles of all pages");
  if (prm.scratch_bytes < 16 * tiles + 9 * pixels) return api_fail(CTD_ERR_INVALID, "texture: scratch_bytes below 16 n_tiles + 9 pixels");
  long long before = 0;
  std::vector<Span> in;
  in.reserve(3 * tab.size());
  for (int32_t i = 0; i < n_pages; ++i) {
    const ctd_texture_page& p = tab[(size_t)i];
    if (p.fld0 != 16 * tiles + 8 * before || p.cls0 != 16 * tiles + 8 * pixels + before)
      return api_fail(CTD_ERR_INVALID, "texture: page " + std::to_string(i) + ": fld0 / cls0 are not the scratch layout's");
    before += (long long)p.H * p.W;
    in.push_back(span_of(p.page_dev, p.H, p.pitch, 3 * p.W));
    in.push_back(span_of(p.hole_dev, p.H, p.hole_pitch, p.W));
    in.push_back(span_of(p.init_dev, p.H, p.init_pitch, 3 * p.W));
  }
  // `out` overlaps no input of any page: the inputs sorted by their start, with the furthest end so far
  std::sort(in.begin(), in.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
  std::vector<uintptr_t> reach(in.size());
  for (size_t k = 0; k < in.size(); ++k) reach[k] = std::max(in[k].hi, k ? reach[k - 1] : (uintptr_t)0);
  for (int32_t i = 0; i < n_pages; ++i) {
    const ctd_texture_page& p = tab[(size_t)i];
    const Span o = span_of(p.out_dev, p.H, p.out_pitch, 3 * p.W);
    // the inputs that start below o.hi; one of them reaches beyond o.lo exactly where one overlaps
    const size_t k = (size_t)(std::lower_bound(in.begin(), in.end(), o.hi, [](const Span& a, uintptr_t v) { return a.lo < v; }) - in.begin());
    if (k > 0 && reach[k - 1] > o.lo) return api_fail(CTD_ERR_INVALID, "texture: page " + std::to_string(i) + ": out overlaps an input");
  }

  const ctd_texture_page* pg = pages_dev;
  uint8_t* scratch = (uint8_t*)scratch_dev;
  const dim3 grid((unsigned)tiles), block(TX_THREADS);
#define TX_LAUNCHED()                                                                                        \
  do {                                                                                                       \
    rc = hipGetLastError();                                                                                  \
    if (rc != hipSuccess) return api_fail(CTD_ERR_HIP, std::string("texture launch: ") + hipGetErrorString(rc)); \
  } while (0)
  hipLaunchKernelGGL(texture_prepare_kernel, grid, block, 0, st, pg, n_pages, scratch);
  TX_LAUNCHED();
  int s = 0;
  for (int em = 0; em < prm.n_em; ++em) {
    for (int k = 0; k < prm.n_sweep + (em == 0); ++k, ++s) {
      hipLaunchKernelGGL(texture_sweep_kernel, grid, block, 0, st, pg, n_pages, scratch, prm.radius, prm.n_init, prm.seed, s);
      TX_LAUNCHED();
    }
    hipLaunchKernelGGL(texture_vote_kernel, grid, block, 0, st, pg, n_pages, scratch, s & 1);   // sweep s - 1 wrote plane s & 1
    TX_LAUNCHED();
  }
  hipLaunchKernelGGL(texture_rows_kernel, dim3((unsigned)n_pages), block, 0, st, pg, (const uint8_t*)scratch, rows_dev);
  TX_LAUNCHED();
#undef TX_LAUNCHED
  return CTD_OK;
}
