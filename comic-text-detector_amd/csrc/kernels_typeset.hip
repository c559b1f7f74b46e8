// Typeset (`ctd_typeset`; the rule is stated in include/ctd_hip.h and restated in numpy, layer by layer over whole pages,
// in tests/typeset_ref.py): pre-rendered 8-bit coverage bitmaps composited into the device pages with a fill colour and an
// outline, the outline being the grey-scale dilation S of the coverage F by a disk of radius r <= 12.  Integers only.
//
// typeset_kernel, ONE launch, one workgroup of 256 threads per row of the tile table (a TILE_W x TILE_H tile of one page):
//   load    the tile of the page into registers, one packed pixel a register, PX pixels a thread (thread t: column t % 64,
//           rows t / 64 + 4 j), by byte loads: pages have 3-byte pixels at any pitch and alignment.
//   layers  the tile's entries in table order, every decision block-uniform.  Per layer that is valid and meets the tile:
//     patch   F on the tile grown by r, zeros outside the bitmap, into LDS (cov, at most 56 rows of 88 bytes).
//     rows    for every patch row that an active pixel can see and every tile column, the running horizontal max
//             m_k = max F(x - k .. x + k), k = 0 .. r, two byte reads a step; m_k is stored to plane slot[k] where k is a
//             half-width floor(sqrt(r^2 - dy^2)) of the disk (at most TS_PLANES distinct ones: 9 at r = 12).
//     blend   S(p) = max over dy of plane[slot[hw(dy)]](px, py + dy), 2 r + 1 byte reads; then blend(blend(P, s, S), f, F)
//             in the register.  About 70 LDS byte reads a pixel at r = 12 where the plain disk takes 441.  r = 0 skips
//             rows and the max.  The counts go wave-reduced to the layer's row by atomicAdd.
//   store   the tile, once.
// A page byte is read once and written once whatever the number of layers; overlapping layers see each other's result in
// table order because one workgroup owns the tile.  The layer loop has no cap.  LDS: 4928 + TS_PLANES * 3584 bytes.
#include "kernels.h"

namespace {

constexpr int TW = CTD_TYPESET_TILE_W, TH = CTD_TYPESET_TILE_H, RMAX = CTD_TYPESET_MAX_RADIUS;
constexpr int TS_THREADS = 256;
constexpr int PX = TW * TH / TS_THREADS;                   // pixels a thread
constexpr int CW = TW + 2 * RMAX, CH = TH + 2 * RMAX;      // the coverage patch
static_assert(TW == 64 && TS_THREADS % TW == 0 && (TW * TH) % TS_THREADS == 0 && TH % (TS_THREADS / TW) == 0,
              "a wave is one tile row; every thread has PX pixels");
static_assert(sizeof(ctd_typeset_page) == 24 && sizeof(ctd_typeset_layer) == 56 && sizeof(ctd_typeset_tile) == 16 &&
              sizeof(ctd_typeset_params) == 32 && sizeof(ctd_typeset_row) == 8, "typeset ABI sizes (typeset.py dtypes)");
static_assert(offsetof(ctd_typeset_page, pitch) == 16 && offsetof(ctd_typeset_layer, page) == 8 &&
              offsetof(ctd_typeset_layer, cov_pitch) == 28 && offsetof(ctd_typeset_layer, clip) == 32 &&
              offsetof(ctd_typeset_layer, fill) == 48 && offsetof(ctd_typeset_layer, radius) == 54 &&
              offsetof(ctd_typeset_params, cov_bytes) == 16, "typeset ABI offsets");

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

__global__ __launch_bounds__(TS_THREADS) void typeset_kernel(const ctd_typeset_page* __restrict__ pages,
                                                             const ctd_typeset_layer* __restrict__ layers,
                                                             const ctd_typeset_tile* __restrict__ tiles,
                                                             const int* __restrict__ entries,
                                                             const unsigned char* __restrict__ cov_dev, ctd_typeset_params prm,
                                                             ctd_typeset_row* __restrict__ rows) {
  __shared__ unsigned char cov[CH][CW];                    // F on the tile grown by r; patch (0, 0) is tile (-r, -r)
  __shared__ unsigned char plane[TS_PLANES][CH][TW];       // running horizontal maxima, one plane a distinct half-width
  __shared__ signed char slot[RMAX + 1];                   // half-width k -> its plane, -1: no row of the disk has it
  __shared__ signed char slot_dy[RMAX + 1];                // |dy| -> the plane of its half-width
  const int t = threadIdx.x, lane = t & 63;
  const int lx = t % TW, ly = t / TW;                      // this thread's pixels: (lx, ly + j * LYS)
  constexpr int LYS = TS_THREADS / TW;

  // ---- the tile (block-uniform; a tile that is no tile of its page does nothing)
  const ctd_typeset_tile T = tiles[blockIdx.x];
  if (T.page < 0 || T.page >= prm.n_pages || T.tx < 0 || T.ty < 0) return;
  const ctd_typeset_page P = pages[T.page];
  if (P.H < 1 || P.W < 1 || P.H > CTD_TYPESET_MAX_SIDE || P.W > CTD_TYPESET_MAX_SIDE) return;
  if ((long long)T.tx * TW >= P.W || (long long)T.ty * TH >= P.H) return;
  const int tx0 = T.tx * TW, ty0 = T.ty * TH;
  const int e_begin = min(max(T.first, 0), prm.n_entries), e_end = min(max(tiles[blockIdx.x + 1].first, 0), prm.n_entries);
  if (e_begin >= e_end) return;

  // ---- load
  unsigned char* __restrict__ base = (unsigned char*)P.page_dev;
  unsigned pix[PX];
  const int gx = tx0 + lx;
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const int gy = ty0 + ly + j * LYS;
    pix[j] = 0;
    if (gx < P.W && gy < P.H) {
      const unsigned char* q = base + (long long)gy * P.pitch + 3 * gx;
      pix[j] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
    }
  }

  // ---- layers
  for (int e = e_begin; e < e_end; ++e) {
    const int li = entries[e];
    if (li < 0 || li >= prm.n_layers) continue;
    const ctd_typeset_layer Ly = layers[li];
    const int r = Ly.radius;
    if (Ly.page != T.page || Ly.w < 1 || Ly.h < 1 || Ly.w > CTD_TYPESET_MAX_SIDE || Ly.h > CTD_TYPESET_MAX_SIDE ||
        r > RMAX || Ly.cov0 < 0 || Ly.cov_pitch < 0 ||
        Ly.cov0 + (long long)(Ly.h - 1) * Ly.cov_pitch + Ly.w > prm.cov_bytes)
      continue;
    // the pixels of this tile the layer writes: page, clip, the bitmap's rectangle grown by r, the tile
    const long long bx1 = (long long)Ly.x0 - r, by1 = (long long)Ly.y0 - r;
    const long long bx2 = (long long)Ly.x0 + Ly.w + r, by2 = (long long)Ly.y0 + Ly.h + r;
    const int ax1 = (int)max(max(bx1, (long long)Ly.clip[0]), (long long)tx0);
    const int ay1 = (int)max(max(by1, (long long)Ly.clip[1]), (long long)ty0);
    const int ax2 = (int)min(min(bx2, (long long)Ly.clip[2]), (long long)min(tx0 + TW, P.W));
    const int ay2 = (int)min(min(by2, (long long)Ly.clip[3]), (long long)min(ty0 + TH, P.H));
    if (ax1 >= ax2 || ay1 >= ay2) continue;
    // the layer meets the tile, so x0 and y0 are within MAX_SIDE + RMAX of it: int from here on
    const int ox = tx0 - r - Ly.x0, oy = ty0 - r - Ly.y0;  // patch (0, 0) in bitmap coordinates
    const int pw = TW + 2 * r;
    const int pr1 = ay1 - ty0, pr2 = ay2 - ty0 + 2 * r;    // the patch rows an active pixel can see

    __syncthreads();                                       // the layer before is done with cov, plane and slot
    for (int i = t; i < (pr2 - pr1) * pw; i += TS_THREADS) {
      const int py = pr1 + i / pw, px = i % pw;
      const int bx = ox + px, by = oy + py;
      unsigned char v = 0;
      if (bx >= 0 && bx < Ly.w && by >= 0 && by < Ly.h) v = cov_dev[Ly.cov0 + (long long)by * Ly.cov_pitch + bx];
      cov[py][px] = v;
    }
    if (t == 0 && r > 0) {
      for (int k = 0; k <= r; ++k) slot[k] = -1;
      int n = 0;
      for (int dy = 0; dy <= r; ++dy) {
        int k = 0;
        while ((k + 1) * (k + 1) + dy * dy <= r * r) ++k;
        if (slot[k] < 0) slot[k] = (signed char)n++;      // half-widths fall as dy grows: n <= TS_PLANES
        slot_dy[dy] = slot[k];
      }
    }
    __syncthreads();
    if (r > 0) {
      for (int i = t; i < (pr2 - pr1) * TW; i += TS_THREADS) {
        const int py = pr1 + i / TW, x = i % TW;
        const unsigned char* __restrict__ row = &cov[py][x + r];
        int m = row[0];
        if (slot[0] >= 0) plane[slot[0]][py][x] = (unsigned char)m;
        for (int k = 1; k <= r; ++k) {
          m = max(m, max((int)row[-k], (int)row[k]));
          const int s = slot[k];
          if (s >= 0) plane[s][py][x] = (unsigned char)m;
        }
      }
      __syncthreads();
    }

    // ---- blend
    const int f0 = Ly.fill[0], f1 = Ly.fill[1], f2 = Ly.fill[2], s0 = Ly.stroke[0], s1 = Ly.stroke[1], s2 = Ly.stroke[2];
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
    if (lane == 0) {
      if (n_fill) atomicAdd(&rows[li].n_fill, n_fill);
      if (n_stroke) atomicAdd(&rows[li].n_stroke, n_stroke);
    }
  }

  // ---- store, once: the pixels some layer wrote
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    if (pix[j] >> 24) {
      unsigned char* q = base + (long long)(ty0 + ly + j * LYS) * P.pitch + 3 * gx;
      q[0] = (unsigned char)pix[j], q[1] = (unsigned char)(pix[j] >> 8), q[2] = (unsigned char)(pix[j] >> 16);
    }
  }
}

}  // namespace

hipError_t launch_typeset(const ctd_typeset_page* pages, const ctd_typeset_layer* layers, const ctd_typeset_tile* tiles,
                          const int32_t* entries, const uint8_t* cov, const ctd_typeset_params& prm, ctd_typeset_row* rows,
                          hipStream_t st) {
  hipLaunchKernelGGL(typeset_kernel, dim3(prm.n_tiles), dim3(TS_THREADS), 0, st, pages, layers, tiles, entries, cov, prm, rows);
  return hipGetLastError();
}
