// Typeset from a glyph atlas in a block's own frame (`ctd_typeset_tilted`; the rule is stated in include/ctd_hip.h, "tilted
// text", and restated in numpy in tests/tilt_ref.py).  A layer carries a pivot and a 16.16 (c, s) pair; its placements are in
// FRAME coordinates, U is their upright max-paste over frame pixels, and the layer's coverage at page pixel p is U resampled
// bilinearly (8 fraction bits) at page -> frame (p).  From there on it is the typeset rule in page space: outline S = disk max
// of F, r <= 12, pixel = blend(blend(P, s, S), f, F).  Integers only, products in 64 bits.  The tile, the outline and the
// blend are typeset_tile.h's; the walk over the tile's entries in groups of equal layer and chunks of NC, the staging and the
// gather are glyph_walk.h's, shared with kernels_glyphs.hip.
//
// tilted_kernel, ONE launch, one workgroup of 256 threads per row of the tile table: load the tile into registers, walk the
// groups, store the tile once.  This file's own, per group:
//   frame box  page -> frame is affine with integer coefficients, so the frame coordinates of the tile's coverage patch (the
//           rows the clip can see, all CW columns) take their extremes at its four corners: UX0 .. and UY0 .., ubw x ubh
//           pixels including the +1 neighbours of the bilinear taps.  (CW - 1) |c| + (CH - 1) |s| <= the patch's diagonal
//           times sqrt(c^2 + s^2) <= 102.93 * 65537, so ubw, ubh <= 105 < UW; the kernel checks the pivot, c^2 + s^2 and both
//           sizes and a layer beyond them draws nothing.  The gather's bytes are the frame box `ubuf`, byte i at row i / ubw,
//           every staged glyph scanned, GB bytes a thread at a time; the box's origin is in 64 bits.
//   resample   every byte of the patch rows from four taps of the frame box; the bounding box of F > 0 by wave shuffles and LDS
//           atomics gives the active rectangle (grown by r, cut to clip and tile) of the rows pass, the blend and the counts.
// LDS: 4928 (patch) + TS_PLANES * 3584 (planes / staged records) + 11236 (frame box) + small tables.
#include "glyph_walk.h"

namespace {

constexpr long long MAX_CS = 65537;                        // c^2 + s^2 <= MAX_CS^2: what rint of a unit vector times 65536 gives
constexpr int UW = 106, UH = 106;                          // the frame box of a patch
constexpr int GB = 8;                                      // frame-box bytes a thread resolves at a time
constexpr int FAR = 1 << 20;                               // a glyph corner this far from the frame box cannot cover a byte of it
static_assert(FAR > CTD_TYPESET_MAX_SIDE + UW, "a clamped corner still misses the box");
// the span of u (or v) over the patch is at most sqrt((CW - 1)^2 + (CH - 1)^2) * MAX_CS sixteenths-of-16.16, that is at most
// UW - 3 whole pixels; floor adds one column, the bilinear neighbour one more, and a count one more
static_assert((long long)(UW - 3) * (UW - 3) * 65536 * 65536 >= (long long)((CW - 1) * (CW - 1) + (CH - 1) * (CH - 1)) * MAX_CS * MAX_CS &&
              UH == UW, "the frame box holds a turned patch");
static_assert(sizeof(ctd_tilt_layer) == 48 && offsetof(ctd_tilt_layer, clip) == 4 && offsetof(ctd_tilt_layer, fill) == 20 &&
              offsetof(ctd_tilt_layer, radius) == 26 && offsetof(ctd_tilt_layer, ax) == 28 && offsetof(ctd_tilt_layer, c) == 36,
              "tilted typeset ABI (glyphs.py dtypes)");

struct FrameBox {                                          // gather's box: ubw x ubh frame pixels, origin (UX0, UY0) = ox, oy
  struct Addr { int x, y; };
  unsigned char (*ubuf)[UW];
  int ubw, n_bytes;
  long long ox, oy;
  __device__ Addr locate(int i) const { return {i - i / ubw * ubw, i / ubw}; }
  __device__ int x(Addr a) const { return a.x; }
  __device__ int y(Addr a) const { return a.y; }
  __device__ int state(Addr) const { return -1; }
  __device__ bool scan() const { return true; }
  // the glyph's corner in the frame box; further out than any box or glyph reaches, it is far enough
  __device__ void corner(const Staged& g, int& gx0, int& gy0) const {
    gx0 = (int)max(min((long long)g.x - ox, (long long)FAR), -(long long)FAR);
    gy0 = (int)max(min((long long)g.y - oy, (long long)FAR), -(long long)FAR);
  }
  __device__ unsigned char& byte(Addr a) const { return ubuf[a.y][a.x]; }
};

__global__ __launch_bounds__(TS_THREADS) void tilted_kernel(const ctd_typeset_page* __restrict__ pages,
                                                            const ctd_tilt_layer* __restrict__ layers,
                                                            const ctd_glyph_place* __restrict__ places,
                                                            const ctd_glyph_record* __restrict__ glyphs,
                                                            const ctd_typeset_tile* __restrict__ tiles,
                                                            const int* __restrict__ entries,
                                                            const unsigned char* __restrict__ atlas, ctd_glyph_params prm,
                                                            ctd_typeset_row* __restrict__ rows) {
  __shared__ unsigned char cov[CH][CW];                    // F on the tile grown by r; patch (0, 0) is tile (-r, -r)
  // running horizontal maxima, one plane a distinct half-width; before the rows pass: the staged records of the chunk
  __shared__ __attribute__((aligned(16))) unsigned char plane_raw[TS_PLANES * CH * TW];
  __shared__ unsigned char ubuf[UH][UW];                   // U on the frame box; (0, 0) is frame (UX0, UY0)
  __shared__ signed char slot[RMAX + 1];                   // half-width k -> its plane, -1: no row of the disk has it
  __shared__ signed char slot_dy[RMAX + 1];                // |dy| -> the plane of its half-width
  __shared__ int s_li;                                     // the group's layer, -1: its first entry names none
  __shared__ ctd_tilt_layer s_layer;                       // ... and its row of the layer table
  __shared__ int s_len;                                    // the group's entries within the chunk
  __shared__ int s_box[4];                                 // where the group's F is above 0, page coordinates, inclusive
  unsigned char(*plane)[CH][TW] = reinterpret_cast<unsigned char(*)[CH][TW]>(plane_raw);
  Staged* staged = reinterpret_cast<Staged*>(plane_raw);
  const int t = threadIdx.x, lane = t & 63;

  ctd_typeset_tile T;
  ctd_typeset_page P;
  int tx0, ty0, e_begin, e_end;
  if (!open_tile(tiles, pages, prm.n_pages, prm.n_entries, T, P, tx0, ty0, e_begin, e_end)) return;
  unsigned pix[PX];
  load_tile(P, tx0, ty0, t, pix);

  // ---- groups
  int e = e_begin;
  while (e < e_end) {
    Group G;
    int n_rows = 0, ubw = 0, ubh = 0, pvx = 0, pvy = 0;
    long long c = 0, s = 0, UX0 = 0, UY0 = 0;
    bool first_chunk = true, more = true;
    while (more) {
      const int n = min(e_end - e, NC);
      __syncthreads();                                     // the group before is done with cov, planes, ubuf, slots and s_*

      Staged sg;
      const int lay = stage_entry(layers, places, glyphs, entries, prm, T.page, e, n, t, first_chunk, staged, &s_layer, &s_li, &s_len, sg);
      if (t == 0) s_box[0] = s_box[1] = INT_MAX, s_box[2] = s_box[3] = INT_MIN;
      __syncthreads();
      if (first_chunk) {
        if (!group_layer(s_li, s_layer, T.page, P, tx0, ty0, t, slot, slot_dy, G)) break;
        c = s_layer.c, s = s_layer.s, pvx = s_layer.ax, pvy = s_layer.ay;
        if (pvx < -MAX_COORD || pvx > MAX_COORD || pvy < -MAX_COORD || pvy > MAX_COORD || c < -MAX_CS || c > MAX_CS || s < -MAX_CS ||
            s > MAX_CS || c * c + s * s > MAX_CS * MAX_CS)
          break;
        n_rows = G.cy2 - G.cy1 + 2 * G.r;
        // the frame box: u and v at the four corners of those patch rows
        const long long dxa = (long long)G.px0 - pvx, dxb = dxa + CW - 1;
        const long long dya = (long long)G.py0 + G.pr1 - pvy, dyb = dya + n_rows - 1;
        const long long u0 = c * dxa + s * dya, u1 = c * dxb + s * dya, u2 = c * dxa + s * dyb, u3 = c * dxb + s * dyb;
        const long long v0 = c * dya - s * dxa, v1 = c * dya - s * dxb, v2 = c * dyb - s * dxa, v3 = c * dyb - s * dxb;
        const long long ua = ((long long)pvx << 16) + min(min(u0, u1), min(u2, u3)), ub = ((long long)pvx << 16) + max(max(u0, u1), max(u2, u3));
        const long long va = ((long long)pvy << 16) + min(min(v0, v1), min(v2, v3)), vb = ((long long)pvy << 16) + max(max(v0, v1), max(v2, v3));
        UX0 = ua >> 16, UY0 = va >> 16;
        const long long bw = (ub >> 16) - UX0 + 2, bh = (vb >> 16) - UY0 + 2;
        if (bw > UW || bh > UH) break;                     // cannot happen within the bound on c^2 + s^2
        ubw = (int)bw, ubh = (int)bh;
      }
      run_length(t < n && lay != G.li, t, &s_len);
      __syncthreads();
      const int len = s_len;                               // >= 1 in the first chunk: entry e is of layer li

      // ---- gather: this thread's bytes of the frame box, the max over the staged glyphs that cover them
      gather<GB>(FrameBox{ubuf, ubw, ubw * ubh, UX0, UY0}, staged, len, atlas, first_chunk, t);
      e += len;
      more = len == n && n == NC && e < e_end;             // the chunk was all of this layer: it may go on
      first_chunk = false;
    }
    if (first_chunk) { ++e; continue; }                    // left by a break: nothing of entry e can be drawn here

    const int r = G.r, pr1 = G.pr1, px0 = G.px0, py0 = G.py0;
    __syncthreads();                                       // the frame box is whole; the staged records are done with

    // ---- resample: F on the patch rows, and where it is above 0
    int bx1 = INT_MAX, by1 = INT_MAX, bx2 = INT_MIN, by2 = INT_MIN;
    // u and v of the first of those patch pixels in 64 bits, once (block-uniform); a pixel adds |c px + s row| < 2^24
    const long long dx0 = (long long)px0 - pvx, dy0 = (long long)py0 + pr1 - pvy;
    const long long u_at0 = ((long long)pvx << 16) + c * dx0 + s * dy0, v_at0 = ((long long)pvy << 16) - s * dx0 + c * dy0;
    const int ci = (int)c, si = (int)s;
    for (int i = t; i < n_rows * CW; i += TS_THREADS) {
      const int row = i / CW, px = i - row * CW, py = pr1 + row;
      const int gx = px0 + px, gy = py0 + py;
      const long long u = u_at0 + (ci * px + si * row), v = v_at0 + (ci * row - si * px);
      const int x0 = (int)((u >> 16) - UX0), y0 = (int)((v >> 16) - UY0);
      const int fx = (int)((u >> 8) & 255), fy = (int)((v >> 8) & 255);
      const int u00 = ubuf[y0][x0], u10 = ubuf[y0][x0 + 1], u01 = ubuf[y0 + 1][x0], u11 = ubuf[y0 + 1][x0 + 1];
      const int F = ((u00 * (256 - fx) + u10 * fx) * (256 - fy) + (u01 * (256 - fx) + u11 * fx) * fy + 32768) >> 16;
      cov[py][px] = (unsigned char)F;
      if (F) bx1 = min(bx1, gx), by1 = min(by1, gy), bx2 = max(bx2, gx), by2 = max(by2, gy);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      bx1 = min(bx1, __shfl_down(bx1, d, 64)), by1 = min(by1, __shfl_down(by1, d, 64));
      bx2 = max(bx2, __shfl_down(bx2, d, 64)), by2 = max(by2, __shfl_down(by2, d, 64));
    }
    if (lane == 0 && bx1 <= bx2)
      atomicMin(&s_box[0], bx1), atomicMin(&s_box[1], by1), atomicMax(&s_box[2], bx2), atomicMax(&s_box[3], by2);
    __syncthreads();                                       // cov is whole
    if (s_box[0] > s_box[2]) continue;                     // F is 0 all over the patch (block-uniform)
    const int ax1 = max(s_box[0] - r, G.cx1), ay1 = max(s_box[1] - r, G.cy1);
    const int ax2 = min(s_box[2] + 1 + r, G.cx2), ay2 = min(s_box[3] + 1 + r, G.cy2);
    if (ax1 >= ax2 || ay1 >= ay2) continue;                // nothing of the group can write here

    const int rr1 = ay1 - ty0, rr2 = ay2 - ty0 + 2 * r;    // the patch rows an active pixel can see (within pr1 ..)
    if (r > 0) {
      rows_pass(cov, plane, slot, r, rr1, rr2, t);
      __syncthreads();                                     // the planes are whole
    }
    const ctd_tilt_layer Ly = s_layer;                     // s_layer is next written behind the next group's first barrier
    blend_count(r, ax1, ay1, ax2, ay2, Ly.fill, Ly.stroke, cov, plane, slot_dy, tx0, ty0, t, pix, rows, G.li);
  }

  store_tile(P, tx0, ty0, t, pix);
}

}  // namespace

hipError_t launch_typeset_tilted(const ctd_typeset_page* pages, const ctd_tilt_layer* layers, const ctd_glyph_place* places,
                                 const ctd_glyph_record* glyphs, const ctd_typeset_tile* tiles, const int32_t* entries,
                                 const uint8_t* atlas, const ctd_glyph_params& prm, ctd_typeset_row* rows, hipStream_t st) {
  hipLaunchKernelGGL(tilted_kernel, dim3(prm.n_tiles), dim3(TS_THREADS), 0, st, pages, layers, places, glyphs, tiles, entries,
                     atlas, prm, rows);
  return hipGetLastError();
}
