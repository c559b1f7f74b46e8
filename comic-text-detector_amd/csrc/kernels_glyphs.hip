// Typeset from a glyph atlas (`ctd_typeset_glyphs`; the rule is stated in include/ctd_hip.h and restated in numpy in
// tests/glyph_ref.py): a layer is a run of placements (layer, glyph, x, y) of atlas glyphs, its coverage F the MAX of the
// glyphs' coverage, and from there on the typeset rule of kernels_typeset.hip: outline S = disk max of F, r <= 12,
// pixel = blend(blend(P, s, S), f, F).  Integers only.  The tile, the outline and the blend are typeset_tile.h's, shared
// with kernels_typeset.hip; the walk over the tile's entries in groups of equal layer and chunks of NC, the staging and the
// gather are glyph_walk.h's, shared with kernels_tilted.hip.
//
// glyphs_kernel, ONE launch, one workgroup of 256 threads per row of the tile table (a TILE_W x TILE_H tile of one page):
// load the tile into registers, walk the groups, store the tile once.  This file's own, per group:
//   box     the stage drops a record whose rectangle, grown by its layer's r and cut to page, clip and tile, is empty, and
//           the bounding box of the others (LDS atomicMin/Max a chunk, ax1 .. ay2 over the chunks) is what the group can write
//           in this tile: the rows pass, the blend and the counts run on it, and a group without one is passed over.
//   patch   the gather's bytes are the visible patch rows of `cov`, byte i at row pr1 + i / CW, column i % CW, kept packed as
//           row * 128 + column; a byte outside the chunk's box grown by r is written (0 in the first chunk) but not scanned,
//           and a chunk without a box scans nothing.  PB bytes a thread at a time: two batches cover the patch.
// LDS: 4928 (patch) + TS_PLANES * 3584 (planes / staged records) + small tables.
#include "glyph_walk.h"

namespace {

constexpr int PB = 11;                                     // patch bytes a thread resolves at a time: CH * CW <= 2 PB threads
static_assert(CH * CW <= 2 * PB * TS_THREADS && CW <= 128, "two batches cover the patch; a patch column fits 7 bits");
static_assert(sizeof(ctd_glyph_layer) == 32 && sizeof(ctd_glyph_place) == 16 && sizeof(ctd_glyph_record) == 16 &&
              sizeof(ctd_glyph_params) == 32, "glyph typeset ABI sizes (glyphs.py dtypes)");
static_assert(offsetof(ctd_glyph_layer, clip) == 4 && offsetof(ctd_glyph_layer, fill) == 20 &&
              offsetof(ctd_glyph_layer, radius) == 26 && offsetof(ctd_glyph_record, w) == 8 &&
              offsetof(ctd_glyph_params, n_places) == 16 && offsetof(ctd_glyph_params, atlas_bytes) == 24,
              "glyph typeset ABI offsets");

struct PatchRows {                                         // gather's box: the visible patch rows, origin (px0, py0) = ox, oy
  using Addr = int;                                        // row * 128 + column
  unsigned char (*cov)[CW];
  int pr1, n_bytes, ox, oy;
  int ux1, uy1, ux2, uy2;                                  // the chunk's box grown by r, patch coordinates; none: empty
  bool any;
  __device__ int locate(int i) const { return (pr1 + i / CW) * 128 + i % CW; }
  __device__ int x(int a) const { return a & 127; }
  __device__ int y(int a) const { return a >> 7; }
  __device__ int state(int a) const { return x(a) >= ux1 && x(a) < ux2 && y(a) >= uy1 && y(a) < uy2 ? -1 : -3; }
  __device__ bool scan() const { return any; }
  __device__ void corner(const Staged& g, int& gx0, int& gy0) const { gx0 = g.x - ox, gy0 = g.y - oy; }
  __device__ unsigned char& byte(int a) const { return cov[y(a)][x(a)]; }
};

__global__ __launch_bounds__(TS_THREADS) void glyphs_kernel(const ctd_typeset_page* __restrict__ pages,
                                                            const ctd_glyph_layer* __restrict__ layers,
                                                            const ctd_glyph_place* __restrict__ places,
                                                            const ctd_glyph_record* __restrict__ glyphs,
                                                            const ctd_typeset_tile* __restrict__ tiles,
                                                            const int* __restrict__ entries,
                                                            const unsigned char* __restrict__ atlas, ctd_glyph_params prm,
                                                            ctd_typeset_row* __restrict__ rows) {
  __shared__ unsigned char cov[CH][CW];                    // F on the tile grown by r; patch (0, 0) is tile (-r, -r)
  // running horizontal maxima, one plane a distinct half-width; before the rows pass: the staged records of the chunk
  __shared__ __attribute__((aligned(16))) unsigned char plane_raw[TS_PLANES * CH * TW];
  __shared__ signed char slot[RMAX + 1];                   // half-width k -> its plane, -1: no row of the disk has it
  __shared__ signed char slot_dy[RMAX + 1];                // |dy| -> the plane of its half-width
  __shared__ int s_li;                                     // the group's layer, -1: its first entry names none
  __shared__ ctd_glyph_layer s_layer;                      // ... and its row of the layer table
  __shared__ int s_len;                                    // the group's entries within the chunk
  __shared__ int s_box[4];                                 // what the chunk's glyphs, grown by r, can write in this tile
  unsigned char(*plane)[CH][TW] = reinterpret_cast<unsigned char(*)[CH][TW]>(plane_raw);
  Staged* staged = reinterpret_cast<Staged*>(plane_raw);
  const int t = threadIdx.x;

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
    int n_bytes = 0;
    int ax1 = INT_MAX, ay1 = INT_MAX, ax2 = INT_MIN, ay2 = INT_MIN;     // the group's box, over its chunks
    bool first_chunk = true, more = true;
    while (more) {
      const int n = min(e_end - e, NC);
      __syncthreads();                                     // the group before is done with cov, planes, slots and s_*

      // ---- stage; what the glyph, grown by r, can write of this tile (page, clip, the tile), none: it is dropped
      int bx1 = 0, by1 = 0, bx2 = 0, by2 = 0;
      Staged sg;
      const auto in_tile = [&](const ctd_glyph_place& pl, const ctd_glyph_record& g, const ctd_glyph_layer& Lt) {
        const int rt = Lt.radius;
        bx1 = max(pl.x - rt, max(Lt.clip[0], tx0)), by1 = max(pl.y - rt, max(Lt.clip[1], ty0));
        bx2 = min(pl.x + g.w + rt, min(Lt.clip[2], min(tx0 + TW, P.W)));
        by2 = min(pl.y + g.h + rt, min(Lt.clip[3], min(ty0 + TH, P.H)));
        return bx1 < bx2 && by1 < by2;
      };
      const int lay = stage_entry(layers, places, glyphs, entries, prm, T.page, e, n, t, first_chunk, staged, &s_layer, &s_li, &s_len, sg,
                                  in_tile);
      if (t == 0) s_box[0] = s_box[1] = INT_MAX, s_box[2] = s_box[3] = INT_MIN;
      __syncthreads();
      if (first_chunk) {
        if (!group_layer(s_li, s_layer, T.page, P, tx0, ty0, t, slot, slot_dy, G)) break;
        n_bytes = (G.cy2 - G.cy1 + 2 * G.r) * CW;
      }
      run_length(t < n && lay != G.li, t, &s_len);
      if (lay == G.li && sg.w > 0)
        atomicMin(&s_box[0], bx1), atomicMin(&s_box[1], by1), atomicMax(&s_box[2], bx2), atomicMax(&s_box[3], by2);
      __syncthreads();
      const int len = s_len;                               // >= 1 in the first chunk: entry e is of layer li
      const int qx1 = s_box[0], qy1 = s_box[1], qx2 = s_box[2], qy2 = s_box[3];

      // ---- patch: this thread's bytes of the visible rows, the max over the staged glyphs that cover them
      const bool any = qx1 < qx2;
      gather<PB>(PatchRows{cov, G.pr1, n_bytes, G.px0, G.py0, any ? qx1 - G.r - G.px0 : 0, any ? qy1 - G.r - G.py0 : 0,
                           any ? qx2 + G.r - G.px0 : 0, any ? qy2 + G.r - G.py0 : 0, any}, staged, len, atlas, first_chunk, t);
      if (any) ax1 = min(ax1, qx1), ay1 = min(ay1, qy1), ax2 = max(ax2, qx2), ay2 = max(ay2, qy2);
      e += len;
      more = len == n && n == NC && e < e_end;             // the chunk was all of this layer: it may go on
      first_chunk = false;
    }
    if (first_chunk) { ++e; continue; }                    // left by a break: nothing of entry e can be drawn here
    if (ax1 >= ax2 || ay1 >= ay2) continue;                // nothing of the group can write here

    __syncthreads();                                       // cov is whole; the staged records are done with
    const int r = G.r, rr1 = ay1 - ty0, rr2 = ay2 - ty0 + 2 * r;   // the patch rows an active pixel can see (within pr1 ..)
    if (r > 0) {
      rows_pass(cov, plane, slot, r, rr1, rr2, t);
      __syncthreads();                                     // the planes are whole
    }
    const ctd_glyph_layer Ly = s_layer;                    // s_layer is next written behind the next group's first barrier
    blend_count(r, ax1, ay1, ax2, ay2, Ly.fill, Ly.stroke, cov, plane, slot_dy, tx0, ty0, t, pix, rows, G.li);
  }

  store_tile(P, tx0, ty0, t, pix);
}

}  // namespace

hipError_t launch_typeset_glyphs(const ctd_typeset_page* pages, const ctd_glyph_layer* layers, const ctd_glyph_place* places,
                                 const ctd_glyph_record* glyphs, const ctd_typeset_tile* tiles, const int32_t* entries,
                                 const uint8_t* atlas, const ctd_glyph_params& prm, ctd_typeset_row* rows, hipStream_t st) {
  hipLaunchKernelGGL(glyphs_kernel, dim3(prm.n_tiles), dim3(TS_THREADS), 0, st, pages, layers, places, glyphs, tiles, entries,
                     atlas, prm, rows);
  return hipGetLastError();
}
