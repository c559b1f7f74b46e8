// Typeset from a glyph atlas (`ctd_typeset_glyphs`; the rule is stated in include/ctd_hip.h and restated in numpy in
// tests/glyph_ref.py): a layer is a run of placements (layer, glyph, x, y) of atlas glyphs, its coverage F the MAX of the
// glyphs' coverage, and from there on the typeset rule of kernels_typeset.hip: outline S = disk max of F, r <= 12,
// pixel = blend(blend(P, s, S), f, F).  Integers only.  The tile, the outline and the blend are typeset_tile.h's, shared
// with kernels_typeset.hip; staging the placements and gathering the patch are this file's.
//
// glyphs_kernel, ONE launch, one workgroup of 256 threads per row of the tile table (a TILE_W x TILE_H tile of one page):
//   load    the tile of the page into registers, as typeset_kernel does.
//   groups  the tile's entries are placement indices, ascending, so the placements of a layer are consecutive.  The workgroup
//           walks them and takes consecutive entries of equal layer as one group, every decision block-uniform.  Per group:
//     stage   up to NC entries at a time, one a thread: the placement, its glyph record and its OWN layer's row are read and
//             checked (every index before use; the record against atlas_bytes; no load waits for the group's layer to be
//             known) and a compact record (off, x, y, w, h; w = 0: contributes nothing) goes to LDS, into the bytes of the
//             planes, which are idle until the rows pass.  The group's layer is its first entry's.  Its length within the
//             chunk (the first entry of another layer, by ballot + LDS atomicMin) and the bounding box of what the group's
//             glyphs, grown by r, can write in this tile (LDS atomicMin/Max) come out of the same pass.
//     patch   GATHER, not scatter: a thread owns patch bytes (byte i = t + 256 k of the visible patch rows) and takes the max
//             over the staged records that cover its byte, reading the atlas.  A patch byte has one writer whatever glyphs
//             overlap, so there is no barrier between glyphs and nothing to prove about their order; the first chunk
//             starts from 0 (that IS the zeroing), a later chunk of the same group from the byte's value.  PB bytes at a
//             time: first which glyph covers each (a scan of the staged records, registers and LDS only), then the PB atlas
//             loads together, one latency for all of them; bytes that two glyphs cover take the others one by one.
//     rows, blend, counts   as typeset_kernel, on the group's bounding box.
//   store   the tile, once.
// A group of more than NC placements takes several chunks: no cap on the glyphs of a tile or of a layer.
// LDS: 4928 (patch) + TS_PLANES * 3584 (planes / staged records) + small tables.
#include <climits>

#include "typeset_tile.h"

namespace {

constexpr int NC = TS_THREADS;                             // staged records a chunk: one a thread
constexpr int PB = 11;                                     // patch bytes a thread resolves at a time: CH * CW <= 2 PB threads
static_assert(CH * CW <= 2 * PB * TS_THREADS && CW <= 128, "two batches cover the patch; a patch column fits 7 bits");
constexpr int MAX_COORD = 1 << 29;
static_assert(sizeof(ctd_glyph_layer) == 32 && sizeof(ctd_glyph_place) == 16 && sizeof(ctd_glyph_record) == 16 &&
              sizeof(ctd_glyph_params) == 32, "glyph typeset ABI sizes (glyphs.py dtypes)");
static_assert(offsetof(ctd_glyph_layer, clip) == 4 && offsetof(ctd_glyph_layer, fill) == 20 &&
              offsetof(ctd_glyph_layer, radius) == 26 && offsetof(ctd_glyph_record, w) == 8 &&
              offsetof(ctd_glyph_params, n_places) == 16 && offsetof(ctd_glyph_params, atlas_bytes) == 24,
              "glyph typeset ABI offsets");

struct Staged {                                            // a checked placement; w == 0: contributes nothing
  long long off;
  int x, y, w, h;
};
static_assert(sizeof(Staged) == 24 && NC * sizeof(Staged) <= (size_t)TS_PLANES * CH * TW, "the staged records fit the planes");

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
    int li = -1, r = 0, cx1 = 0, cy1 = 0, cx2 = 0, cy2 = 0;             // the group's layer and what it may write of this tile
    int pr1 = 0, n_bytes = 0, px0 = 0, py0 = 0;
    int ax1 = INT_MAX, ay1 = INT_MAX, ax2 = INT_MIN, ay2 = INT_MIN;     // the group's box, over its chunks
    bool first_chunk = true, more = true;
    while (more) {
      const int n = min(e_end - e, NC);
      __syncthreads();                                     // the group before is done with cov, planes, slots and s_*

      // ---- stage: entry e + t, checked against its OWN layer, so that no load waits for the group's layer to be known
      int lay = -1, bx1 = 0, by1 = 0, bx2 = 0, by2 = 0;
      Staged sg = {0, 0, 0, 0, 0};
      if (t < n) {
        const int pi = entries[e + t];
        if (pi >= 0 && pi < prm.n_places) {
          const ctd_glyph_place pl = places[pi];
          if (pl.layer >= 0 && pl.layer < prm.n_layers) {
            lay = pl.layer;
            const ctd_glyph_layer* __restrict__ Lt = layers + lay;
            if (t == 0 && first_chunk) s_layer = *Lt;
            const int rt = Lt->radius;
            if (pl.glyph >= 0 && pl.glyph < prm.n_glyphs && pl.x >= -MAX_COORD && pl.x <= MAX_COORD && pl.y >= -MAX_COORD &&
                pl.y <= MAX_COORD && Lt->page == T.page && rt <= RMAX) {
              const ctd_glyph_record g = glyphs[pl.glyph];
              if (g.w >= 1 && g.h >= 1 && g.w <= CTD_TYPESET_MAX_SIDE && g.h <= CTD_TYPESET_MAX_SIDE && g.off >= 0 &&
                  g.off <= prm.atlas_bytes && (long long)g.w * g.h <= prm.atlas_bytes - g.off) {
                // what the glyph, grown by r, can write of this tile: page, clip, the tile
                bx1 = max(pl.x - rt, max(Lt->clip[0], tx0)), by1 = max(pl.y - rt, max(Lt->clip[1], ty0));
                bx2 = min(pl.x + g.w + rt, min(Lt->clip[2], min(tx0 + TW, P.W)));
                by2 = min(pl.y + g.h + rt, min(Lt->clip[3], min(ty0 + TH, P.H)));
                if (bx1 < bx2 && by1 < by2) sg.off = g.off, sg.x = pl.x, sg.y = pl.y, sg.w = g.w, sg.h = g.h;
              }
            }
          }
        }
        staged[t] = sg;
      }
      if (t == 0) {
        if (first_chunk) s_li = lay;                       // s_layer: in the stage above, where lay names a layer
        s_len = n;
        s_box[0] = s_box[1] = INT_MAX, s_box[2] = s_box[3] = INT_MIN;
      }
      __syncthreads();
      if (first_chunk) {
        // the group's layer, from its first entry; an entry that names nothing, or a layer that cannot write here, is passed
        // over (block-uniform)
        li = s_li;
        if (li < 0) break;
        const ctd_glyph_layer Ly = s_layer;
        r = Ly.radius;
        cx1 = max(Ly.clip[0], tx0), cy1 = max(Ly.clip[1], ty0);
        cx2 = min(Ly.clip[2], min(tx0 + TW, P.W)), cy2 = min(Ly.clip[3], min(ty0 + TH, P.H));
        if (Ly.page != T.page || r > RMAX || cx1 >= cx2 || cy1 >= cy2) break;
        pr1 = cy1 - ty0;                                   // the patch rows a pixel of that rectangle can see: pr1 ..
        n_bytes = (cy2 - cy1 + 2 * r) * CW;
        px0 = tx0 - r, py0 = ty0 - r;                      // patch (0, 0) in page coordinates
        if (t == 0 && r > 0) slot_table(r, slot, slot_dy); // read behind the barriers below
      }
      // the group's length within the chunk: up to the first entry of another layer; its box
      const unsigned long long others = __ballot(t < n && lay != li);
      if (lane == 0 && others) atomicMin(&s_len, (t & ~63) + __ffsll((long long)others) - 1);
      if (lay == li && sg.w > 0)
        atomicMin(&s_box[0], bx1), atomicMin(&s_box[1], by1), atomicMax(&s_box[2], bx2), atomicMax(&s_box[3], by2);
      __syncthreads();
      const int len = s_len;                               // >= 1 in the first chunk: entry e is of layer li
      const int qx1 = s_box[0], qy1 = s_box[1], qx2 = s_box[2], qy2 = s_box[3];

      // ---- patch: this thread's bytes of the visible rows, PB at a time, the max over the staged glyphs that cover them
      const bool any = qx1 < qx2;                          // the box grown by r, patch coordinates; none: empty
      const int ux1 = any ? qx1 - r - px0 : 0, uy1 = any ? qy1 - r - py0 : 0;
      const int ux2 = any ? qx2 + r - px0 : 0, uy2 = any ? qy2 + r - py0 : 0;
      for (int base = 0; base < n_bytes; base += PB * TS_THREADS) {
        // which glyph covers each byte: the scan touches no global memory.  where[k]: the first such glyph, -1: none, -2: the
        // byte is not this thread's; bit k of `several`: a later one covers it too
        int where[PB], at[PB];
        unsigned several = 0;
#pragma unroll
        for (int k = 0; k < PB; ++k) {
          const int i = base + k * TS_THREADS + t;
          const int py = pr1 + i / CW, px = i % CW;
          at[k] = py * 128 + px;
          where[k] = i < n_bytes ? (px >= ux1 && px < ux2 && py >= uy1 && py < uy2 ? -1 : -3) : -2;
        }
        if (any) {
          for (int j = 0; j < len; ++j) {
            const Staged g = staged[j];
            if (g.w == 0) continue;
            const int gx0 = g.x - px0, gy0 = g.y - py0;    // the glyph in patch coordinates
#pragma unroll
            for (int k = 0; k < PB; ++k) {
              const bool in = (unsigned)((at[k] & 127) - gx0) < (unsigned)g.w && (unsigned)((at[k] >> 7) - gy0) < (unsigned)g.h;
              if (in && where[k] >= 0) several |= 1u << k;
              if (in && where[k] == -1) where[k] = j;
            }
          }
        }
        // the loads, all in flight together
        int val[PB];
#pragma unroll
        for (int k = 0; k < PB; ++k) {
          val[k] = 0;
          if (where[k] >= 0) {
            const Staged g = staged[where[k]];
            val[k] = atlas[g.off + (long long)((at[k] >> 7) + py0 - g.y) * g.w + ((at[k] & 127) + px0 - g.x)];
          }
        }
#pragma unroll
        for (int k = 0; k < PB; ++k) {
          if (where[k] == -2) continue;
          const int py = at[k] >> 7, px = at[k] & 127;
          int v = val[k];
          if ((several >> k) & 1) {                        // glyphs of the layer overlap here: the rest of them, one by one
            for (int j = where[k] + 1; j < len; ++j) {
              const Staged g = staged[j];
              const int bx = px + px0 - g.x, by = py + py0 - g.y;
              if (bx >= 0 && bx < g.w && by >= 0 && by < g.h) v = max(v, (int)atlas[g.off + (long long)by * g.w + bx]);
            }
          }
          cov[py][px] = (unsigned char)(first_chunk ? v : max(v, (int)cov[py][px]));
        }
      }
      if (qx1 < qx2) ax1 = min(ax1, qx1), ay1 = min(ay1, qy1), ax2 = max(ax2, qx2), ay2 = max(ay2, qy2);
      e += len;
      more = len == n && n == NC && e < e_end;             // the chunk was all of this layer: it may go on
      first_chunk = false;
    }
    if (first_chunk) { ++e; continue; }                    // left by a break: nothing of entry e can be drawn here
    if (ax1 >= ax2 || ay1 >= ay2) continue;                // nothing of the group can write here

    __syncthreads();                                       // cov is whole; the staged records are done with
    const int rr1 = ay1 - ty0, rr2 = ay2 - ty0 + 2 * r;    // the patch rows an active pixel can see (within pr1 ..)
    if (r > 0) {
      rows_pass(cov, plane, slot, r, rr1, rr2, t);
      __syncthreads();                                     // the planes are whole
    }
    const ctd_glyph_layer Ly = s_layer;                    // s_layer is next written behind the next group's first barrier
    blend_count(r, ax1, ay1, ax2, ay2, Ly.fill, Ly.stroke, cov, plane, slot_dy, tx0, ty0, t, pix, rows, li);
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
