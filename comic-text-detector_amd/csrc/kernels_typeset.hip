// Typeset (`ctd_typeset`; the rule is stated in include/ctd_hip.h and restated in numpy, layer by layer over whole pages,
// in tests/typeset_ref.py): pre-rendered 8-bit coverage bitmaps composited into the device pages with a fill colour and an
// outline, the outline being the grey-scale dilation S of the coverage F by a disk of radius r <= 12.  Integers only.
//
// typeset_kernel, ONE launch, one workgroup of 256 threads per row of the tile table (a TILE_W x TILE_H tile of one page).
// The tile, the outline and the blend are typeset_tile.h's, shared with kernels_glyphs.hip; the patch is this file's:
//   load    the tile of the page into registers, one packed pixel a register, PX pixels a thread.
//   layers  the tile's entries in table order, every decision block-uniform.  Per layer that is valid and meets the tile:
//     patch   F on the tile grown by r, zeros outside the bitmap, into LDS (cov, at most 56 rows of 88 bytes).
//     rows    the running horizontal maxima of the patch rows that an active pixel can see, into the half-width planes.
//     blend   S from the planes, 2 r + 1 byte reads, then blend(blend(P, s, S), f, F) in the register: about 70 LDS byte
//             reads a pixel at r = 12 where the plain disk takes 441.  r = 0 skips rows and the max.
//   store   the tile, once.
// A page byte is read once and written once whatever the number of layers; overlapping layers see each other's result in
// table order because one workgroup owns the tile.  The layer loop has no cap.  LDS: 4928 + TS_PLANES * 3584 bytes.
#include "typeset_tile.h"

namespace {

static_assert(sizeof(ctd_typeset_page) == 24 && sizeof(ctd_typeset_layer) == 56 && sizeof(ctd_typeset_tile) == 16 &&
              sizeof(ctd_typeset_params) == 32 && sizeof(ctd_typeset_row) == 8, "typeset ABI sizes (typeset.py dtypes)");
static_assert(offsetof(ctd_typeset_page, pitch) == 16 && offsetof(ctd_typeset_layer, page) == 8 &&
              offsetof(ctd_typeset_layer, cov_pitch) == 28 && offsetof(ctd_typeset_layer, clip) == 32 &&
              offsetof(ctd_typeset_layer, fill) == 48 && offsetof(ctd_typeset_layer, radius) == 54 &&
              offsetof(ctd_typeset_params, cov_bytes) == 16, "typeset ABI offsets");

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
  const int t = threadIdx.x;

  ctd_typeset_tile T;
  ctd_typeset_page P;
  int tx0, ty0, e_begin, e_end;
  if (!open_tile(tiles, pages, prm.n_pages, prm.n_entries, T, P, tx0, ty0, e_begin, e_end)) return;
  unsigned pix[PX];
  load_tile(P, tx0, ty0, t, pix);

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
    if (t == 0 && r > 0) slot_table(r, slot, slot_dy);
    __syncthreads();                                       // the patch and thread 0's slots are whole
    if (r > 0) {
      rows_pass(cov, plane, slot, r, pr1, pr2, t);
      __syncthreads();                                     // the planes are whole
    }
    blend_count(r, ax1, ay1, ax2, ay2, Ly.fill, Ly.stroke, cov, plane, slot_dy, tx0, ty0, t, pix, rows, li);
  }

  store_tile(P, tx0, ty0, t, pix);
}

}  // namespace

hipError_t launch_typeset(const ctd_typeset_page* pages, const ctd_typeset_layer* layers, const ctd_typeset_tile* tiles,
                          const int32_t* entries, const uint8_t* cov, const ctd_typeset_params& prm, ctd_typeset_row* rows,
                          hipStream_t st) {
  hipLaunchKernelGGL(typeset_kernel, dim3(prm.n_tiles), dim3(TS_THREADS), 0, st, pages, layers, tiles, entries, cov, prm, rows);
  return hipGetLastError();
}
