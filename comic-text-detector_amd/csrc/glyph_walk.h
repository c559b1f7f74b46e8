// The walk over a tile's glyph entries that glyphs_kernel (kernels_glyphs.hip) and tilted_kernel (kernels_tilted.hip) share.
// The entries of a tile are placement indices, ascending, so the placements of a layer are consecutive: the workgroup takes
// consecutive entries of equal layer as one GROUP, NC entries (a CHUNK) at a time, every decision block-uniform, with no cap
// on the glyphs of a tile or of a layer.  A kernel's chunk reads: barrier; stage_entry; barrier; in the first chunk
// group_layer (false: `break`, and `++e` behind the loop); run_length; barrier; len = s_len; gather into the kernel's own box
// of bytes; e += len, more = len == n && n == NC && e < e_end.  The kernels differ in that box (the patch rows of `cov`, the
// frame box `ubuf`), which a policy struct describes to gather, and in what they do with it afterwards.  Device code only.
//
// As in typeset_tile.h no helper holds a barrier, each states what it reads and writes of LDS, and the helpers take plain
// values and pointers; the layer struct is a template parameter: ctd_glyph_layer and ctd_tilt_layer have page, clip, fill,
// stroke and radius at the same offsets (each kernel asserts its own).
#pragma once
#include <climits>

#include "typeset_tile.h"

namespace {

constexpr int NC = TS_THREADS;                             // staged records a chunk: one a thread
constexpr int MAX_COORD = 1 << 29;

struct Staged {                                            // a checked placement; w == 0: contributes nothing
  long long off;
  int x, y, w, h;
};
static_assert(sizeof(Staged) == 24 && NC * sizeof(Staged) <= (size_t)TS_PLANES * CH * TW, "the staged records fit the planes");

struct KeepAll {                                           // stage_entry's default hook: no record is dropped
  template <class... A> __device__ bool operator()(const A&...) const { return true; }
};

// Stage entry e + t of a chunk of n: the placement, its glyph record and its OWN layer's row are read and checked (every
// index before use; the record against atlas_bytes; no load waits for the group's layer to be known).  sg: the compact record,
// all 0 where the entry contributes nothing or keep(placement, record, layer row) says so.  Returns the entry's layer, -1: it
// names none.  Writes staged[t] (t < n, into the bytes of the planes, idle until the rows pass); thread 0 writes *s_len = n and
// in the first chunk *s_li, the group's layer, and *s_layer, its row (where s_li >= 0).  Reads no LDS.
template <class Layer, class Keep = KeepAll>
__device__ __forceinline__ int stage_entry(const Layer* __restrict__ layers, const ctd_glyph_place* __restrict__ places,
                                           const ctd_glyph_record* __restrict__ glyphs, const int* __restrict__ entries,
                                           const ctd_glyph_params& prm, int page, int e, int n, int t, bool first_chunk,
                                           Staged* staged, Layer* s_layer, int* s_li, int* s_len, Staged& sg, Keep keep = Keep()) {
  int lay = -1;
  sg = {0, 0, 0, 0, 0};
  if (t < n) {
    const int pi = entries[e + t];
    if (pi >= 0 && pi < prm.n_places) {
      const ctd_glyph_place pl = places[pi];
      if (pl.layer >= 0 && pl.layer < prm.n_layers) {
        lay = pl.layer;
        const Layer* __restrict__ Lt = layers + lay;
        if (t == 0 && first_chunk) *s_layer = *Lt;
        if (pl.glyph >= 0 && pl.glyph < prm.n_glyphs && pl.x >= -MAX_COORD && pl.x <= MAX_COORD && pl.y >= -MAX_COORD &&
            pl.y <= MAX_COORD && Lt->page == page && Lt->radius <= RMAX) {
          const ctd_glyph_record g = glyphs[pl.glyph];
          if (g.w >= 1 && g.h >= 1 && g.w <= CTD_TYPESET_MAX_SIDE && g.h <= CTD_TYPESET_MAX_SIDE && g.off >= 0 &&
              g.off <= prm.atlas_bytes && (long long)g.w * g.h <= prm.atlas_bytes - g.off && keep(pl, g, *Lt))
            sg.off = g.off, sg.x = pl.x, sg.y = pl.y, sg.w = g.w, sg.h = g.h;
        }
      }
    }
    staged[t] = sg;
  }
  if (t == 0 && first_chunk) *s_li = lay;
  if (t == 0) *s_len = n;
  return lay;
}

struct Group {                                             // a group's layer and what it may write of this tile
  int li = -1, r = 0;
  int cx1 = 0, cy1 = 0, cx2 = 0, cy2 = 0;                  // its clip cut to the tile and the page
  int pr1 = 0, px0 = 0, py0 = 0;                           // the patch rows that rectangle can see: pr1 ..; patch (0, 0) on the page
};

// The group's layer, from its first entry (li = s_li, Ly = s_layer, both read by the caller behind a barrier).  false: the entry
// names nothing, or the layer cannot write here, and is passed over (block-uniform).  Thread 0 writes the slot tables of r > 0,
// read behind the caller's later barriers.
template <class Layer>
__device__ __forceinline__ bool group_layer(int li, const Layer& Ly, int page, const ctd_typeset_page& P, int tx0, int ty0, int t,
                                            signed char* slot, signed char* slot_dy, Group& G) {
  G.li = li;
  if (li < 0) return false;
  G.r = Ly.radius;
  G.cx1 = max(Ly.clip[0], tx0), G.cy1 = max(Ly.clip[1], ty0);
  G.cx2 = min(Ly.clip[2], min(tx0 + TW, P.W)), G.cy2 = min(Ly.clip[3], min(ty0 + TH, P.H));
  if (Ly.page != page || G.r > RMAX || G.cx1 >= G.cx2 || G.cy1 >= G.cy2) return false;
  G.pr1 = G.cy1 - ty0;
  G.px0 = tx0 - G.r, G.py0 = ty0 - G.r;
  if (t == 0 && G.r > 0) slot_table(G.r, slot, slot_dy);
  return true;
}

// The group's length within the chunk: *s_len (n from stage_entry, behind a barrier) down to the first entry whose thread says
// `other` (t < n and another layer), by one ballot a wave and an LDS atomicMin.  All threads.
__device__ __forceinline__ void run_length(bool other, int t, int* s_len) {
  const unsigned long long others = __ballot(other);
  if ((t & 63) == 0 && others) atomicMin(s_len, (t & ~63) + __ffsll((long long)others) - 1);
}

// GATHER, not scatter: a thread owns bytes of the box (byte i = base + t + 256 k) and takes the max over the staged records
// [0, len) that cover its byte, reading the atlas.  A byte has one writer whatever glyphs overlap, so there is no barrier
// between glyphs and nothing to prove about their order; the first chunk starts from 0 (that IS the zeroing), a later chunk of
// the same group from the byte's value.  PB bytes at a time: first which glyph covers each (a scan of the staged records,
// registers and LDS only), then the PB atlas loads together, one latency for all of them; bytes that two glyphs cover take the
// others one by one.  Reads staged, reads and writes the box's bytes.  The box `B` gives:
//   n_bytes; Addr locate(i), x(a), y(a): byte i's place in the box; byte(a): the byte itself
//   state(a): -1, or -3: written (0 in the first chunk) but not scanned; scan(): false skips the scan, every byte then keeps -1 / -3
//   ox, oy: the box's origin in the glyphs' coordinates (int or long long); corner(g, gx0, gy0): g's corner in the box
template <int PB, class Box>
__device__ __forceinline__ void gather(const Box& B, const Staged* staged, int len, const unsigned char* __restrict__ atlas,
                                       bool first_chunk, int t) {
  for (int base = 0; base < B.n_bytes; base += PB * TS_THREADS) {
    int where[PB];                                         // the first glyph that covers byte k, -1: none, -2: not this thread's
    typename Box::Addr at[PB];
    unsigned several = 0;                                  // bit k: a later glyph covers byte k too
#pragma unroll
    for (int k = 0; k < PB; ++k) {
      const int i = base + k * TS_THREADS + t;
      at[k] = B.locate(i);
      where[k] = i < B.n_bytes ? B.state(at[k]) : -2;
    }
    if (B.scan()) {
      for (int j = 0; j < len; ++j) {
        const Staged g = staged[j];
        if (g.w == 0) continue;
        int gx0, gy0;                                      // the glyph in the box's coordinates
        B.corner(g, gx0, gy0);
#pragma unroll
        for (int k = 0; k < PB; ++k) {
          const bool in = (unsigned)(B.x(at[k]) - gx0) < (unsigned)g.w && (unsigned)(B.y(at[k]) - gy0) < (unsigned)g.h;
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
        val[k] = atlas[g.off + (long long)(B.y(at[k]) + B.oy - g.y) * g.w + (B.x(at[k]) + B.ox - g.x)];
      }
    }
#pragma unroll
    for (int k = 0; k < PB; ++k) {
      if (where[k] == -2) continue;
      int v = val[k];
      if ((several >> k) & 1) {                            // glyphs of the layer overlap here: the rest of them, one by one
        for (int j = where[k] + 1; j < len; ++j) {
          const Staged g = staged[j];
          const auto bx = B.x(at[k]) + B.ox - g.x, by = B.y(at[k]) + B.oy - g.y;
          if (bx >= 0 && bx < g.w && by >= 0 && by < g.h) v = max(v, (int)atlas[g.off + (long long)by * g.w + bx]);
        }
      }
      unsigned char& b = B.byte(at[k]);
      b = (unsigned char)(first_chunk ? v : max(v, (int)b));
    }
  }
}

}  // namespace
