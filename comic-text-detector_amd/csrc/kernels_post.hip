// Post-processing kernels: class-aware greedy NMS and connected-component
// labelling with statistics (one union-find engine on row runs behind `launch_ccl`
// and `launch_ccl_dual`).  Integer / comparison work, HBM- and latency-bound.
#include <algorithm>
#include <cstdint>

#include "kernels.h"

// the big-grid kernels of the tail are launched with at most "tail_max_blocks" blocks and walk their tiles (tuning.def: why)

namespace {

// ===========================================================================
// NMS  (reference utils/yolov5_utils.py:124-218 `non_max_suppression`,
//       multi_label=False, agnostic=False; torchvision.ops.nms at :202)
// ===========================================================================
struct Cand {
  float x1, y1, x2, y2;  // un-offset xyxy
  float score;
  int cls;
  int idx;               // original row (tie-break: lower row first)
  int alive;
};

// stage 1: obj > conf (:136,155), conf = obj*cls (:171), best class (:181),
// conf > conf_thres (:182), xywh -> xyxy (:174, :220-227); compact per page.
__global__ void nms_filter_kernel(const float* __restrict__ blks, int B, int rows, int no, float conf_thres,
                                  Cand* __restrict__ cands, int* __restrict__ counts) {
  const long long total = (long long)B * rows;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / rows), r = (int)(i % rows);
    const float* x = blks + i * no;
    const float obj = x[4];
    if (!(obj > conf_thres)) continue;
    float best = x[5] * obj;
    int bj = 0;
    for (int j = 1; j < no - 5; ++j) {
      const float c = x[5 + j] * obj;
      if (c > best) { best = c; bj = j; }
    }
    if (!(best > conf_thres)) continue;
    const int pos = atomicAdd(&counts[b], 1);
    Cand c;
    c.x1 = x[0] - x[2] / 2;
    c.y1 = x[1] - x[3] / 2;
    c.x2 = x[0] + x[2] / 2;
    c.y2 = x[1] + x[3] / 2;
    c.score = best;
    c.cls = bj;
    c.idx = r;
    c.alive = 1;
    cands[(size_t)b * rows + pos] = c;
  }
}

struct Best { float s; int idx; int pos; };
constexpr int NMS_THREADS = 256;   // 4 waves: a round's two barriers and its 4-entry argmax cost a quarter of the 16-wave block's
constexpr int NMS_REG = 8;         // candidates a thread of nms_greedy_kernel keeps in registers (2048 per page)

__device__ __forceinline__ bool better(const Best& a, const Best& b) {
  return a.s > b.s || (a.s == b.s && a.idx < b.idx);
}

__device__ __forceinline__ Best block_argmax(Best v, Best* sh) {
  for (int off = 32; off > 0; off >>= 1) {
    Best o;
    o.s = __shfl_down(v.s, off);
    o.idx = __shfl_down(v.idx, off);
    o.pos = __shfl_down(v.pos, off);
    if (better(o, v)) v = o;
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  Best r = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i)
    if (better(sh[i], r)) r = sh[i];
  return r;
}

// stage 2: one block per page.  Greedy: repeatedly take the best alive candidate
// (score desc, row asc), suppress every alive candidate of IoU > thr computed on
// the class-offset boxes in fp32 exactly as torchvision's nms kernel does
// (ovr = inter / (iarea + area_j - inter), strict >), stop at max_det (:203-204).
__global__ __launch_bounds__(NMS_THREADS) void nms_greedy_kernel(Cand* __restrict__ cands_all, const int* __restrict__ counts,
                                                          int rows, float iou_thres, int max_det, int max_nms,
                                                          float max_wh, float* __restrict__ dets,
                                                          int* __restrict__ out_counts) {
  __shared__ Best sh[16];
  __shared__ unsigned cnt_sh;
  const int b = blockIdx.x;
  Cand* c = cands_all + (size_t)b * rows;
  const int n = counts[b];
  float* out = dets + (size_t)b * max_det * 6;

  // max_nms cap (:196-197): keep the max_nms highest scores (ties at the cut are all kept;
  // the reference's argsort leaves their order unspecified)
  if (n > max_nms) {
    unsigned prefix = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned trial = prefix | (1u << bit);
      if (threadIdx.x == 0) cnt_sh = 0;
      __syncthreads();
      unsigned local = 0;
      for (int j = threadIdx.x; j < n; j += blockDim.x) local += __float_as_uint(c[j].score) >= trial;
      atomicAdd(&cnt_sh, local);
      __syncthreads();
      if (cnt_sh >= (unsigned)max_nms) prefix = trial;
      __syncthreads();
    }
    for (int j = threadIdx.x; j < n; j += blockDim.x)
      if (__float_as_uint(c[j].score) < prefix) c[j].alive = 0;
    __syncthreads();
  }

  // Up to NMS_REG candidates per thread live in registers and the round's winner is handed round through LDS: a round
  // is then two barriers.  With the candidates in HBM every round was three dependent memory round trips (the winner, the
  // flags, the boxes) -- ~6 us a round, 0.19 ms for a page's ~30 kept boxes, on a block that fills a CU's wave slots.
  // Same comparisons and the same fp32 expressions on the same values, in the same order per pair.
  if (n <= NMS_REG * (int)blockDim.x) {
    __shared__ Cand ksh;
    Cand r[NMS_REG];
    Best mine{-1.f, 0x7fffffff, -1};
#pragma unroll
    for (int q = 0; q < NMS_REG; ++q) {
      const int j = threadIdx.x + q * blockDim.x;
      r[q].alive = 0;
      if (j < n) r[q] = c[j];
      if (r[q].alive) {
        Best t{r[q].score, r[q].idx, j};
        if (better(t, mine)) mine = t;
      }
    }
    int kept = 0;
    while (kept < max_det) {
      const Best top = block_argmax(mine, sh);
      if (top.pos < 0) break;
#pragma unroll
      for (int q = 0; q < NMS_REG; ++q)
        if (top.pos == (int)(threadIdx.x + q * blockDim.x)) ksh = r[q];
      __syncthreads();
      const Cand k = ksh;
      const float off = (float)k.cls * max_wh;
      const float ix1 = k.x1 + off, iy1 = k.y1 + off, ix2 = k.x2 + off, iy2 = k.y2 + off;
      const float iarea = (ix2 - ix1) * (iy2 - iy1);
      if (threadIdx.x == 0) {
        float* o = out + (size_t)kept * 6;
        o[0] = k.x1; o[1] = k.y1; o[2] = k.x2; o[3] = k.y2; o[4] = k.score; o[5] = (float)k.cls;
      }
      ++kept;
      mine = Best{-1.f, 0x7fffffff, -1};
#pragma unroll
      for (int q = 0; q < NMS_REG; ++q) {
        const int j = threadIdx.x + q * blockDim.x;
        if (!r[q].alive) continue;
        if (j == top.pos) { r[q].alive = 0; continue; }
        const float o2 = (float)r[q].cls * max_wh;
        const float jx1 = r[q].x1 + o2, jy1 = r[q].y1 + o2, jx2 = r[q].x2 + o2, jy2 = r[q].y2 + o2;
        const float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1);
        const float xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
        const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
        const float inter = w * h;
        const float ovr = inter / (iarea + (jx2 - jx1) * (jy2 - jy1) - inter);
        if (ovr > iou_thres) { r[q].alive = 0; continue; }
        Best t{r[q].score, r[q].idx, j};
        if (better(t, mine)) mine = t;
      }
    }
    if (threadIdx.x == 0) out_counts[b] = kept;
    return;
  }

  Best mine{-1.f, 0x7fffffff, -1};
  for (int j = threadIdx.x; j < n; j += blockDim.x)
    if (c[j].alive) {
      Best t{c[j].score, c[j].idx, j};
      if (better(t, mine)) mine = t;
    }
  int kept = 0;
  while (kept < max_det) {
    const Best top = block_argmax(mine, sh);
    if (top.pos < 0) break;
    const Cand k = c[top.pos];
    const float off = (float)k.cls * max_wh;
    const float ix1 = k.x1 + off, iy1 = k.y1 + off, ix2 = k.x2 + off, iy2 = k.y2 + off;
    const float iarea = (ix2 - ix1) * (iy2 - iy1);
    if (threadIdx.x == 0) {
      float* o = out + (size_t)kept * 6;
      o[0] = k.x1; o[1] = k.y1; o[2] = k.x2; o[3] = k.y2; o[4] = k.score; o[5] = (float)k.cls;
    }
    ++kept;
    __syncthreads();
    mine = Best{-1.f, 0x7fffffff, -1};
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
      if (!c[j].alive) continue;
      if (j == top.pos) { c[j].alive = 0; continue; }
      const float o2 = (float)c[j].cls * max_wh;
      const float jx1 = c[j].x1 + o2, jy1 = c[j].y1 + o2, jx2 = c[j].x2 + o2, jy2 = c[j].y2 + o2;
      const float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1);
      const float xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
      const float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
      const float inter = w * h;
      const float ovr = inter / (iarea + (jx2 - jx1) * (jy2 - jy1) - inter);
      if (ovr > iou_thres) { c[j].alive = 0; continue; }
      Best t{c[j].score, c[j].idx, j};
      if (better(t, mine)) mine = t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out_counts[b] = kept;
}

// ===========================================================================
// CCL with stats (replaces cv2.connectedComponentsWithStats, reference
// utils/textmask.py:93,113,138, and the DB stage's two labellings).  ONE engine:
// a union-find over row runs with atomicMin links (root = the run that holds the
// component's first pixel in raster order), then the roots of a class are ranked
// in run order, so label ids follow the first-pixel order (OpenCV SAUF numbering
// for 4-connectivity).  `launch_ccl_dual` keeps both classes of its answer,
// `launch_ccl` one.  First the pieces both share with nothing else in between.
// ===========================================================================
// (agent scope: every thread that links or flattens a parent array runs on this GPU; the default system scope made each
// hop a load that bypasses the caches)
__device__ __forceinline__ int uf_load(const int* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int uf_find(int* parent, int x) {
  int p = uf_load(parent, x);
  while (p != x) {
    x = p;
    p = uf_load(parent, x);
  }
  return x;
}

__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + b, a);
    if (old == b) return;
    b = old;
  }
}

// the same on a table in LDS (a band's runs: no HBM atomics, no cross-CU traffic)
__device__ __forceinline__ int lds_find(int* lp, int x) {
  int p = __atomic_load_n(lp + x, __ATOMIC_RELAXED);
  while (p != x) {
    x = p;
    p = __atomic_load_n(lp + x, __ATOMIC_RELAXED);
  }
  return x;
}

__device__ __forceinline__ void lds_union(int* lp, int a, int b) {
  while (true) {
    a = lds_find(lp, a);
    b = lds_find(lp, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lp + b, a);
    if (old == b) return;
    b = old;
  }
}

constexpr int RK_CHUNK = 4096;  // runs flattened / ranked / spread per block
constexpr int RK_PER_T = RK_CHUNK / 256;

__device__ __forceinline__ int block_exclusive_scan(int v, int* sh, int* total) {
  // 256 threads
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  if (lane == 63) sh[w] = incl;
  __syncthreads();
  int base = 0;
  for (int i = 0; i < w; ++i) base += sh[i];
  *total = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return base + incl - v;
}

// rows of labels that exist (1..n, capped at max_labels) only: n is on the device by now
__global__ void ccl_stats_init_kernel(int* __restrict__ stats, const int* __restrict__ n_out, int max_labels, int H, int W) {
  const int b = blockIdx.y;
  const int n = min(n_out[b], max_labels);
  for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < n; l += gridDim.x * blockDim.x) {
    int* s = stats + ((size_t)b * max_labels + l) * 5;
    s[0] = W; s[1] = H; s[2] = -1; s[3] = -1; s[4] = 0;
  }
}

constexpr int LB_CHUNK = 8192;  // pixels painted per block
constexpr int LB_SLOTS = 128;   // labels a block aggregates in LDS before its statistics reach HBM

__global__ void ccl_stats_final_kernel(int* __restrict__ stats, const int* __restrict__ n_out, int max_labels) {
  const int b = blockIdx.y;
  const int n = min(n_out[b], max_labels);
  for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < n; l += gridDim.x * blockDim.x) {
    int* s = stats + ((size_t)b * max_labels + l) * 5;
    s[2] = s[2] - s[0] + 1;
    s[3] = s[3] - s[1] + 1;
  }
}

// ======================================================================================================
// Dual labelling: the 8-connected components of the FOREGROUND (img > thresh) and the 4-connected components
// of the BACKGROUND of one image in ONE union-find.  The DB stage needs both (cv2.findContours(RETR_LIST)
// yields a contour per foreground component and per enclosed background region); the two pixel sets are
// disjoint, so one parent array, one border merge, one flattening, one ranking sweep and one label pass serve
// both -- the two separate launches read and wrote every int32 plane twice.  Output: ONE signed label image
// (+id foreground, -id background, ids per class in raster order of the first pixel) and per-class stats.
//
// The union-find runs over ROW RUNS, not pixels.  A run is a maximal horizontal stretch of one class
// inside a row; a page of speckle has a tenth as many runs as pixels, a real page far fewer.  With the page as
// wp = ceil(W / 32) words per row:
//   bits[word]    bit i = pixel 32 * wx + i is foreground (0 beyond W)
//   starts[word]  bit i = that pixel starts a run: x == 0 or class(x) != class(x - 1) (0 beyond W)
//   base[word]    exclusive prefix sum of popcount(starts) over the page's words
//   run of bit i  base[word] + popcount(starts[word] & ((2u << i) - 1)) - 1   -- ids in raster order of the runs' first pixels
// Unions happen only between a row and the row above, group of set bits against group of set bits (8-connected for
// the foreground: one halo bit from each neighbouring word above; 4-connected for the background).  The smaller root
// wins, so a component's root is the run that holds its first pixel, and ranking the roots of each class in run order
// gives the ids of the per-pixel labelling.  Kernels, in launch order:
//   ccl2_pack          u8 -> bits, starts, the start count of every 128 words
//   ccl2_run_scan      base, and the page's run count R (stays on the device: every kernel over runs is sized for
//                      R <= H * W and exits on R)
//   ccl2_band          unions inside a band of RB_ROWS full-width rows in LDS, rparent[] and the class byte of every
//                      run; a band with more than RB_CAP runs does the same unions on rparent[] in global memory
//   ccl2_band_border   the same unions for rows 32k, k >= 1, on rparent[]   (full-width bands: no vertical borders)
//   ccl2_flatten_count / ccl2_scan_chunks / ccl2_rank / ccl2_spread         rlabel[run] = 2 * (+-id) + root, over runs
//   ccl2_label         paints the plane from base / starts / rlabel, once; statistics, first pixels, seg_live
// rparent[] lives in the label plane (R <= H * W) and is dead before the paint overwrites it.
//
// Single-class labelling (`launch_ccl`) is the same engine with half of its answer kept:
//   conn 8   the foreground class of the page as it is
//   conn 4   the BACKGROUND class of the flipped page (ccl2_pack sets a bit where (pixel > thresh) != flip): 4-connected,
//            ranked in raster order of first pixels
// Everything up to the paint runs on both classes as above; the other class's count goes to a scratch int of the
// workspace, and ccl2_label<KEEP> paints |id| on the kept class, the caller's background value on the other, and
// aggregates the kept class only.
// ======================================================================================================
// what the paint reads (all of it in the workspace)
struct RunTables {
  const unsigned* starts;              // (B, H, wp)
  const unsigned* base;                // (B, H, wp)
  const int* rlabel;                   // (B, H * W), the first R of a page in use: 2 * (+-id) + (the run is a root)
  int wp;
};
constexpr int RB_ROWS = 32;    // rows of a band: a row's word is 32 pixels, a band's words are 32 x 32 pixel tiles as before
constexpr int RB_THREADS = 1024;   // of a band's block: a 1024-wide band is 1024 words, one per thread and one round trip
constexpr int RB_CAP = 8192;   // runs a band's LDS table holds (32 KB).  The benchmark's 1024-wide speckle pages have at most
                               // 4 264 runs in a band (mean 3 000-3 500); alternating pixels have 32 768 and go through global memory.

// four pixels per thread, eight lanes per word; a virtual block is a segment of PK_SEG consecutive words of one page and
// leaves the segment's number of starts for the scan.  flip: the classes change places, a bit is set where
// (pixel > thresh) != flip (launch_ccl's 4-connected labelling; the dual call passes none)
constexpr int PK_U = 4;   // steps of 256 groups = 32 words each per virtual block: all their loads first
constexpr int PK_SEG = 32 * PK_U;
__device__ __forceinline__ void ccl2_pack_body(int vb, const uint8_t* __restrict__ img, unsigned* __restrict__ bits_all,
                                                        unsigned* __restrict__ starts_all, int* __restrict__ segsum, int nseg, int H,
                                                        int W, int wp, int thresh, int flip, int aligned4) {
  __shared__ int segc;
  const int nw = H * wp;
  const size_t hw = (size_t)H * W;
  const int b = vb / nseg, seg = vb - b * nseg;
  if (threadIdx.x == 0) segc = 0;
  __syncthreads();
  unsigned px[PK_U];
  int prev[PK_U], xs[PK_U], ws[PK_U];
#pragma unroll
  for (int u = 0; u < PK_U; ++u) {
    const int g = (int)threadIdx.x;                                       // group of 4 pixels of the padded rows
    const int rem = seg * PK_SEG + u * 32 + (g >> 3);                     // word of the page
    const bool valid = rem < nw;
    const int y = valid ? rem / wp : 0, wx = valid ? rem - y * wp : 0;
    const int x = wx * 32 + 4 * (g & 7);
    const uint8_t* row = img + (size_t)b * hw + (size_t)y * W;
    unsigned v = 0;
    if (valid && x < W) {
      if (aligned4) {
        v = *reinterpret_cast<const unsigned*>(row + x);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (x + k < W) v |= (unsigned)row[x + k] << (8 * k);
      }
    }
    px[u] = v;
    prev[u] = (valid && ((int)g & 7) == 0 && wx > 0) ? (int)row[x - 1] : -1;   // the left word's last pixel
    xs[u] = x;
    ws[u] = valid ? rem : -1;
  }
  unsigned* bits = bits_all + (size_t)b * nw;
  unsigned* starts = starts_all + (size_t)b * nw;
  int nstart = 0;
#pragma unroll
  for (int u = 0; u < PK_U; ++u) {
    const int x = xs[u];
    unsigned nib = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < W && ((int)((px[u] >> (8 * k)) & 255u) > thresh) != (flip != 0)) nib |= 1u << k;
    unsigned v = nib << (4 * (threadIdx.x & 7));
    v |= __shfl_xor(v, 1);
    v |= __shfl_xor(v, 2);
    v |= __shfl_xor(v, 4);
    if ((threadIdx.x & 7) == 0 && ws[u] >= 0) {
      const int nbit = min(32, W - x);                                  // x = the word's first pixel here
      const unsigned vmask = nbit >= 32 ? 0xffffffffu : ((1u << nbit) - 1u);
      const unsigned pb = prev[u] >= 0 ? ((prev[u] > thresh) != (flip != 0) ? 1u : 0u) : (~v & 1u);   // x == 0 always starts a run
      const unsigned s = (v ^ ((v << 1) | pb)) & vmask;
      bits[ws[u]] = v;
      starts[ws[u]] = s;
      nstart += __popc(s);
    }
  }
  if (nstart) atomicAdd(&segc, nstart);                                   // LDS: the 32 word owners of the block
  __syncthreads();
  if (threadIdx.x == 0) segsum[vb] = segc;
}
__global__ __launch_bounds__(256) void ccl2_pack_kernel(const uint8_t* __restrict__ img, unsigned* __restrict__ bits_all,
                                                        unsigned* __restrict__ starts_all, int* __restrict__ segsum, int nseg, int H,
                                                        int W, int wp, int thresh, int flip, int aligned4, int nvb) {
  for (int vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
    ccl2_pack_body(vb, img, bits_all, starts_all, segsum, nseg, H, W, wp, thresh, flip, aligned4);
    __syncthreads();
  }
}

// base[]: a block scans one tile of SC_TILE words of one page, 16 consecutive words per thread in one round trip; what
// lies before the tile is the sum of the pack's segment counts before it.  The block of a page's last tile leaves the
// page's run count.  (One block per page and a sweep over its words was 44 us for eight pages: eight blocks, nothing to
// hide a round trip behind.)
constexpr int SC_TILE = 4096;
static_assert(SC_TILE % PK_SEG == 0 && SC_TILE == 256 * 16, "whole segments; 16 words per thread");
__device__ __forceinline__ void ccl2_run_scan_body(int vb, const unsigned* __restrict__ starts_all, const int* __restrict__ segsum,
                                                            unsigned* __restrict__ base_all, int* __restrict__ rcount, int nw, int nseg,
                                                            int ntiles) {
  __shared__ int sh[4];
  const int b = vb / ntiles, tile = vb - b * ntiles;
  const unsigned* starts = starts_all + (size_t)b * nw;
  unsigned* base = base_all + (size_t)b * nw;
  const int i0 = tile * SC_TILE + 16 * (int)threadIdx.x;
  unsigned sv[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) sv[k] = i0 + k < nw ? starts[i0 + k] : 0u;
  int before = 0;
  for (int i = threadIdx.x; i < tile * (SC_TILE / PK_SEG); i += 256) before += segsum[(size_t)b * nseg + i];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) mine += __popc(sv[k]);
  int prefix, total;
  block_exclusive_scan(before, sh, &prefix);                // only its total: the starts before this tile
  int e = prefix + block_exclusive_scan(mine, sh, &total);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (i0 + k < nw) base[i0 + k] = (unsigned)e;
    e += __popc(sv[k]);
  }
  if (tile == ntiles - 1 && threadIdx.x == 0) rcount[b] = prefix + total;
}
__global__ __launch_bounds__(256) void ccl2_run_scan_kernel(const unsigned* __restrict__ starts_all, const int* __restrict__ segsum,
                                                            unsigned* __restrict__ base_all, int* __restrict__ rcount, int nw, int nseg,
                                                            int ntiles, int nvb) {
  for (int vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
    ccl2_run_scan_body(vb, starts_all, segsum, base_all, rcount, nw, nseg, ntiles);
    __syncthreads();
  }
}

// The unions of word (y, wx), y >= 1, with the row above: every group of set bits of either class against every group of
// the same class above that it touches, one union per pair.  `unite(a, b)` gets two run ids of the page.
template <class U>
__device__ __forceinline__ void ccl2_word_unions(const unsigned* __restrict__ bits, const unsigned* __restrict__ starts,
                                                          const unsigned* __restrict__ base, int y, int wx, int wp, int W, U&& unite) {
  const int w = y * wp + wx, wa = w - wp;
  const bool hl = wx > 0, hr = wx + 1 < wp;
  // every load first (the halo words of the foreground too), their use after
  const unsigned c = bits[w], sc = starts[w], a = bits[wa], sa = starts[wa];
  const int bc = (int)base[w], ba = (int)base[wa];
  const unsigned al = hl ? bits[wa - 1] : 0u, sal = hl ? starts[wa - 1] : 0u;
  const int bal = hl ? (int)base[wa - 1] : 0;
  const unsigned ar = hr ? bits[wa + 1] : 0u, sar = hr ? starts[wa + 1] : 0u;
  const int bar = hr ? (int)base[wa + 1] : 0;
  const int nbit = min(32, W - 32 * wx);
  const unsigned vmask = nbit >= 32 ? 0xffffffffu : ((1u << nbit) - 1u);
#pragma unroll
  for (int cls = 0; cls < 2; ++cls) {                       // 1 = foreground
    const unsigned m = (cls ? c : ~c) & vmask, ma = (cls ? a : ~a) & vmask;
    unsigned rest = m;
    while (rest) {
      const int lo = __ffs(rest) - 1;
      const unsigned from = m >> lo;
      const int len = (~from) ? __ffs(~from) - 1 : 32 - lo;
      const unsigned g = (len >= 32 ? 0xffffffffu : ((1u << len) - 1u)) << lo;
      rest &= ~g;
      const int me = bc + __popc(sc & ((2u << lo) - 1u)) - 1;
      const bool cont = lo == 0 && !(sc & 1u);              // my run began in an earlier word
      unsigned reach = g;
      if (cls) reach |= (g << 1) | (g >> 1);                // 8-connected: the diagonal neighbours above
      unsigned ov = ma & reach;
      while (ov) {
        const int bpos = __ffs(ov) - 1;
        // both runs come over from the word to the left: that word has united them
        if (!(cont && bpos == 0 && !(sa & 1u))) unite(me, ba + __popc(sa & ((2u << bpos) - 1u)) - 1);
        const unsigned froma = ma >> bpos;                  // clear the rest of that group above
        const int lena = (~froma) ? __ffs(~froma) - 1 : 32 - bpos;
        ov &= ~((lena >= 32 ? 0xffffffffu : ((1u << lena) - 1u)) << bpos);
      }
      if (cls) {                                            // the halo bits: last pixel of the word above-left, first of above-right
        if (lo == 0 && (al >> 31)) unite(me, bal + __popc(sal) - 1);
        if (lo + len == 32 && (ar & 1u)) unite(me, bar + (int)(sar & 1u) - 1);
      }
    }
  }
}

__device__ __forceinline__ void ccl2_band_body(int vb, const unsigned* __restrict__ bits_all, const unsigned* __restrict__ starts_all,
                                                        const unsigned* __restrict__ base_all, const int* __restrict__ rcount,
                                                        int* __restrict__ rparent_all, uint8_t* __restrict__ rcls_all, int H, int W,
                                                        int wp, int nbands) {
  __shared__ int lp[RB_CAP];
  const int b = vb / nbands, k = vb % nbands;
  const int y0 = k * RB_ROWS, y1 = min(H, y0 + RB_ROWS);
  const size_t nw = (size_t)H * wp, hw = (size_t)H * W;
  const unsigned* bits = bits_all + b * nw;
  const unsigned* starts = starts_all + b * nw;
  const unsigned* base = base_all + b * nw;
  int* rparent = rparent_all + b * hw;
  uint8_t* rcls = rcls_all + b * hw;
  // a band's runs are contiguous in id space: local id = id - gbase
  const int gbase = (int)base[y0 * wp];
  const int n = (y1 < H ? (int)base[y1 * wp] : rcount[b]) - gbase;
  const bool in_lds = n <= RB_CAP;                          // the same for the whole block
  if (in_lds) {
    for (int i = threadIdx.x; i < n; i += RB_THREADS) lp[i] = i;
  } else {
    for (int i = threadIdx.x; i < n; i += RB_THREADS) rparent[gbase + i] = gbase + i;
    __threadfence();
  }
  __syncthreads();
  for (int wi = y0 * wp + threadIdx.x; wi < y1 * wp; wi += RB_THREADS) {
    const int y = wi / wp, wx = wi - y * wp;
    unsigned s = starts[wi];
    const unsigned c = bits[wi];
    int id = (int)base[wi];
    while (s) {                                             // the class byte of every run that starts in this word
      const int pos = __ffs(s) - 1;
      s &= s - 1u;
      rcls[id++] = (uint8_t)((c >> pos) & 1u);
    }
    if (y == y0) continue;
    if (in_lds)
      ccl2_word_unions(bits, starts, base, y, wx, wp, W, [&](int p, int q) { lds_union(lp, p - gbase, q - gbase); });
    else
      ccl2_word_unions(bits, starts, base, y, wx, wp, W, [&](int p, int q) { uf_union(rparent, p, q); });
  }
  __syncthreads();
  if (in_lds)
    for (int i = threadIdx.x; i < n; i += RB_THREADS) rparent[gbase + i] = gbase + lds_find(lp, i);
}
// a block walks several bands: the launcher caps the grid (tail_max_blocks counts blocks of 256 threads) so that these
// kernels hold a few waves per SIMD next to the network, not all of them
__global__ __launch_bounds__(RB_THREADS) void ccl2_band_kernel(const unsigned* __restrict__ bits_all, const unsigned* __restrict__ starts_all,
                                                        const unsigned* __restrict__ base_all, const int* __restrict__ rcount,
                                                        int* __restrict__ rparent_all, uint8_t* __restrict__ rcls_all, int H, int W,
                                                        int wp, int nbands, int nvb) {
  for (int vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
    ccl2_band_body(vb, bits_all, starts_all, base_all, rcount, rparent_all, rcls_all, H, W, wp, nbands);
    __syncthreads();
  }
}

// rows y = RB_ROWS * k, k >= 1, with the last row of the band above: one thread per word
__global__ __launch_bounds__(256) void ccl2_band_border_kernel(const unsigned* __restrict__ bits_all,
                                                               const unsigned* __restrict__ starts_all,
                                                               const unsigned* __restrict__ base_all, int* __restrict__ rparent_all,
                                                               int B, int H, int W, int wp, int nbord) {
  int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= B * nbord * wp) return;
  const int wx = t % wp;
  t /= wp;
  const int k = t % nbord, b = t / nbord;
  const size_t nw = (size_t)H * wp;
  int* rparent = rparent_all + (size_t)b * H * W;
  ccl2_word_unions(bits_all + b * nw, starts_all + b * nw, base_all + b * nw, RB_ROWS * (k + 1), wx, wp, W,
                   [&](int p, int q) { uf_union(rparent, p, q); });
}

// Path flattening fused with pass 1 of the ranking, over the page's R runs: a block owns one chunk of RK_CHUNK runs,
// replaces every rparent[] by its root and counts the roots of the chunk per class (a run is a root iff it is its own
// parent; a chunk beyond R counts nothing).  It also leaves the chunk's root bitmaps: bit (r % 64) of word (r / 64) = run
// r is a root of that class.  The ranking numbers the roots from these words (8 B per 64 runs) instead of reading
// rparent[] again (256 B).
// chunk_cnt: (B, 2, nchunks) -- class 0 = foreground roots, 1 = background roots
__device__ __forceinline__ void ccl2_flatten_count_body(int vb, int* __restrict__ parent_all, const uint8_t* __restrict__ rcls_all,
                                                                 const int* __restrict__ rcount, int B, int hw, int nchunks,
                                                                 int* __restrict__ chunk_cnt, unsigned long long* __restrict__ rootmask) {
  __shared__ int sh[4];
  // chunk-major: the chunks that hold runs are the first few of every page, and a capped grid walks virtual blocks with a
  // stride -- page-major, the same few blocks got the live chunks of every page and the rest of the grid none
  const int b = vb % B, ch = vb / B;
  const int R = rcount[b];
  if (ch * RK_CHUNK >= R) {                     // the whole block
    if (threadIdx.x == 0) chunk_cnt[((size_t)b * 2 + 0) * nchunks + ch] = 0, chunk_cnt[((size_t)b * 2 + 1) * nchunks + ch] = 0;
    return;
  }
  int* parent = parent_all + (size_t)b * hw;
  const uint8_t* rcls = rcls_all + (size_t)b * hw;
  const int p0 = ch * RK_CHUNK + threadIdx.x;
  int lf = 0, lb = 0;
  // Four runs per thread at a time, hop by hop: the parents of all four, then the parents' parents of all four -- after
  // the band kernel nearly every run is a root or points at one, i.e. done after these two loads -- and only what is
  // left walks its chain alone.  One run at a time was a chain of 2-3 dependent loads, 16 times in a row.
  constexpr int FU = 4;
  static_assert(RK_PER_T % FU == 0, "whole batches");
  for (int j0 = 0; j0 < RK_PER_T; j0 += FU) {
    int v[FU], g[FU], px[FU];
#pragma unroll
    for (int j = 0; j < FU; ++j) {
      const int p = p0 + 256 * (j0 + j);
      v[j] = p < R ? uf_load(parent, p) : -1;   // every run has a class: parents are never negative
      px[j] = rcls[min(p, R - 1)];
    }
#pragma unroll
    for (int j = 0; j < FU; ++j) g[j] = v[j] >= 0 ? uf_load(parent, v[j]) : -1;
#pragma unroll
    for (int j = 0; j < FU; ++j) {
      const int p = p0 + 256 * (j0 + j);
      bool rf = false, rb = false;
      if (v[j] >= 0) {
        const int r = g[j] == v[j] ? v[j] : uf_find(parent, g[j]);
        if (r != v[j]) parent[p] = r;
        // v is the root its band gave the run, r the component's: the band borders chain the band roots of a component
        // that spans the page (the background: one hop per band), and every run of the band walks that chain unless the
        // first to get there shortens it (no union runs next to this kernel: any ancestor is a valid parent)
        if (g[j] != v[j] && r != g[j]) parent[v[j]] = r;
        if (r == p) {
          if (px[j]) ++lf, rf = true; else ++lb, rb = true;
        }
      }
      // root bitmaps per class, from this wave's 64 consecutive runs: (B, 2, nchunks, 64) words
      const unsigned long long mf = __ballot(rf), mb = __ballot(rb);
      if ((threadIdx.x & 63) == 0) {
        const size_t wi = (size_t)ch * 64 + 4 * (j0 + j) + (threadIdx.x >> 6);
        rootmask[((size_t)b * 2 + 0) * nchunks * 64 + wi] = mf;
        rootmask[((size_t)b * 2 + 1) * nchunks * 64 + wi] = mb;
      }
    }
  }
  int tf, tb;
  block_exclusive_scan(lf, sh, &tf);
  block_exclusive_scan(lb, sh, &tb);
  if (threadIdx.x == 0) {
    chunk_cnt[((size_t)b * 2 + 0) * nchunks + ch] = tf;
    chunk_cnt[((size_t)b * 2 + 1) * nchunks + ch] = tb;
  }
}
// a block walks several tiles / chunks: the launcher caps the grid (tail_max_blocks) so that these kernels hold a few
// waves per SIMD next to the network, not all of them
__global__ __launch_bounds__(256) void ccl2_flatten_count_kernel(int* __restrict__ parent_all, const uint8_t* __restrict__ rcls_all,
                                                                 const int* __restrict__ rcount, int B, int hw, int nchunks,
                                                                 int* __restrict__ chunk_cnt, unsigned long long* __restrict__ rootmask,
                                                                 int nvb) {
  for (int vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
    ccl2_flatten_count_body(vb, parent_all, rcls_all, rcount, B, hw, nchunks, chunk_cnt, rootmask);
    __syncthreads();
  }
}

// one block per (image, class): exclusive scan of that class's chunk counts; the totals go to n_f / n_b
__global__ __launch_bounds__(256) void ccl2_scan_chunks_kernel(int* __restrict__ chunk_cnt, int nchunks, int* __restrict__ n_f,
                                                               int* __restrict__ n_b) {
  __shared__ int sh[4];
  int* c = chunk_cnt + (size_t)blockIdx.x * nchunks;
  int carry = 0;
  for (int base = 0; base < nchunks; base += 256) {
    const int i = base + threadIdx.x;
    const int v = i < nchunks ? c[i] : 0;
    int total;
    const int excl = block_exclusive_scan(v, sh, &total);
    if (i < nchunks) c[i] = carry + excl;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) ((blockIdx.x & 1) ? n_b : n_f)[blockIdx.x >> 1] = carry;
}

// rlabel of the root runs: 2 * id + 1, id = +rank for a foreground root, -rank for a background root (ranks per class, in run
// order = raster order of the components' first pixels); the low bit says "root" to the paint.  A wave owns 1024
// consecutive runs of the chunk, 64 at a time; the root masks of its 16 groups stay in registers between the counting and
// the numbering sweep.
__device__ __forceinline__ void ccl2_rank_body(int vb, const unsigned long long* __restrict__ rootmask, const int* __restrict__ rcount,
                                                        int B, int hw, int nchunks, const int* __restrict__ chunk_cnt,
                                                        int* __restrict__ ids_all) {
  __shared__ int sh[2][4];
  const int b = vb % B, ch = vb / B;            // chunk-major (see ccl2_flatten_count_body)
  if (ch * RK_CHUNK >= rcount[b]) return;       // the whole block: no run, no root bitmap
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int base = ch * RK_CHUNK + w * 1024 + lane;
  unsigned long long mf[16], mb[16];
  int cf = 0, cb = 0;
  const unsigned long long* wf = rootmask + ((size_t)b * 2 + 0) * nchunks * 64 + (size_t)ch * 64 + w * 16;   // the flattening's root bitmaps
  const unsigned long long* wb = rootmask + ((size_t)b * 2 + 1) * nchunks * 64 + (size_t)ch * 64 + w * 16;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    mf[j] = wf[j];
    mb[j] = wb[j];
    cf += __popcll(mf[j]);
    cb += __popcll(mb[j]);
  }
  if (lane == 0) sh[0][w] = cf, sh[1][w] = cb;
  __syncthreads();
  int idf = chunk_cnt[((size_t)b * 2 + 0) * nchunks + ch], idb = chunk_cnt[((size_t)b * 2 + 1) * nchunks + ch];
  for (int i = 0; i < w; ++i) idf += sh[0][i], idb += sh[1][i];
  int* ids = ids_all + (size_t)b * hw;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int p = base + 64 * j;
    if ((mf[j] >> lane) & 1ull) {
      const int id = idf + __popcll(mf[j] & below) + 1;
      ids[p] = 2 * id + 1;
    } else if ((mb[j] >> lane) & 1ull) {
      const int id = idb + __popcll(mb[j] & below) + 1;
      ids[p] = -2 * id + 1;
    }
    idf += __popcll(mf[j]);
    idb += __popcll(mb[j]);
  }
}
// a block walks several tiles / chunks: the launcher caps the grid (tail_max_blocks) so that these kernels hold a few
// waves per SIMD next to the network, not all of them
__global__ __launch_bounds__(256) void ccl2_rank_kernel(const unsigned long long* __restrict__ rootmask, const int* __restrict__ rcount,
                                                        int B, int hw, int nchunks, const int* __restrict__ chunk_cnt,
                                                        int* __restrict__ ids_all, int nvb) {
  for (int vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
    ccl2_rank_body(vb, rootmask, rcount, B, hw, nchunks, chunk_cnt, ids_all);
    __syncthreads();
  }
}

// rlabel of every other run: its root's without the root bit (rparent[] is flat by now).  After this the label plane that
// held rparent[] is free.
__global__ __launch_bounds__(256) void ccl2_spread_kernel(const int* __restrict__ rparent_all, const int* __restrict__ rcount, int B,
                                                          int hw, int nchunks, int* __restrict__ rlabel_all, int nvb) {
  for (int vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
    const int b = vb % B, ch = vb / B;          // chunk-major (see ccl2_flatten_count_body)
    const int R = rcount[b];
    const int* rparent = rparent_all + (size_t)b * hw;
    int* rlabel = rlabel_all + (size_t)b * hw;
    constexpr int SU = 4;                         // parents of four runs, then their labels
    for (int j0 = 0; j0 < RK_PER_T && ch * RK_CHUNK + 256 * j0 < R; j0 += SU) {
      int par[SU], lab[SU];
#pragma unroll
      for (int j = 0; j < SU; ++j) {
        const int r = ch * RK_CHUNK + 256 * (j0 + j) + threadIdx.x;
        par[j] = r < R ? rparent[r] : -1;
      }
#pragma unroll
      for (int j = 0; j < SU; ++j) {
        const int r = ch * RK_CHUNK + 256 * (j0 + j) + threadIdx.x;
        lab[j] = (par[j] >= 0 && par[j] != r) ? rlabel[par[j]] : 0;
      }
#pragma unroll
      for (int j = 0; j < SU; ++j) {
        const int r = ch * RK_CHUNK + 256 * (j0 + j) + threadIdx.x;
        if (par[j] >= 0 && par[j] != r) rlabel[r] = lab[j] & ~1;
      }
    }
  }
}

// The paint: final labels + statistics.  A block owns LB_CHUNK consecutive pixels of one page.  A pixel's label is its
// run's: run = base[word] + popcount(starts[word] up to its bit) - 1, label = rlabel[run] >> 1.  The plane is written once
// and never read.  The pixel that starts a root run (rlabel[run] & 1) is its component's first pixel in raster order: it
// writes first_*.
// Statistics go through two levels of aggregation before they reach HBM: (1) a wave covers 64 consecutive pixels, each
// horizontal stretch of one label is handled by its first lane; (2) the stretches of a block are merged per label in a
// small LDS hash table that is flushed once at the end.  Big components (a page's background, a window's complement)
// otherwise serialise tens of thousands of atomics on the same five words of `stats` (rocprofv3: 1.2-2.7 ms per launch
// before the block-level table).
// KEEP 0 (launch_ccl_dual): signed labels, the tables of both classes.  KEEP +1 / -1 (launch_ccl): the foreground /
// background class alone -- its pixels get |id|, the other class's pixels get `other` (0, or the -1 of bg_negative) and
// take no part in anything below; st_f / first_f are the kept class's tables and may be null, st_b / first_b / seg_live
// are not used.
// seg_live (null: not wanted): a wave's 64 pixels are one 64-aligned segment of the page's linear index (chunks and steps
// are multiples of 256), and the wave has their labels in registers: lane 0 notes whether any differs from -1.
template <int KEEP>
__device__ __forceinline__ void ccl2_label_body(int vb, int* __restrict__ labels_all, const RunTables t, int B, int H,
                                                         int W, int chunks, int* __restrict__ st_f, int* __restrict__ st_b,
                                                         int* __restrict__ first_f, int* __restrict__ first_b, int max_labels,
                                                         uint8_t* __restrict__ seg_live, int other) {
  constexpr int EMPTY = (int)0x80000000;
  __shared__ int hkey[LB_SLOTS];
  __shared__ int hst[LB_SLOTS * 5];
  const int hw = H * W;
  const int b = vb / chunks, ch = vb % chunks;
  const int p_begin = ch * LB_CHUNK, p_end = min(hw, p_begin + LB_CHUNK);
  const size_t base = (size_t)b * hw;
  const unsigned* starts = t.starts + (size_t)b * H * t.wp;
  const unsigned* wbase = t.base + (size_t)b * H * t.wp;
  const int* rlabel = t.rlabel + base;
  for (int s = threadIdx.x; s < LB_SLOTS; s += 256) {
    hkey[s] = EMPTY;
    hst[5 * s] = W, hst[5 * s + 1] = H, hst[5 * s + 2] = -1, hst[5 * s + 3] = -1, hst[5 * s + 4] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  auto row_of = [&](int id) { return (id > 0 ? st_f : st_b) + ((size_t)b * max_labels + ((id > 0 ? id : -id) - 1)) * 5; };
  // eight steps' words, then their runs' labels (a dependent gather): two memory round trips per 2048 pixels, and the
  // capped grid leaves a block little else to hide them behind
  constexpr int LU = 8;
  static_assert(LB_CHUNK % (256 * LU) == 0, "whole batches");
  for (int pb = p_begin; pb < p_end; pb += 256 * LU) {
    unsigned sw[LU];
    int run[LU], idv[LU];
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      const int p = pb + 256 * u + threadIdx.x;
      const int y = p / W, w = y * t.wp + ((p - y * W) >> 5);
      sw[u] = p < p_end ? starts[w] : 0u;
      run[u] = p < p_end ? (int)wbase[w] : 0;
    }
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      const int p = pb + 256 * u + threadIdx.x;
      const int bit = (p % W) & 31;
      run[u] += __popc(sw[u] & ((2u << bit) - 1u)) - 1;
      idv[u] = p < p_end ? rlabel[run[u]] : 0;
      sw[u] = (sw[u] >> bit) & 1u;                            // this pixel starts its run
    }
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      sw[u] &= (unsigned)idv[u];                              // ... a root run: the component's first pixel
      idv[u] >>= 1;
      if (KEEP) idv[u] = (KEEP > 0 ? idv[u] > 0 : idv[u] < 0) ? (KEEP > 0 ? idv[u] : -idv[u]) : 0;   // the other class: 0
    }
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      const int p = pb + 256 * u + threadIdx.x;
      if (p < p_end) labels_all[base + p] = (KEEP && !idv[u]) ? other : idv[u];
    }
    if (KEEP && !st_f && !first_f) continue;
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      const int p0 = pb + 256 * u;
      if (p0 >= p_end) break;
      const int p = p0 + threadIdx.x;
      const bool live = p < p_end;
      // 0 = dead lane, or (KEEP) a pixel of the other class, set to 0 above: every pixel has a class, so no real id is 0
      const int id = idv[u];
      const int x = live ? p % W : 0, y = live ? p / W : 0;
      if (!KEEP && seg_live) {
        const unsigned long long other = __ballot(live && id != -1);
        const int q0 = p0 + ((int)threadIdx.x & ~63);
        if (lane == 0 && q0 < p_end) seg_live[(size_t)b * ((hw + 63) >> 6) + (q0 >> 6)] = other ? 1 : 0;
      }
      const int prev = __shfl_up(id, 1);
      const bool head = lane == 0 || prev != id || x == 0;
      const unsigned long long heads = __ballot(head);
      const int mag = id > 0 ? id : -id;
      if (sw[u] && (!KEEP || (id != 0 && first_f)) && mag <= max_labels)
        (id > 0 ? first_f : first_b)[(size_t)b * max_labels + mag - 1] = p;
      if (head && id != 0 && mag <= max_labels && (!KEEP || st_f)) {
        const unsigned long long later = lane == 63 ? 0ull : (heads >> (lane + 1));
        const int len = later ? __ffsll((long long)later) : 64 - lane;
        int slot = -1;
        const unsigned hsh = ((unsigned)id * 2654435761u) >> 25;    // 7 bits
        for (int probe = 0; probe < 4; ++probe) {
          const int sidx = (hsh + probe) & (LB_SLOTS - 1);
          const int old = atomicCAS(&hkey[sidx], EMPTY, id);
          if (old == EMPTY || old == id) {
            slot = sidx;
            break;
          }
        }
        int* s = slot >= 0 ? hst + 5 * slot : row_of(id);
        atomicMin(s + 0, x);
        atomicMin(s + 1, y);
        atomicMax(s + 2, x + len - 1);
        atomicMax(s + 3, y);
        atomicAdd(s + 4, len);
      }
    }
  }
  __syncthreads();
  for (int sl = threadIdx.x; sl < LB_SLOTS; sl += 256) {
    const int id = hkey[sl];
    if (id == EMPTY) continue;
    int* s = row_of(id);
    atomicMin(s + 0, hst[5 * sl]);
    atomicMin(s + 1, hst[5 * sl + 1]);
    atomicMax(s + 2, hst[5 * sl + 2]);
    atomicMax(s + 3, hst[5 * sl + 3]);
    atomicAdd(s + 4, hst[5 * sl + 4]);
  }
}
// a block walks several tiles / chunks: the launcher caps the grid (tail_max_blocks) so that these kernels hold a few
// waves per SIMD next to the network, not all of them
template <int KEEP>
__global__ __launch_bounds__(256) void ccl2_label_kernel(int* __restrict__ labels_all, const RunTables t, int B, int H,
                                                         int W, int chunks, int* __restrict__ st_f, int* __restrict__ st_b,
                                                         int* __restrict__ first_f, int* __restrict__ first_b, int max_labels,
                                                         int nvb, uint8_t* __restrict__ seg_live, int other) {
  for (int vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
    ccl2_label_body<KEEP>(vb, labels_all, t, B, H, W, chunks, st_f, st_b, first_f, first_b, max_labels, seg_live, other);
    __syncthreads();
  }
}


// grid of a kernel whose blocks walk `nvb` tiles / chunks: at most g_tail_max_blocks blocks
inline int capped(int nvb) { return std::max(1, std::min(nvb, g_tail_max_blocks)); }

inline int grid_for(long long total, int block = 256) {
  long long g = (total + block - 1) / block;
  if (g > (long long)g_tail_max_blocks) g = g_tail_max_blocks;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

size_t nms_workspace_bytes(int B, int rows) { return (size_t)B * rows * sizeof(Cand) + (size_t)B * sizeof(int) + 256; }

void launch_nms(const float* blks, int B, int rows, int no, float conf, float iou, int max_det, int max_nms,
                float max_wh, float* dets, int* counts, void* ws, hipStream_t st) {
  int* cnt = (int*)ws;
  Cand* cands = (Cand*)((char*)ws + ((size_t)B * sizeof(int) + 255) / 256 * 256);
  (void)hipMemsetAsync(cnt, 0, (size_t)B * sizeof(int), st);
  (void)hipMemsetAsync(dets, 0, (size_t)B * max_det * 6 * sizeof(float), st);
  hipLaunchKernelGGL(nms_filter_kernel, dim3(grid_for((long long)B * rows)), dim3(256), 0, st, blks, B, rows, no, conf,
                     cands, cnt);
  hipLaunchKernelGGL(nms_greedy_kernel, dim3(B), dim3(NMS_THREADS), 0, st, cands, cnt, rows, iou, max_det, max_nms, max_wh,
                     dets, counts);
}

namespace {

// The labelling's workspace, sub-buffer by sub-buffer in the order they are carved; each starts a multiple of 256 bytes
// after `ws`.  With hw = H * W, nchunks = ceil(hw / RK_CHUNK), wp = ceil(W / 32), nw = H * wp, nseg = ceil(nw / PK_SEG):
//   rlabel     (B, hw) int                 a run's 2 * (+-id) + root bit; the first R of a page in use
//   chunk_cnt  (B, 2, nchunks) int         roots per chunk and class, then their exclusive scan
//   rootmask   (B, 2, nchunks, 64) u64     root bitmaps per chunk and class
//   rcls       (B, hw) u8                  a run's class
//   bits, starts, base   (B, nw) u32 each  the page as words (the header of the engine above)
//   rcount     (B) int                     runs of a page
//   segsum     (B, nseg) int               starts per segment of PK_SEG words
//   n_other    (B) int                     launch_ccl: the count of the class it does not keep
// The tables are laid out for the H x W they were sized for: a workspace for one shape serves no other, whatever its
// pixel count.  ccl_workspace_bytes is where this carve ends, so the two cannot disagree.
struct CclWs {
  int* rlabel;
  int* chunk_cnt;
  unsigned long long* rootmask;
  uint8_t* rcls;
  unsigned *bits, *starts, *base;
  int *rcount, *segsum, *n_other;
  size_t bytes;
};
CclWs ccl_carve(void* ws, int B, int H, int W) {
  const size_t hw = (size_t)H * W, nchunks = (hw + RK_CHUNK - 1) / RK_CHUNK;
  const size_t nw = (size_t)H * ((W + 31) / 32), nseg = (nw + PK_SEG - 1) / PK_SEG;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    void* p = (void*)((uintptr_t)ws + off);
    off += (bytes + 255) / 256 * 256;
    return p;
  };
  CclWs w;
  w.rlabel = (int*)take(B * hw * sizeof(int));
  w.chunk_cnt = (int*)take(2 * B * nchunks * sizeof(int));
  w.rootmask = (unsigned long long*)take(2 * B * nchunks * 64 * 8);
  w.rcls = (uint8_t*)take(B * hw);
  w.bits = (unsigned*)take(B * nw * sizeof(unsigned));
  w.starts = (unsigned*)take(B * nw * sizeof(unsigned));
  w.base = (unsigned*)take(B * nw * sizeof(unsigned));
  w.rcount = (int*)take(B * sizeof(int));
  w.segsum = (int*)take(B * nseg * sizeof(int));
  w.n_other = (int*)take(B * sizeof(int));
  w.bytes = off;
  return w;
}

// The engine.  keep 0: both classes (launch_ccl_dual).  keep +1 / -1: the foreground / background class alone; the other
// class's n_*, st_*, first_* are null and `other` is what its pixels get in the plane.  Refuses, launching nothing, a
// workspace smaller than ccl_workspace_bytes(B, H, W).
hipError_t ccl_on_runs(const uint8_t* img, int B, int H, int W, int thresh, int flip, int keep, int other, int* labels, int* n_f,
                       int* n_b, int* st_f, int* st_b, int* first_f, int* first_b, int max_labels, void* ws, size_t ws_bytes,
                       hipStream_t st, uint8_t* seg_live) {
  const CclWs w = ccl_carve(ws, B, H, W);
  if (ws_bytes < w.bytes) return hipErrorInvalidValue;
  const int hw = H * W;
  const int nchunks = (hw + RK_CHUNK - 1) / RK_CHUNK;
  const int wp = (W + 31) / 32, nw = H * wp;
  const int nseg = (nw + PK_SEG - 1) / PK_SEG, ntiles = (nw + SC_TILE - 1) / SC_TILE;
  if (!n_f) n_f = w.n_other;
  if (!n_b) n_b = w.n_other;
  int* rparent = labels;                                                                     // dead before the paint
  const int aligned4 = (W % 4 == 0 && ((uintptr_t)img & 3) == 0) ? 1 : 0;
  hipLaunchKernelGGL(ccl2_pack_kernel, dim3(capped(B * nseg)), dim3(256), 0, st, img, w.bits, w.starts, w.segsum, nseg, H, W, wp,
                     thresh, flip, aligned4, B * nseg);
  hipLaunchKernelGGL(ccl2_run_scan_kernel, dim3(capped(B * ntiles)), dim3(256), 0, st, w.starts, w.segsum, w.base, w.rcount, nw, nseg,
                     ntiles, B * ntiles);
  const int nbands = (H + RB_ROWS - 1) / RB_ROWS;
  const int band_grid = std::max(1, std::min(B * nbands, g_tail_max_blocks / (RB_THREADS / 256)));   // the cap counts 256 threads
  hipLaunchKernelGGL(ccl2_band_kernel, dim3(band_grid), dim3(RB_THREADS), 0, st, w.bits, w.starts, w.base, w.rcount, rparent, w.rcls, H,
                     W, wp, nbands, B * nbands);
  if (nbands > 1)
    hipLaunchKernelGGL(ccl2_band_border_kernel, dim3((B * (nbands - 1) * wp + 255) / 256), dim3(256), 0, st, w.bits, w.starts, w.base,
                       rparent, B, H, W, wp, nbands - 1);
  hipLaunchKernelGGL(ccl2_flatten_count_kernel, dim3(capped(B * nchunks)), dim3(256), 0, st, rparent, w.rcls, w.rcount, B, hw, nchunks,
                     w.chunk_cnt, w.rootmask, B * nchunks);
  hipLaunchKernelGGL(ccl2_scan_chunks_kernel, dim3(2 * B), dim3(256), 0, st, w.chunk_cnt, nchunks, n_f, n_b);
  hipLaunchKernelGGL(ccl2_rank_kernel, dim3(capped(B * nchunks)), dim3(256), 0, st, w.rootmask, w.rcount, B, hw, nchunks, w.chunk_cnt,
                     w.rlabel, B * nchunks);
  hipLaunchKernelGGL(ccl2_spread_kernel, dim3(capped(B * nchunks)), dim3(256), 0, st, rparent, w.rcount, B, hw, nchunks, w.rlabel,
                     B * nchunks);
  const int sgrid = std::max(1, std::min(64, (max_labels + 255) / 256));
  if (st_f) hipLaunchKernelGGL(ccl_stats_init_kernel, dim3(sgrid, B), dim3(256), 0, st, st_f, n_f, max_labels, H, W);
  if (st_b) hipLaunchKernelGGL(ccl_stats_init_kernel, dim3(sgrid, B), dim3(256), 0, st, st_b, n_b, max_labels, H, W);
  const int lchunks = (hw + LB_CHUNK - 1) / LB_CHUNK;
  const RunTables t{w.starts, w.base, w.rlabel, wp};
  const dim3 lgrid(capped(B * lchunks));
  if (keep == 0)
    hipLaunchKernelGGL((ccl2_label_kernel<0>), lgrid, dim3(256), 0, st, labels, t, B, H, W, lchunks, st_f, st_b, first_f, first_b,
                       max_labels, B * lchunks, seg_live, 0);
  else if (keep > 0)
    hipLaunchKernelGGL((ccl2_label_kernel<1>), lgrid, dim3(256), 0, st, labels, t, B, H, W, lchunks, st_f, nullptr, first_f, nullptr,
                       max_labels, B * lchunks, nullptr, other);
  else
    hipLaunchKernelGGL((ccl2_label_kernel<-1>), lgrid, dim3(256), 0, st, labels, t, B, H, W, lchunks, st_b, nullptr, first_b, nullptr,
                       max_labels, B * lchunks, nullptr, other);
  if (st_f) hipLaunchKernelGGL(ccl_stats_final_kernel, dim3(sgrid, B), dim3(256), 0, st, st_f, n_f, max_labels);
  if (st_b) hipLaunchKernelGGL(ccl_stats_final_kernel, dim3(sgrid, B), dim3(256), 0, st, st_b, n_b, max_labels);
  return hipSuccess;
}

}  // namespace

size_t ccl_workspace_bytes(int B, int H, int W) { return ccl_carve(nullptr, B, H, W).bytes; }

hipError_t launch_ccl(const uint8_t* img, int B, int H, int W, int thresh, int conn, int* labels, int* n_out, int* stats,
                      int max_labels, void* ws, size_t ws_bytes, hipStream_t st, int* first, int bg_negative) {
  const int other = bg_negative ? -1 : 0;
  if (conn == 8)   // the foreground half of the dual labelling
    return ccl_on_runs(img, B, H, W, thresh, 0, +1, other, labels, n_out, nullptr, stats, nullptr, first, nullptr, max_labels, ws,
                       ws_bytes, st, nullptr);
  // conn 4: the background half of the dual labelling of the flipped page
  return ccl_on_runs(img, B, H, W, thresh, 1, -1, other, labels, nullptr, n_out, nullptr, stats, nullptr, first, max_labels, ws,
                     ws_bytes, st, nullptr);
}

hipError_t launch_ccl_dual(const uint8_t* img, int B, int H, int W, int thresh, int* labels, int* n_f, int* n_b, int* st_f,
                           int* st_b, int* first_f, int* first_b, int max_labels, void* ws, size_t ws_bytes, hipStream_t st,
                           uint8_t* seg_live) {
  return ccl_on_runs(img, B, H, W, thresh, 0, 0, 0, labels, n_f, n_b, st_f, st_b, first_f, first_b, max_labels, ws, ws_bytes, st,
                     seg_live);
}
