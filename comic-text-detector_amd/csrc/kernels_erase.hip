// Erase text on plain backgrounds (`ctd_erase_text`; the rule is stated in include/ctd_hip.h and restated in numpy in
// tests/erase_ref.py): per block, is the background next to its glyphs one colour; per page, the glyphs of such blocks filled
// with that colour and the mask of what an inpainter still has to do.  Integers only: counts, comparisons and copies.
//
// Two launches, no host step between them.
//
// erase_stats_kernel, one workgroup per block: walks the block's box grown by g + r in 64 x 64 tiles.  A tile stages the
// mask with a halo of g + r as a bit plane in LDS -- three 64-bit words a row, one __ballot per 64 mask bytes, the halo
// words load only the lanes they need -- and gets D_g(T), D_{g+r}(T) and D_g(M) for its 64 columns by word shifts and ORs,
// rows first (one thread a staged row), then columns (one thread an output row).  A tile without a text bit of the block in
// reach is left after the first step.  The ring pixels go into per-wave sub-histograms (u32 LDS atomics): on a plain balloon
// every ring pixel of a row has the same value, so a wave first collapses the lanes that agree with its first active lane
// into ONE add (twice: a balloon and its outline), and only what is left adds by lane.  The sub-histograms are summed at
// the end, one wave per channel finds the median and the count near it with a prefix sum in registers, thread 0 stores
// the row.
//
// erase_paint_kernel, one workgroup per 64 x 32 page tile of all pages: every thread walks the page's blocks (uniform
// loads) and keeps those whose box grown by g reaches the tile and whose row says PLAIN, TEXTURED or NO_RING -- typically
// none, and then the tile is a copy.  Otherwise the tile stages its mask bit plane with a halo of g and, for the survivors
// in ascending index, tests p in D_g(M & X_b) from it; the last PLAIN block to cover a pixel wins, in registers, no atomics.
// Every byte of `out` and `rest` is written exactly once.  The 3-byte pixels move as dwords: a wave owns a tile row, a lane
// one ALIGNED dword of the output row segment (the few bytes before the first and after the last go by byte), read from the
// page as one or two aligned dwords and a funnel shift, since page and output rows have any alignment.
#include "kernels.h"

namespace {

constexpr int ES_THREADS = 512, ES_WAVES = ES_THREADS / 64;
constexpr int ES_TILE = 64;                                            // stats tile: 64 x 64 pixels
constexpr int ES_MAXK = CTD_ERASE_MAX_GROW + CTD_ERASE_MAX_RING;       // 24 < 64: one halo word either side is enough
constexpr int ES_ROWS = ES_TILE + 2 * ES_MAXK;
constexpr int EP_THREADS = 256, EP_WAVES = EP_THREADS / 64;
constexpr int EP_TW = CTD_ERASE_TILE_W, EP_TH = CTD_ERASE_TILE_H;
constexpr int EP_ROWS = EP_TH + 2 * CTD_ERASE_MAX_GROW;
constexpr int EP_RPW = EP_TH / EP_WAVES;                               // tile rows a wave owns
static_assert(EP_TW == 64 && ES_TILE == 64, "a tile row is one 64-bit word");
static_assert(3 * EP_TW / 4 + 2 <= 64, "a lane per dword of a tile row of `out`");
static_assert(sizeof(ctd_erase_job) == 32 && sizeof(ctd_erase_page) == 72 && sizeof(ctd_erase_params) == 32 &&
              sizeof(ctd_erase_row) == 32, "erase ABI sizes (erase.py dtypes)");
static_assert(offsetof(ctd_erase_page, H) == 32 && offsetof(ctd_erase_page, block0) == 56 && offsetof(ctd_erase_page, tile0) == 64 &&
              offsetof(ctd_erase_row, cnt) == 12 && offsetof(ctd_erase_row, med) == 24, "erase ABI offsets");

typedef unsigned long long u64;

// bits lo .. hi - 1 of a word whose bit 0 is pixel x0 (the pixels x0 <= lo' <= x < hi' <= x0 + 64)
__device__ __forceinline__ u64 span_bits(int x0, int lo, int hi) {
  const int a = max(lo - x0, 0), b = min(hi - x0, 64);
  if (a >= b) return 0ull;
  return (b == 64 ? ~0ull : ((1ull << b) - 1ull)) & ~((1ull << a) - 1ull);
}

// the middle word of a 192-pixel row dilated by k pixels either way (k < 64)
__device__ __forceinline__ u64 hdil(u64 l, u64 m, u64 r, int k) {
  u64 v = m;
  for (int s = 1; s <= k; ++s) v |= (m << s) | (l >> (64 - s)) | (m >> s) | (r << (64 - s));
  return v;
}

// Stages the mask bits of rows y0 .. y0 + rows - 1, pixels x0 - 64 .. x0 + 127, into plane[row][3]; only pixels x0 - k ..
// x0 + 63 + k of the page are loaded, everything else is 0.
template <int NWAVES>
__device__ __forceinline__ void stage_mask(u64 (*plane)[3], const uint8_t* mask, long long mpitch, int H, int W, int x0, int y0,
                                           int rows, int k) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int task = wave; task < rows * 3; task += NWAVES) {
    const int row = task / 3, w = task - row * 3;
    const int x = x0 - 64 + 64 * w + lane, y = y0 + row;
    const bool need = x >= x0 - k && x < x0 + 64 + k && x >= 0 && x < W && y >= 0 && y < H;
    bool bit = false;
    if (need) bit = mask[y * mpitch + x] != 0;
    const u64 word = __ballot(bit);
    if (lane == 0) plane[row][w] = word;
  }
}

struct EraseBox {
  int x1, y1, x2, y2;  // X_b, clipped
  int status;          // CTD_ERASE_EMPTY / TOO_LARGE, or -1: to be computed
};

__device__ __forceinline__ EraseBox erase_box(const int32_t* xyxy, int H, int W, int k) {
  EraseBox b;
  bool far = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) far = far || xyxy[i] > CTD_ERASE_MAX_COORD || xyxy[i] < -CTD_ERASE_MAX_COORD;
  b.x1 = max(xyxy[0], 0), b.y1 = max(xyxy[1], 0), b.x2 = min(xyxy[2], W), b.y2 = min(xyxy[3], H);
  b.status = -1;
  if (far) {
    b.status = CTD_ERASE_TOO_LARGE;
  } else if (b.x1 >= b.x2 || b.y1 >= b.y2) {
    b.status = CTD_ERASE_EMPTY;
  } else if ((long long)(b.x2 - b.x1 + 2 * k) * (long long)(b.y2 - b.y1 + 2 * k) > (long long)CTD_ERASE_MAX_PIXELS) {
    b.status = CTD_ERASE_TOO_LARGE;
  }
  return b;
}

// one channel's values of a wave's ring pixels into its sub-histogram: two rounds of "everybody who agrees with the first
// active lane is one add", the rest by lane
__device__ __forceinline__ void hist_add(unsigned* h, unsigned v, bool on, int lane) {
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const u64 act = __ballot(on);
    if (!act) return;
    const int leader = __ffsll((long long)act) - 1;
    const unsigned lv = (unsigned)__shfl((int)v, leader, 64);
    const u64 eq = __ballot(on && v == lv);
    if (lane == leader) atomicAdd(h + lv, (unsigned)__popcll(eq));
    on = on && v != lv;
  }
  if (on) atomicAdd(h + v, 1u);
}

__global__ __launch_bounds__(ES_THREADS) void erase_stats_kernel(const ctd_erase_job* __restrict__ jobs,
                                                                 const ctd_erase_page* __restrict__ pages, int n_pages,
                                                                 ctd_erase_params prm, ctd_erase_row* __restrict__ rows) {
  __shared__ unsigned hist[ES_WAVES][768];
  __shared__ u64 plane[ES_ROWS][3];
  __shared__ u64 hA[ES_ROWS], hB[ES_ROWS], hC[ES_ROWS];   // rows dilated: D_g(T), D_{g+r}(T), D_g(M), the tile's 64 columns
  __shared__ u64 ringw[ES_TILE];
  __shared__ unsigned n_fill_sh, res_cnt[3], res_med[3], res_n[3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const ctd_erase_job J = jobs[blockIdx.x];
  ctd_erase_row* __restrict__ row = rows + blockIdx.x;
  const int g = prm.grow, K = prm.grow + prm.ring;

  int status = CTD_ERASE_EMPTY;
  EraseBox B;
  B.status = CTD_ERASE_EMPTY;
  ctd_erase_page P;
  const bool has_page = J.page >= 0 && J.page < n_pages;
  if (has_page) {
    P = pages[J.page];
    B = erase_box(J.xyxy, P.H, P.W, K);
  }
  if (B.status >= 0) {                                    // block-uniform; decided before any pixel is read
    if (t == 0) {
      row->status = B.status;
      row->n_fill = 0, row->n_ring = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) row->cnt[c] = 0, row->med[c] = 0;
#pragma unroll
      for (int c = 0; c < 5; ++c) row->pad_[c] = 0;
    }
    return;
  }

  for (int i = t; i < ES_WAVES * 768; i += ES_THREADS) (&hist[0][0])[i] = 0u;
  if (t == 0) n_fill_sh = 0u;
  __syncthreads();

  // the box grown by g + r, clipped: what the tiles cover
  const int ex0 = max(B.x1 - K, 0), ey0 = max(B.y1 - K, 0), ex1 = min(B.x2 + K, P.W), ey1 = min(B.y2 + K, P.H);
  const int rows_staged = ES_TILE + 2 * K;
  const long long pitch = P.pitch, mpitch = P.mask_pitch;
  unsigned my_fill = 0;
  for (int ty0 = ey0; ty0 < ey1; ty0 += ES_TILE) {
    for (int tx0 = ex0; tx0 < ex1; tx0 += ES_TILE) {
      stage_mask<ES_WAVES>(plane, P.mask_dev, mpitch, P.H, P.W, tx0, ty0 - K, rows_staged, K);
      __syncthreads();
      int any = 0;
      if (t < rows_staged) {
        const int y = ty0 - K + t;
        const u64 ml = plane[t][0], mm = plane[t][1], mr = plane[t][2];
        const bool inbox = y >= B.y1 && y < B.y2;
        const u64 tl = inbox ? ml & span_bits(tx0 - 64, B.x1, B.x2) : 0ull, tm = inbox ? mm & span_bits(tx0, B.x1, B.x2) : 0ull,
                  tr = inbox ? mr & span_bits(tx0 + 64, B.x1, B.x2) : 0ull;
        any = (tl | tm | tr) != 0ull;
        hA[t] = hdil(tl, tm, tr, g);
        hB[t] = hdil(tl, tm, tr, K);
        hC[t] = hdil(ml, mm, mr, g);
      }
      if (!__syncthreads_or(any)) continue;               // no text of this block within g + r of the tile
      if (t < ES_TILE) {
        const int y = ty0 + t;
        u64 f = 0ull, d = 0ull, m = 0ull;
        if (y < ey1) {
          for (int dy = -K; dy <= K; ++dy) d |= hB[K + t + dy];
          for (int dy = -g; dy <= g; ++dy) f |= hA[K + t + dy], m |= hC[K + t + dy];
          const u64 valid = span_bits(tx0, tx0, ex1);
          f &= valid;
          d &= valid & ~m;
        }
        ringw[t] = d;
        my_fill += (unsigned)__popcll(f);
      }
      __syncthreads();
      for (int j = wave; j < ES_TILE; j += ES_WAVES) {
        const u64 rw = ringw[j];
        if (!rw) continue;                                // wave-uniform
        const bool on = (rw >> lane) & 1ull;
        unsigned c0 = 0, c1 = 0, c2 = 0;
        if (on) {
          const uint8_t* p = P.page_dev + (ty0 + j) * pitch + 3ll * (tx0 + lane);
          c0 = p[0], c1 = p[1], c2 = p[2];
        }
        hist_add(hist[wave], c0, on, lane);
        hist_add(hist[wave] + 256, c1, on, lane);
        hist_add(hist[wave] + 512, c2, on, lane);
      }
      // the next tile's first two barriers lie between these reads of ringw and its next writes
    }
  }
  if (my_fill) atomicAdd(&n_fill_sh, my_fill);
  __syncthreads();
  for (int i = t; i < 768; i += ES_THREADS) {
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < ES_WAVES; ++w) s += hist[w][i];
    hist[0][i] = s;
  }
  __syncthreads();
  if (wave < 3) {                                         // channel = wave: lane l holds bins 4 l .. 4 l + 3
    const unsigned* h = hist[0] + 256 * wave;
    unsigned b[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = h[4 * lane + k], s += b[k];
    unsigned inc = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned v = __shfl_up(inc, off, 64);
      if (lane >= off) inc += v;
    }
    const unsigned n = __shfl(inc, 63, 64);               // <= 2^24
    const u64 reach = __ballot(2u * inc >= n);            // lane 63 always does
    const int ml = __ffsll((long long)reach) - 1;
    unsigned med = 0;
    if (lane == ml) {
      unsigned cum = inc - s;
      med = 4 * lane + 3;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        cum += b[k];
        if (2u * cum >= n) { med = 4 * lane + k; break; }
      }
    }
    med = __shfl(med, ml, 64);
    const int lo = (int)med - prm.tol, hi = (int)med + prm.tol;
    unsigned near = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = 4 * lane + k;
      near += (v >= lo && v <= hi) ? b[k] : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) near += __shfl_down(near, d, 64);
    if (lane == 0) res_cnt[wave] = near, res_med[wave] = n ? med : 0u, res_n[wave] = n;
  }
  __syncthreads();
  if (t == 0) {
    const unsigned n_ring = res_n[0], n_fill = n_fill_sh;
    const unsigned cmin = min(res_cnt[0], min(res_cnt[1], res_cnt[2]));
    if (n_fill == 0) status = CTD_ERASE_NO_MASK;          // F_b contains T_b
    else if (n_ring < (unsigned)prm.min_ring) status = CTD_ERASE_NO_RING;
    else status = 16ull * cmin >= 15ull * n_ring ? CTD_ERASE_PLAIN : CTD_ERASE_TEXTURED;
    row->status = status;
    row->n_fill = (int)n_fill, row->n_ring = (int)n_ring;
#pragma unroll
    for (int c = 0; c < 3; ++c) row->cnt[c] = (int)res_cnt[c], row->med[c] = (uint8_t)res_med[c];
#pragma unroll
    for (int c = 0; c < 5; ++c) row->pad_[c] = 0;
  }
}

// ---- paint ------------------------------------------------------------------------------------------------------------------

// does job b of page P reach the tile (x0, y0), and how: 0 no, 1 paints (PLAIN), 2 adds to rest (TEXTURED / NO_RING)
__device__ __forceinline__ int paint_kind(const ctd_erase_job& J, const ctd_erase_row& R, const ctd_erase_page& P, int x0, int y0,
                                          int g, EraseBox& B) {
  const int st = R.status;
  if (st != CTD_ERASE_PLAIN && st != CTD_ERASE_TEXTURED && st != CTD_ERASE_NO_RING) return 0;
  B = erase_box(J.xyxy, P.H, P.W, 0);
  if (B.status >= 0) return 0;
  if (B.x1 - g >= x0 + EP_TW || B.x2 + g <= x0 || B.y1 - g >= y0 + EP_TH || B.y2 + g <= y0) return 0;
  return st == CTD_ERASE_PLAIN ? 1 : 2;
}

__global__ __launch_bounds__(EP_THREADS) void erase_paint_kernel(const ctd_erase_job* __restrict__ jobs,
                                                                 int n_jobs, const ctd_erase_page* __restrict__ pages,
                                                                 int n_pages, ctd_erase_params prm,
                                                                 const ctd_erase_row* __restrict__ rows) {
  __shared__ u64 plane[EP_ROWS][3];
  __shared__ u64 hA[EP_ROWS];
  __shared__ unsigned win[EP_TH][EP_TW];                  // B | G << 8 | R << 16 | 1 << 24 where painted, else 0
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int g = prm.grow;
  // the page of this tile: the last one whose tile0 <= blockIdx.x (uniform)
  int lo = 0, hi = n_pages - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pages[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const ctd_erase_page P = pages[lo];
  const int tiles_x = (P.W + EP_TW - 1) / EP_TW, tiles_y = (P.H + EP_TH - 1) / EP_TH;
  const int local = (int)blockIdx.x - P.tile0;
  if (local < 0 || local >= tiles_x * tiles_y) return;
  const int tyi = local / tiles_x, txi = local - tyi * tiles_x;
  const int x0 = txi * EP_TW, y0 = tyi * EP_TH;
  const int tw = min(EP_TW, P.W - x0), th = min(EP_TH, P.H - y0);

  // the page's rows of the job table, never beyond the table
  const int nb = P.block0 >= 0 && P.block0 <= n_jobs ? min(P.n_blocks, n_jobs - P.block0) : 0;
  int survivors = 0;
  for (int b = 0; b < nb; ++b) {
    EraseBox B;
    survivors += paint_kind(jobs[P.block0 + b], rows[P.block0 + b], P, x0, y0, g, B) != 0;
  }

  unsigned restf = 0;                                     // bit r: pixel (lane, wave * EP_RPW + r) lies in F of a TEXTURED / NO_RING block
  if (survivors) {                                        // block-uniform
    unsigned mine[EP_RPW];
#pragma unroll
    for (int r = 0; r < EP_RPW; ++r) mine[r] = 0u;
    stage_mask<EP_WAVES>(plane, P.mask_dev, (long long)P.mask_pitch, P.H, P.W, x0, y0 - g, EP_TH + 2 * g, g);
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
      EraseBox B;
      const ctd_erase_row R = rows[P.block0 + b];
      const int kind = paint_kind(jobs[P.block0 + b], R, P, x0, y0, g, B);
      if (!kind) continue;
      if (t < EP_TH + 2 * g) {
        const int y = y0 - g + t;
        u64 v = 0ull;
        if (y >= B.y1 && y < B.y2)
          v = hdil(plane[t][0] & span_bits(x0 - 64, B.x1, B.x2), plane[t][1] & span_bits(x0, B.x1, B.x2),
                   plane[t][2] & span_bits(x0 + 64, B.x1, B.x2), g);
        hA[t] = v;
      }
      __syncthreads();
      const unsigned colour = (unsigned)R.med[0] | (unsigned)R.med[1] << 8 | (unsigned)R.med[2] << 16 | 1u << 24;
#pragma unroll
      for (int r = 0; r < EP_RPW; ++r) {
        const int j = wave * EP_RPW + r;
        u64 f = 0ull;
        for (int dy = 0; dy <= 2 * g; ++dy) f |= hA[j + dy];
        if ((f >> lane) & 1ull) {
          if (kind == 1) mine[r] = colour;
          else restf |= 1u << r;
        }
      }
      __syncthreads();                                    // hA is free again
    }
#pragma unroll
    for (int r = 0; r < EP_RPW; ++r) win[wave * EP_RPW + r][lane] = mine[r];
    __syncthreads();
  }

  // ---- every byte of the tile's `out` and `rest`: a wave per row, a lane per aligned dword of the row's 3 * tw bytes;
  // all loads of a wave's rows first (the inputs overlap no output, so they may fly together), then the stores
  const int nbytes = 3 * tw;
  unsigned val[EP_RPW], text = 0;
  int offs[EP_RPW], lens[EP_RPW];
#pragma unroll
  for (int r = 0; r < EP_RPW; ++r) {
    const int j = wave * EP_RPW + r, y = y0 + j;
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
    if (lane < tw && P.mask_dev[(long long)y * P.mask_pitch + x0 + lane] != 0) text |= 1u << r;
  }
#pragma unroll
  for (int r = 0; r < EP_RPW; ++r) {
    const int j = wave * EP_RPW + r, y = y0 + j;
    if (j >= th) continue;
    uint8_t* dst = P.out_dev + (long long)y * P.out_pitch + 3ll * x0;
    const int off = offs[r], len = lens[r];
    unsigned v = val[r];
    if (survivors) {
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
    if (lane < tw) {
      const bool painted = survivors && (win[j][lane] >> 24) != 0;
      P.rest_dev[(long long)y * P.rest_pitch + x0 + lane] = (!painted && (((text | restf) >> r) & 1u)) ? 255 : 0;
    }
  }
}

}  // namespace

void launch_erase_stats(const ctd_erase_job* jobs, int n_blocks, const ctd_erase_page* pages, int n_pages,
                        const ctd_erase_params& prm, ctd_erase_row* rows, hipStream_t st) {
  hipLaunchKernelGGL(erase_stats_kernel, dim3(n_blocks), dim3(ES_THREADS), 0, st, jobs, pages, n_pages, prm, rows);
}

void launch_erase_paint(const ctd_erase_job* jobs, int n_blocks, const ctd_erase_page* pages, int n_pages,
                        const ctd_erase_params& prm, const ctd_erase_row* rows, hipStream_t st) {
  hipLaunchKernelGGL(erase_paint_kernel, dim3(prm.n_tiles), dim3(EP_THREADS), 0, st, jobs, n_blocks, pages, n_pages, prm, rows);
}
