// Balloon regions (`ctd_balloon_regions`; the rule is stated in include/ctd_hip.h and restated in numpy, with a queue flood
// fill, in tests/balloon_ref.py): per block whose erase row says PLAIN, the 4-connected region of balloon-coloured pixels
// around its glyphs inside a window around its box -- area, bounding box, coordinate sums, which window sides it touches --
// and the region itself as a bit plane.  Integers only; a connected component does not depend on the order in which it is
// found, so nothing below can change a bit of the result.
//
// balloon_kernel, ONE launch, one workgroup per block, two bit planes of the window in dynamic LDS (nw = ceil(ww / 64)
// 64-bit words a row, at most CTD_BALLOON_MAX_WORDS words each; the launch is sized to the call's largest window):
//   seed    T_b = M & X_b by one __ballot per 64 mask bytes into plane R, D_g of it by word shifts and ORs: rows R -> O,
//           columns O -> R.  X_b lies g or more inside the window except at a page edge, where D_g is clipped anyway: no halo.
//           (The window, this pass and the reduce are balloon_bits.h's, shared with kernels_footprint.hip.)
//   open    one __ballot per 64 page pixels (three byte loads a lane: rows and pixels have any alignment; a wave loads four
//           consecutive words' pixels before the first compare) of "every channel within tol of the erase row's median",
//           ORed with the seed, into plane O.
//   grow    R to the fixed point of "R contains every open 4-neighbour of R".  A round is a row sweep -- one thread a row:
//           every open run that holds a reached pixel is filled whole, in a word by the carry of an addition (upwards) and
//           the same on the bit-reversed word (downwards), across the words of the row by a carry, left to right and back --
//           and a column sweep -- one thread a word column, top-down then bottom-up: the reached pixels of a row step into
//           the next row's open pixels and fill their runs in the word.  Rounds repeat while any thread changed a word
//           (__syncthreads_or); R only grows inside the finite O, so this ends, and the fixed point is the component union
//           whatever the sweeps' order.  There is no cap on the rounds.
//   reduce  popcount, bounding box, coordinate sums and edge contact per word, wave shuffles, one LDS step across the waves;
//           the plane goes out as aligned 8-byte stores, thread 0 writes the row with ordinary stores.
#include <mutex>

#include "balloon_bits.h"

namespace {

using namespace blbits;

constexpr int BL_COL = 8;                                    // rows a column sweep loads ahead
constexpr int BL_UNROLL = 4;                                 // words a wave stages per step of the open plane
static_assert(sizeof(ctd_balloon_job) == 32 && sizeof(ctd_balloon_params) == 32 && sizeof(ctd_balloon_row) == 48,
              "balloon ABI sizes (balloons.py dtypes)");
static_assert(offsetof(ctd_balloon_job, erase_row) == 20 && offsetof(ctd_balloon_job, word0) == 24 &&
              offsetof(ctd_balloon_row, flags) == 24 && offsetof(ctd_balloon_row, sum_x) == 32, "balloon ABI offsets");

// the bits of `open` in runs of `open` that hold a bit of seed (seed is a subset of open).  Adding the seed to the word
// carries through every run from its lowest seed upwards and flips exactly those bits (and the 0 above the run, which
// `& open` drops; a seed above the lowest stays 1, `| seed`); an all-ones word wraps, which flips the same bits.
__device__ __forceinline__ u64 fill_up(u64 seed, u64 open) { return (((open + seed) ^ open) & open) | seed; }
__device__ __forceinline__ u64 runfill(u64 seed, u64 open) {
  return fill_up(seed, open) | __brevll(fill_up(__brevll(seed), __brevll(open)));
}

__device__ __forceinline__ void zero_row(ctd_balloon_row* row, int status) {
  row->status = status, row->area = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) row->bbox[c] = 0;
  row->flags = 0, row->n_seed = 0, row->sum_x = 0, row->sum_y = 0;
}

__global__ __launch_bounds__(BL_THREADS) void balloon_kernel(const ctd_balloon_job* __restrict__ jobs,
                                                             const ctd_erase_page* __restrict__ pages, int n_pages,
                                                             const ctd_erase_row* __restrict__ erows, ctd_balloon_params prm,
                                                             ctd_balloon_row* __restrict__ rows, u64* __restrict__ bits) {
  extern __shared__ u64 planes[];                          // O: words 0 .. max_words - 1, R: max_words .. 2 max_words - 1
  __shared__ int red_i[BL_WAVES][8];                       // area, n_seed, min x, min y, max x, max y, flags
  __shared__ long long red_l[BL_WAVES][2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const ctd_balloon_job J = jobs[blockIdx.x];
  ctd_balloon_row* __restrict__ row = rows + blockIdx.x;

  // ---- the window, from the box and the page alone (block-uniform, before any pixel is read)
  const bool has_page = J.page >= 0 && J.page < n_pages;
  ctd_erase_page P;
  window w = {0, 0, 0, 0, 0, 0, 0, 0};
  if (has_page) {
    P = pages[J.page];
    w = window_of(J.xyxy, P.W, P.H, prm.reach, prm.reach_min);
  }
  const int wx1 = w.wx1, wy1 = w.wy1, ww = w.ww, wh = w.wh;
  const int nw = (ww + 63) >> 6;
  const long long words_ll = (long long)nw * wh;
  const bool owns = words_ll <= (long long)min(prm.max_words, CTD_BALLOON_MAX_WORDS);   // what fits this launch's planes
  const int words = owns ? (int)words_ll : 0;
  u64* __restrict__ out = bits + J.word0;

  const bool plain = has_page && J.erase_row >= 0 && erows[max(J.erase_row, 0)].status == CTD_ERASE_PLAIN;
  if (!plain || !owns) {                                   // block-uniform
    for (int i = t; i < words; i += BL_THREADS) out[i] = 0ull;
    if (t == 0) zero_row(row, plain ? CTD_BALLOON_TOO_LARGE : CTD_BALLOON_NOT_PLAIN);
    return;
  }
  const ctd_erase_row E = erows[J.erase_row];
  u64* __restrict__ O = planes;
  u64* __restrict__ R = planes + prm.max_words;
  const int g = prm.grow;

  // ---- seed: F_b into R
  int n_seed = load_seed(O, R, P, w, nw, words, g, t);
  // ---- open: near the median in every channel, or seed
  {
    const int lo0 = (int)E.med[0] - prm.tol, hi0 = (int)E.med[0] + prm.tol, lo1 = (int)E.med[1] - prm.tol,
              hi1 = (int)E.med[1] + prm.tol, lo2 = (int)E.med[2] - prm.tol, hi2 = (int)E.med[2] + prm.tol;
    // BL_UNROLL consecutive words a wave and step: their loads are in flight together
    for (int base = wave * BL_UNROLL; base < words; base += BL_WAVES * BL_UNROLL) {
      int c0[BL_UNROLL], c1[BL_UNROLL], c2[BL_UNROLL];
#pragma unroll
      for (int u = 0; u < BL_UNROLL; ++u) {
        const int task = min(base + u, words - 1);
        const int y = task / nw, j = task - y * nw;
        const int x = 64 * j + lane;
        c0[u] = -1, c1[u] = 0, c2[u] = 0;                          // -1: beyond the window, never open
        if (x < ww) {
          const uint8_t* p = P.page_dev + (long long)(wy1 + y) * P.pitch + 3ll * (wx1 + x);
          c0[u] = p[0], c1[u] = p[1], c2[u] = p[2];
        }
      }
#pragma unroll
      for (int u = 0; u < BL_UNROLL; ++u) {
        const bool bit = c0[u] >= lo0 && c0[u] <= hi0 && c1[u] >= lo1 && c1[u] <= hi1 && c2[u] >= lo2 && c2[u] <= hi2;
        const u64 word = __ballot(bit && c0[u] >= 0);
        if (lane == 0 && base + u < words) O[base + u] = word | R[base + u];
      }
    }
  }
  __syncthreads();

  // ---- grow R to the fixed point
  for (;;) {
    int changed = 0;
    for (int y = t; y < wh; y += BL_THREADS) {              // row sweep
      u64* __restrict__ r = R + y * nw;
      const u64* __restrict__ o = O + y * nw;
      u64 carry = 0ull;
      for (int j = 0; j < nw; ++j) {
        const u64 ow = o[j], rw = r[j];
        const u64 s = rw | (carry & ow);
        const u64 f = s ? runfill(s, ow) : 0ull;
        if (f != rw) r[j] = f, changed = 1;
        carry = f >> 63;
      }
      carry = 0ull;
      for (int j = nw - 1; j >= 0; --j) {
        const u64 ow = o[j];
        u64 rw = r[j];
        const u64 s = rw | ((carry << 63) & ow);
        if (s != rw) rw = runfill(s, ow), r[j] = rw, changed = 1;
        carry = rw & 1ull;
      }
    }
    __syncthreads();
    for (int j = t; j < nw; j += BL_THREADS) {              // column sweep: down from row 0, then up from the last row
      u64 prev = R[j];
      for (int dir = 0; dir < 2; ++dir) {
        const int y0 = dir ? wh - 2 : 1, step = dir ? -nw : nw;
        // nobody else writes this word column during the sweep: BL_COL rows' words are loaded before the first is used, so
        // the chain from row to row is arithmetic only
        for (int k = 0; k < wh - 1; k += BL_COL) {
          u64 ow[BL_COL], rw[BL_COL];
          const int at = y0 * nw + j + k * step;
#pragma unroll
          for (int u = 0; u < BL_COL; ++u) {
            ow[u] = 0ull, rw[u] = 0ull;
            if (k + u < wh - 1) ow[u] = O[at + u * step], rw[u] = R[at + u * step];
          }
#pragma unroll
          for (int u = 0; u < BL_COL; ++u) {
            if (k + u < wh - 1) {
              const u64 s = prev & ow[u] & ~rw[u];
              if (s) rw[u] = runfill(rw[u] | s, ow[u]), R[at + u * step] = rw[u], changed = 1;
              prev = rw[u];
            }
          }
        }
      }
    }
    if (!__syncthreads_or(changed)) break;
  }

  // ---- the plane goes out; area, box, sums, contact
  tally a = tally_none();
  for (int i = t; i < words; i += BL_THREADS) {
    const u64 rw = R[i];
    out[i] = rw;
    tally_word(a, rw, i, nw, w);
  }
  write_row(a, n_seed, red_i, red_l, row, w, P.W, P.H, 0, t);
}

std::once_flag g_lds_once[BL_MAX_DEVICES];
hipError_t g_lds_rc[BL_MAX_DEVICES];

}  // namespace

hipError_t launch_balloon_regions(const ctd_balloon_job* jobs, int n, const ctd_erase_page* pages, int n_pages,
                                  const ctd_erase_row* erase_rows, const ctd_balloon_params& prm, ctd_balloon_row* rows,
                                  uint64_t* bits, hipStream_t st) {
  // the kernel may ask for more dynamic LDS than the default limit: raised ONCE per device to the most a call can need, so
  // that concurrent callers never see each other's setting
  constexpr int max_bytes = 2 * CTD_BALLOON_MAX_WORDS * (int)sizeof(u64);
  int dev = -1;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  if (dev < 0 || dev >= BL_MAX_DEVICES) return hipErrorInvalidDevice;
  std::call_once(g_lds_once[dev], [dev] {
    g_lds_rc[dev] = hipFuncSetAttribute((const void*)balloon_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
  });
  if (g_lds_rc[dev] != hipSuccess) return g_lds_rc[dev];
  const size_t bytes = (size_t)2 * prm.max_words * sizeof(u64);
  hipLaunchKernelGGL(balloon_kernel, dim3(n), dim3(BL_THREADS), bytes, st, jobs, pages, n_pages, erase_rows, prm, rows,
                     (u64*)bits);
  return hipGetLastError();
}
