// Footprint regions (`ctd_balloon_footprints`; the rule is stated in include/ctd_hip.h and restated in numpy, with per-row and
// per-column spans, in tests/footprint_ref.py): per block whose erase row says TEXTURED or NO_RING -- text off a plain
// background, for which the balloon rule has no region -- the place where the old text stood: the orthogonally convex closure
// of the block's filled glyphs, padded, minus other blocks' text, written as an OK balloon row and a bit plane in the balloon
// layout.  Integers only; the smallest orthogonally convex superset is unique, so no sweep order can change a bit.
//
// footprint_kernel, ONE launch behind the balloon launch, one workgroup per block, two bit planes of the window in dynamic
// LDS (as balloon_kernel; the window, the seed and the reduce are balloon_bits.h's).  A block that is not eligible returns
// before it reads a pixel or writes anything.
//   seed     F_b into plane R: one __ballot per 64 mask bytes, rows and columns dilated by g.
//   closure  R to the fixed point of "a row's and a column's pixels between two pixels of R are in R".  A round is a row sweep
//            -- one thread a row: from the lowest set bit of the row's first non-zero word to the highest of its last,
//            every bit is set -- and a column sweep -- one wave a word column, one lane a row, 64 rows a step: going down, the
//            OR over the rows so far (six shuffle steps, a carry from step to step) goes into plane O; coming up, the OR over
//            the rows from here on stays in registers and `prefix & suffix` is stored.  Both stay inside the rows and
//            words of X_b grown by g, which hold F_b and so its closure.  Rounds repeat while any thread changed a word
//            (__syncthreads_or); R only grows inside that finite box, so this ends.  There is no cap on the rounds.
//   pad      the same word-shift dilation by `pad`, over the whole window, the last word of a row masked to it.
//   holes    one __ballot per 64 mask bytes of "mask != 0 and outside X_b" into plane O, only where R has a bit.
//   reduce   R & ~O goes out as aligned 8-byte stores; popcount, box, sums and contact per word, wave shuffles, one LDS step
//            across the waves, thread 0 writes the row with ordinary stores.
#include <mutex>

#include "balloon_bits.h"

namespace {

using namespace blbits;

static_assert(sizeof(ctd_footprint_params) == 32, "footprint ABI size (balloons.py)");
static_assert(CTD_FOOTPRINT_MAX_PAD < 64, "a dilation shift stays inside the neighbouring word");

// the OR of a value over the lanes up to and including this one / from this one on: six shuffle steps
__device__ __forceinline__ u64 scan_or_up(u64 v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_up(v, d, 64);
    if (lane >= d) v |= o;
  }
  return v;
}
__device__ __forceinline__ u64 scan_or_down(u64 v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_down(v, d, 64);
    if (lane + d < 64) v |= o;
  }
  return v;
}

__global__ __launch_bounds__(BL_THREADS) void footprint_kernel(const ctd_balloon_job* __restrict__ jobs,
                                                               const ctd_erase_page* __restrict__ pages, int n_pages,
                                                               const ctd_erase_row* __restrict__ erows, ctd_footprint_params prm,
                                                               ctd_balloon_row* __restrict__ rows, u64* __restrict__ bits) {
  extern __shared__ u64 planes[];                          // O: words 0 .. max_words - 1, R: max_words .. 2 max_words - 1
  __shared__ int red_i[BL_WAVES][8];                       // area, n_seed, min x, min y, max x, max y, flags
  __shared__ long long red_l[BL_WAVES][2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const ctd_balloon_job J = jobs[blockIdx.x];

  // ---- eligible?  Block-uniform, from the tables alone
  if (J.page < 0 || J.page >= n_pages || J.erase_row < 0) return;
  const int estatus = erows[J.erase_row].status;
  if (estatus != CTD_ERASE_TEXTURED && estatus != CTD_ERASE_NO_RING) return;
  const ctd_erase_page P = pages[J.page];
  const window w = window_of(J.xyxy, P.W, P.H, prm.reach, prm.reach_min);
  const int wx1 = w.wx1, wy1 = w.wy1, ww = w.ww, wh = w.wh;
  const int nw = (ww + 63) >> 6;
  if ((long long)nw * wh > (long long)min(prm.max_words, CTD_BALLOON_MAX_WORDS)) return;   // what fits this launch's planes
  const int words = nw * wh;
  u64* __restrict__ out = bits + J.word0;
  u64* __restrict__ O = planes;
  u64* __restrict__ R = planes + prm.max_words;
  const int g = prm.grow;

  // ---- seed: F_b into R
  const int n_seed = load_seed(O, R, P, w, nw, words, g, t);

  // ---- closure, inside the window rows y0 .. y1 - 1 and the words j0 .. j1 - 1 of X_b grown by g
  {
    const int y0 = max(w.by1 - g - wy1, 0), y1 = min(w.by2 + g - wy1, wh);
    const int j0 = max(w.bx1 - g - wx1, 0) >> 6, j1 = min((min(w.bx2 + g - wx1, ww) + 63) >> 6, nw);
    for (;;) {
      int changed = 0;
      for (int y = y0 + t; y < y1; y += BL_THREADS) {         // row sweep
        u64* __restrict__ r = R + y * nw;
        int jf = j0, jl = j1 - 1;
        while (jf < j1 && !r[jf]) ++jf;
        if (jf == j1) continue;
        while (!r[jl]) --jl;
        const u64 from = ~0ull << (__ffsll((long long)r[jf]) - 1), to = ~0ull >> __clzll((long long)r[jl]);
        for (int j = jf; j <= jl; ++j) {
          u64 m = ~0ull;
          if (j == jf) m &= from;
          if (j == jl) m &= to;
          if (r[j] != m) r[j] = m, changed = 1;
        }
      }
      __syncthreads();
      for (int j = j0 + wave; j < j1; j += BL_WAVES) {        // column sweep: one wave a word column, one lane a row
        u64 carry = 0ull;
        for (int yb = y0; yb < y1; yb += 64) {                // down: the prefix into O
          const int y = yb + lane;
          const u64 p = scan_or_up(y < y1 ? R[y * nw + j] : 0ull, lane) | carry;
          if (y < y1) O[y * nw + j] = p;
          carry = __shfl(p, 63, 64);
        }
        carry = 0ull;
        for (int yb = y0 + ((y1 - y0 - 1) & ~63); yb >= y0; yb -= 64) {   // up: prefix & suffix, by the lane that stored the prefix
          const int y = yb + lane;
          const u64 rw = y < y1 ? R[y * nw + j] : 0ull;
          const u64 sfx = scan_or_down(rw, lane) | carry;
          if (y < y1) {
            const u64 v = O[y * nw + j] & sfx;
            if (v != rw) R[y * nw + j] = v, changed = 1;
          }
          carry = __shfl(sfx, 0, 64);
        }
      }
      if (!__syncthreads_or(changed)) break;
    }
  }

  // ---- pad: P_b into R
  dilate_plane(R, O, nw, wh, words, prm.pad, last_valid_of(ww), t);

  // ---- holes: other text, N_b, into O where R has a bit to lose
  for (int task = wave; task < words; task += BL_WAVES) {
    u64 word = 0ull;
    if (R[task]) {                                            // wave-uniform
      const int y = task / nw, j = task - y * nw;
      const int x = 64 * j + lane, px = wx1 + x, py = wy1 + y;
      bool bit = false;
      if (x < ww && !(py >= w.by1 && py < w.by2 && px >= w.bx1 && px < w.bx2))
        bit = P.mask_dev[(long long)py * P.mask_pitch + px] != 0;
      word = __ballot(bit);
    }
    if (lane == 0) O[task] = word;
  }
  __syncthreads();

  // ---- B_b goes out; area, box, sums, contact
  tally a = tally_none();
  for (int i = t; i < words; i += BL_THREADS) {
    const u64 rw = R[i] & ~O[i];
    out[i] = rw;
    tally_word(a, rw, i, nw, w);
  }
  write_row(a, n_seed, red_i, red_l, rows + blockIdx.x, w, P.W, P.H, CTD_BALLOON_FOOTPRINT, t);
}

std::once_flag g_lds_once[BL_MAX_DEVICES];
hipError_t g_lds_rc[BL_MAX_DEVICES];

}  // namespace

hipError_t launch_balloon_footprints(const ctd_balloon_job* jobs, int n, const ctd_erase_page* pages, int n_pages,
                                     const ctd_erase_row* erase_rows, const ctd_footprint_params& prm, ctd_balloon_row* rows,
                                     uint64_t* bits, hipStream_t st) {
  // the kernel may ask for more dynamic LDS than the default limit: raised ONCE per device to the most a call can need, so
  // that concurrent callers never see each other's setting
  constexpr int max_bytes = 2 * CTD_BALLOON_MAX_WORDS * (int)sizeof(u64);
  int dev = -1;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  if (dev < 0 || dev >= BL_MAX_DEVICES) return hipErrorInvalidDevice;
  std::call_once(g_lds_once[dev], [dev] {
    g_lds_rc[dev] = hipFuncSetAttribute((const void*)footprint_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
  });
  if (g_lds_rc[dev] != hipSuccess) return g_lds_rc[dev];
  const size_t bytes = (size_t)2 * prm.max_words * sizeof(u64);
  hipLaunchKernelGGL(footprint_kernel, dim3(n), dim3(BL_THREADS), bytes, st, jobs, pages, n_pages, erase_rows, prm, rows,
                     (u64*)bits);
  return hipGetLastError();
}
