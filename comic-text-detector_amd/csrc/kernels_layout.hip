// Layout boxes (`ctd_layout_boxes`; the rule is stated in include/ctd_hip.h and restated in numpy, with the row-histogram /
// stack enumeration of maximal rectangles, in tests/layout_ref.py): per block whose balloon row says OK, the largest
// axis-aligned rectangle inside the balloon region eroded by `inset`, and the largest one that contains the block's anchor.
// Integers only; the order among rectangles is total, so the answer is a function of the plane whatever enumerates them.
//
// layout_kernel, ONE launch, one workgroup per block, two bit planes of the window in dynamic LDS (nw = ceil(ww / 64)
// 64-bit words a row, at most CTD_BALLOON_MAX_WORDS words each; the launch is sized by params.max_words):
//   load    B_b from bits_dev into plane A (read only; the last word of a row is masked to the window).  This step and the
//           next are layout_bits.h's `load_eroded`, shared with kernels_fit.hip.
//   erode   by shifted ANDs: rows A -> Q (shifts cross the word boundaries of a row, zeros come in at the window's sides),
//           columns Q -> A = E_b (rows beyond the window count as zero); |E_b| by popcount on the way.
//   search  one thread a top row y, no barrier: for k = 1, 2, ... the row P_k[y] = E[y] & ... & E[y + k - 1] is kept in
//           plane Q and updated in place, P[y] &= E[y + k - 1].  Only when a word of it changed is the row looked at again:
//           its leftmost longest run of ones (per word the leading run, the trailing run and the leftmost longest run inside
//           by six doubling steps; joined across the words by a carry) and, for y <= ay, the run that contains column ax.
//           Each step offers run * k to the thread's best rectangle, and the anchored run * k once y + k > ay.  The row ends
//           when P_k[y] is empty or y + k reaches wh: P_{k+1} is a subset of P_k, so there is no other cap on k.
//           Every maximal rectangle has a top row y and a height k at which it is the row's run; the candidates that are not
//           maximal are rectangles of E_b all the same, so offering them changes nothing.  Ties are compared in full.
//   reduce  the order (area, then smaller y1, x1, y2) over the wave by shuffles, one LDS step across the waves; thread 0
//           writes the row with ordinary stores.
// Worst case: an all-ones 64 x 8192 window (nw = 1): 8192 top rows of up to 8192 steps each, 16 rows a thread, and every
// step is one AND and one comparison because no row ever changes after its first step.
#include <mutex>

#include "layout_bits.h"

namespace {

using namespace lybits;                                    // u64, LY_THREADS, hero3 / load_eroded, run_at

constexpr int LY_MAX_DEVICES = 64;
static_assert(sizeof(ctd_layout_job) == 32 && sizeof(ctd_layout_params) == 16 && sizeof(ctd_layout_row) == 48,
              "layout ABI sizes (layout.py dtypes)");
static_assert(offsetof(ctd_layout_job, ax) == 16 && offsetof(ctd_layout_job, word0) == 24 && offsetof(ctd_layout_row, rect) == 12 &&
              offsetof(ctd_layout_row, a_area) == 28 && offsetof(ctd_layout_row, a_rect) == 32 && alignof(ctd_layout_row) == 4,
              "layout ABI offsets");

// a rectangle of the search, in window coordinates; area 0: none yet
struct Rect {
  int area, y1, x1, y2;
};

__device__ __forceinline__ bool better(const Rect& a, const Rect& b) {
  if (a.area != b.area) return a.area > b.area;
  if (a.y1 != b.y1) return a.y1 < b.y1;
  if (a.x1 != b.x1) return a.x1 < b.x1;
  return a.y2 < b.y2;
}

__device__ __forceinline__ void offer(Rect& best, int w, int y, int x, int k) {
  const Rect c = {w * k, y, x, y + k};
  if (better(c, best)) best = c;
}

// the leftmost longest run of ones of a word that is neither 0 nor all ones: s2, s4, ... mark the starts of runs of at
// least that length; the length is built from its binary digits, highest first, `at` keeping the starts of runs of `len`
__device__ __forceinline__ void word_run(u64 x, int& len, int& pos) {
  const u64 s2 = x & (x >> 1), s4 = s2 & (s2 >> 2), s8 = s4 & (s4 >> 4), s16 = s8 & (s8 >> 8), s32 = s16 & (s16 >> 16);
  u64 at = ~0ull, t;
  int n = 0;
  t = s32;
  if (t) at = t, n = 32;
  t = at & (s16 >> n);
  if (t) at = t, n += 16;
  t = at & (s8 >> n);
  if (t) at = t, n += 8;
  t = at & (s4 >> n);
  if (t) at = t, n += 4;
  t = at & (s2 >> n);
  if (t) at = t, n += 2;
  t = at & (x >> n);
  if (t) at = t, n += 1;
  len = n, pos = __builtin_ctzll(at);
}

// the leftmost longest run of ones of a row of nw words: its width (0: the row is empty) and first column
__device__ __forceinline__ void row_run(const u64* __restrict__ p, int nw, int& width, int& x) {
  int bw = 0, bx = 0, cur = 0, cx = 0;                       // cur: the run that reaches the end of the words so far, from cx
  for (int j = 0; j < nw; ++j) {
    const u64 w = p[j];
    if (w == ~0ull) {
      if (!cur) cx = 64 * j;
      cur += 64;
      continue;
    }
    const int lead = __builtin_ctzll(~w);
    if (cur + lead > bw) bw = cur + lead, bx = cur ? cx : 64 * j;
    cur = 0;
    if (w) {
      int len, pos;
      word_run(w, len, pos);
      if (len > bw) bw = len, bx = 64 * j + pos;
      cur = __builtin_clzll(~w), cx = 64 * j + 64 - cur;
    }
  }
  if (cur > bw) bw = cur, bx = cx;
  width = bw, x = bx;
}

__device__ __forceinline__ Rect shfl_down(const Rect& r, int d) {
  return {__shfl_down(r.area, d, 64), __shfl_down(r.y1, d, 64), __shfl_down(r.x1, d, 64), __shfl_down(r.y2, d, 64)};
}

__global__ __launch_bounds__(LY_THREADS) void layout_kernel(const ctd_layout_job* __restrict__ jobs,
                                                            const ctd_balloon_row* __restrict__ brows, ctd_layout_params prm,
                                                            const u64* __restrict__ bits, ctd_layout_row* __restrict__ rows) {
  extern __shared__ u64 planes[];                          // A / E: words 0 .. max_words - 1, Q / P: max_words .. 2 max_words - 1
  __shared__ int red[LY_WAVES][12];                        // free rectangle, anchored rectangle, n_inner
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const ctd_layout_job J = jobs[blockIdx.x];
  int* __restrict__ out = (int*)(rows + blockIdx.x);       // twelve int32: the row is 4-byte aligned, no more

  // ---- the window and what the block may read (block-uniform, before any word is read)
  const int wx1 = J.win[0], wy1 = J.win[1];
  const long long ww_ll = max((long long)J.win[2] - wx1, 0ll), wh_ll = max((long long)J.win[3] - wy1, 0ll);
  const long long nw_ll = (ww_ll + 63) >> 6, words_ll = ww_ll > 0 && wh_ll > 0 ? nw_ll * wh_ll : 0ll;
  const bool has_row = (int)blockIdx.x < prm.n_rows && brows[blockIdx.x].status == CTD_BALLOON_OK;
  if (!has_row || words_ll > (long long)min(prm.max_words, CTD_BALLOON_MAX_WORDS) || words_ll == 0) {
    if (t == 0) {
      out[0] = has_row && words_ll == 0 ? CTD_LAYOUT_EMPTY : CTD_LAYOUT_NO_REGION;
#pragma unroll
      for (int c = 1; c < 12; ++c) out[c] = 0;
    }
    return;
  }
  const int ww = (int)ww_ll, wh = (int)wh_ll, nw = (int)nw_ll, m = prm.inset;
  u64* __restrict__ A = planes;
  u64* __restrict__ Q = planes + prm.max_words;

  // ---- load B_b and erode it: plane A = E_b, |E_b| by popcount on the way
  int n_inner = load_eroded(A, Q, bits + J.word0, ww, wh, nw, m, t);

  // ---- search: one thread a top row; plane Q holds P_k[y] of every row, each touched by its own thread alone
  const bool anchored = J.ax >= wx1 && J.ax < J.win[2] && J.ay >= wy1 && J.ay < J.win[3];
  const int acx = anchored ? J.ax - wx1 : 0, acy = anchored ? J.ay - wy1 : -1;
  Rect best = {0, 0, 0, 0}, a_best = {0, 0, 0, 0};
  for (int y = t; y < wh; y += LY_THREADS) {
    u64* __restrict__ p = Q + y * nw;
    int width = 0, x = 0, ax1 = 0, ax2 = 0;
    bool a_live = y <= acy;                                  // column ax is still set in P_k[y]
    for (int k = 1; y + k <= wh; ++k) {
      const u64* __restrict__ e = A + (y + k - 1) * nw;
      bool changed = k == 1;
      if (k == 1) {
        for (int j = 0; j < nw; ++j) p[j] = e[j];
      } else {
        for (int j = 0; j < nw; ++j) {
          const u64 was = p[j], now = was & e[j];
          if (now != was) p[j] = now, changed = true;
        }
      }
      if (changed) {
        row_run(p, nw, width, x);
        if (!width) break;
        if (a_live) a_live = run_at(p, nw, acx, ax1, ax2);
      }
      offer(best, width, y, x, k);
      if (a_live && y + k > acy) offer(a_best, ax2 - ax1, y, ax1, k);
    }
  }

  // ---- reduce by the order
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const Rect o = shfl_down(best, d), ao = shfl_down(a_best, d);
    if (better(o, best)) best = o;
    if (better(ao, a_best)) a_best = ao;
    n_inner += __shfl_down(n_inner, d, 64);
  }
  if (lane == 0) {
    red[wave][0] = best.area, red[wave][1] = best.y1, red[wave][2] = best.x1, red[wave][3] = best.y2;
    red[wave][4] = a_best.area, red[wave][5] = a_best.y1, red[wave][6] = a_best.x1, red[wave][7] = a_best.y2;
    red[wave][8] = n_inner;
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < LY_WAVES; ++w) {
      const Rect o = {red[w][0], red[w][1], red[w][2], red[w][3]}, ao = {red[w][4], red[w][5], red[w][6], red[w][7]};
      if (better(o, best)) best = o;
      if (better(ao, a_best)) a_best = ao;
      n_inner += red[w][8];
    }
    out[0] = n_inner ? CTD_LAYOUT_OK : CTD_LAYOUT_EMPTY, out[1] = n_inner, out[2] = best.area;
    out[3] = best.area ? wx1 + best.x1 : 0, out[4] = best.area ? wy1 + best.y1 : 0;
    out[5] = best.area ? wx1 + best.x1 + best.area / (best.y2 - best.y1) : 0, out[6] = best.area ? wy1 + best.y2 : 0;
    out[7] = a_best.area;
    out[8] = a_best.area ? wx1 + a_best.x1 : 0, out[9] = a_best.area ? wy1 + a_best.y1 : 0;
    out[10] = a_best.area ? wx1 + a_best.x1 + a_best.area / (a_best.y2 - a_best.y1) : 0, out[11] = a_best.area ? wy1 + a_best.y2 : 0;
  }
}

std::once_flag g_lds_once[LY_MAX_DEVICES];
hipError_t g_lds_rc[LY_MAX_DEVICES];

}  // namespace

hipError_t launch_layout_boxes(const ctd_layout_job* jobs, int n, const ctd_balloon_row* balloon_rows,
                               const uint64_t* bits, const ctd_layout_params& prm, ctd_layout_row* rows, hipStream_t st) {
  // the kernel may ask for more dynamic LDS than the default limit: raised ONCE per device to the most a call can need, so
  // that concurrent callers never see each other's setting
  constexpr int max_bytes = 2 * CTD_BALLOON_MAX_WORDS * (int)sizeof(u64);
  int dev = -1;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  if (dev < 0 || dev >= LY_MAX_DEVICES) return hipErrorInvalidDevice;
  std::call_once(g_lds_once[dev], [dev] {
    g_lds_rc[dev] = hipFuncSetAttribute((const void*)layout_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
  });
  if (g_lds_rc[dev] != hipSuccess) return g_lds_rc[dev];
  const size_t bytes = (size_t)2 * prm.max_words * sizeof(u64);
  hipLaunchKernelGGL(layout_kernel, dim3(n), dim3(LY_THREADS), bytes, st, jobs, balloon_rows, prm, (const u64*)bits, rows);
  return hipGetLastError();
}
