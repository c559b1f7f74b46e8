// Shaped fit (`ctd_layout_fit`; the rule is stated in include/ctd_hip.h and restated in numpy, glyph by glyph, in
// tests/fit_ref.py): per block whose balloon row says OK, the largest candidate size at which the block's glyph run sets in
// line slots that follow the balloon region eroded by `inset`, symmetric about the anchor's column.  Integers only.
//
// fit_kernel, ONE launch, one workgroup per block, layout_kernel's two bit planes in dynamic LDS (layout_bits.h):
//   load    B_b into plane A and erode it by the shifted ANDs layout_kernel uses: A = E_b, plane Q is free.
//   table   one thread a row: the run of ones of E_b's row y that contains column ax as two int16 (l, r) in plane Q -- a window
//           has at most 8192 rows, 32 KB of the 64-KB plane; a row without such a run is (32767, 0), which no max / min
//           survives.  The slot of rows t .. t + h - 1 is the max l and the min r of the table over those rows.
//   walk    one thread a (candidate, n) pair, 16 x 32 = 512 pairs = the block: lanes 0 .. 31 of a wave hold n = 1 .. 32 of an
//           even candidate, lanes 32 .. 63 those of the odd one behind it.  A thread walks its stack of n lines: the slot,
//           then the line's end by a binary search in the candidate's cumulative advances (global memory, at most
//           CTD_FIT_MAX_GLYPHS + 1 int32, read by 32 lanes at once: cache lines shared), then back to the last allowed break.
//           It stops at the first line that has no slot, that does not hold its first glyph, or that has no glyph left.
//   reduce  a ballot gives the smallest n that fits per candidate, one LDS word a candidate; the largest candidate with one
//           wins.  Thread 0 walks the winning stack once more and writes its line records; the threads behind it zero the
//           records beyond n_lines.  Ordinary stores, each int32 of the row written once.
// Worst case: a 64 x 8192 window with h = 1 and n = 32 is 32 table reads and 32 searches a thread; a stack of tall lines
// reads at most the window's rows once.
//
// fit_balanced_kernel (`ctd_layout_fit_balanced`; the rule is the header's "balanced lines", restated in tests/balance_ref.py) is
// the same kernel up to the winner; then, in the same block, while the axis-run table is still in LDS:
//   greedy  thread 0 walks the winning stack into LDS records: the slots' widths w_k and the forward-greedy starts f_k.
//   bands   thread 0: line k of an admissible vector starts in lo_k .. f_k, lo_k the backward-greedy start (the smallest s with
//           cum[s] >= cum[lo_(k+1)] - w_k, breaks ignored, at least k).  The states of all lines lie one band behind the other,
//           int64 each: in plane A where their number is at most max_words (E_b is not read after the table), else in the
//           block's part of the workspace, 256 (G_j + 1) bytes a block j in front of it (summed by the block).
//   table   g(k, s), the least cost of lines k .. n - 1 from glyph s, line by line from the last: one state a thread, 512 at
//           a time; a state that is no allowed boundary is INF at once, the others search the furthest end in `cum` and
//           scan the ends inside line k + 1's band.  A barrier a line.
//   forward from s = 0 the largest end that attains g(k, s), found by all threads with an LDS max; a barrier a line.
//   rows    where g(0, 0) is INF the greedy records stand.  One int32 of the two rows a thread, each written once.
// Worst case: the pruning is sound without being needed for the result (every end is checked in full), so a state's work is
// bounded by the glyphs that fit its slot and a line's by its band: at most 32 x 4097 states of at most 4096 ends over 512
// threads, and far less wherever the greedy stack needs its 32 lines because its slots are nearly full.
#include <mutex>

#include "layout_bits.h"

namespace {

using namespace lybits;

constexpr int FT_MAX_DEVICES = 64;
constexpr int FT_ROW_INTS = (int)(sizeof(ctd_fit_row) / 4);
static_assert(sizeof(ctd_fit_job) == 24 && sizeof(ctd_fit_cand) == 16 && sizeof(ctd_fit_params) == 32 &&
                  sizeof(ctd_fit_line) == 20 && sizeof(ctd_fit_row) == 16 + 20 * CTD_FIT_MAX_LINES,
              "fit ABI sizes (layout.py dtypes)");
static_assert(offsetof(ctd_fit_job, break0) == 16 && offsetof(ctd_fit_cand, cum0) == 8 && offsetof(ctd_fit_params, n_cum) == 16 &&
                  offsetof(ctd_fit_row, lines) == 16 && alignof(ctd_fit_row) == 4,
              "fit ABI offsets");
static_assert(CTD_FIT_MAX_CANDS * CTD_FIT_MAX_LINES == LY_THREADS, "one (candidate, n) pair a thread");
static_assert(CTD_FIT_MAX_LINES == 32, "two candidates a wave: the ballot's halves");
static_assert(FT_ROW_INTS <= LY_THREADS, "one int32 of the row a thread");
static_assert(CTD_BALLOON_MAX_WORDS * 8 >= 8192 * 4, "the axis-run table fits plane Q");
constexpr int FT_BAL_INTS = (int)(sizeof(ctd_fit_balance) / 4);
static_assert(sizeof(ctd_fit_balance) == 16 && offsetof(ctd_fit_balance, cost) == 8, "balance ABI (layout.py dtype)");
static_assert(FT_ROW_INTS + FT_BAL_INTS <= LY_THREADS, "one int32 of both rows a thread");
static_assert(fit_work_block_bytes(1) % 8 == 0 && fit_work_block_bytes(CTD_FIT_MAX_GLYPHS) >= 8ll * CTD_FIT_MAX_LINES * (CTD_FIT_MAX_GLYPHS + 1),
              "a block's part of the workspace holds 32 bands of G + 1 int64 states");
constexpr long long FT_INF = 1ll << 62;                    // no admissible vector; a cost is below 2^35

// the window's axis-run table and the block's run
struct Fit {
  const short2* tab;                 // per window row (l, r); (32767, 0): none
  int wh, acx, acy;                  // the window's rows, the anchor in window coordinates
  int G;
  const int* __restrict__ cum;       // the candidate's G + 1 cumulative advances
  const uint8_t* __restrict__ brk;   // G break bytes, or null
};

// Whether the stack of n lines of height h, g apart, fits; with `out` the line records are written on the way (page
// coordinates: the window's corner is (wx1, wy1)), which is meant for a stack that is known to fit.
__device__ __forceinline__ bool walk(const Fit& F, int h, int g, int n, int* __restrict__ out, int wx1, int wy1) {
  if (h > F.wh) return false;
  const long long total = (long long)n * h + (long long)(n - 1) * g;
  long long top = (long long)F.acy - (total >> 1);
  int s = 0;
  for (int k = 0; k < n; ++k, top += (long long)h + g) {
    if (s >= F.G) return false;                               // a line without a glyph
    if (top < 0 || top + h > F.wh) return false;              // the stack passes the window
    int L = 0, R = 32767;
    for (int y = (int)top; y < (int)top + h; ++y) {
      const short2 v = F.tab[y];
      L = max(L, (int)v.x), R = min(R, (int)v.y);
    }
    if (L > F.acx || R <= F.acx) return false;                // a row of the line has no axis run
    const int half = min(F.acx - L, R - F.acx), width = 2 * half;
    // the largest e in s .. G with cum[e] - cum[s] <= width
    const long long lim = (long long)F.cum[s] + width;
    int lo = s, hi = F.G;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((long long)F.cum[mid] <= lim) lo = mid;
      else hi = mid - 1;
    }
    int end = lo;
    if (end == s) return false;                               // the line's first glyph does not fit its slot
    if (end < F.G && F.brk) {
      for (int j = end - 1; j >= s; --j)
        if (F.brk[j]) {
          end = j + 1;
          break;
        }
    }
    if (out) {
      int* __restrict__ rec = out + 5 * k;
      rec[0] = s, rec[1] = wx1 + F.acx - half, rec[2] = wy1 + (int)top, rec[3] = width, rec[4] = F.cum[end] - F.cum[s];
    }
    s = end;
  }
  return s == F.G;
}

// whether a line may end in front of glyph e (1 <= e <= G)
__device__ __forceinline__ bool may_end(const Fit& F, int e) { return e == F.G || !F.brk || F.brk[e - 1]; }

// The balanced lines of the winning stack of n lines (F.cum is the winner's): every thread of the block calls it, behind a
// barrier after which plane A and the static LDS of the walk are free.  Writes both rows.
__device__ __forceinline__ void balance_block(const Fit& F, int h, int g, int n, int inner, int wc, int wx1, int wy1,
                                              long long* lds_g, int lds_states, const ctd_fit_job* __restrict__ fjobs,
                                              long long* work, long long work_bytes, int* __restrict__ out,
                                              int* __restrict__ bal) {
  __shared__ int s_rec[5 * CTD_FIT_MAX_LINES];             // the greedy records
  __shared__ int s_lo[CTD_FIT_MAX_LINES], s_off[CTD_FIT_MAX_LINES + 1];   // a line's band starts at lo, its states at off
  __shared__ int s_start[CTD_FIT_MAX_LINES + 1];           // the answer's s_0 .. s_n
  __shared__ int s_pick;
  __shared__ long long s_sum[LY_WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, G = F.G;
  if (t == 0) {
    walk(F, h, g, n, s_rec, wx1, wy1);
    int lo_next = G;
    s_off[0] = 0;
    for (int k = n - 1; k >= 1; --k) {
      // the smallest s in 0 .. lo_next with cum[s] >= cum[lo_next] - w_k
      const long long need = (long long)F.cum[lo_next] - s_rec[5 * k + 3];
      int lo = 0, hi = lo_next;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)F.cum[mid] >= need) hi = mid;
        else lo = mid + 1;
      }
      lo_next = s_lo[k] = min(max(lo, k), s_rec[5 * k]);   // never behind the greedy start: a band has a state
    }
    s_lo[0] = 0;
    for (int k = 0; k < n; ++k) s_off[k + 1] = s_off[k] + s_rec[5 * k] - s_lo[k] + 1;
  }
  __syncthreads();
  // ---- where the states live (block-uniform)
  const int states = s_off[n];
  long long* gt = lds_g;
  bool have = states <= lds_states;
  if (!have) {
    long long before = 0;                                  // the bytes of the blocks in front of this one
    for (int j = t; j < (int)blockIdx.x; j += LY_THREADS) before += fit_work_block_bytes(fjobs[j].n_glyphs);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) before += __shfl_down(before, d, 64);
    if (lane == 0) s_sum[wave] = before;
    __syncthreads();
    before = 0;
    for (int w = 0; w < LY_WAVES; ++w) before += s_sum[w];
    have = work && before + 8ll * states <= work_bytes && 8ll * states <= fit_work_block_bytes(G);
    gt = work + (before >> 3);
  }
  if (have) {
    // ---- g(k, s), from the last line
    for (int k = n - 1; k >= 0; --k) {
      const int lo = s_lo[k], hi = s_rec[5 * k], wk = s_rec[5 * k + 3];
      const int lo1 = k + 1 < n ? s_lo[k + 1] : G, hi1 = k + 1 < n ? s_rec[5 * k + 5] : G;
      const long long* g1 = gt + s_off[k + 1] - lo1;
      for (int s = lo + t; s <= hi; s += LY_THREADS) {
        long long best = FT_INF;
        if (k == 0 || may_end(F, s)) {
          const long long base = F.cum[s], lim = base + wk;
          int a = s, b = G;                                // the largest e in s .. G with cum[e] <= lim
          while (a < b) {
            const int mid = (a + b + 1) >> 1;
            if ((long long)F.cum[mid] <= lim) a = mid;
            else b = mid - 1;
          }
          const int e1 = min(a, hi1);
          for (int e = max(s + 1, lo1); e <= e1; ++e) {
            if (!may_end(F, e)) continue;
            const long long rest = k + 1 < n ? g1[e] : 0ll;
            if (rest >= FT_INF) continue;
            const long long d = lim - F.cum[e];
            best = min(best, d * d + rest);
          }
        }
        gt[s_off[k] + s - lo] = best;
      }
      __syncthreads();
    }
    have = gt[0] < FT_INF;
  }
  if (have) {
    // ---- forward: the largest end that attains g(k, s)
    if (t == 0) s_start[0] = 0;
    for (int k = 0; k < n; ++k) {
      if (t == 0) s_pick = -1;
      __syncthreads();
      const int s = s_start[k], wk = s_rec[5 * k + 3];
      const int lo1 = k + 1 < n ? s_lo[k + 1] : G, hi1 = k + 1 < n ? s_rec[5 * k + 5] : G;
      const long long* g1 = gt + s_off[k + 1] - lo1;
      const long long want = gt[s_off[k] + s - s_lo[k]], lim = (long long)F.cum[s] + wk;
      for (int e = max(s + 1, lo1) + t; e <= hi1; e += LY_THREADS) {
        const long long d = lim - F.cum[e];
        if (d < 0 || !may_end(F, e)) continue;
        const long long rest = k + 1 < n ? g1[e] : 0ll;
        if (rest < FT_INF && d * d + rest == want) atomicMax(&s_pick, e);
      }
      __syncthreads();
      if (t == 0) s_start[k + 1] = s_pick;
      __syncthreads();
      if (s_start[k + 1] < 0) {                             // never, where `cum` keeps its precondition
        have = false;
        break;
      }
    }
    have = have && s_start[n] == G;
  }
  // ---- the rows: one int32 a thread
  if (t < 4) {
    out[t] = t == 0 ? CTD_FIT_OK : t == 1 ? wc : t == 2 ? n : inner;
  } else if (t < FT_ROW_INTS) {
    const int k = (t - 4) / 5, f = (t - 4) % 5;
    int v = 0;
    if (k < n) {
      v = s_rec[5 * k + f];
      if (have && f == 0) v = s_start[k];
      if (have && f == 4) v = F.cum[s_start[k + 1]] - F.cum[s_start[k]];
    }
    out[t] = v;
  } else if (t < FT_ROW_INTS + FT_BAL_INTS) {
    long long cost = 0;
    if (have) {
      cost = gt[0];
    } else {
      for (int k = 0; k < n; ++k) {
        const long long d = s_rec[5 * k + 3] - s_rec[5 * k + 4];
        cost += d * d;
      }
    }
    const int f = t - FT_ROW_INTS;
    bal[f] = f == 0 ? (int)have : f == 1 ? 0 : f == 2 ? (int)(unsigned)cost : (int)(cost >> 32);
  }
}

// a row of zeros behind its status; with BAL the balance row's zeros too
template <bool BAL>
__device__ __forceinline__ void no_row(int* __restrict__ out, int* __restrict__ bal, int t, int status) {
  if (t < FT_ROW_INTS) out[t] = t == 0 ? status : 0;
  else if (BAL && t < FT_ROW_INTS + FT_BAL_INTS) bal[t - FT_ROW_INTS] = 0;
}

// The block's work.  BAL: ctd_layout_fit_balanced's; without it `bals`, `work` and `work_bytes` are not read
template <bool BAL>
__device__ __forceinline__ void fit_block(const ctd_layout_job* __restrict__ jobs, const ctd_fit_job* __restrict__ fjobs,
                                          const ctd_balloon_row* __restrict__ brows, const ctd_fit_params prm,
                                          const u64* __restrict__ bits, const ctd_fit_cand* __restrict__ cands,
                                          const int* __restrict__ cum, const uint8_t* __restrict__ breaks,
                                          ctd_fit_row* __restrict__ rows, ctd_fit_balance* __restrict__ bals, long long* work,
                                          long long work_bytes) {
  extern __shared__ u64 planes[];                          // A / E: words 0 .. max_words - 1, Q / the table behind it
  __shared__ int s_inner[LY_WAVES];
  __shared__ int s_n[CTD_FIT_MAX_CANDS];                   // per candidate the smallest n that fits, 0: none
  __shared__ int s_win[4];                                 // the winner: candidate, n
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const ctd_layout_job J = jobs[blockIdx.x];
  const ctd_fit_job FJ = fjobs[blockIdx.x];
  int* __restrict__ out = (int*)(rows + blockIdx.x);       // FT_ROW_INTS int32: the row is 4-byte aligned, no more
  int* __restrict__ bal = BAL ? (int*)(bals + blockIdx.x) : nullptr;   // FT_BAL_INTS int32, likewise

  // ---- the window and what the block may read (block-uniform, before any word is read)
  const int wx1 = J.win[0], wy1 = J.win[1];
  const long long ww_ll = max((long long)J.win[2] - wx1, 0ll), wh_ll = max((long long)J.win[3] - wy1, 0ll);
  const long long nw_ll = (ww_ll + 63) >> 6, words_ll = ww_ll > 0 && wh_ll > 0 ? nw_ll * wh_ll : 0ll;
  const bool has_row = (int)blockIdx.x < prm.n_rows && brows[blockIdx.x].status == CTD_BALLOON_OK;
  const bool in_win = J.ax >= wx1 && J.ax < J.win[2] && J.ay >= wy1 && J.ay < J.win[3];
  int status = CTD_FIT_OK;
  if (!has_row || words_ll > (long long)min(prm.max_words, CTD_BALLOON_MAX_WORDS)) status = CTD_FIT_NO_REGION;
  else if (FJ.n_glyphs <= 0 || FJ.n_cands <= 0) status = CTD_FIT_NO_TEXT;
  else if (words_ll == 0 || !in_win) status = CTD_FIT_NO_ANCHOR;
  if (status != CTD_FIT_OK) {
    no_row<BAL>(out, bal, t, status);
    return;
  }
  const int ww = (int)ww_ll, wh = (int)wh_ll, nw = (int)nw_ll, acx = J.ax - wx1, acy = J.ay - wy1;
  u64* __restrict__ A = planes;
  u64* __restrict__ Q = planes + prm.max_words;

  // ---- load B_b and erode it: plane A = E_b
  int n_inner = load_eroded(A, Q, bits + J.word0, ww, wh, nw, prm.inset, t);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n_inner += __shfl_down(n_inner, d, 64);
  if (lane == 0) s_inner[wave] = n_inner;

  // ---- the axis-run table, in plane Q
  short2* __restrict__ tab = (short2*)Q;
  for (int y = t; y < wh; y += LY_THREADS) {
    int l = 32767, r = 0;
    run_at(A + y * nw, nw, acx, l, r);
    tab[y] = make_short2((short)l, (short)r);
  }
  if (t < CTD_FIT_MAX_CANDS) s_n[t] = 0;
  __syncthreads();
  if (tab[acy].y == 0) {                                    // the anchor is no pixel of E_b
    no_row<BAL>(out, bal, t, CTD_FIT_NO_ANCHOR);
    return;
  }

  // ---- one (candidate, n) pair a thread
  Fit F;
  F.tab = tab, F.wh = wh, F.acx = acx, F.acy = acy, F.G = FJ.n_glyphs;
  F.brk = FJ.break0 >= 0 ? breaks + FJ.break0 : nullptr;
  const int c = t >> 5, n = (t & 31) + 1;
  bool fits = false;
  if (c < FJ.n_cands) {
    const ctd_fit_cand K = cands[FJ.cand0 + c];
    F.cum = cum + K.cum0;
    fits = walk(F, K.line, K.gap, n, nullptr, 0, 0);
  }
  const u64 ballot = __ballot(fits);
  if ((lane & 31) == 0) {
    const unsigned half = lane ? (unsigned)(ballot >> 32) : (unsigned)ballot;
    s_n[c] = half ? __builtin_ctz(half) + 1 : 0;
  }
  __syncthreads();
  if (t == 0) {
    int wc = -1;
    for (int k = 0; k < FJ.n_cands; ++k)
      if (s_n[k]) wc = k;
    s_win[0] = wc, s_win[1] = wc >= 0 ? s_n[wc] : 0;
  }
  __syncthreads();
  const int wc = s_win[0], wn = s_win[1];
  if (wc < 0) {
    no_row<BAL>(out, bal, t, CTD_FIT_NO_FIT);
    return;
  }
  if constexpr (BAL) {
    // ---- the balanced lines of the winner, both rows (plane A is free: E_b is not read behind the table)
    int inner = 0;
    for (int w = 0; w < LY_WAVES; ++w) inner += s_inner[w];
    const ctd_fit_cand K = cands[FJ.cand0 + wc];
    F.cum = cum + K.cum0;
    balance_block(F, K.line, K.gap, wn, inner, wc, wx1, wy1, (long long*)A, prm.max_words, fjobs, work, work_bytes, out, bal);
    return;
  }
  // ---- the row: thread 0 the head and the winner's lines, the threads behind the lines the zeros
  if (t == 0) {
    int inner = 0;
    for (int w = 0; w < LY_WAVES; ++w) inner += s_inner[w];
    out[0] = CTD_FIT_OK, out[1] = wc, out[2] = wn, out[3] = inner;
    const ctd_fit_cand K = cands[FJ.cand0 + wc];
    F.cum = cum + K.cum0;
    walk(F, K.line, K.gap, wn, out + 4, wx1, wy1);
  } else if (t >= 4 + 5 * wn && t < FT_ROW_INTS) {
    out[t] = 0;
  }
}

__global__ __launch_bounds__(LY_THREADS) void fit_kernel(const ctd_layout_job* __restrict__ jobs,
                                                         const ctd_fit_job* __restrict__ fjobs,
                                                         const ctd_balloon_row* __restrict__ brows, ctd_fit_params prm,
                                                         const u64* __restrict__ bits, const ctd_fit_cand* __restrict__ cands,
                                                         const int* __restrict__ cum, const uint8_t* __restrict__ breaks,
                                                         ctd_fit_row* __restrict__ rows) {
  fit_block<false>(jobs, fjobs, brows, prm, bits, cands, cum, breaks, rows, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(LY_THREADS) void fit_balanced_kernel(const ctd_layout_job* __restrict__ jobs,
                                                                  const ctd_fit_job* __restrict__ fjobs,
                                                                  const ctd_balloon_row* __restrict__ brows, ctd_fit_params prm,
                                                                  const u64* __restrict__ bits,
                                                                  const ctd_fit_cand* __restrict__ cands,
                                                                  const int* __restrict__ cum, const uint8_t* __restrict__ breaks,
                                                                  ctd_fit_row* __restrict__ rows, ctd_fit_balance* __restrict__ bals,
                                                                  long long* work, long long work_bytes) {
  fit_block<true>(jobs, fjobs, brows, prm, bits, cands, cum, breaks, rows, bals, work, work_bytes);
}

std::once_flag g_lds_once[2][FT_MAX_DEVICES];
hipError_t g_lds_rc[2][FT_MAX_DEVICES];

// dynamic LDS beyond the default limit, as launch_layout_boxes: raised ONCE per device and kernel to the most a call can need
hipError_t raise_lds(const void* kernel, int which) {
  constexpr int max_bytes = 2 * CTD_BALLOON_MAX_WORDS * (int)sizeof(u64);
  int dev = -1;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  if (dev < 0 || dev >= FT_MAX_DEVICES) return hipErrorInvalidDevice;
  std::call_once(g_lds_once[which][dev], [=] {
    g_lds_rc[which][dev] = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
  });
  return g_lds_rc[which][dev];
}

}  // namespace

hipError_t launch_layout_fit(const ctd_layout_job* jobs, const ctd_fit_job* fit_jobs, int n, const ctd_balloon_row* balloon_rows,
                             const uint64_t* bits, const ctd_fit_cand* cands, const int32_t* cum, const uint8_t* breaks,
                             const ctd_fit_params& prm, ctd_fit_row* rows, hipStream_t st) {
  const hipError_t rc = raise_lds((const void*)fit_kernel, 0);
  if (rc != hipSuccess) return rc;
  // plane Q holds the axis-run table of a window of one word a row too: 4 bytes a row against the plane's 8
  const size_t bytes = (size_t)2 * prm.max_words * sizeof(u64);
  hipLaunchKernelGGL(fit_kernel, dim3(n), dim3(LY_THREADS), bytes, st, jobs, fit_jobs, balloon_rows, prm, (const u64*)bits, cands,
                     cum, breaks, rows);
  return hipGetLastError();
}

hipError_t launch_layout_fit_balanced(const ctd_layout_job* jobs, const ctd_fit_job* fit_jobs, int n,
                                      const ctd_balloon_row* balloon_rows, const uint64_t* bits, const ctd_fit_cand* cands,
                                      const int32_t* cum, const uint8_t* breaks, const ctd_fit_params& prm, ctd_fit_row* rows,
                                      ctd_fit_balance* bals, void* work, long long work_bytes, hipStream_t st) {
  if (work_bytes < 0 || ((uintptr_t)work & 7)) return hipErrorInvalidValue;
  const hipError_t rc = raise_lds((const void*)fit_balanced_kernel, 1);
  if (rc != hipSuccess) return rc;
  const size_t bytes = (size_t)2 * prm.max_words * sizeof(u64);
  hipLaunchKernelGGL(fit_balanced_kernel, dim3(n), dim3(LY_THREADS), bytes, st, jobs, fit_jobs, balloon_rows, prm, (const u64*)bits,
                     cands, cum, breaks, rows, bals, (long long*)work, work_bytes);
  return hipGetLastError();
}

long long fit_work_bytes(const ctd_fit_job* fit_jobs, int n) {
  long long bytes = 0;
  for (int i = 0; i < n; ++i) bytes += fit_work_block_bytes(fit_jobs[i].n_glyphs);
  return bytes;
}
