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

__global__ __launch_bounds__(LY_THREADS) void fit_kernel(const ctd_layout_job* __restrict__ jobs,
                                                         const ctd_fit_job* __restrict__ fjobs,
                                                         const ctd_balloon_row* __restrict__ brows, ctd_fit_params prm,
                                                         const u64* __restrict__ bits, const ctd_fit_cand* __restrict__ cands,
                                                         const int* __restrict__ cum, const uint8_t* __restrict__ breaks,
                                                         ctd_fit_row* __restrict__ rows) {
  extern __shared__ u64 planes[];                          // A / E: words 0 .. max_words - 1, Q / the table behind it
  __shared__ int s_inner[LY_WAVES];
  __shared__ int s_n[CTD_FIT_MAX_CANDS];                   // per candidate the smallest n that fits, 0: none
  __shared__ int s_win[4];                                 // the winner: candidate, n
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const ctd_layout_job J = jobs[blockIdx.x];
  const ctd_fit_job FJ = fjobs[blockIdx.x];
  int* __restrict__ out = (int*)(rows + blockIdx.x);       // FT_ROW_INTS int32: the row is 4-byte aligned, no more

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
    if (t < FT_ROW_INTS) out[t] = t == 0 ? status : 0;
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
    if (t < FT_ROW_INTS) out[t] = t == 0 ? CTD_FIT_NO_ANCHOR : 0;
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
    if (t < FT_ROW_INTS) out[t] = t == 0 ? CTD_FIT_NO_FIT : 0;
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

std::once_flag g_lds_once[FT_MAX_DEVICES];
hipError_t g_lds_rc[FT_MAX_DEVICES];

}  // namespace

hipError_t launch_layout_fit(const ctd_layout_job* jobs, const ctd_fit_job* fit_jobs, int n, const ctd_balloon_row* balloon_rows,
                             const uint64_t* bits, const ctd_fit_cand* cands, const int32_t* cum, const uint8_t* breaks,
                             const ctd_fit_params& prm, ctd_fit_row* rows, hipStream_t st) {
  // dynamic LDS beyond the default limit, as launch_layout_boxes: raised ONCE per device to the most a call can need
  constexpr int max_bytes = 2 * CTD_BALLOON_MAX_WORDS * (int)sizeof(u64);
  int dev = -1;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  if (dev < 0 || dev >= FT_MAX_DEVICES) return hipErrorInvalidDevice;
  std::call_once(g_lds_once[dev], [dev] {
    g_lds_rc[dev] = hipFuncSetAttribute((const void*)fit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
  });
  if (g_lds_rc[dev] != hipSuccess) return g_lds_rc[dev];
  // plane Q holds the axis-run table of a window of one word a row too: 4 bytes a row against the plane's 8
  const size_t bytes = (size_t)2 * prm.max_words * sizeof(u64);
  hipLaunchKernelGGL(fit_kernel, dim3(n), dim3(LY_THREADS), bytes, st, jobs, fit_jobs, balloon_rows, prm, (const u64*)bits, cands,
                     cum, breaks, rows);
  return hipGetLastError();
}
