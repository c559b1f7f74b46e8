// Tilted regions (`ctd_balloon_tilt`; the rule is stated in include/ctd_hip.h, "tilted text", and restated in numpy in
// tests/tilt_ref.py): a block's balloon plane B_b turned into the block's own frame, in the block's own window and word
// layout, so that the layout and fit kernels run on it unchanged.  Frame pixel q is set iff the page pixel nearest to
// frame -> page (q) lies in the window and in B_b; the frame is a pivot and a 16.16 (c, s) pair made by the host.  Integers
// only, every product in 64 bits.
//
// tilt_kernel, ONE launch, one workgroup per block, the SOURCE plane of the window in dynamic LDS (prm.max_words words; the
// window, the tally and the reduce are balloon_bits.h's).  A block whose source row is not OK has its words cleared and its
// row copied, before a bit is read.
//   stage    the block's source words into LDS, one coalesced pass.
//   turn     one wave per output word: lane i maps bit i's frame pixel to its page pixel and reads that bit of the staged
//            plane; the word is one __ballot.  The map is linear with integer coefficients, so from one word to the next a
//            lane's 16.16 page position only takes a 64-bit sum; the four products are formed once a chunk.  A wave takes 64
//            consecutive words at a time and lane k keeps word k, so
//   reduce   the 64 words go out as one run of aligned 8-byte stores, each lane's popcount, box, sums and contact in the same
//            pass; wave shuffles, one LDS step across the waves, thread 0 writes the row with ordinary stores.
#include <mutex>

#include "balloon_bits.h"

namespace {

using namespace blbits;

static_assert(sizeof(ctd_tilt_job) == 48 && sizeof(ctd_tilt_params) == 16, "tilt ABI sizes (balloons.py dtypes)");
static_assert(offsetof(ctd_tilt_job, ax) == 16 && offsetof(ctd_tilt_job, c) == 24 && offsetof(ctd_tilt_job, W) == 32 &&
              offsetof(ctd_tilt_job, word0) == 40, "tilt ABI offsets");
constexpr int TILT_MAX_CS = 65537, TILT_MAX_PIVOT = 1 << 29;   // beyond these a job is refused: the products stay in 64 bits

__global__ __launch_bounds__(BL_THREADS) void tilt_kernel(const ctd_tilt_job* __restrict__ jobs,
                                                          const ctd_balloon_row* __restrict__ brows, const u64* __restrict__ bits,
                                                          ctd_tilt_params prm, ctd_balloon_row* __restrict__ rows,
                                                          u64* __restrict__ bits_out) {
  extern __shared__ u64 src[];                             // B_b: words 0 .. max_words - 1
  __shared__ int red_i[BL_WAVES][8];                       // area, n_seed, min x, min y, max x, max y, flags
  __shared__ long long red_l[BL_WAVES][2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const ctd_tilt_job J = jobs[blockIdx.x];
  ctd_balloon_row B = brows[blockIdx.x];

  // ---- the window and what the block owns (block-uniform, before any bit is read)
  const long long ww_ll = (long long)J.win[2] - J.win[0], wh_ll = (long long)J.win[3] - J.win[1];
  const long long words_ll = ww_ll > 0 && wh_ll > 0 ? ((ww_ll + 63) >> 6) * wh_ll : -1;
  const bool owns = words_ll >= 0 && words_ll <= (long long)min(prm.max_words, CTD_BALLOON_MAX_WORDS);
  const int words = owns ? (int)words_ll : 0;
  window w = {0, 0, 0, 0, 0, 0, 0, 0};
  if (owns) w.wx1 = J.win[0], w.wy1 = J.win[1], w.ww = (int)ww_ll, w.wh = (int)wh_ll;
  const int wx1 = w.wx1, wy1 = w.wy1, ww = w.ww, wh = w.wh;
  const int nw = (ww + 63) >> 6;
  u64* __restrict__ out = bits_out + J.word0;

  const bool frame_ok = abs((long long)J.c) <= TILT_MAX_CS && abs((long long)J.s) <= TILT_MAX_CS &&
                        abs((long long)J.ax) <= TILT_MAX_PIVOT && abs((long long)J.ay) <= TILT_MAX_PIVOT;
  if (B.status != CTD_BALLOON_OK || !owns || !frame_ok) {  // block-uniform
    for (int i = t; i < words; i += BL_THREADS) out[i] = 0ull;
    if (t == 0) {
      if (B.status == CTD_BALLOON_OK) {                    // no plane to turn, or no frame to turn it into: a row of zeros
        B.status = frame_ok ? CTD_BALLOON_TOO_LARGE : CTD_BALLOON_NOT_PLAIN, B.area = 0, B.flags = 0, B.n_seed = 0;
        B.bbox[0] = B.bbox[1] = B.bbox[2] = B.bbox[3] = 0, B.sum_x = 0, B.sum_y = 0;
      }
      rows[blockIdx.x] = B;
    }
    return;
  }

  // ---- stage
  {
    const u64* __restrict__ in = bits + J.word0;
    for (int i = t; i < words; i += BL_THREADS) src[i] = in[i];
  }
  __syncthreads();

  // ---- turn and reduce
  const long long c = J.c, s = J.s, ax16 = (long long)J.ax << 16, ay16 = (long long)J.ay << 16;
  tally a = tally_none();
  for (int base = wave * 64; base < words; base += BL_WAVES * 64) {
    const int cnt = min(64, words - base);                 // wave-uniform
    const int y0 = base / nw;
    int j = base - y0 * nw, x = 64 * j + lane;
    // PX + 32768 and PY + 32768 of this lane's frame pixel of the chunk's first word; the map is linear with integer
    // coefficients, so from word to word the two only take sums: 64 (c, s) along a row, (-s, c) less the row's length at its end
    const long long dx = (long long)wx1 + x - J.ax, dy = (long long)wy1 + y0 - J.ay;
    long long PX = ax16 + c * dx - s * dy + 32768, PY = ay16 + s * dx + c * dy + 32768;
    const long long wrap_x = -s - 64 * c * (nw - 1), wrap_y = c - 64 * s * (nw - 1);
    u64 mine = 0ull;
    for (int k = 0; k < cnt; ++k) {
      bool bit = false;
      if (x < ww) {
        const long long px = (PX >> 16) - wx1, py = (PY >> 16) - wy1;
        if (px >= 0 && px < ww && py >= 0 && py < wh) bit = (src[(int)py * nw + ((int)px >> 6)] >> ((int)px & 63)) & 1ull;
      }
      const u64 word = __ballot(bit);
      if (lane == k) mine = word;
      if (++j == nw) j = 0, x = lane, PX += wrap_x, PY += wrap_y;
      else x += 64, PX += 64 * c, PY += 64 * s;
    }
    if (lane < cnt) {
      out[base + lane] = mine;
      tally_word(a, mine, base + lane, nw, w);
    }
  }
  write_row(a, t == 0 ? B.n_seed : 0, red_i, red_l, rows + blockIdx.x, w, J.W, J.H,
            (B.flags & CTD_BALLOON_FOOTPRINT) | CTD_BALLOON_TILTED, t);
}

std::once_flag g_lds_once[BL_MAX_DEVICES];
hipError_t g_lds_rc[BL_MAX_DEVICES];

}  // namespace

hipError_t launch_balloon_tilt(const ctd_tilt_job* jobs, int n, const ctd_balloon_row* balloon_rows, const uint64_t* bits,
                               const ctd_tilt_params& prm, ctd_balloon_row* rows_out, uint64_t* bits_out, hipStream_t st) {
  // the kernel may ask for more dynamic LDS than the default limit: raised ONCE per device to the most a call can need, so
  // that concurrent callers never see each other's setting
  constexpr int max_bytes = CTD_BALLOON_MAX_WORDS * (int)sizeof(u64);
  int dev = -1;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return rc;
  if (dev < 0 || dev >= BL_MAX_DEVICES) return hipErrorInvalidDevice;
  std::call_once(g_lds_once[dev], [dev] {
    g_lds_rc[dev] = hipFuncSetAttribute((const void*)tilt_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
  });
  if (g_lds_rc[dev] != hipSuccess) return g_lds_rc[dev];
  const size_t bytes = (size_t)prm.max_words * sizeof(u64);
  hipLaunchKernelGGL(tilt_kernel, dim3(n), dim3(BL_THREADS), bytes, st, jobs, balloon_rows, (const u64*)bits, prm, rows_out,
                     (u64*)bits_out);
  return hipGetLastError();
}
