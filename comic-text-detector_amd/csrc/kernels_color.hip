// Font colours: the fill and the surround colour of every text line of a batch in one launch (`ctd_line_colors`; the rule is
// stated in include/ctd_hip.h and restated in numpy in tests/color_ref.py).  Integers only, so a row is a function of
// (page, mask, quad) to the bit and does not depend on the order of addition.
// One block per line, its result is its own row: no global atomics.  Byte work bound by memory LATENCY, not bandwidth: a
// line is a few thousand pixels and the longest line of a batch sets the kernel's time, so the block is built to need few
// dependent round trips.  It walks the quad's clipped bounding box in raster order, consecutive lanes on consecutive pixels
// of a page row (a narrow box wraps to the next row inside a pass, so a 30-pixel-wide vertical line still fills the lanes).
// A ROUND is CL_UNROLL passes of the 512 threads = 4096 box pixels: every thread issues the four byte loads (B, G, R, mask)
// of its 8 pixels unconditionally -- every box pixel lies on the page, so the load needs no inside test in front of it and
// all 32 are in flight together -- and evaluates the inside test while they fly.
//   pass 1: per-thread u32 n_on, n_off, g_on, g_off  ->  wave reduction in registers  ->  8 waves through LDS in 64 bits
//   one __syncthreads; every thread then holds the line's totals and derives status and the text-like grey range itself
//   pass 2: u32 n_fg, s_fg[3], n_bg, s_bg[3] over the same walk, the same reduction; the first round's pixels are still in
//   registers (a line of up to 4096 box pixels, the common case, reads memory once), later rounds re-read what pass 1 pulled
//   through L2; thread 0 divides and stores the row.
// A per-thread sum is at most 255 * 2^24 < 2^32 because of the CTD_COLOR_MAX_PIXELS cap, and so is the sum over a wave.
// The inside test is the definition itself, four int64 edge functions per box pixel (v_mad_i64_i32: the coordinate cap
// makes every factor an int32).  Per-row spans of the same functions would skip the box pixels of a thin tilted line without
// loading them; the detector's lines are near axis-aligned (4 % of the box pixels lie outside) and it is
// not done.
#include "kernels.h"

namespace {

constexpr int CL_THREADS = 512;
constexpr int CL_WAVES = CL_THREADS / 64;
constexpr int CL_UNROLL = 8;
static_assert(sizeof(ctd_color_job) == 64, "ctd_color_job layout (colors.py JOB_DTYPE)");
static_assert(sizeof(ctd_line_color) == 104, "ctd_line_color layout (colors.py OUT_DTYPE)");
static_assert(offsetof(ctd_color_job, quad) == 32 && offsetof(ctd_line_color, g_on) == 64 &&
              offsetof(ctd_line_color, n_on) == 80 && offsetof(ctd_line_color, fg) == 92, "font-colour ABI offsets");
static_assert(255ull * CTD_COLOR_MAX_PIXELS < (1ull << 32), "a line's sums fit the u32 partials");

// The line, block-uniform: the quad, its clipped box (never empty where a walk runs) and where the bytes are.
struct ColorGeom {
  int px[4], py[4];    // the points
  int ex[4], ey[4];    // p[k+1] - p[k]
  int x0, y0, bw, bh;  // box origin and size
  int total;           // bw * bh <= 2^24
  const uint8_t* page; // rows `pitch` bytes apart
  const uint8_t* mask;
  long long pitch, mpitch;
};

// A thread's place in the box: box pixel i = (bx, by); it visits i = threadIdx.x + 512 j, kept without a division per pixel.
struct ColorWalk {
  int i, bx, by;
};

__device__ __forceinline__ void walk_seek(ColorWalk& w, const ColorGeom& g, int i) {
  w.i = i;
  w.by = i / g.bw;
  w.bx = i - w.by * g.bw;
}

// One round: the thread's next CL_UNROLL box pixels.  v[u] = B | G << 8 | R << 16 | (mask != 0) << 24, bit u of `in` = the
// pixel exists (i < total) and is inside the quad.  A pixel beyond the box's end reads the box's first pixel instead.
__device__ __forceinline__ void load_round(const ColorGeom& g, ColorWalk& w, unsigned (&v)[CL_UNROLL], unsigned& in) {
  const int step_y = CL_THREADS / g.bw, step_x = CL_THREADS - step_y * g.bw;
  in = 0;
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u) {
    const bool valid = w.i < g.total;
    const int x = g.x0 + (valid ? w.bx : 0), y = g.y0 + (valid ? w.by : 0);
    const uint8_t* p = g.page + y * g.pitch + 3ll * x;
    v[u] = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | (g.mask[y * g.mpitch + x] != 0 ? 1u << 24 : 0u);
    bool ge = true, le = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // |ex|, |ey| <= 2^30 and |x - px|, |y - py| < 2^31 (CTD_COLOR_MAX_COORD, W and H int32): each product < 2^61
      const long long c = (long long)g.ex[k] * (long long)(y - g.py[k]) - (long long)g.ey[k] * (long long)(x - g.px[k]);
      ge = ge && c >= 0;
      le = le && c <= 0;
    }
    if (valid && (ge || le)) in |= 1u << u;
    w.i += CL_THREADS;
    w.bx += step_x;
    w.by += step_y;
    if (w.bx >= g.bw) { w.bx -= g.bw; ++w.by; }
  }
}

// Calls f(v, inside) for every box pixel of the calling thread.  The first round is kept in (v0, in0): FIRST loads it, the
// other pass finds it there.
template <bool FIRST, typename F>
__device__ __forceinline__ void for_box(const ColorGeom& g, unsigned (&v0)[CL_UNROLL], unsigned& in0, F&& f) {
  ColorWalk w;
  if (FIRST) {
    walk_seek(w, g, threadIdx.x);
    load_round(g, w, v0, in0);
  } else {
    walk_seek(w, g, threadIdx.x + CL_UNROLL * CL_THREADS);
  }
#pragma unroll
  for (int u = 0; u < CL_UNROLL; ++u) f(v0[u], (in0 >> u & 1u) != 0);
  while (w.i < g.total) {
    unsigned v[CL_UNROLL], in;
    load_round(g, w, v, in);
#pragma unroll
    for (int u = 0; u < CL_UNROLL; ++u) f(v[u], (in >> u & 1u) != 0);
  }
}

__device__ __forceinline__ unsigned color_grey(unsigned v) {
  return ((v & 255u) * 3735u + (v >> 8 & 255u) * 19235u + (v >> 16 & 255u) * 9798u + 16384u) >> 15;
}

// sum over the block of N u32 values per thread; every thread gets the totals (one __syncthreads; `sh` is this call's own)
template <int N>
__device__ __forceinline__ void block_sum(const unsigned (&v)[N], unsigned long long (&tot)[N],
                                          unsigned long long (*sh)[CL_WAVES]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    unsigned s = v[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if (lane == 0) sh[k][wave] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < CL_WAVES; ++w) t += sh[k][w];
    tot[k] = t;
  }
}

__global__ __launch_bounds__(CL_THREADS) void line_color_kernel(const ctd_color_job* __restrict__ jobs,
                                                                ctd_line_color* __restrict__ out) {
  __shared__ unsigned long long sh1[4][CL_WAVES], sh2[8][CL_WAVES];
  const ctd_color_job& J = jobs[blockIdx.x];
  ctd_line_color* __restrict__ row = out + blockIdx.x;
  const int H = J.H, W = J.W;

  ColorGeom g;
  g.page = J.page_dev;
  g.mask = J.mask_dev;
  g.pitch = J.pitch;
  g.mpitch = J.mask_pitch;
  bool far = false;
  int xmin = 0x7fffffff, xmax = -0x7fffffff - 1, ymin = xmin, ymax = xmax;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    g.px[k] = J.quad[2 * k];
    g.py[k] = J.quad[2 * k + 1];
    far = far || g.px[k] > CTD_COLOR_MAX_COORD || g.px[k] < -CTD_COLOR_MAX_COORD || g.py[k] > CTD_COLOR_MAX_COORD ||
          g.py[k] < -CTD_COLOR_MAX_COORD;
    xmin = min(xmin, g.px[k]); xmax = max(xmax, g.px[k]);
    ymin = min(ymin, g.py[k]); ymax = max(ymax, g.py[k]);
  }
  g.x0 = max(xmin, 0); g.y0 = max(ymin, 0);
  const int x1 = min(xmax, W - 1), y1 = min(ymax, H - 1);
  const bool none = H < 1 || W < 1 || x1 < g.x0 || y1 < g.y0;
  g.bw = none ? 1 : x1 - g.x0 + 1;
  g.bh = none ? 0 : y1 - g.y0 + 1;
  const bool too_large = far || (long long)g.bw * g.bh > (long long)CTD_COLOR_MAX_PIXELS;
  g.total = too_large ? 0 : g.bw * g.bh;

  // everything the row holds, as thread 0 stores it at the end
  unsigned long long t1[4] = {0, 0, 0, 0};               // n_on, n_off, g_on, g_off
  unsigned long long t2[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // n_fg, s_fg[3], n_bg, s_bg[3]
  int status = CTD_COLOR_EMPTY;

  if (too_large) {                                       // block-uniform; decided before any load
    status = CTD_COLOR_TOO_LARGE;
  } else if (!none) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      g.ex[k] = g.px[(k + 1) & 3] - g.px[k];             // within int32: |coordinates| <= 2^29
      g.ey[k] = g.py[(k + 1) & 3] - g.py[k];
    }
    unsigned v0[CL_UNROLL], in0;
    unsigned a[4] = {0, 0, 0, 0};
    for_box<true>(g, v0, in0, [&](unsigned v, bool inside) {
      const unsigned gr = color_grey(v);
      const bool on = inside && (v >> 24) != 0, off = inside && (v >> 24) == 0;
      a[0] += on; a[1] += off;
      a[2] += on ? gr : 0u; a[3] += off ? gr : 0u;
    });
    block_sum<4>(a, t1, sh1);                            // the one barrier between the passes
    const unsigned long long n_on = t1[0], n_off = t1[1], g_on = t1[2], g_off = t1[3];
    if (n_on + n_off == 0) {
      status = CTD_COLOR_EMPTY;
    } else if (n_on == 0) {
      status = CTD_COLOR_NO_MASK;
    } else {
      // text-like <=> lo <= g <= hi.  Means tie or no OFF pixel (NO_CONTRAST): the ON pixels are the fill, the OFF ones the surround
      const unsigned long long lhs = g_on * n_off, rhs = g_off * n_on;     // < 2^32 * 2^24
      const bool contrast = n_off != 0 && lhs != rhs;
      status = contrast ? CTD_COLOR_OK : CTD_COLOR_NO_CONTRAST;
      unsigned lo = 256, hi = 0;
      if (contrast) {
        const unsigned long long D = 2 * n_on * n_off, S = lhs + rhs;      // text-like: g D > S (ON mean above) or g D < S
        if (lhs > rhs) { lo = (unsigned)(S / D) + 1; hi = 255; }           // g > S / D
        else { lo = 0; hi = (unsigned)((S + D - 1) / D) - 1; }             // g < S / D; S >= rhs > 0
      }
      unsigned b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for_box<false>(g, v0, in0, [&](unsigned v, bool inside) {
        const unsigned c0 = v & 255u, c1 = v >> 8 & 255u, c2 = v >> 16 & 255u;
        const unsigned gr = color_grey(v);
        const bool on = (v >> 24) != 0;
        const bool like = contrast ? (gr >= lo && gr <= hi) : on;
        const bool fg = inside && on && like, bg = inside && !like;
        b[0] += fg; b[1] += fg ? c0 : 0u; b[2] += fg ? c1 : 0u; b[3] += fg ? c2 : 0u;
        b[4] += bg; b[5] += bg ? c0 : 0u; b[6] += bg ? c1 : 0u; b[7] += bg ? c2 : 0u;
      });
      block_sum<8>(b, t2, sh2);
    }
  }

  if (threadIdx.x == 0) {
    const bool counted = status != CTD_COLOR_EMPTY && status != CTD_COLOR_TOO_LARGE;
    row->n_fg = (long long)t2[0];
    row->n_bg = (long long)t2[4];
    uint8_t fg[3] = {0, 0, 0}, bg[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      row->s_fg[c] = (long long)t2[1 + c];
      row->s_bg[c] = (long long)t2[5 + c];
      if (t2[0]) fg[c] = (uint8_t)((2 * t2[1 + c] + t2[0]) / (2 * t2[0]));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bg[c] = t2[4] ? (uint8_t)((2 * t2[5 + c] + t2[4]) / (2 * t2[4])) : (status == CTD_COLOR_NO_CONTRAST ? fg[c] : (uint8_t)0);
      row->fg[c] = fg[c];
      row->bg[c] = bg[c];
    }
    row->g_on = counted ? (long long)t1[2] : 0;
    row->g_off = counted ? (long long)t1[3] : 0;
    row->n_on = counted ? (int)t1[0] : 0;
    row->n_off = counted ? (int)t1[1] : 0;
    row->status = status;
#pragma unroll
    for (int c = 0; c < 6; ++c) row->pad_[c] = 0;
  }
}

}  // namespace

void launch_line_colors(const ctd_color_job* jobs, int n, ctd_line_color* out, hipStream_t st) {
  hipLaunchKernelGGL(line_color_kernel, dim3(n), dim3(CL_THREADS), 0, st, jobs, out);
}
