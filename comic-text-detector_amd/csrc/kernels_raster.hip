// Glyph outlines rasterised into the atlas (`ctd_rasterise_glyphs`; the rule is stated in include/ctd_hip.h and restated in
// numpy in tests/raster_ref.py): an instance is a glyph's quadratic segments at a 16.16 scale, its coverage the clamped,
// signed area of its flattened edges on 16 sample rows a pixel row, exact to 1/256 pixel along x.  Integers only.
//
// raster_kernel, ONE launch, RS_BANDS_Y workgroups of 256 threads per job; workgroup y of a job takes the bands y,
// y + RS_BANDS_Y, ... of RS_BAND_H pixel rows (= 64 sample rows: a wave's lanes) and, within a band, one chunk of
// RS_CHUNK_W pixel columns after the other.  Every decision is block-uniform.  Per (band, chunk):
//   zero    the delta cells: 64 sample rows x (1 carry cell + the chunk's columns).
//   stage   RS_SEG_CHUNK segments at a time, 8 threads a segment: the segment is read, transformed and flattened, a thread
//           computes the edges k = t % 8, + 8, ... of its segment, and every edge that can cross a sample row of the band goes
//           to LDS (the slot from an LDS counter; sums of integers do not depend on the order).  32 segments of at most 32
//           edges fit the 1024 slots, so nothing overflows.
//   cross   wave v takes the edges v, v + 4, ...; lane l is sample row l.  A crossing at Xc = 256 i + f adds d (256 - f) to
//           cell i and d f to cell i + 1 of its row (LDS integer atomics), so that the prefix sum of the row at pixel px
//           is A(px) of the rule.  A cell left of the chunk is the carry cell; a cell right of it is dropped.  A chunk thus
//           needs nothing of the chunks before it, and the result does not depend on the band height or the chunk width.
//   scan    thread (row, quarter) prefix-sums its quarter of the row in place; the quarters' totals give each quarter's base.
//   write   a thread per pixel sums min(|A|, 256) over the pixel row's 16 sample rows and stores the byte.
// LDS: 64 x 129 cells + 1024 edges + small tables, 51 460 B: three workgroups a CU.
#include "kernels.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_ROWS = 16 * RS_BAND_H;                    // sample rows of a band
constexpr int RS_PITCH = RS_CHUNK_W + 1;                   // cell 0 is the carry; odd, so the rows fall on different banks
constexpr int RS_SEG_THREADS = RS_THREADS / RS_SEG_CHUNK;  // threads a segment
constexpr int RS_MAX_EDGES = RS_SEG_CHUNK * 32;            // flatten level 5
constexpr int RS_Q = 4, RS_QW = RS_CHUNK_W / RS_Q;         // the scan's quarters
static_assert(RS_ROWS == 64 && RS_THREADS == 4 * RS_ROWS, "a lane is a sample row; the scan has a thread per (row, quarter)");
static_assert(RS_SEG_THREADS == 8 && RS_PITCH % 2 == 1 && RS_CHUNK_W % RS_Q == 0, "8 threads a segment; an odd pitch");
static_assert(sizeof(ctd_raster_job) == 40 && offsetof(ctd_raster_job, w) == 8 && offsetof(ctd_raster_job, seg_first) == 24 &&
              offsetof(ctd_raster_job, scale) == 32, "raster ABI (glyphs.py dtype)");
constexpr int RS_COORD = 1 << 15, RS_REL = 1 << 30;

struct Edge {                                              // lo.Y < hi.Y; x relative to the box's left, 26.6
  int xlo, ylo, xhi, yhi;
};

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ long long floor_div(long long a, long long b) {   // b > 0
  long long q = a / b;
  return q - ((a % b) < 0);
}

__global__ __launch_bounds__(RS_THREADS) void raster_kernel(const int* __restrict__ segs, long long n_segs,
                                                            const ctd_raster_job* __restrict__ jobs, int n_jobs,
                                                            unsigned char* __restrict__ atlas, long long atlas_bytes,
                                                            int* __restrict__ status) {
  __shared__ int cell[RS_ROWS * RS_PITCH];
  __shared__ Edge edge[RS_MAX_EDGES];
  __shared__ signed char edge_d[RS_MAX_EDGES];
  __shared__ int part[RS_Q][RS_ROWS];                      // the quarters' totals, then their bases
  __shared__ unsigned n_edges;                            // counts on across the stages: a stage's slots start at `start`
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ji = blockIdx.x / RS_BANDS_Y, y = blockIdx.x % RS_BANDS_Y;
  if (ji >= n_jobs) return;

  const ctd_raster_job J = jobs[ji];
  const bool refused = J.seg_first < 0 || J.seg_count < 0 || (long long)J.seg_first + J.seg_count > n_segs || J.w < 0 ||
                       J.h < 0 || J.w > CTD_RASTER_MAX_SIDE || J.h > CTD_RASTER_MAX_SIDE || J.scale < 1 ||
                       J.scale > CTD_RASTER_MAX_SCALE || J.off < 0 || J.off > atlas_bytes ||
                       (long long)J.w * J.h > atlas_bytes - J.off;
  const bool empty = J.w == 0 || J.h == 0 || J.seg_count == 0;
  if (y == 0 && t == 0) status[ji] = refused ? CTD_RASTER_REFUSED : (empty ? CTD_RASTER_EMPTY : CTD_RASTER_OK);
  if (refused || empty) return;                            // block-uniform

  if (t == 0) n_edges = 0;                                 // read behind the barriers below
  unsigned start = 0;
  const long long S = J.scale, left = 64ll * J.bx;
  const int n_bands = (J.h + RS_BAND_H - 1) / RS_BAND_H;
  for (int band = y; band < n_bands; band += RS_BANDS_Y) {
    const int py0 = band * RS_BAND_H;
    const long long Y0 = 64ll * ((long long)J.by + py0);   // the band's sample row l is at Y0 + 4 l + 2
    for (int c0 = 0; c0 < J.w; c0 += RS_CHUNK_W) {
      const int ncols = min(RS_CHUNK_W, J.w - c0);
      __syncthreads();                                     // the chunk before is done with the cells
      for (int i = t; i < RS_ROWS * RS_PITCH; i += RS_THREADS) cell[i] = 0;

      for (int s0 = 0; s0 < J.seg_count; s0 += RS_SEG_CHUNK) {
        __syncthreads();                                   // the cells are zero; the edges before are done with
        // ---- stage
        const int si = s0 + t / RS_SEG_THREADS, sub = t % RS_SEG_THREADS;
        if (si < J.seg_count) {
          const int* __restrict__ sg = segs + ((long long)J.seg_first + si) * 6;
          long long P[6];
          int raw[6];
#pragma unroll
          for (int k = 0; k < 6; ++k) raw[k] = max(-RS_COORD, min(RS_COORD, sg[k]));
#pragma unroll
          for (int k = 0; k < 6; k += 2) {
            P[k] = ((long long)raw[k] * S + 512) >> 10;
            P[k + 1] = (-(long long)raw[k + 1] * S + 512) >> 10;
          }
          const bool is_line = (raw[2] == raw[0] && raw[3] == raw[1]) || (raw[2] == raw[4] && raw[3] == raw[5]);
          int lvl = 0;
          if (!is_line) {
            long long ddx = P[0] - 2 * P[2] + P[4], ddy = P[1] - 2 * P[3] + P[5];
            ddx = ddx < 0 ? -ddx : ddx, ddy = ddy < 0 ? -ddy : ddy;
            const long long dd = ddx > ddy ? ddx : ddy;
            while (lvl < 5 && (dd >> (2 * lvl)) > 16) ++lvl;
          }
          const int N = 1 << lvl;
          const long long half = ((long long)N * N) >> 1;
          for (int k = sub; k < N; k += RS_SEG_THREADS) {
            long long q[4];                                // Q_k, Q_k+1
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const long long a = N - (k + e), b = k + e;
              q[2 * e] = (a * a * P[0] + 2 * a * b * P[2] + b * b * P[4] + half) >> (2 * lvl);
              q[2 * e + 1] = (a * a * P[1] + 2 * a * b * P[3] + b * b * P[5] + half) >> (2 * lvl);
            }
            if (q[1] == q[3]) continue;                    // horizontal: crosses nothing
            const bool down = q[1] < q[3];
            const long long xlo = down ? q[0] : q[2], ylo = down ? q[1] : q[3];
            const long long xhi = down ? q[2] : q[0], yhi = down ? q[3] : q[1];
            // lo.Y <= Ys < hi.Y for some sample row Y0 + 2 .. Y0 + 4 (RS_ROWS - 1) + 2 of the band
            if (ylo > Y0 + 4 * (RS_ROWS - 1) + 2 || yhi <= Y0 + 2) continue;
            const int slot = (int)(atomicAdd(&n_edges, 1u) - start);
            Edge E;
            E.xlo = (int)clampll(xlo - left, -RS_REL, RS_REL), E.xhi = (int)clampll(xhi - left, -RS_REL, RS_REL);
            E.ylo = (int)ylo, E.yhi = (int)yhi;            // |Y| < 2^28: the coordinates and the scale are bounded
            edge[slot] = E;
            edge_d[slot] = down ? 1 : -1;
          }
        }
        __syncthreads();
        // ---- cross: lane = sample row
        const int ne = (int)(n_edges - start);             // nobody adds again before the next barrier
        start += (unsigned)ne;
        const long long Ys = Y0 + 4 * lane + 2;
        for (int e = wave; e < ne; e += RS_THREADS / 64) {
          const Edge E = edge[e];
          if (E.ylo <= Ys && Ys < E.yhi) {
            const long long num = 4 * ((long long)E.xlo * (E.yhi - Ys) + (long long)E.xhi * (Ys - E.ylo));
            const int Xc = (int)clampll(floor_div(num, (long long)E.yhi - E.ylo), 0, 256ll * J.w);
            const int d = edge_d[e], i = Xc >> 8, f = Xc & 255;
            const int j0 = max(i - c0 + 1, 0), j1 = max(i + 1 - c0 + 1, 0);   // the cells of the chunk; 0: the carry
            int* row = cell + lane * RS_PITCH;
            if (j0 <= ncols) atomicAdd(row + j0, d * (256 - f));
            if (j1 <= ncols && f) atomicAdd(row + j1, d * f);
          }
        }
      }
      __syncthreads();                                     // the cells hold every crossing of the band

      // ---- scan: thread (row, quarter), in place; cells 1 .. ncols hold pixels c0 .. c0 + ncols - 1
      {
        const int row = lane, q = wave;
        int* r = cell + row * RS_PITCH;
        const int j1 = min((q + 1) * RS_QW, ncols);
        int acc = 0;
        for (int j = q * RS_QW + 1; j <= j1; ++j) acc += r[j], r[j] = acc;
        part[q][row] = acc;
      }
      __syncthreads();
      if (t < RS_ROWS) {                                   // totals -> bases: the carry plus the quarters before
        int base = cell[t * RS_PITCH];
#pragma unroll
        for (int q = 0; q < RS_Q; ++q) {
          const int v = part[q][t];
          part[q][t] = base;
          base += v;
        }
      }
      __syncthreads();
      // ---- write
      for (int i = t; i < RS_BAND_H * ncols; i += RS_THREADS) {
        const int py = i / ncols, px = i % ncols;
        if (py0 + py >= J.h) break;
        const int q = px / RS_QW;
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int row = py * 16 + k;
          const int a = cell[row * RS_PITCH + px + 1] + part[q][row];
          sum += min(a < 0 ? -a : a, 256);
        }
        atlas[J.off + (long long)(py0 + py) * J.w + c0 + px] = (unsigned char)((255 * sum + 2048) >> 12);
      }
    }
  }
}

}  // namespace

hipError_t launch_rasterise_glyphs(const int32_t* segs, int64_t n_segs, const ctd_raster_job* jobs, int n_jobs, uint8_t* atlas,
                                   int64_t atlas_bytes, int32_t* status, hipStream_t st) {
  hipLaunchKernelGGL(raster_kernel, dim3((unsigned)n_jobs * RS_BANDS_Y), dim3(RS_THREADS), 0, st, segs, (long long)n_segs, jobs,
                     n_jobs, atlas, (long long)atlas_bytes, status);
  return hipGetLastError();
}
