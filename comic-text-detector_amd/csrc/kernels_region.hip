// OCR line crops: cv2.warpPerspective(page, M, (w, h)) [+ cv2.rotate(ROTATE_90_COUNTERCLOCKWISE) for vertical blocks] of
// `TextBlock.get_transformed_region` (reference utils/textblock.py:184,190-191) for ALL text lines of a batch in one launch.
// OpenCV's classic fixed-point path for INTER_LINEAR / BORDER_CONSTANT 0 (imgproc/imgwarp.cpp, 4.1.2 - 4.10):
//   W = Minv[6] x + Minv[7] y + Minv[8];  W = W ? 32 / W : 0                     (double; INTER_TAB_SIZE = 32)
//   X = rint(clamp((Minv[0] x + Minv[1] y + Minv[2]) W, INT_MIN, INT_MAX)),  Y likewise
//   taps (X >> 5, Y >> 5) + {0,1}^2, weights 32 (32 - ax)(32 - ay), 32 ax (32 - ay), 32 (32 - ax) ay, 32 ax ay of
//   ax = X & 31, ay = Y & 31 (they sum to 1 << 15 exactly), taps outside the page read 0,  dst = (sum + (1 << 14)) >> 15
// The doubles are evaluated in ONE order on the full column index -- (M0 x + M1 y) + M2, no contraction, IEEE division,
// round-half-even -- so a crop is a function of (page, Minv) to the bit (include/ctd_hip.h).
// Byte work bound by HBM / L2 latency, like kernels_pre.hip: one lane per output pixel, lanes along the OUTPUT layout (for
// rotated crops too: consecutive lanes store consecutive bytes and walk a source column), four pixels per lane in flight.
// One block = one CTD_REGION_TILE-pixel tile of one crop, found by a binary search of the tile prefix array: block-uniform,
// so the search and the job row are scalar loads.
#include "kernels.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_PER_LANE = CTD_REGION_TILE / RG_THREADS;
static_assert(CTD_REGION_TILE % RG_THREADS == 0, "a tile is a whole number of passes of the block");
static_assert(sizeof(ctd_region_job) == 120, "ctd_region_job layout (regions.py JOB_DTYPE)");

// crop pixel (x, y) -> fixed-point page coordinates (1/32 px)
__device__ __forceinline__ void region_map(const double* __restrict__ m, int x, int y, int& X, int& Y) {
#pragma clang fp contract(off)
  const double dx = (double)x, dy = (double)y;
  double w = (m[6] * dx + m[7] * dy) + m[8];
  w = (w != 0.) ? 32. / w : 0.;
  const double fx = ((m[0] * dx + m[1] * dy) + m[2]) * w;
  const double fy = ((m[3] * dx + m[4] * dy) + m[5]) * w;
  // std::max((double)INT_MIN, std::min((double)INT_MAX, v)), then cvRound
  X = (int)rint(fmax(-2147483648., fmin(2147483647., fx)));
  Y = (int)rint(fmax(-2147483648., fmin(2147483647., fy)));
}

// the pixels of one tile; C is a compile-time constant so the channel loops unroll into byte loads
template <int C>
__device__ __forceinline__ void region_tile(const ctd_region_job& J, int first_pixel, uint8_t* __restrict__ out) {
  const int w = J.w, h = J.h, rot = J.rotate;
  const int H = J.H, W = J.W;
  const long long pitch = J.pitch;
  const uint8_t* __restrict__ page = J.page_dev;
  double m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = J.Minv[k];
  const int cols = rot ? h : w;               // row length of the stored crop
  const int total = w * h;
  uint8_t* __restrict__ dst = out + J.out_off;
#pragma unroll
  for (int r = 0; r < RG_PER_LANE; ++r) {
    const int p = first_pixel + r * RG_THREADS;
    if (p >= total) break;
    const int i = p / cols, j = p - i * cols;
    // rotated: out[i][j] = region[j][w - 1 - i]
    const int x = rot ? (w - 1 - i) : j, y = rot ? j : i;
    int X, Y;
    region_map(m, x, y, X, Y);
    const int sx = X >> 5, sy = Y >> 5, ax = X & 31, ay = Y & 31;
    const int w00 = 32 * (32 - ax) * (32 - ay), w01 = 32 * ax * (32 - ay), w10 = 32 * (32 - ax) * ay, w11 = 32 * ax * ay;
    const bool x0 = sx >= 0 && sx < W, x1 = sx >= -1 && sx < W - 1;
    const bool y0 = sy >= 0 && sy < H, y1 = sy >= -1 && sy < H - 1;
    const uint8_t* r0 = page + (long long)sy * pitch + (long long)sx * C;   // dereferenced only where the tap is inside
    const uint8_t* r1 = r0 + pitch;
    uint8_t v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int p00 = (x0 && y0) ? r0[c] : 0, p01 = (x1 && y0) ? r0[C + c] : 0;
      const int p10 = (x0 && y1) ? r1[c] : 0, p11 = (x1 && y1) ? r1[C + c] : 0;
      v[c] = (uint8_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + (1 << 14)) >> 15);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) dst[(long long)p * C + c] = v[c];
  }
}

__global__ __launch_bounds__(RG_THREADS) void region_warp_kernel(const ctd_region_job* __restrict__ jobs, int n,
                                                                 const int* __restrict__ tile_first,
                                                                 uint8_t* __restrict__ out) {
  const int tile = blockIdx.x;
  int lo = 0, hi = n;                         // the last crop whose first tile is <= tile (crops without tiles are skipped)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_first[mid] <= tile) lo = mid; else hi = mid;
  }
  const ctd_region_job& J = jobs[lo];
  const int first_pixel = (tile - tile_first[lo]) * CTD_REGION_TILE + threadIdx.x;
  if (J.C == 3) region_tile<3>(J, first_pixel, out);
  else if (J.C == 1) region_tile<1>(J, first_pixel, out);
}

}  // namespace

void launch_region_warp(const ctd_region_job* jobs, int n, const int* tile_first, int n_tiles, uint8_t* out, hipStream_t st) {
  hipLaunchKernelGGL(region_warp_kernel, dim3(n_tiles), dim3(RG_THREADS), 0, st, jobs, n, tile_first, out);
}
