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
// `region_batch_kernel` (below) is the same warp through the same device function, stored as the normalised, padded,
// width-bucketed tensors an OCR network reads instead of the packed bytes.
#include "kernels.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_PER_LANE = CTD_REGION_TILE / RG_THREADS;
static_assert(CTD_REGION_TILE % RG_THREADS == 0, "a tile is a whole number of passes of the block");
static_assert(sizeof(ctd_region_job) == 120, "ctd_region_job layout (regions.py JOB_DTYPE)");
static_assert(sizeof(ctd_region_batch_job) == 136, "ctd_region_batch_job layout (regions.py BATCH_JOB_DTYPE)");
static_assert(RG_THREADS == 256, "one pass of the block loads one 256-entry value table");

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

// The u8 value of crop pixel (x, y) in every channel: the map, the four bounds-checked taps, (sum + (1 << 14)) >> 15.
// ONE function for `region_warp_kernel` and `region_batch_kernel`, so the two cannot drift.  C is a compile-time constant so
// the channel loops unroll into byte loads.
template <int C>
__device__ __forceinline__ void region_pixel(const double* __restrict__ m, int x, int y, const uint8_t* __restrict__ page,
                                             long long pitch, int H, int W, uint8_t (&v)[C]) {
  int X, Y;
  region_map(m, x, y, X, Y);
  const int sx = X >> 5, sy = Y >> 5, ax = X & 31, ay = Y & 31;
  const int w00 = 32 * (32 - ax) * (32 - ay), w01 = 32 * ax * (32 - ay), w10 = 32 * (32 - ax) * ay, w11 = 32 * ax * ay;
  const bool x0 = sx >= 0 && sx < W, x1 = sx >= -1 && sx < W - 1;
  const bool y0 = sy >= 0 && sy < H, y1 = sy >= -1 && sy < H - 1;
  const uint8_t* r0 = page + (long long)sy * pitch + (long long)sx * C;   // dereferenced only where the tap is inside
  const uint8_t* r1 = r0 + pitch;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int p00 = (x0 && y0) ? r0[c] : 0, p01 = (x1 && y0) ? r0[C + c] : 0;
    const int p10 = (x0 && y1) ? r1[c] : 0, p11 = (x1 && y1) ? r1[C + c] : 0;
    v[c] = (uint8_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + (1 << 14)) >> 15);
  }
}

// the pixels of one tile of a packed crop
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
    uint8_t v[C];
    region_pixel<C>(m, x, y, page, pitch, H, W, v);
#pragma unroll
    for (int c = 0; c < C; ++c) dst[(long long)p * C + c] = v[c];
  }
}

// the block's crop: the last one whose first tile is <= tile (crops without tiles are skipped); block-uniform
__device__ __forceinline__ int region_find(const int* __restrict__ tile_first, int n, int tile) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile_first[mid] <= tile) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(RG_THREADS) void region_warp_kernel(const ctd_region_job* __restrict__ jobs, int n,
                                                                 const int* __restrict__ tile_first,
                                                                 uint8_t* __restrict__ out) {
  const int tile = blockIdx.x;
  const int lo = region_find(tile_first, n, tile);
  const ctd_region_job& J = jobs[lo];
  const int first_pixel = (tile - tile_first[lo]) * CTD_REGION_TILE + threadIdx.x;
  if (J.C == 3) region_tile<3>(J, first_pixel, out);
  else if (J.C == 1) region_tile<1>(J, first_pixel, out);
}

// ---- OCR input batches: the same warp written straight into the tensors a recogniser reads ---------------------------------
// One block = one CTD_REGION_TILE-pixel tile of one SLOT: the rows x Wk pixels of one line inside its batch tensor, padding
// included.  Column < cut (and row < the crop's rows): `region_pixel`; elsewhere the page value `pad`, no map, no loads.  Each
// channel's u8 value then goes through the 256-entry table of its output channel (built on the host IN the output type: the
// kernel moves bit patterns and does no floating-point arithmetic on values; u8 output has no table) and is stored at
// nchw ((slot C + c) rows + y) Wk + x or nhwc ((slot rows + y) Wk + x) C + c from the batch's element offset, 64-bit.  Lanes
// run along the output row: consecutive lanes store consecutive elements of a plane (nchw) / consecutive pixels (nhwc).
// T = the output type as an unsigned integer of its size.
template <typename T, int C, bool NHWC>
__device__ __forceinline__ void region_batch_tile(const ctd_region_batch_job& B, int first_pixel, const T* __restrict__ tab,
                                                  T* __restrict__ out, bool reverse, int pad) {
  const ctd_region_job& J = B.warp;
  const int w = J.w, h = J.h, rot = J.rotate;
  const int H = J.H, W = J.W;
  const long long pitch = J.pitch;
  const uint8_t* __restrict__ page = J.page_dev;
  double m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = J.Minv[k];
  const int rows = B.rows, Wk = B.Wk;
  const int crop_rows = rot ? w : h, crop_cols = rot ? h : w;
  const int cut = min(min(B.cut, crop_cols), Wk);
  const int total = rows * Wk;
  const long long plane = (long long)rows * Wk;
  T* __restrict__ dst = out + J.out_off + (long long)B.slot * C * plane;
#pragma unroll
  for (int r = 0; r < RG_PER_LANE; ++r) {
    const int p = first_pixel + r * RG_THREADS;
    if (p >= total) break;
    const int i = p / Wk, j = p - i * Wk;
    uint8_t v[C];
    if (j < cut && i < crop_rows) {
      const int x = rot ? (w - 1 - i) : j, y = rot ? j : i;
      region_pixel<C>(m, x, y, page, pitch, H, W, v);
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = (uint8_t)pad;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int sc = reverse ? C - 1 - c : c;
      T e;
      if constexpr (sizeof(T) == 1) e = v[sc]; else e = tab[c * 256 + v[sc]];
      if constexpr (NHWC) dst[(long long)p * C + c] = e; else dst[c * plane + p] = e;
    }
  }
}

template <typename T, bool NHWC>
__global__ __launch_bounds__(RG_THREADS) void region_batch_kernel(const ctd_region_batch_job* __restrict__ jobs, int n,
                                                                  const int* __restrict__ tile_first,
                                                                  const T* __restrict__ tables, T* __restrict__ out,
                                                                  int reverse, int pad) {
  __shared__ T tab[sizeof(T) == 1 ? 1 : 3 * 256];
  const int tile = blockIdx.x;
  const int lo = region_find(tile_first, n, tile);
  const ctd_region_batch_job& B = jobs[lo];
  const int C = B.warp.C;
  if constexpr (sizeof(T) > 1) {              // the value tables: C x 256 entries, one pass of the block per channel
    for (int c = 0; c < C && c < 3; ++c) tab[c * 256 + threadIdx.x] = tables[c * 256 + threadIdx.x];
    __syncthreads();
  }
  const int first_pixel = (tile - tile_first[lo]) * CTD_REGION_TILE + threadIdx.x;
  if (C == 3) region_batch_tile<T, 3, NHWC>(B, first_pixel, tab, out, reverse != 0, pad);
  else if (C == 1) region_batch_tile<T, 1, NHWC>(B, first_pixel, tab, out, false, pad);
}

template <typename T>
void launch_batch_t(const ctd_region_batch_job* jobs, int n, const int* tile_first, int n_tiles, const void* tables, void* out,
                    int layout, int reverse, int pad, hipStream_t st) {
  if (layout == CTD_LAYOUT_NHWC)
    hipLaunchKernelGGL((region_batch_kernel<T, true>), dim3(n_tiles), dim3(RG_THREADS), 0, st, jobs, n, tile_first,
                       (const T*)tables, (T*)out, reverse, pad);
  else
    hipLaunchKernelGGL((region_batch_kernel<T, false>), dim3(n_tiles), dim3(RG_THREADS), 0, st, jobs, n, tile_first,
                       (const T*)tables, (T*)out, reverse, pad);
}

}  // namespace

void launch_region_warp(const ctd_region_job* jobs, int n, const int* tile_first, int n_tiles, uint8_t* out, hipStream_t st) {
  hipLaunchKernelGGL(region_warp_kernel, dim3(n_tiles), dim3(RG_THREADS), 0, st, jobs, n, tile_first, out);
}

void launch_region_batches(const ctd_region_batch_job* jobs, int n, const int* tile_first, int n_tiles, const void* tables,
                           void* out, int dtype, int layout, int reverse, int pad, hipStream_t st) {
  if (dtype == CTD_REGION_U8) launch_batch_t<uint8_t>(jobs, n, tile_first, n_tiles, tables, out, layout, reverse, pad, st);
  else if (dtype == CTD_REGION_F16) launch_batch_t<uint16_t>(jobs, n, tile_first, n_tiles, tables, out, layout, reverse, pad, st);
  else launch_batch_t<uint32_t>(jobs, n, tile_first, n_tiles, tables, out, layout, reverse, pad, st);
}
