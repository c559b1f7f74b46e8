// Host-side launchers of every device kernel (definitions in the .hip files).
#pragma once
#include <string>
#include <vector>

#include "ctd_common.h"
#include "tuning.h"   // the g_* dispatch knobs of ctd_tuning_set

// ---- kernels_basic.hip : direct (VALU) kernels, T = float | half_t -------
// weights for the direct conv: f32 [KH*KW][cin_total][N]
void launch_conv_direct(const ConvArgs& a, bool f16, hipStream_t st);
// generic transposed conv; weights f32 [k*k][cin][N]; a.stride = s, a.dy0 = pad, a.KH = k
void launch_convt_direct(const ConvArgs& a, bool f16, hipStream_t st);
// dst: NHWC with `pitch` >= 3 channels per pixel; channels 3.. are zero filled
void launch_input_nchw(const float* in, void* dst, int pitch, int B, int H, int W, bool f16, hipStream_t st);
void launch_input_u8(const uint8_t* in, void* dst, int pitch, int B, int H, int W, bool f16, hipStream_t st);
void launch_maxpool(const void* src, int pitchS, void* dst, int pitchD, int C, int B, int H, int W, int k,
                    bool f16, hipStream_t st);
// SPPF: the three chained stride-1 max pools of one cat tensor in one launch (esize 2: fp16 tensors, 4: fp32)
bool sppf_pool3_supported(int pitch, int slot, int C, int H, int W, int k, const void* cat, int esize = 2);
void launch_sppf_pool3(void* cat, int pitch, int slot, int C, int B, int H, int W, int k, hipStream_t st, int esize = 2);
void launch_avgpool2(const void* src, int pitchS, void* dst, int pitchD, int C, int B, int Ho, int Wo,
                     bool f16, hipStream_t st);
// raw: (B,ny,nx,pitch) with na*no used channels -> blks rows [row_off, row_off+na*ny*nx)
void launch_detect_decode(const void* raw, int pitch, bool raw_f16, float* blks, int rows_total, int row_off,
                          int B, int ny, int nx, int na, int no, float stride, const float* anchors_px,
                          hipStream_t st);
// 1-channel activation -> plane `plane` of an (B,nplanes,H,W) f32 tensor (+ optional u8)
// u8_mode: 0 none, 1 = (uint8)(v*255) (truncate), 2 = v > thresh
void launch_export_plane(const void* src, int pitch, bool f16, float* out, int nplanes, int plane, uint8_t* u8,
                         int u8_mode, float thresh, int B, int H, int W, hipStream_t st);

// DBHead.step_function on the two planes of lines_map (B,2,H,W) -> out (B,1,H,W) f32 (+ bitmap u8 = out > thresh)
void launch_db_step(const float* lines, float k, float* out, uint8_t* bitmap, float thresh, int B, int H, int W,
                    hipStream_t st);

// ---- kernels_igemm.hip : MFMA implicit-GEMM conv (fp16 in, fp32 acc) ------
// weights: half [nphase][Npad][K], K index = (ty*KW+tx)*(c0+c1) + c
extern int g_igemm_force_bk;  // tuning knob: 0 = heuristic, 32 / 64 = forced K step
int igemm_pick_bk(int c0, int c1, int K, int N, int log2_down);
void igemm_pack_weights(const float* logical, int nphase, int N, int K, int bn, int bk, bool tiled,
                        std::vector<half_t>& out);
bool igemm_supported(const ConvArgs& a);
int igemm_ntile(int N);  // N tile the dispatcher will use (weights must be padded to it)
// dispatches to a halo kernel when one applies; returns the name of the kernel it launched
const char* launch_conv_igemm(const ConvArgs& a, bool dst_f32, hipStream_t st);

// ---- kernels_f32.hip : f32-operand MFMA implicit-GEMM conv (the exact-fp32 engine) ----
// weights: f32 [nphase][Npad][K], K index = (ty*KW+tx)*(c0+c1) + c; bias f32 padded to Npad
int f32_mfma_ntile(int N);
bool conv_f32_mfma_supported(const ConvArgs& a);
void launch_conv_f32_mfma(const ConvArgs& a, hipStream_t st);

// ---- kernels_split.hip : split-operand (fp16 hi + lo, 3 MFMAs per product) conv on f32 tensors: the "fp32s" engine ----
bool conv_split_supported(const ConvArgs& a);
// dispatches to the halo kernel below when it applies; returns the name of the kernel it launched
const char* launch_conv_split(const ConvArgs& a, hipStream_t st);
// ---- kernels_split_stem.hip : the fp32s engine's first layer straight from the network input (no INPUT launch) ----
bool stem_split_supported(const ConvArgs& a);
void launch_stem_split(const ConvArgs& a, const void* input, int in_fmt, hipStream_t st);
// ---- kernels_split_halo.hip : the same arithmetic on a 256-pixel haloed patch staged once per channel chunk (3x3 / ConvT) ----
bool conv_split_halo_supported(const ConvArgs& a);
void launch_conv_split_halo(const ConvArgs& a, hipStream_t st);
// logical f32 [nphase][N][K] -> hi plane + lo plane (halves, [nphase][npad/32][K/32][32][32] each) + oscale[npad]
void split_pack_weights(const float* logical, int nphase, int N, int K, int npad, std::vector<half_t>& out,
                        std::vector<float>& oscale);

// ---- kernels_halo.hip : halo-tile MFMA conv (stride-1 3x3, ConvTranspose phases) ----
bool conv_halo_supported(const ConvArgs& a, bool dst_f32);
void launch_conv_halo(const ConvArgs& a, hipStream_t st);

// ---- kernels_halo3.hip : ConvTranspose phases on 256-pixel x 128-column tiles, four waves per block, two blocks per CU ----
bool conv_halo3_supported(const ConvArgs& a, bool dst_f32);
bool conv_halo3_post_supported(const ConvArgs& a);
bool conv_halo3_segp_supported(const ConvArgs& a);   // `a` carries post_w = seg-final taps, post_dst = P, post_n = -16   // `a` carries post_*: the layer + its single 1x1 consumer in one launch
void launch_conv_halo3(const ConvArgs& a, hipStream_t st);

// ---- kernels_c3.hip : one-kernel C3 block (32 hidden channels, one bottleneck) -------------
// Weights / biases are the packed arrays of the four unfused ops (tile-major, 32-channel K step):
// w12 [Cin/32][64][32] (cv1 rows 0-31, cv2 rows 32-63), wm1 [32][32], wm2 [9 taps][32][32], wc3 [2][64][32].
struct C3Args {
  SrcView s0, s1;          // x = cat(s0, s1); s1.c == 0 when unused
  int B, H, W;
  const half_t *w12, *wm1, *wm2, *wc3;
  const float *b12, *bm1, *bm2, *bc3;
  void* dst;               // (B,H,W,pitchD) fp16, 64 channels written, already offset by the channel offset
  int pitchD;
  int act;
  const void* zeros;       // >= 16 B of zeros in HBM (source of out-of-image rows)
  int prio;                // as ConvArgs::prio
  half_t* dbg;             // selftest only: three (B,H,W,32) planes receiving y2, t, b of every patch pixel; null in the product
};
bool c3_fused_supported(const C3Args& a);
void launch_c3_fused(const C3Args& a, hipStream_t st);

// ---- kernels_c3b.hip : bottleneck (m.cv1 1x1 + m.cv2 3x3 + shortcut) [+ cv3] of a C3 block with 64 / 128 hidden channels ----
// Weights / biases are the packed arrays of the unfused ops (tile-major, 32-channel K step, N tile = igemm_ntile):
// wm1 [ch/32][ch][32], wm2 [9 ch/32][ch][32] (K step = tap * ch/32 + chunk), wc3 [2ch/128][2ch/32][128][32].
struct C3bArgs {
  SrcView y1;              // the bottleneck's input (ch channels), read with a one-pixel halo
  SrcView y2;              // cv3 only: the C3's second branch (ch channels), cv3's K rows ch .. 2ch-1
  int B, H, W;
  int ch;                  // hidden channels: 64 or 128
  const half_t *wm1, *wm2, *wc3;
  const float *bm1, *bm2, *bc3;
  void* dst;               // (B,H,W,pitchD) fp16: 2 ch channels (cv3) or ch channels (the bottleneck's output), already offset
  int pitchD;
  int act;
  int add;                 // the bottleneck has a shortcut
  int cv3;                 // 1: cv3 follows in the same launch
  int tap_major;           // K walk of the 3x3: 1 = K-linear (kernels_igemm.hip), 0 = channel chunk outer (kernels_halo.hip)
  const void* zeros;       // >= 16 B of zeros in HBM (source of out-of-image rows)
  int prio;                // as ConvArgs::prio
};
bool c3b_supported(const C3bArgs& a);
const char* launch_c3b(const C3bArgs& a, hipStream_t st);

// ---- kernels_stem2.hip : stem (6x6/s2, 3 -> 32) + layer 1 (3x3/s2, 32 -> 64) in one kernel -----------
struct Stem2Args {
  const void* in; int in_fmt;          // network input (CTD_IN_NCHW_F32 / CTD_IN_NHWC_U8), filled per launch
  int B, H, W;
  const half_t* wfrag; const float* bias0; int act0;    // stem: stem_pack_weights fragments
  const half_t* w1; const float* bias1; int act1;       // layer 1: implicit-GEMM packing [9 taps][64][32]
  half_t* dst; int pitchD;             // (B, H/4, W/4, pitchD), 64 channels written
  int prio;                            // as ConvArgs::prio
};
bool stem_conv2_supported(const Stem2Args& a);
void launch_stem_conv2(const Stem2Args& a, hipStream_t st);

// ---- kernels_fused.hip ----------------------------------------------------
// stem: 6x6 s2 p2, 3 -> N (N <= 32... multiple of 8), reads the network input directly.
// weights: MFMA A fragments from stem_pack_weights (two variants: float / uint8 input), bias f32 [N]
void launch_stem(const void* in, int in_fmt, half_t* dst, int pitchD, int B, int H, int W, int N,
                 const half_t* wfrag, const float* bias, int act, hipStream_t st);
void stem_pack_weights(const float* W /* (32, 3, 6, 6) */, std::vector<half_t>& out);
// seg final: ConvT 4x4 s2 p1 (C -> 1) + sigmoid; src (B,H,W,C) half; weights f32 [16][C] (ky*4+kx); returns the kernel's name
const char* launch_seg_final(const half_t* src, int pitch, int C, int B, int H, int W, const float* w, float bias,
                             float* mask, uint8_t* mask_u8, hipStream_t st);
// db tail: src (B,H,W, 2q) half [binarize q | thresh q] (already conv3x3+BN+ReLU)
// params f32 per branch: W1[q][q][2][2] (cin,cout,ky,kx) b1[q] W2[q][1][2][2] b2[1]
void launch_seg_final_f32(const float* src, int pitch, int C, int B, int H, int W, const float* w, float* mask,
                          uint8_t* mask_u8, hipStream_t st);
// the same layer from the per-tap products P (B,H,W,16) f32 its producer left (kernels_halo3.hip SEGP): col2im + sigmoid + u8
void launch_seg_final_gather(const float* P, int B, int H, int W, float bias, float* mask, uint8_t* mask_u8, hipStream_t st);
// returns the name of the kernel it launched
const char* launch_db_up(const void* src, bool f32in, int pitch, int q, int nbr, int B, int H, int W, const float* params,
                         float* lines, uint8_t* bitmap, float thresh, hipStream_t st);

// ---- kernels_post.hip -------------------------------------------------------
size_t nms_workspace_bytes(int B, int rows);
void launch_nms(const float* blks, int B, int rows, int no, float conf, float iou, int max_det, int max_nms,
                float max_wh, float* dets, int* counts, void* ws, hipStream_t st);
// One labelling engine on row runs serves both launchers.  Its workspace is laid out for the (B, H, W) it was sized for --
// a size for one shape serves no other, whatever its pixel count -- and both launchers take the size of the workspace
// they are handed: with less than ccl_workspace_bytes(B, H, W) they return hipErrorInvalidValue and launch nothing.
size_t ccl_workspace_bytes(int B, int H, int W);
// The components of img > thresh, 4- or 8-connected, ids in raster order of first pixels; n_out is exact, stats (rows
// [x, y, w, h, area]) and first hold the first max_labels.  stats may be null.  first (B,max_labels): linear index of
// every component's first pixel in raster order, or null; bg_negative: background pixels of `labels` get -1, not 0.
hipError_t launch_ccl(const uint8_t* img, int B, int H, int W, int thresh, int conn, int* labels, int* n_out, int* stats,
                      int max_labels, void* ws, size_t ws_bytes, hipStream_t st, int* first = nullptr, int bg_negative = 0);
// Foreground (img > thresh, 8-connected) and background (4-connected) components in one union-find:
// labels (B,H,W) signed (+id / -id, per-class raster order), n / stats / first per class, same workspace.
// seg_live (B, ceil(H*W / 64)) or null: one byte per 64 consecutive linear pixels of a page, 1 where some pixel of the
// segment has a label other than -1 (the background component that holds the page's first background pixel).
hipError_t launch_ccl_dual(const uint8_t* img, int B, int H, int W, int thresh, int* labels, int* n_f, int* n_b, int* st_f,
                           int* st_b, int* first_f, int* first_b, int max_labels, void* ws, size_t ws_bytes, hipStream_t st,
                           uint8_t* seg_live = nullptr);

// ---- kernels_pre.hip ----------------------------------------------------------
// cv2.resize(INTER_LINEAR) u8 (C = 1 or 3) into the top-left (dH,dW) of a zero-padded canvas
void launch_resize_linear_u8(const uint8_t* src, int sH, int sW, int C, uint8_t* dst, int dH, int dW, int canvasH,
                             int canvasW, hipStream_t st);

// ---- kernels_region.hip ---------------------------------------------------------
// cv2.warpPerspective (INTER_LINEAR, BORDER_CONSTANT 0) [+ rotate 90 ccw] of n crops in one launch; n >= 1, n_tiles >= 1
void launch_region_warp(const ctd_region_job* jobs, int n, const int* tile_first, int n_tiles, uint8_t* out, hipStream_t st);
// the same warp + value table + layout + padding into batch tensors (ctd_warp_region_batches); n >= 1, n_tiles >= 1
void launch_region_batches(const ctd_region_batch_job* jobs, int n, const int* tile_first, int n_tiles, const void* tables,
                           void* out, int dtype, int layout, int reverse, int pad, hipStream_t st);

// ---- kernels_color.hip ----------------------------------------------------------
// fill / surround colour of n text lines in one launch (ctd_line_colors), one block per line; n >= 1
void launch_line_colors(const ctd_color_job* jobs, int n, ctd_line_color* out, hipStream_t st);

// ---- kernels_erase.hip ----------------------------------------------------------
// ctd_erase_text's two launches: the row of every block (one workgroup per block; n_blocks >= 1), then every byte of every
// page's `out` and `rest` from the rows (one workgroup per page tile; prm.n_tiles >= 1, n_blocks >= 0)
void launch_erase_stats(const ctd_erase_job* jobs, int n_blocks, const ctd_erase_page* pages, int n_pages,
                        const ctd_erase_params& prm, ctd_erase_row* rows, hipStream_t st);
void launch_erase_paint(const ctd_erase_job* jobs, int n_blocks, const ctd_erase_page* pages, int n_pages,
                        const ctd_erase_params& prm, const ctd_erase_row* rows, hipStream_t st);

// ---- kernels_balloon.hip --------------------------------------------------------
// ctd_balloon_regions' one launch (one workgroup per block; n >= 1, prm checked by the caller): raises the kernel's dynamic
// LDS limit once per device, launches, and returns what hipGetLastError says right after the launch
hipError_t launch_balloon_regions(const ctd_balloon_job* jobs, int n, const ctd_erase_page* pages, int n_pages,
                                  const ctd_erase_row* erase_rows, const ctd_balloon_params& prm, ctd_balloon_row* rows,
                                  uint64_t* bits, hipStream_t st);

// ---- kernels_footprint.hip ------------------------------------------------------
// ctd_balloon_footprints' one launch behind the balloon launch (one workgroup per block; n >= 1, prm checked by the caller):
// the dynamic-LDS limit under a once-flag of its own, and what hipGetLastError says right after the launch
hipError_t launch_balloon_footprints(const ctd_balloon_job* jobs, int n, const ctd_erase_page* pages, int n_pages,
                                     const ctd_erase_row* erase_rows, const ctd_footprint_params& prm, ctd_balloon_row* rows,
                                     uint64_t* bits, hipStream_t st);

// ---- kernels_layout.hip ---------------------------------------------------------
// ctd_layout_boxes' one launch (one workgroup per block; n >= 1, prm checked by the caller): raises the kernel's dynamic
// LDS limit once per device, launches, and returns what hipGetLastError says right after the launch
hipError_t launch_layout_boxes(const ctd_layout_job* jobs, int n, const ctd_balloon_row* balloon_rows,
                               const uint64_t* bits, const ctd_layout_params& prm, ctd_layout_row* rows, hipStream_t st);

// ---- kernels_fit.hip ------------------------------------------------------------
// ctd_layout_fit's one launch (one workgroup per block; n >= 1, prm and every offset of the two small tables checked by the
// caller): the dynamic-LDS limit as above
hipError_t launch_layout_fit(const ctd_layout_job* jobs, const ctd_fit_job* fit_jobs, int n, const ctd_balloon_row* balloon_rows,
                             const uint64_t* bits, const ctd_fit_cand* cands, const int32_t* cum, const uint8_t* breaks,
                             const ctd_fit_params& prm, ctd_fit_row* rows, hipStream_t st);
// ctd_layout_fit_balanced's one launch: the same kernel with the balanced breaker behind the winner.  A block's table of
// states lies in LDS where it fits and in its part of `work` otherwise: fit_work_block_bytes(G_j) bytes a block, one behind
// the other in job order, which is where fit_work_bytes ends.  The caller has checked work_bytes against fit_work_bytes;
// a `work` that is not 8-byte aligned is hipErrorInvalidValue and launches nothing.
constexpr long long fit_work_block_bytes(int n_glyphs) {
  return n_glyphs > 0 && n_glyphs <= CTD_FIT_MAX_GLYPHS ? 8ll * CTD_FIT_MAX_LINES * (n_glyphs + 1) : 0ll;
}
long long fit_work_bytes(const ctd_fit_job* fit_jobs_host, int n);
hipError_t launch_layout_fit_balanced(const ctd_layout_job* jobs, const ctd_fit_job* fit_jobs, int n,
                                      const ctd_balloon_row* balloon_rows, const uint64_t* bits, const ctd_fit_cand* cands,
                                      const int32_t* cum, const uint8_t* breaks, const ctd_fit_params& prm, ctd_fit_row* rows,
                                      ctd_fit_balance* bals, void* work, long long work_bytes, hipStream_t st);

// ---- kernels_typeset.hip --------------------------------------------------------
// ctd_typeset's one launch (one workgroup per row of the tile table; n_tiles >= 1, n_layers >= 1, the counts and pointers
// checked and the rows cleared by the caller): returns what hipGetLastError says right after the launch
hipError_t launch_typeset(const ctd_typeset_page* pages, const ctd_typeset_layer* layers, const ctd_typeset_tile* tiles,
                          const int32_t* entries, const uint8_t* cov, const ctd_typeset_params& prm, ctd_typeset_row* rows,
                          hipStream_t st);

// ---- kernels_glyphs.hip ---------------------------------------------------------
// ctd_typeset_glyphs' one launch (one workgroup per row of the tile table; n_tiles >= 1, n_layers >= 1, the counts and
// pointers checked and the rows cleared by the caller): returns what hipGetLastError says right after the launch
hipError_t launch_typeset_glyphs(const ctd_typeset_page* pages, const ctd_glyph_layer* layers, const ctd_glyph_place* places,
                                 const ctd_glyph_record* glyphs, const ctd_typeset_tile* tiles, const int32_t* entries,
                                 const uint8_t* atlas, const ctd_glyph_params& prm, ctd_typeset_row* rows, hipStream_t st);

// ---- kernels_tilt.hip -----------------------------------------------------------
// ctd_balloon_tilt's one launch (one workgroup per block; n >= 1, prm checked by the caller): the dynamic-LDS limit under a
// once-flag of its own, and what hipGetLastError says right after the launch
hipError_t launch_balloon_tilt(const ctd_tilt_job* jobs, int n, const ctd_balloon_row* balloon_rows, const uint64_t* bits,
                               const ctd_tilt_params& prm, ctd_balloon_row* rows_out, uint64_t* bits_out, hipStream_t st);

// ---- kernels_tilted.hip ---------------------------------------------------------
// ctd_typeset_tilted's one launch (as launch_typeset_glyphs: n_tiles >= 1, n_layers >= 1, the counts and pointers checked
// and the rows cleared by the caller): returns what hipGetLastError says right after the launch
hipError_t launch_typeset_tilted(const ctd_typeset_page* pages, const ctd_tilt_layer* layers, const ctd_glyph_place* places,
                                 const ctd_glyph_record* glyphs, const ctd_typeset_tile* tiles, const int32_t* entries,
                                 const uint8_t* atlas, const ctd_glyph_params& prm, ctd_typeset_row* rows, hipStream_t st);

// ---- kernels_raster.hip ---------------------------------------------------------
// the shape of ctd_rasterise_glyphs' launch (mirrored in _lib.py for the tests, which probe every boundary; no result
// depends on any of them): pixel rows a band, pixel columns a chunk, segments a staging pass, workgroups a job
constexpr int RS_BAND_H = 4, RS_CHUNK_W = 128, RS_SEG_CHUNK = 32, RS_BANDS_Y = 8;
// ctd_rasterise_glyphs' one launch (RS_BANDS_Y workgroups per job; 1 <= n_jobs <= 2^24, the counts and pointers checked by
// the caller): returns what hipGetLastError says right after the launch
hipError_t launch_rasterise_glyphs(const int32_t* segs, int64_t n_segs, const ctd_raster_job* jobs, int n_jobs, uint8_t* atlas,
                                   int64_t atlas_bytes, int32_t* status, hipStream_t st);

// ---- kernels_fill.hip -----------------------------------------------------------
// ctd_fill_rest's three launches (pull per tile, the page launch, push per tile; n_pages >= 1, n_tiles >= 1 and the page
// table checked by the caller): raises the page kernel's dynamic LDS limit once per device and returns what hipGetLastError
// says right after the first launch that failed
hipError_t launch_fill_rest(const ctd_fill_page* pages, int n_pages, int n_tiles, void* scratch, ctd_fill_row* rows,
                            hipStream_t st);

// ---- kernels_texture.hip --------------------------------------------------------
// ctd_texture_fill is defined there, next to its kernels; this is how it sets the message ctd_last_error returns (engine.hip):
// returns `code`
int api_fail(int code, const std::string& msg);

// ---- mfma layout probe (selftest) -------------------------------------------
void launch_mfma_probe(const half_t* a, const half_t* b, float* out, hipStream_t st);
