/*
 * ctd_hip.h -- C ABI of the MI355X (gfx950) comic-text-detector hot path.
 *
 * This library is the third backend behind the reference's backend seam:
 *
 *     blks, mask, lines_map = self.net(img_in)          (reference inference.py:146)
 *
 * next to `TextDetBase.forward` (reference basemodel.py:240-244, torch) and
 * `TextDetBaseDNN.__call__` (reference basemodel.py:252-256, OpenCV-DNN/ONNX,
 * tensor names `images` -> `blk, seg, det`, reference utils/export.py:43-44).
 *
 * Plain pointers and sizes only; no torch types.  All pointers named *_dev are
 * device (HBM) pointers on the engine's device; everything else is host memory.
 * Every entry point returns CTD_OK (0) or a negative error code, never throws;
 * `ctd_last_error()` returns a thread-local human readable message.
 * Calls are asynchronous on the `stream` argument (a hipStream_t passed as
 * void*; NULL = the null stream) unless stated otherwise.
 */
#ifndef CTD_HIP_H
#define CTD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTD_ABI_VERSION 10

/* ---- error codes ------------------------------------------------------ */
#define CTD_OK 0
#define CTD_ERR_INVALID (-1)     /* bad argument / malformed program            */
#define CTD_ERR_HIP (-2)         /* a HIP runtime call failed                   */
#define CTD_ERR_UNSUPPORTED (-3) /* op/shape outside what the engine implements */
#define CTD_ERR_NOMEM (-4)

/* ---- arithmetic modes -------------------------------------------------- */
#define CTD_PREC_F32 0 /* fp32 activations, exact fmaf chains (parity / config 2)   */
#define CTD_PREC_F16 1 /* fp16 activations+weights, fp32 accumulate on MFMA (config 3) */
#define CTD_PREC_F32S 2 /* fp32 activations and weights, every product computed on the fp16 MFMA from
                           split operands (x = hi + lo: 3 MFMAs per product, ~22 mantissa bits,
                           fp32 accumulate): the fp32 engine's results at several times its rate */

/* ---- activations (reference models/yolov5/common.py:36-44, basemodel.py) -- */
#define CTD_ACT_NONE 0
#define CTD_ACT_SILU 1
#define CTD_ACT_LEAKY 2 /* LeakyReLU(0.1) */
#define CTD_ACT_RELU 3
#define CTD_ACT_SIGMOID 4

/* ---- network input formats -------------------------------------------- */
#define CTD_IN_NCHW_F32 0 /* (B,3,H,W) float in [0,1]: what preprocess_img hands the net
                             (reference inference.py:72-83)                           */
#define CTD_IN_NHWC_U8 1  /* (B,H,W,3) uint8 letterboxed page, channel order as the net
                             sees it (BGR, reference SURVEY App.C-1); /255 is fused    */

/* ---- op kinds of the lowered program ----------------------------------- */
#define CTD_OP_INPUT 1     /* network input -> 3-channel NHWC activation tensor          */
#define CTD_OP_CONV 2      /* conv2d k x k / stride / pad, <=2 concatenated sources with
                              optional nearest x2 upsample each, bias, act, residual     */
#define CTD_OP_CONVT 3     /* ConvTranspose2d k x k / stride / pad, bias, act            */
#define CTD_OP_MAXPOOL 4   /* k x k, stride 1, pad k/2 (SPPF, reference common.py:188)   */
#define CTD_OP_AVGPOOL2 5  /* 2x2 stride 2 (reference basemodel.py:38)                   */
#define CTD_OP_DETECT 6    /* YOLO Detect decode of one level (reference yolo.py:23-44)  */
#define CTD_OP_EXPORT 7    /* 1-channel activation -> plane of an f32 NCHW output,
                              optional u8 side output                                    */
#define CTD_OP_STEM 8      /* fused CTD_OP_INPUT + 6x6/s2/p2 conv (3 -> cout)            */
#define CTD_OP_SEG_FINAL 9 /* fused ConvT 4x4/s2/p1 (cin -> 1) + sigmoid + exports       */
#define CTD_OP_DB_UP 10    /* fused DB tail: per branch ConvT2x2(q->q)+ReLU, ConvT2x2(q->1),
                              sigmoid, exports (reference basemodel.py:99-102,138-142)   */

/* ---- external outputs (selected by ctd_op.aux[0] of EXPORT-like ops) ---- */
#define CTD_OUT_MASK 0    /* mask      (B,1,H,W) f32 + mask_u8 (B,H,W) = (uint8)(p*255)
                             (reference inference.py:85-99 postprocess_mask)             */
#define CTD_OUT_LINES 1   /* lines_map (B,2,H,W) f32 + bitmap (B,H,W) = plane0 > thresh
                             (reference utils/db_utils.py:71-72 binarize)                */

/* A tensor of the program: NHWC activation with `channels` channels at
 * spatial size (H >> log2_down, W >> log2_down). */
typedef struct ctd_tensor {
  int32_t channels;
  int32_t log2_down;
  int32_t dtype; /* 0 = the engine's activation type (f32 / f16), 1 = always f32
                    (used for the raw Detect logits so the box decode stays fp32) */
} ctd_tensor;

/* One op.  Sources are (tensor id, channel offset, channel count, upsample
 * flag); the op reads the channel-concatenation [src0 | src1]. */
typedef struct ctd_op {
  int32_t kind;
  int32_t src0, src0_coff, src0_c, src0_up;
  int32_t src1, src1_coff, src1_c, src1_up; /* src1 = -1: unused */
  int32_t res, res_coff;                    /* residual added AFTER act (reference common.py:104); -1: none */
  int32_t dst, dst_coff;
  int32_t cout;
  int32_t k, stride, pad;
  int32_t act;
  int64_t w_off; /* element offset of the weights in the f32 parameter blob:
                    CONV : (cout, cin, k, k)   [torch Conv2d layout, BN folded]
                    CONVT: (cin, cout, k, k)   [torch ConvTranspose2d layout, BN folded] */
  int64_t b_off; /* element offset of the bias (cout floats), or -1 */
  int32_t aux[8];
  /* DETECT   : aux[0]=level stride, aux[1]=row offset into blks PER 64x64 INPUT UNIT
                (scaled by (H/64)*(W/64) at run time), aux[2]=na, aux[3]=no
     EXPORT   : aux[0]=CTD_OUT_*, aux[1]=plane index, aux[2]=planes of that output (0 = the default: 2 for
                CTD_OUT_LINES) -- a program lowered without the DB threshold branch has ONE plane
     SEG_FINAL: aux[0]=CTD_OUT_MASK
     DB_UP    : aux[0]=CTD_OUT_LINES, aux[1]=q (branch channels), aux[2]=branches lowered (0 or 2: binarize and
                thresh; 1: binarize only = the shrink map `SegDetectorRepresenter` reads); parameter
                layout at w_off: for branch in (binarize, thresh)[:aux[2]]:
                  W1 (q,q,2,2), b1 (q), W2 (q,1,2,2), b2 (1)                          */
  float faux[8];
  /* DETECT   : faux[0..2*na) = anchors in pixels (anchor * stride)
     EXPORT / DB_UP : faux[0] = binarisation threshold for the u8 bitmap               */
} ctd_op;

typedef struct ctd_engine ctd_engine;

/* ---- engine ------------------------------------------------------------ */

/* Builds an engine from a lowered program.  `params` is a host blob of
 * `n_params` floats holding every (BN-folded) weight and bias; the engine
 * repacks (and for CTD_PREC_F16 converts) them into its own device layouts, so
 * the caller may free the blob afterwards.  Synchronous. */
int ctd_engine_create(ctd_engine** out, const ctd_tensor* tensors, int32_t n_tensors,
                      const ctd_op* ops, int32_t n_ops, const float* params, int64_t n_params,
                      int32_t precision, int32_t device);

void ctd_engine_destroy(ctd_engine* e);

/* Row count of `blks` for an H x W input (sum over Detect levels of na*ny*nx),
 * and the per-row width `no` (5 + nc). */
int ctd_engine_blks_shape(const ctd_engine* e, int32_t H, int32_t W, int32_t* rows, int32_t* no);

/* The fused forward: replaces `TextDetBase.forward` (reference basemodel.py:240-244).
 *   input_dev : B pages in `input_fmt`
 *   blks_dev  : (B, rows, no) f32           (`blk`, reference yolo.py:44)
 *   mask_dev  : (B, 1, H, W) f32            (`seg`, reference basemodel.py:74); NULL: not written (the u8
 *               side output below is what the detector consumes)
 *   lines_dev : (B, P, H, W) f32            (`det`, reference basemodel.py:125); P = 2, or 1 for a program
 *               lowered without the threshold branch
 *   mask_u8_dev / bitmap_dev : (B, H, W) u8 fused post-processing side outputs
 *               (reference inference.py:96-99 / utils/db_utils.py:71-72); may be NULL.
 * H and W must be multiples of 64 (reference SURVEY section 5).  Workspace is
 * (re)planned internally when (B,H,W) changes (synchronous in that case). */
int ctd_engine_forward(ctd_engine* e, const void* input_dev, int32_t input_fmt, int32_t B, int32_t H,
                       int32_t W, float* blks_dev, float* mask_dev, float* lines_dev,
                       uint8_t* mask_u8_dev, uint8_t* bitmap_dev, void* stream);

/* Introspection for tests / bench: per-op algorithmic work for the last
 * planned (B,H,W).  Arrays have ctd_engine_n_ops() entries. */
int32_t ctd_engine_n_ops(const ctd_engine* e);
int ctd_engine_op_work(const ctd_engine* e, double* flops, double* bytes, int32_t* kernel_class);
/* kernel_class: 0 = pointwise/pool/export, 1 = MFMA implicit-GEMM conv, 2 = MFMA convT,
 *               3 = direct (VALU) conv, 4 = fused stem / seg-final / db-up */

/* ABI v5.  Name of the kernel op `op_index` launched in the last forward / profile ("conv_halo3_kernel",
 * "conv_igemm_kernel", "c3b_kernel", ...; "(fused)" for an op whose work another op's launch did; "(none)" for an op that
 * launched nothing because the caller passed no buffer for any of its outputs): lets a test assert WHICH dispatch a parity
 * comparison ran through (grid thresholds pick different kernels at B = 1 and B = 32).  `name` gets at most cap - 1
 * characters and a terminator.  Valid after a forward / profile. */
int ctd_engine_op_kernel(const ctd_engine* e, int32_t op_index, char* name, int32_t cap);

/* Runs one forward with a hipEvent pair around every op on `stream` and
 * returns the per-op milliseconds (synchronous). */
int ctd_engine_profile(ctd_engine* e, const void* input_dev, int32_t input_fmt, int32_t B, int32_t H,
                       int32_t W, float* blks_dev, float* mask_dev, float* lines_dev,
                       uint8_t* mask_u8_dev, uint8_t* bitmap_dev, void* stream, float* op_ms);

/* Copies activation tensor `tensor_id` of the last forward to host as f32
 * NHWC (debug / per-layer parity tests).  Synchronous. */
int ctd_engine_read_tensor(ctd_engine* e, int32_t tensor_id, float* host_out, int64_t n_floats);

/* Bytes of HBM held by the activation arena for the current plan. */
int64_t ctd_engine_workspace_bytes(const ctd_engine* e);
/* Counter that changes whenever the arena is reallocated (a forward with a (B,H,W) that needs more than the
 * arena holds).  A hipGraph captured from ctd_engine_forward bakes the arena's addresses in: it may only be
 * replayed while this value equals the one read at capture time.  Re-planning for a shape that fits does NOT
 * change it (tensor offsets differ per shape, the allocation stays), so graphs of several shapes can coexist
 * when the largest shape was run first.  A forward that would have to grow the arena inside a stream capture
 * fails with CTD_ERR_INVALID. */
int32_t ctd_engine_arena_generation(const ctd_engine* e);

/* Kernel-dispatch knobs (process-wide; no reference counterpart).  Keys: "halo_min_patches" (maps with fewer 16x16
 * patches take the implicit-GEMM kernel), "halo" (0: never the halo kernel), "halo_pair";
 * "fuse" = bit mask of the fp16 engine's multi-layer kernels (1: C3 block with 32 hidden channels,
 * 2: SPPF's three pools, 4: stem + layer 1, 8: C3 bottlenecks with 64 / 128 hidden channels, 16: ConvTranspose + its 1x1
 * consumer, 32: the last ConvTranspose + seg-final's tap products; 0 = one launch per layer; results are
 * bit-identical either way), "c3_min_patches" (smaller grids take the per-layer kernels);
 * "db_up_mfma" / "seg_final_mfma" (1: the DB tail / the seg-final layer with their channel reductions on the MFMA, 0: the
 * VALU kernels; same results within 2e-4 / 1e-6); "halo3" (0: the ConvTranspose layers stay with the halo kernel) and
 * "halo3_min_blocks" (smaller grids do not take the big-tile ConvTranspose kernel); "c3b_min_patches",
 * "c3b_max_ch" (64: only the 64-channel bottlenecks) and "c3b_cfg64" (0 / 1 / 2) / "c3b_cfg128" (0 / 1), the tilings of
 * the bit-8 kernel per hidden width (bit-identical results);
 * "f32_mfma" (0: engines created afterwards run the fp32 convolutions on the exact-order direct kernels);
 * the fp32s engine: "split_planes" (1: conv-to-conv tensors stored as fp16 hi / lo planes; 0: fp32 tensors, split
 * in the K loop), "split_halo" (0: never the haloed-patch kernel) with "split_halo_min_patches",
 * "split_stem" (1: the first layer reads the page itself; 0: an input copy and the generic kernel);
 * "fwd_prio" (wave priority of the network's kernels), "no_reuse" (engines created afterwards keep every activation
 * readable) and the tail's "tail_*" keys.
 * Every key, with its default, its lower bound and the measurements behind it, is one row of csrc/tuning.def.
 * The library reads no environment variables; an unknown key returns CTD_ERR_INVALID.
 * Engines re-plan on their next forward after any key but the tail_* keys.  For tests and A/B
 * measurements. */
int ctd_tuning_set(const char* key, int64_t value);
/* The value a key holds now (as stored: after its lower bound and the narrowing to its variable's type), so that a caller
 * can put back what was there.  An unknown key or a null pointer returns CTD_ERR_INVALID. */
int ctd_tuning_get(const char* key, int64_t* value);

/* ---- post-processing kernels ------------------------------------------- */

/* Class-aware greedy NMS on the decoded Detect rows; replaces
 * `non_max_suppression` (reference utils/yolov5_utils.py:124-218, incl. the
 * torchvision.ops.nms call at :202) for multi_label=False, agnostic=False.
 *   blks_dev   : (B, rows, no) f32 [cx,cy,w,h,obj,cls...]
 *   dets_dev   : (B, max_det, 6) f32 [x1,y1,x2,y2,conf,cls], score-descending
 *   counts_dev : (B) i32 number of valid rows in dets
 * `ws_dev` scratch of at least ctd_nms_workspace_bytes(B, rows) bytes. */
size_t ctd_nms_workspace_bytes(int32_t B, int32_t rows);
int ctd_nms(const float* blks_dev, int32_t B, int32_t rows, int32_t no, float conf_thres,
            float iou_thres, int32_t max_det, int32_t max_nms, float max_wh, float* dets_dev,
            int32_t* counts_dev, void* ws_dev, size_t ws_bytes, void* stream);

/* Connected-component labelling with statistics of (img > thresh) on a batch
 * of u8 images; replaces `cv2.connectedComponentsWithStats` (reference
 * utils/textmask.py:93,113,138).  connectivity 4 or 8.
 *   labels_dev : (B, H, W) i32; 0 = background, components numbered 1..n in
 *                raster order of their first pixel
 *   n_dev      : (B) i32 number of components (excluding background)
 *   stats_dev  : (B, max_labels, 5) i32 [x, y, w, h, area] for labels 1..n at
 *                row label-1 (rows beyond max_labels are dropped, n still counts them;
 *                rows of labels that do not exist are not written) */
size_t ctd_ccl_workspace_bytes(int32_t B, int32_t H, int32_t W);
int ctd_ccl(const uint8_t* img_dev, int32_t B, int32_t H, int32_t W, int32_t thresh,
            int32_t connectivity, int32_t* labels_dev, int32_t* n_dev, int32_t* stats_dev,
            int32_t max_labels, void* ws_dev, size_t ws_bytes, void* stream);

/* Both labellings `SegDetectorRepresenter.boxes_from_bitmap` needs (reference utils/db_utils.py:134-136:
 * `cv2.findContours(bitmap, RETR_LIST)` = one contour per 8-connected foreground component and per enclosed
 * 4-connected background region) in ONE union-find over the image:
 *   labels_dev : (B, H, W) i32 signed: +id = foreground component (img > thresh, 8-connected),
 *                -id = background region (4-connected); ids per class in raster order of the first pixel
 *   n_f / n_b  : (B) counts; stats_f / stats_b : (B, max_labels, 5) as ctd_ccl; first_f / first_b :
 *                (B, max_labels) linear index of each component's first pixel
 * Label for label what ctd_ccl(img, connectivity 8) and ctd_ccl(complement of img, connectivity 4) give. */
int ctd_ccl_dual(const uint8_t* img_dev, int32_t B, int32_t H, int32_t W, int32_t thresh, int32_t* labels_dev,
                 int32_t* n_f_dev, int32_t* n_b_dev, int32_t* stats_f_dev, int32_t* stats_b_dev, int32_t* first_f_dev,
                 int32_t* first_b_dev, int32_t max_labels, void* ws_dev, size_t ws_bytes, void* stream);

/* `DBHead.step_function` (reference basemodel.py:159-160), the differentiable binarisation
 * 1 / (1 + exp(-k (P - T))) of the shrink map P and the threshold map T = the two planes of `lines_map`
 * (B,2,H,W); out (B,1,H,W) f32 is what `DBHead.forward(step_eval=True)` returns (basemodel.py:121-122);
 * bitmap (B,H,W) u8 = out > thresh, or NULL.  k = 50 in the reference (basemodel.py:84). */
int ctd_db_step(const float* lines_dev, int32_t B, int32_t H, int32_t W, float k, float* out_dev, uint8_t* bitmap_dev,
                float thresh, void* stream);

/* ---- pre / post resampling ---------------------------------------------- */

/* cv2.resize(src, (dW,dH), INTER_LINEAR) for uint8 images with C = 1 or 3 interleaved
 * channels, OpenCV's fixed-point arithmetic, written into the top-left corner of a
 * (canvasH, canvasW, C) buffer whose remaining bottom/right area is zero filled.
 * With canvas > d this is the reference's `letterbox` (utils/imgproc_utils.py:86-117:
 * resize :113 + copyMakeBorder :116); with canvas == d it is the mask resize of
 * inference.py:165. */
int ctd_resize_linear_u8(const uint8_t* src_dev, int32_t sH, int32_t sW, int32_t C, uint8_t* dst_dev,
                         int32_t dH, int32_t dW, int32_t canvasH, int32_t canvasW, void* stream);

/* ---- OCR line crops: `TextBlock.get_transformed_region`, batched (ABI v7) ------------------------ */

/* Steps of the reference's `TextBlock.get_transformed_region` (utils/textblock.py:162-194) that need no pixels, for n
 * text lines in one call.  HOST memory only, no device work, plain float64 without contraction.  Per line i:
 *   quads (n,8) i32      the line's four points in the order the detector emits them
 *   language (n) i32     0 eng, 1 ja, 2 unknown; vertical (n) i32; font_size (n) f64: fields of the line's block
 *   im_w / im_h (n) i32  size of the page the line lies on (lines of several pages may share a call)
 * the margin of English / unknown-horizontal lines (font_size / 3, clipped to [0, im_w] x [0, im_h], :167-172), the
 * edge-midpoint ratio (:174-177), the crop size (:180-181 / :186-187; round-half-even), and the homography of
 * cv2.findHomography on four points = the unique one through the four correspondences with h22 = 1, solved as
 * cv2.getPerspectiveTransform does (8x8 system, LU with partial pivoting).  Outputs:
 *   wh (n,2) i32 = (w, h) of the warp (BEFORE the rotation of vertical lines); M (n,9) f64 source -> crop;
 *   Minv (n,9) f64 = inverse of M by the adjugate formula (what cv2.warpPerspective maps output pixels with);
 *   status (n) i32: CTD_REGION_OK, or CTD_REGION_DEGENERATE (w < 1, h < 1, a side beyond CTD_REGION_MAX_SIDE, a
 *   non-finite ratio, a singular system = one whose solution does not map the four points onto the crop's corners
 *   within 1e-4 px: the reference raises from inside cv2 / int(round(nan))) with wh = 0. */
#define CTD_REGION_OK 0
#define CTD_REGION_DEGENERATE 1
#define CTD_REGION_MAX_SIDE 32766
int ctd_region_transforms(const int32_t* quads, const int32_t* language, const int32_t* vertical, const double* font_size,
                          const int32_t* im_w, const int32_t* im_h, int32_t n, double textheight, int32_t* wh, double* M,
                          double* Minv, int32_t* status);

/* One crop of a ctd_warp_regions launch (a row of the device job table). */
typedef struct ctd_region_job {
  const uint8_t* page_dev; /* the page: u8, C interleaved channels, rows `pitch` bytes apart                        */
  int32_t H, W, C;         /* page size; C = 1 or 3                                                                 */
  int32_t pitch;           /* >= W * C                                                                              */
  double Minv[9];          /* crop pixel (x, y) -> page coordinates                                                 */
  int32_t w, h;            /* size of the warp                                                                      */
  int32_t rotate;          /* 1: the crop is stored turned by 90 degrees counter-clockwise, (w, h, C) instead of
                              (h, w, C) (cv2.rotate(.., ROTATE_90_COUNTERCLOCKWISE), textblock.py:191)              */
  int32_t pad_;
  int64_t out_off;         /* byte offset of the crop in out_dev                                                    */
} ctd_region_job;

#define CTD_REGION_TILE 1024 /* output pixels of a crop per block */

/* cv2.warpPerspective(page, M, (w, h)) with the defaults INTER_LINEAR / BORDER_CONSTANT 0 (+ the rotation) for n crops
 * in ONE launch: OpenCV's fixed-point path (imgproc/imgwarp.cpp of 4.1.2 - 4.10): per output pixel in double, without
 * contraction, W = (Minv[6] x + Minv[7] y) + Minv[8], W = W ? 32 / W : 0, X = rint(clamp(((Minv[0] x + Minv[1] y) +
 * Minv[2]) W)), Y likewise; taps (X >> 5, Y >> 5) + {0,1}^2 with weights 32 (32 - ax)(32 - ay) ... of ax = X & 31,
 * ay = Y & 31, taps outside the page read 0, dst = (sum + 16384) >> 15.  jobs_dev: n jobs; tile_first_dev (n + 1) i32:
 * tile_first[i] = number of CTD_REGION_TILE-pixel tiles of the crops before crop i (a crop of w * h pixels has
 * ceil(w h / CTD_REGION_TILE) of them, a crop with w = 0 none), n_tiles = tile_first[n]; each crop is written at
 * out_dev + out_off as (h, w, C), or (w, h, C) when rotated, contiguous.  n = 0 / n_tiles = 0 launch nothing. */
int ctd_warp_regions(const ctd_region_job* jobs_dev, int32_t n, const int32_t* tile_first_dev, int32_t n_tiles,
                     uint8_t* out_dev, void* stream);

/* ---- OCR input batches: the same crops as the tensors a recogniser reads (ABI v8) ------------------ */

#define CTD_REGION_U8 0  /* element types of the batch tensors */
#define CTD_REGION_F16 1
#define CTD_REGION_F32 2
#define CTD_LAYOUT_NCHW 0
#define CTD_LAYOUT_NHWC 1

/* One SLOT of a ctd_warp_region_batches launch: the rows x Wk pixels that one line takes inside its batch tensor, padding
 * included.  `warp` is the line's crop exactly as in ctd_warp_regions, except that warp.out_off is the ELEMENT offset of
 * the slot's batch tensor in out_dev.  A job with rows = 0 or Wk = 0 has no slot and no tiles. */
typedef struct ctd_region_batch_job {
  ctd_region_job warp;
  int32_t slot; /* position of the line in its batch                                                             */
  int32_t rows; /* rows of the slot (the textheight of the batch): crop rows beyond it are lost, slot rows below
                   the crop are padding                                                                            */
  int32_t Wk;   /* columns of the slot: the width of the batch tensor                                             */
  int32_t cut;  /* columns of the stored crop that are kept (<= Wk); the crop's right end beyond it is lost       */
} ctd_region_batch_job;

/* ctd_warp_regions fused with what an OCR network's input needs, for n slots in ONE launch.  Per slot pixel (y, x) and
 * page channel s: u = the ctd_warp_regions value of stored-crop pixel (y, x) (same doubles, same taps, (sum + 16384) >> 15;
 * rotated crops read region[x][w - 1 - y]) where x < cut and y < the crop's rows, else u = pad (no map, no loads).  Output
 * channel c reads page channel s = c, or C - 1 - c when `reverse` (a BGR page into RGB planes).  The element is
 * tables[c][u]: tables_dev holds C tables of 256 entries IN THE OUTPUT TYPE (the caller builds them, e.g.
 * ((0..255) - mean[c]) / std[c]); the kernel copies bit patterns and does no floating-point arithmetic on values, so the
 * result is the table's to the bit.  dtype CTD_REGION_U8: no table (tables_dev may be NULL), the element is u.  It is
 * stored at element out_off + ((slot C + c) rows + y) Wk + x (CTD_LAYOUT_NCHW) or out_off + ((slot rows + y) Wk + x) C + c
 * (CTD_LAYOUT_NHWC) of out_dev, all in 64 bits.  tile_first_dev (n + 1) i32 as in ctd_warp_regions with rows * Wk pixels
 * per slot; n_tiles = tile_first[n].  pad in 0 .. 255.  n = 0 / n_tiles = 0 launch nothing. */
int ctd_warp_region_batches(const ctd_region_batch_job* jobs_dev, int32_t n, const int32_t* tile_first_dev, int32_t n_tiles,
                            const void* tables_dev, void* out_dev, int32_t dtype, int32_t layout, int32_t reverse,
                            int32_t pad, void* stream);

/* ---- font colours: fill and surround colour of every text line (added within ABI v10) ------------ */

/* An addition to ABI v10: one new entry point and two new structs, nothing existing changes, so CTD_ABI_VERSION stays (a
 * caller built against the earlier v10 header keeps working; one that needs the entry point looks the symbol up).
 * What colour a text line is and what it stands on, from the page, a text mask (normally the page's `mask_refined`, either
 * refine mode) and the line's quad.  Integers only: a row of the result is a function of (page, mask, quad) to the bit.
 * The reference has no such code: its OCR models fill `TextBlock.fg_* / bg_*` line by line; this is this library's own
 * rule.  Per line:
 *   INSIDE  pixel (x, y) with 0 <= x < W, 0 <= y < H inside the quad's bounding box for which the four cross products
 *           (p[k+1] - p[k]) x ((x, y) - p[k]), k = 0..3 (p[4] = p[0]), in int64, are all >= 0 or all <= 0: either winding,
 *           edges included, a degenerate quad selects what the formula selects.
 *   GREY    g = (B*3735 + G*19235 + R*9798 + 16384) >> 15 (the grey of csrc/kernels_tail.hip).
 *   PASS 1  over the inside pixels, ON = mask != 0, OFF = mask == 0: n_on, n_off, g_on = sum of g over ON, g_off over OFF.
 *   PASS 2  a pixel is TEXT-LIKE when its grey is strictly nearer to the ON mean than to the OFF mean, exactly:
 *           |g n_on - g_on| n_off < |g n_off - g_off| n_on (= one integer threshold per line: 2 g n_on n_off above, or below,
 *           g_on n_off + g_off n_on).  Fill: n_fg, s_fg[3] over ON and text-like pixels.  Surround: n_bg, s_bg[3] over inside
 *           pixels that are NOT text-like, ON or OFF.  OFF pixels that are text-like count for neither.
 *   COLOURS fg[c] = (2 s_fg[c] + n_fg) / (2 n_fg), bg likewise (integer division), c in page channel order.
 * A dilated mask covers text plus a ring of background: the ON mean then lies between the two greys, text lies beyond it
 * and is text-like, the ring is not; on a page of two flat colours fg and bg are exactly those colours.  Text whose grey
 * equals its background's (isoluminant) ends in CTD_COLOR_NO_CONTRAST.  "Surround" is the colour around the glyphs; it is
 * an outline colour only where the text has an outline.
 * status:
 *   CTD_COLOR_OK
 *   CTD_COLOR_EMPTY        no inside pixel; the whole row is 0
 *   CTD_COLOR_NO_MASK      n_on == 0: n_on, n_off, g_on, g_off as counted, everything else 0
 *   CTD_COLOR_NO_CONTRAST  n_off == 0 or g_on n_off == g_off n_on (the means tie): fill = mean of the ON pixels (n_fg = n_on),
 *                          surround = mean of the OFF pixels (n_bg = n_off), or the fill where there are none
 *   CTD_COLOR_TOO_LARGE    the bounding box clipped to the page holds more than CTD_COLOR_MAX_PIXELS (2^24) pixels, or a
 *                          coordinate of the quad lies beyond +-CTD_COLOR_MAX_COORD (2^29); decided from the quad, H and W
 *                          before any pixel is read; the rest of the row is 0.  The two bounds are what keeps every
 *                          product above inside int64 (sums <= 255 * 2^24 < 2^32, counts <= 2^24, their products < 2^57;
 *                          edge vectors < 2^30, point offsets < 2^31) and every per-thread partial sum inside uint32. */
#define CTD_COLOR_OK 0
#define CTD_COLOR_EMPTY 1
#define CTD_COLOR_NO_MASK 2
#define CTD_COLOR_NO_CONTRAST 3
#define CTD_COLOR_TOO_LARGE 4
#define CTD_COLOR_MAX_PIXELS (1 << 24)
#define CTD_COLOR_MAX_COORD (1 << 29)

/* One line of a ctd_line_colors launch (a row of the device job table). */
typedef struct ctd_color_job {
  const uint8_t* page_dev; /* the page: BGR u8, 3 interleaved channels, rows `pitch` bytes apart            */
  const uint8_t* mask_dev; /* the mask: u8, rows `mask_pitch` bytes apart                                   */
  int32_t H, W;            /* size of page and mask, >= 1                                                   */
  int32_t pitch;           /* >= 3 W                                                                        */
  int32_t mask_pitch;      /* >= W                                                                          */
  int32_t quad[8];         /* the line's four points (x, y) in the order the detector emits them            */
} ctd_color_job;

/* One row of the result. */
typedef struct ctd_line_color {
  int64_t n_fg, s_fg[3]; /* fill: pixels and per-channel sums (page channel order)                          */
  int64_t n_bg, s_bg[3]; /* surround                                                                        */
  int64_t g_on, g_off;   /* grey sums of pass 1                                                             */
  int32_t n_on, n_off;
  int32_t status;        /* CTD_COLOR_*                                                                     */
  uint8_t fg[3], bg[3];  /* the colours, page channel order                                                 */
  uint8_t pad_[6];
} ctd_line_color;

/* The rule above for n lines in ONE launch (one block per line, no atomics; integer sums: the result does not depend on
 * the order of addition); row i of out_dev is line i's.  Pages of any mix of sizes may share a launch.  n = 0 launches
 * nothing. */
int ctd_line_colors(const ctd_color_job* jobs_dev, int32_t n, ctd_line_color* out_dev, void* stream);

/* ---- erase text on plain backgrounds: cleaned pages and the mask an inpainter still needs (added within ABI v10) ---- */

/* An addition to ABI v10 like the font colours above: one entry point, four structs, nothing existing changes.
 * Most text of a comic page sits on a flat balloon.  Such text needs no inpainting network: look at the background next to
 * the glyphs, and where it is one colour, fill the text with that colour; only the other blocks go to the inpainter.  The
 * reference stops at the mask for that step (`refine_mask(..., REFINEMASK_INPAINT)`); the decision and the fill are this
 * library's own rule, integers only (counts, comparisons, copies: nothing depends on the order of an addition), restated
 * in numpy in tests/erase_ref.py.
 * Per page: the page (BGR u8, H x W x 3, any row pitch), a text mask (u8, H x W, any pitch; a pixel is text where the mask
 * is not 0; normally `mask_refined`, either refine mode) and the page's blocks in blk_list order, each with its `xyxy`.
 * Parameters (ctd_erase_params): grow g (0 .. 8, default 2), ring r (1 .. 16, default 4), tol (0 .. 255, default 12),
 * min_ring (>= 1, default 16).
 * All sets are clipped to the page:
 *   M       the text pixels of the page.
 *   D_k(S)  the pixels of the page within Chebyshev distance <= k of some pixel of S: a (2k+1)^2 square dilation;
 *           D_0(S) = S.
 *   X_b     the box x1 <= x < x2, y1 <= y < y2 of block b's xyxy, clipped to the page (the reference's own slicing).
 *   T_b     = M & X_b, the block's own text.
 *   F_b     = D_g(T_b), what is filled for block b.
 *   R_b     = D_{g+r}(T_b) \ D_g(M), the ring: near this block's text and not near anybody's text.
 * Decision per block: h_c = the 256-bin histogram of page channel c over R_b (c = 0, 1, 2), n_ring = |R_b|,
 *   med_c   = the smallest v with 2 * sum_{u <= v} h_c[u] >= n_ring (the lower median; 0 where n_ring = 0),
 *   cnt_c   = sum of h_c[u] over |u - med_c| <= tol,
 *   PLAIN   iff n_ring >= min_ring and 16 * min_c(cnt_c) >= 15 * n_ring.
 * status, the first that applies:
 *   CTD_ERASE_TOO_LARGE  a coordinate of xyxy lies beyond +-CTD_ERASE_MAX_COORD (2^29)
 *   CTD_ERASE_EMPTY      X_b is empty
 *   CTD_ERASE_TOO_LARGE  X_b (w x h pixels) grown by g + r, (w + 2 (g + r)) (h + 2 (g + r)), holds more than
 *                        CTD_ERASE_MAX_PIXELS (2^24) pixels.  EMPTY and TOO_LARGE are decided before any pixel is read,
 *                        every other field of the row is 0, and the block neither paints nor adds to `rest`.
 *   CTD_ERASE_NO_MASK    T_b is empty (n_fill = n_ring = 0, cnt = med = 0)
 *   CTD_ERASE_NO_RING    n_ring < min_ring
 *   CTD_ERASE_TEXTURED   the histogram test failed
 *   CTD_ERASE_PLAIN
 * Row per block: status, n_fill = |F_b|, n_ring, cnt[3], med[3] (page channel order), pad bytes 0.
 * Outputs per page:
 *   out  (H x W x 3)  out[p] = med of the PLAIN block with the HIGHEST index on that page among those with p in F_b;
 *                     page[p] where there is none.
 *   rest (H x W)      0 where p was painted; otherwise 255 where mask[p] != 0 or p in F_b of a TEXTURED or NO_RING block;
 *                     otherwise 0.
 * Limits: a balloon with a gradient is TEXTURED; text that touches the balloon's outline puts outline pixels into the
 * ring (the 1/16 allowance is for them); a block whose ring is swallowed by its neighbours' text is NO_RING. */
#define CTD_ERASE_PLAIN 0
#define CTD_ERASE_TEXTURED 1
#define CTD_ERASE_NO_RING 2
#define CTD_ERASE_NO_MASK 3
#define CTD_ERASE_EMPTY 4
#define CTD_ERASE_TOO_LARGE 5
#define CTD_ERASE_MAX_PIXELS (1 << 24)
#define CTD_ERASE_MAX_COORD (1 << 29)
#define CTD_ERASE_MAX_GROW 8
#define CTD_ERASE_MAX_RING 16
#define CTD_ERASE_TILE_W 64 /* the paint launch's page tiles */
#define CTD_ERASE_TILE_H 32

/* One block of a ctd_erase_text call (a row of the device job table).  The blocks of one page are consecutive rows, in
 * blk_list order: "index" in the rule above is the row number. */
typedef struct ctd_erase_job {
  int32_t page;    /* row of the page table */
  int32_t xyxy[4]; /* x1, y1, x2, y2 */
  int32_t pad_[3];
} ctd_erase_job;

/* One page of a ctd_erase_text call (a row of the device page table). */
typedef struct ctd_erase_page {
  const uint8_t* page_dev; /* BGR u8, rows `pitch` bytes apart                                              */
  const uint8_t* mask_dev; /* u8, rows `mask_pitch` bytes apart                                             */
  uint8_t* out_dev;        /* H x W x 3, rows `out_pitch` bytes apart; overlaps no input                    */
  uint8_t* rest_dev;       /* H x W, rows `rest_pitch` bytes apart; overlaps no input                       */
  int32_t H, W;            /* >= 1                                                                          */
  int32_t pitch, mask_pitch, out_pitch, rest_pitch; /* >= 3 W, W, 3 W, W                                    */
  int32_t block0, n_blocks; /* the page's rows of the job table                                             */
  int32_t tile0;           /* paint tiles of the pages before this one: each page has ceil(W / CTD_ERASE_TILE_W) *
                              ceil(H / CTD_ERASE_TILE_H)                                                    */
  int32_t pad_;
} ctd_erase_page;

typedef struct ctd_erase_params {
  int32_t grow, ring, tol, min_ring;
  int32_t n_tiles; /* paint tiles of all pages (tile0 of a page after the last) */
  int32_t pad_[3];
} ctd_erase_params;

/* One row of the result. */
typedef struct ctd_erase_row {
  int32_t status; /* CTD_ERASE_* */
  int32_t n_fill, n_ring;
  int32_t cnt[3];
  uint8_t med[3];
  uint8_t pad_[5];
} ctd_erase_row;

/* The rule above for all blocks of all pages of a batch in TWO launches on `stream` with no host wait between them,
 * whatever the number of pages and blocks: the stats launch (one workgroup per block) writes rows_dev[i] for job i, the
 * paint launch (one workgroup per page tile) reads them and writes every byte of every page's `out` and `rest` exactly
 * once.  `params` is read on the host during the call.  n_blocks = 0: the pages are copied and rest = 255 (mask != 0) (one
 * launch); n_pages = 0 launches nothing.  A parameter outside its bounds, a negative count, blocks without pages or a
 * missing table is an error rc and launches nothing. */
int ctd_erase_text(const ctd_erase_job* blocks_dev, int32_t n_blocks, const ctd_erase_page* pages_dev, int32_t n_pages,
                   const ctd_erase_params* params, ctd_erase_row* rows_dev, void* stream);

/* ---- balloon regions: the free area around every plain block (added within ABI v10) ------------------------------- */

/* An addition to ABI v10 like the two above: one entry point, three structs, nothing existing changes.
 * A caller that puts translated text back needs the extent of the free area the old text stood in: the balloon.
 * Downstream tools flood-fill on the host from the text outwards over pixels of the balloon's colour and read the bounding
 * box, the area and the centre of the fill.  This is that step for every block of a batch, this library's own rule, integers
 * only; a connected component does not depend on the order in which it is found, so the result is a function of (page,
 * mask, boxes, erase rows, parameters) to the bit.  Restated in numpy with a queue flood fill in tests/balloon_ref.py.
 * It reuses the erase section's definitions M, D_k, X_b, T_b and F_b = D_g(T_b).
 * Per page: the page and the text mask as in ctd_erase_text, and the page's blocks with their xyxy.  Per block: its
 * ctd_erase_row of a ctd_erase_text call on the same page, mask and box with the same `grow`, read on the device.
 * Parameters (ctd_balloon_params): grow g (0 .. 8, default 2; the value the erase rows were made with), tol (0 .. 255,
 * default 12), reach (0 .. 32, default 8; window growth in eighths of the box side), reach_min (8 .. 1024, default 32;
 * the least window growth in pixels).
 *   Win_b   the window: with w, h the sides of the clipped box X_b, ex = max(reach_min, (w * reach) >> 3) and
 *           ey = max(reach_min, (h * reach) >> 3) (in 64 bits), X_b grown by ex to the left and right and by ey up and down,
 *           then clipped to the page; ww x wh pixels from (wx1, wy1), nw = ceil(ww / 64) words a row.  Where X_b is empty
 *           the window is empty (ww = wh = nw = 0).  The window depends on xyxy, H, W, reach and reach_min alone.
 *           reach_min >= 8 >= g: F_b lies inside the window.
 *   O_b     the open pixels: the p of Win_b with |page[p][c] - med_c| <= tol for c = 0, 1 and 2 (med of the block's erase
 *           row), or p in F_b.  Other blocks' text is not open: it is a hole.
 *   B_b     the region: the union of the 4-CONNECTED components of O_b, taken inside the window only, that contain a pixel
 *           of F_b.
 * status, the first that applies:
 *   CTD_BALLOON_NOT_PLAIN  the job's page or erase_row is no row of its table, or the erase row's status is not
 *                          CTD_ERASE_PLAIN: every other field of the row is 0 and the block's words are all 0.
 *   CTD_BALLOON_TOO_LARGE  nw * wh > CTD_BALLOON_MAX_WORDS (8192: two bit planes of 64 KB in LDS), or > params.max_words:
 *                          every other field of the row is 0.
 *   CTD_BALLOON_OK
 * Row per block (ctd_balloon_row, 48 bytes, no padding): status; area = |B_b|; bbox = x1, y1, x2, y2 of B_b in page
 * coordinates, x2 and y2 exclusive; n_seed = |F_b| (= the erase row's n_fill); sum_x, sum_y = the sums of the page
 * coordinates over B_b (the centre is sum / area); flags:
 *   bits 0 .. 3  left, top, right, bottom: B_b has a pixel in the window's outermost column / row on that side and that
 *                side is NOT the page's edge: the region was cut by the window, or it leaked through a gap in the outline.
 *   bits 4 .. 7  the same order: B_b has such a pixel and that side IS the page's edge.
 * Bits: a block with nw * wh <= CTD_BALLOON_MAX_WORDS owns the words word0 .. word0 + nw * wh - 1 of bits_dev, whatever
 * its status (the caller lays the buffer out from the boxes alone); a block beyond that owns none.  Word word0 + y nw + j
 * covers window row y, window columns 64 j .. 64 j + 63; bit i (the least significant is 0) is window column 64 j + i and
 * is set iff that pixel lies in B_b; bits beyond ww are 0.  Every owned word of an OK or NOT_PLAIN block is written
 * exactly once, nothing else of the buffer is touched.
 * Limits: a balloon whose outline has a gap leaks (the cut flags show it); a balloon with a gradient is TEXTURED for the
 * erase rule and so NOT_PLAIN here; a window holds at most 8192 words (e.g. 512 x 1024 pixels). */
#define CTD_BALLOON_OK 0
#define CTD_BALLOON_NOT_PLAIN 1
#define CTD_BALLOON_TOO_LARGE 2
#define CTD_BALLOON_MAX_WORDS 8192
#define CTD_BALLOON_MAX_REACH 32
#define CTD_BALLOON_MIN_REACH_MIN 8
#define CTD_BALLOON_MAX_REACH_MIN 1024
#define CTD_BALLOON_CUT_LEFT 1 /* flags; the page-edge flags are these << 4 */
#define CTD_BALLOON_CUT_TOP 2
#define CTD_BALLOON_CUT_RIGHT 4
#define CTD_BALLOON_CUT_BOTTOM 8

/* One block of a ctd_balloon_regions call (a row of the device job table).  The page table is ctd_erase_page as it stands
 * (page_dev, mask_dev, H, W, pitch, mask_pitch are read; the out / rest / block / tile fields are not). */
typedef struct ctd_balloon_job {
  int32_t page;      /* row of the page table                          */
  int32_t xyxy[4];   /* x1, y1, x2, y2                                 */
  int32_t erase_row; /* the block's row of the erase rows table        */
  int64_t word0;     /* the block's first word of bits_dev             */
} ctd_balloon_job;

typedef struct ctd_balloon_params {
  int32_t grow, tol, reach, reach_min;
  int32_t max_words; /* the largest nw * wh <= CTD_BALLOON_MAX_WORDS among the call's blocks: sizes the launch's LDS */
  int32_t pad_[3];
} ctd_balloon_params;

/* One row of the result. */
typedef struct ctd_balloon_row {
  int32_t status; /* CTD_BALLOON_* */
  int32_t area;
  int32_t bbox[4];
  int32_t flags;
  int32_t n_seed;
  int64_t sum_x, sum_y;
} ctd_balloon_row;

/* The rule above for n blocks in ONE launch on `stream`, one workgroup per block: rows_dev[i] and the owned words of
 * bits_dev are job i's.  erase_rows_dev may be the rows_dev of a ctd_erase_text call earlier on the same stream (no host
 * step between them).  `params` is read on the host during the call.  n = 0 launches nothing.  A parameter outside its
 * bounds, a negative count, blocks without pages or a missing table is an error rc and launches nothing (bits_dev may be
 * NULL where no block owns a word). */
int ctd_balloon_regions(const ctd_balloon_job* jobs_dev, int32_t n, const ctd_erase_page* pages_dev, int32_t n_pages,
                        const ctd_erase_row* erase_rows_dev, const ctd_balloon_params* params, ctd_balloon_row* rows_dev,
                        uint64_t* bits_dev, void* stream);

/* ---- footprint regions (added within ABI v10) ------------------------------------------------------------------------ */

/* An addition to ABI v10 like the three above: one entry point, one struct, three constants, nothing existing changes.
 * The balloon rule gives a region only to a block whose erase row is PLAIN.  A caption on screentone, narration over artwork,
 * a sound effect, a balloon with a gradient: each comes back NOT_PLAIN with an all-zero plane, the layout and fit calls answer
 * NO_REGION, and the text that the fill calls removed is never put back.  The only honest notion of "where the text may go"
 * there is where the old text stood: the block's footprint.  This call writes it into the SAME rows and the SAME bit buffer as
 * an OK row, so that everything downstream runs unchanged on all blocks.  Integers only.  Restated in numpy, with per-row and
 * per-column spans, in tests/footprint_ref.py.  It reuses M, D_k, X_b, T_b, F_b = D_g(T_b) and Win_b (wx1, wy1, ww, wh, nw)
 * exactly as the erase and balloon sections define them.
 * Parameters (ctd_footprint_params): grow g (0 .. 8; the value the erase rows were made with), pad (0 .. CTD_FOOTPRINT_MAX_PAD,
 * default 4), reach and reach_min (as the balloon call's: they only reproduce the window), max_words (as the balloon call's).
 * Block b is ELIGIBLE iff its job's page is a row of the page table, its erase_row is a row of the erase table, that row's
 * status is CTD_ERASE_TEXTURED or CTD_ERASE_NO_RING (so T_b is not empty), and nw * wh <= min(CTD_BALLOON_MAX_WORDS,
 * params.max_words).  For a block that is not eligible nothing is read beyond that decision and nothing is written: its balloon
 * row and its words keep what the balloon call left there.  For an eligible block:
 *   C_b     the orthogonally convex closure of F_b inside the window: the smallest set Q of window pixels that contains F_b
 *           such that whenever two pixels of Q lie in one row every pixel between them is in Q, and likewise for columns.
 *           Such sets are closed under intersection, so the smallest exists and is unique, whatever order it is found in.
 *           C_b lies inside the bounding box of F_b.  This is what closes the gaps between lines and between words, which a
 *           union of line quads would leave open as stripes.
 *   P_b     = D_pad(C_b), clipped to the window (and so to the page).
 *   N_b     = (M \ X_b) & Win_b, other text: the mask pixels of the page outside the block's own box.  A hole, as in the
 *           balloon rule.
 *   B_b     = P_b \ N_b.
 * Row (ctd_balloon_row, overwritten): status = CTD_BALLOON_OK; area = |B_b| (where it is 0 the bbox is 0); bbox, sum_x, sum_y
 * over B_b; n_seed = |F_b| (= the erase row's n_fill); flags = the balloon rule's eight cut bits computed on B_b, plus bit 8,
 * CTD_BALLOON_FOOTPRINT.
 * Bits: every owned word of an eligible block is written exactly once, bits beyond ww are 0; no other word of the buffer is
 * touched.
 * Limits: the closure of two pieces that share no row and no column stays two pieces; pad is a square dilation; where
 * g + pad > reach_min the window cuts the region, and bits 0 .. 3 of the flags say so; boxes that overlap share mask pixels, as
 * in the erase rule; a block whose window holds more than 8192 words gets no region. */
#define CTD_BALLOON_FOOTPRINT 256 /* flags, bit 8: the row and the plane are the block's footprint */
#define CTD_FOOTPRINT_MAX_PAD 16
#define CTD_FOOTPRINT_DEFAULT_PAD 4

typedef struct ctd_footprint_params {
  int32_t grow, pad, reach, reach_min;
  int32_t max_words; /* as ctd_balloon_params': sizes the launch's LDS */
  int32_t pad_[3];
} ctd_footprint_params;

/* The rule above for n blocks in ONE launch on `stream`, one workgroup per block.  jobs_dev, pages_dev, erase_rows_dev,
 * rows_dev and bits_dev are those of the ctd_balloon_regions call it follows on the same stream (no host step between the
 * two): rows_dev[i] and the owned words of bits_dev are overwritten for the eligible blocks only.  `params` is read on the
 * host during the call.  n = 0 launches nothing.  A parameter outside its bounds, a negative count, blocks without pages or a
 * missing table is an error rc and launches nothing (bits_dev may be NULL where no block owns a word). */
int ctd_balloon_footprints(const ctd_balloon_job* jobs_dev, int32_t n, const ctd_erase_page* pages_dev, int32_t n_pages,
                           const ctd_erase_row* erase_rows_dev, const ctd_footprint_params* params, ctd_balloon_row* rows_dev,
                           uint64_t* bits_dev, void* stream);

/* ---- fill what erase leaves: smooth pull-push fill of a hole mask (added within ABI v10) --------------------------- */

/* An addition to ABI v10 like the three above: one entry point, three structs, nothing existing changes.
 * ctd_erase_text cleans a page only where the background is one colour; text on a gradient or a screentone, text that
 * touches the balloon's outline and text outside every box come back as its `rest` mask.  This is the step that fills that
 * mask: a deterministic smooth fill by pull-push, this library's own rule, integers only, so the result is a function of
 * (page, hole mask) to the byte.  Pull builds an image pyramid of the known pixels; push fills the hole from coarse to fine
 * by bilinear upsampling.  Restated in numpy in tests/fill_ref.py.
 *
 * Inputs, per page: P (H x W x 3 u8, any pitch) and a hole mask R (H x W u8, any pitch).  A pixel is a HOLE where R != 0
 * and KNOWN otherwise.
 * Levels: level 0 is H x W; level l + 1 is ceil(H_l / 2) x ceil(W_l / 2).  The top level T is the first that is 1 x 1 (a
 *   1 x 1 page has T = 0).  Every level pixel carries a colour c[3] (u8) and a flag k.
 * Pull: at level 0, k = KNOWN and c = P.  At level l + 1, pixel (y, x) looks at its up to four children (2y + dy, 2x + dx),
 *   dy, dx in {0, 1}, that lie inside level l and have k = 1; n is their count and S their per-channel sum.
 *     n > 0: k = 1 and c = (2 S + n) / (2 n), integer division, per channel (round half up, the colour code's formula);
 *     n = 0: k = 0.
 * Push: from level T - 1 down to 0.  At level l a pixel (y, x) with k = 0 takes a value bilinearly upsampled from the
 *   FINISHED level l + 1: py = y >> 1, px = x >> 1, ny = clamp(py + (y & 1 ? 1 : -1), 0, H_{l+1} - 1), nx likewise from x
 *   and W_{l+1}, and
 *     c = (9 c[py][px] + 3 c[py][nx] + 3 c[ny][px] + c[ny][nx] + 8) >> 4, per channel;
 *   the pixel then counts as finished.  Pixels with k = 1 keep their pulled colour.
 * Output: `out` is P on KNOWN pixels and the pushed level-0 colour on HOLE pixels.
 * Row per page (ctd_fill_row, 32 bytes, padding 0): status; n_hole, the number of hole pixels; levels = T; top[3], the
 * colour of the top pixel in PAGE channel order, or 0 where it has k = 0.  status:
 *   CTD_FILL_OK        filled by the rule
 *   CTD_FILL_NO_HOLE   n_hole = 0: `out` is a copy of P
 *   CTD_FILL_NO_KNOWN  no known pixel: `out` is a copy of P
 * Properties: every filled value lies within [min, max] of the page's known pixels, per channel; a page whose known pixels
 * all have one colour c is filled with exactly c ((16 c + 8) >> 4 = c); with one known pixel the whole page takes its colour.
 * Limit: a side above CTD_FILL_MAX_SIDE (8192) is an error rc, decided by the shapes alone, and nothing launches.
 * What the rule cannot do: it does not reproduce texture (screentone comes back as its local mean); it does not continue
 * lines or panel borders through the hole; a hole at the page's edge is extrapolated from one side only; the hole is R as
 * given, so anti-aliased fringes outside the mask stay (ctd_erase_text's `grow`, or the INPAINT refine mode's dilation, is
 * where to widen it).
 *
 * Scratch: the launches hand each other the pyramid through scratch_dev, 4-byte aligned, dwords.  One dword a level pixel:
 * c[0] | c[1] << 8 | c[2] << 16 | k << 24, and 0 where k = 0.  With tiles(page) = ceil(H / 64) * ceil(W / 64) and
 * dim(n, l) = ceil(n / 2^l):
 *   dwords 0 .. n_tiles - 1                 the hole count of every 64 x 64 tile, tile tile0 + ty * ceil(W / 64) + tx
 *   dwords lvl0 .. lvl0 + plane(page) - 1   the page's levels 1 .. 6, one after the other, each row-major,
 *                                           plane(page) = sum over l = 1 .. 6 of dim(H, l) * dim(W, l)
 * where a page's tile0 is the sum of tiles() of the pages before it and its lvl0 is n_tiles plus the sum of plane() of the
 * pages before it: scratch_dev holds n_tiles + sum of plane() dwords.  Levels 7 .. T never leave the chip; where T < 6 the
 * levels T + 1 .. 6 are 1 x 1 copies of the top, which changes nothing of the rule.  The contents after the call are not
 * part of the interface. */
#define CTD_FILL_OK 0
#define CTD_FILL_NO_HOLE 1
#define CTD_FILL_NO_KNOWN 2
#define CTD_FILL_MAX_SIDE 8192
#define CTD_FILL_TILE 64

/* One page of a ctd_fill_rest call (a row of the device page table). */
typedef struct ctd_fill_page {
  const uint8_t* page_dev; /* 3 x u8 a pixel, rows `pitch` bytes apart                                      */
  const uint8_t* hole_dev; /* u8, rows `hole_pitch` bytes apart                                             */
  uint8_t* out_dev;        /* H x W x 3, rows `out_pitch` bytes apart; overlaps no input                    */
  int32_t H, W;            /* 1 .. CTD_FILL_MAX_SIDE                                                        */
  int32_t pitch, hole_pitch, out_pitch; /* >= 3 W, W, 3 W                                                   */
  int32_t tile0;           /* tiles of the pages before this one                                            */
  int64_t lvl0;            /* the page's first pyramid dword of scratch_dev                                 */
} ctd_fill_page;

typedef struct ctd_fill_params {
  int32_t n_tiles; /* tiles of all pages (tile0 of a page after the last) */
  int32_t pad_[7];
} ctd_fill_params;

/* One row of the result. */
typedef struct ctd_fill_row {
  int32_t status; /* CTD_FILL_* */
  int32_t n_hole;
  int32_t levels;
  uint8_t top[3];
  uint8_t pad_[17];
} ctd_fill_row;

/* The rule above for all pages of a batch in THREE launches on `stream`, whatever the number and sizes of the pages, with no
 * host wait between them: a pull launch (one workgroup per tile: levels 1 .. 6 and the tile's hole count), a page launch
 * (one workgroup per page: levels 7 .. T, the push down to level 6, rows_dev[i] for page i) and a push launch (one
 * workgroup per tile) that writes every byte of every page's `out` exactly once.  n_hole is a sum of integers: no result
 * depends on an order.  The page table and `params` are read on the host during the call (the table is fetched from the
 * device behind whatever `stream` holds, before the first launch).  n_pages = 0 launches nothing and returns CTD_OK.  A
 * null table, row or scratch pointer with n_pages > 0, a negative count, a null page, hole or out pointer, a side < 1 or
 * > CTD_FILL_MAX_SIDE, a pitch below the row size, a negative lvl0, or tile0 / n_tiles that are not the sums above is an
 * error rc and launches nothing. */
int ctd_fill_rest(const ctd_fill_page* pages_dev, int32_t n_pages, const ctd_fill_params* params, void* scratch_dev,
                  ctd_fill_row* rows_dev, void* stream);

/* ---- texture fill: screentone in the hole by patch matching (added within ABI v10) ----------------------------------- */

/* An addition to ABI v10 like those above: one entry point, three structs, nothing existing changes.
 * ctd_fill_rest gives a hole its smooth surroundings; screentone comes back as its local mean.  This is the step that
 * starts from that result: an exemplar-based fill, a nearest-neighbour field of 7 x 7 patches found by propagation and
 * random search (PatchMatch) with patch voting, this library's own rule, integers only, so the result is a function of
 * (page, hole mask, init, parameters) to the byte, whatever the page's position in the batch and whatever the launch order.
 * Restated in numpy in tests/texture_ref.py.
 *
 * Inputs, per page (any pitches): P (H x W x 3 u8), a hole mask M (H x W u8; a pixel is a HOLE where M != 0) and `init`
 *   (H x W x 3 u8), normally ctd_fill_rest's output for the same P and M.
 * Parameters: the patch radius is 3 (CTD_TEXTURE_PATCH 7); R, the search radius, 1 .. CTD_TEXTURE_MAX_RADIUS (default 32);
 *   n_em 1 .. 16 (5); n_sweep 1 .. 8 (2); n_init 1 .. 16 (8); seed, a u32.
 * Sets: the working image C is `init` on hole pixels and P elsewhere.  A pixel s is a VALID source centre, V(s), where its
 *   whole 7 x 7 patch lies inside the page and holds no hole pixel.  A pixel t is a TARGET where its patch holds a hole
 *   pixel; patch coordinates are clamped to the page for targets.  Each target carries an offset (dy, dx) and a flag ok;
 *   initially ok = 0 and the offset is (0, 0).
 * Cost: D(t, off) = the sum over the 49 patch offsets o and the 3 channels of (C[clamp(t + o)] - C[t + off + o])^2, at most
 *   49 * 3 * 255^2: a u32.  A candidate `off` is ADMISSIBLE where |dy|, |dx| <= R, t + off lies inside the page and
 *   V(t + off) holds.  (A source patch holds no hole pixel, so C is P there.)
 * Hash (mod 2^32): h = x * 0x9E3779B1 + y * 0x85EBCA77 + s * 0xC2B2AE3D + k * 0x27D4EB2F + seed;
 *   h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16
 *   with (x, y) the target, s the sweep index counted from 0 over the whole call, k the draw index inside the sweep.  A draw
 *   of radius rho is (h mod (2 rho + 1)) - rho; draw 2j gives dy and draw 2j + 1 gives dx.
 * Sweeps are Jacobi: a sweep reads the field of the sweep before it and writes a new one.  There are n_em rounds of n_sweep
 *   sweeps and one vote each; round 0 has one extra sweep in front, the INITIAL sweep.  In every sweep a target takes as its
 *   best its own entry of the old field, its cost computed anew (C has changed); where ok = 0 the best is "none".  It then
 *   tries candidates in a fixed order; an admissible candidate replaces the best where its cost is STRICTLY lower (or the
 *   best is none).
 *     initial sweep:   n_init candidates, candidate j = (draw 2j, draw 2j + 1) of radius R.
 *     other sweeps:    propagation: for d in 1, 2, 4, 8 and for each d the neighbours t + (0, -d), (0, +d), (-d, 0), (+d, 0)
 *                      as (dy, dx): a neighbour that lies inside the page, is a target and has ok = 1 in the OLD field gives
 *                      its old offset as the candidate.  Then random search: for rho = R, R >> 1, .., 1 (the j-th of them
 *                      uses draws 2j and 2j + 1) the candidate is the best so far in this sweep, or (0, 0) where it is
 *                      none, plus the draw pair of radius rho.
 * Vote, in place on C (it reads C at source pixels only, which are known, and writes hole pixels only): for a hole pixel p
 *   and every patch offset o let t = p - o; where t lies inside the page and has ok = 1, add C[t + off(t) + o] to S and 1
 *   to n.  n > 0: C[p] = (2 S + n) / (2 n) per channel; n = 0: C[p] keeps its value.
 * Output: `out` is the last C: P on known pixels, bytes untouched.
 * Row per page (ctd_texture_row, 32 bytes, padding 0): status; n_hole; n_target; n_source, the number of valid centres;
 * n_unmatched, the targets with ok = 0 at the end.  status:
 *   CTD_TEXTURE_NO_HOLE    n_hole = 0: `out` is a copy of P
 *   CTD_TEXTURE_NO_SOURCE  n_hole > 0 and n_source = 0: `out` is P with `init` on the holes
 *   CTD_TEXTURE_OK         otherwise: the last C
 * (no status is a special case of the rule: without a hole there is no target, without a source no candidate is admissible).
 * Properties: known pixels are unchanged; every filled value lies within the per-channel [min, max] of P's known pixels and
 * `init`'s hole pixels; where those are all one colour, `out` is that colour.
 * What the rule cannot do: it works at a single scale, so structure wider than a patch -- panel borders, long lines -- is
 * not continued; a target further than R from every valid centre stays unmatched and keeps the smooth fill; a page smaller
 * than 7 x 7 has no source; the defaults come from a measurement of the rule on synthetic screentone (DESIGN.md section
 * 4.30) and have not been tuned on real pages.
 *
 * Scratch: scratch_dev, 16-byte aligned, scratch_bytes long.  With tiles(page) = ceil(H / 64) * ceil(W / 64) and
 * px(page) = H * W:
 *   bytes 0 .. 16 n_tiles - 1        four int32 a 64 x 64 tile (tile tile0 + ty * ceil(W / 64) + tx): its hole pixels, targets,
 *                                    valid centres and, after every sweep, unmatched targets
 *   bytes fld0 .. fld0 + 8 px - 1    the page's two field planes, one after the other, a dword a pixel:
 *                                    (dy & 255) | (dx & 255) << 8 | ok << 16; sweep s reads plane s & 1 and writes the other
 *   bytes cls0 .. cls0 + px - 1      the page's class plane, a byte a pixel: 1 hole, 2 target, 4 valid centre
 * where fld0 = 16 n_tiles + 8 * (px of the pages before) and cls0 = 16 n_tiles + 8 * (px of all pages) + (px of the pages
 * before): 16 bytes a tile and 9 bytes a pixel.  The contents after the call are not part of the interface. */
#define CTD_TEXTURE_OK 0
#define CTD_TEXTURE_NO_HOLE 1
#define CTD_TEXTURE_NO_SOURCE 2
#define CTD_TEXTURE_PATCH 7
#define CTD_TEXTURE_MAX_RADIUS 127
#define CTD_TEXTURE_MAX_SIDE 8192
#define CTD_TEXTURE_TILE 64

/* One page of a ctd_texture_fill call (a row of the device page table). */
typedef struct ctd_texture_page {
  const uint8_t* page_dev; /* 3 x u8 a pixel, rows `pitch` bytes apart                                      */
  const uint8_t* hole_dev; /* u8, rows `hole_pitch` bytes apart                                             */
  const uint8_t* init_dev; /* 3 x u8 a pixel, rows `init_pitch` bytes apart                                 */
  uint8_t* out_dev;        /* H x W x 3, rows `out_pitch` bytes apart; overlaps no input of any page; read back
                              as the aligned dwords that hold its bytes                                     */
  int32_t H, W;            /* 1 .. CTD_TEXTURE_MAX_SIDE                                                     */
  int32_t pitch, hole_pitch, init_pitch, out_pitch; /* >= 3 W, W, 3 W, 3 W                                  */
  int32_t tile0;           /* tiles of the pages before this one                                            */
  int32_t pad_;
  int64_t fld0, cls0;      /* the page's field planes and class plane in scratch_dev, byte offsets          */
} ctd_texture_page;

typedef struct ctd_texture_params {
  int32_t n_tiles; /* tiles of all pages (tile0 of a page after the last) */
  int32_t radius, n_em, n_sweep, n_init;
  uint32_t seed;
  int64_t scratch_bytes; /* >= 16 n_tiles + 9 * (px of all pages) */
} ctd_texture_params;

/* One row of the result. */
typedef struct ctd_texture_row {
  int32_t status; /* CTD_TEXTURE_* */
  int32_t n_hole, n_target, n_source, n_unmatched;
  int32_t pad_[3];
} ctd_texture_row;

/* The rule above for all pages of a batch in 1 + (n_em * n_sweep + 1) + n_em + 1 launches on `stream`, a number the
 * parameters fix, with no host wait between them: a prepare launch (one workgroup per tile: classes, C into `out`, the
 * tile's counts), the sweeps and votes (one workgroup per tile; a tile without a target, or without a hole, returns after
 * reading its count) and a rows launch (one workgroup per page: rows_dev[i] for page i).  All counts are sums of integers.
 * The page table and `params` are read on the host during the call (the table is fetched from the device behind whatever
 * `stream` holds, before the first launch).  n_pages = 0 launches nothing and returns CTD_OK.  A null table, params, row or
 * scratch pointer with n_pages > 0, a negative count, a null page, hole, init or out pointer, a side < 1 or
 * > CTD_TEXTURE_MAX_SIDE, a pitch below the row size, tile0 / n_tiles / fld0 / cls0 that are not the sums above, a
 * scratch_bytes below the layout's size, a parameter outside its range, or an `out` that overlaps an input of any page is
 * an error rc and launches nothing. */
int ctd_texture_fill(const ctd_texture_page* pages_dev, int32_t n_pages, const ctd_texture_params* params, void* scratch_dev,
                     ctd_texture_row* rows_dev, void* stream);

/* ---- layout boxes: the largest free rectangle in every balloon (added within ABI v10) ------------------------------- */

/* An addition to ABI v10 like the four above: one entry point, three structs, nothing existing changes.
 * A typesetter lays translated text into a box, not into a bit plane.  This is the step from the balloon section's region
 * to that box, for every block of a batch, this library's own rule, integers only: the largest axis-aligned rectangle
 * inside the region, and the largest one that still contains the spot the old text stood on, both with a margin to the
 * outline.  Restated in numpy in tests/layout_ref.py.  It builds on the balloon section's Win_b (ww x wh pixels at
 * (wx1, wy1), nw words a row), B_b and word0.
 * Parameters: inset m (0 .. CTD_LAYOUT_MAX_INSET, default 2), the margin in pixels.
 *   E_b     the inner plane: a pixel p of Win_b is in E_b when every pixel q with |qx - px| <= m and |qy - py| <= m lies
 *           inside the window and in B_b: the erosion of B_b by a (2m + 1)-square, clipped at the window.  A page edge
 *           erodes like any other edge.  With m = 0, E_b = B_b.
 *   rectangles  x1, y1, x2, y2 with x2 and y2 exclusive, x1 < x2, y1 < y2, every pixel in E_b.
 *   order   rectangle R is better than S when it has the larger area; at equal area the smaller y1 wins, then the smaller
 *           x1, then the smaller y2.  The order is total and a best rectangle is a maximal one, so the answer is a
 *           function of the plane alone, whatever scheme enumerates the candidates.
 *   rect    the best rectangle of E_b.
 *   a_rect  the best rectangle among those that contain the block's anchor pixel (ax, ay), given in page coordinates.
 *           Where the anchor is no pixel of E_b (or lies outside the window) a_area = 0 and a_rect is all 0.
 * status, the first that applies:
 *   CTD_LAYOUT_NO_REGION  the job's index is no row of the balloon row table (it is params.n_rows or more), the block's
 *                         balloon row has a status other than CTD_BALLOON_OK, or the window holds more than
 *                         params.max_words words (its balloon row is TOO_LARGE anyway): every other field of the row is 0.
 *   CTD_LAYOUT_EMPTY      E_b has no pixel: every other field of the row is 0.
 *   CTD_LAYOUT_OK
 * Row per block, 48 bytes, twelve int32, no padding: status; n_inner = |E_b|; area and rect; a_area and a_rect.  Rectangles
 * are in page coordinates.  Areas fit int32: a window has at most 8192 x 64 pixels.
 * Limits: an L-shaped balloon gets its larger arm; rotated text gets an axis-aligned box (unless the plane is first turned
 * into the block's frame: the "tilted text" section below); a region that leaked through a gap
 * in the outline gives a box cut at the window, and the balloon row's flags say so. */
#define CTD_LAYOUT_OK 0
#define CTD_LAYOUT_NO_REGION 1
#define CTD_LAYOUT_EMPTY 2
#define CTD_LAYOUT_MAX_INSET 16

/* One block of a layout call (a row of the device job table).  Job i belongs to row i of the balloon row table. */
typedef struct ctd_layout_job {
  int32_t win[4]; /* the block's window x1, y1, x2, y2 in page coordinates, as the balloon call's caller laid it out */
  int32_t ax, ay; /* the anchor, page coordinates                                                                      */
  int64_t word0;  /* the block's first word of bits_dev                                                                */
} ctd_layout_job;

typedef struct ctd_layout_params {
  int32_t inset;
  int32_t max_words; /* the largest nw * wh <= CTD_BALLOON_MAX_WORDS among the call's blocks: sizes the launch's LDS */
  int32_t n_rows;    /* the rows of balloon_rows_dev: a job at or beyond it is NO_REGION and reads none of the table  */
  int32_t pad_;
} ctd_layout_params;

/* One row of the result. */
typedef struct ctd_layout_row {
  int32_t status; /* CTD_LAYOUT_* */
  int32_t n_inner;
  int32_t area;
  int32_t rect[4];
  int32_t a_area;
  int32_t a_rect[4];
} ctd_layout_row;

/* The rule above for n blocks in ONE launch on `stream`, one workgroup per block: rows_dev[i] is job i's.
 * balloon_rows_dev and bits_dev may be the rows_dev and bits_dev of a balloon call earlier on the same stream (no host step
 * between them); bits_dev is read only, 8-byte aligned; rows_dev needs 4-byte alignment.  `params` is read on the host during
 * the call.  n = 0 launches nothing.  inset outside 0 .. 16, max_words outside 0 .. 8192, a negative n or n_rows, or a missing
 * table with n > 0 is an error rc and launches nothing (bits_dev may be NULL where max_words is 0). */
int ctd_layout_boxes(const ctd_layout_job* jobs_dev, int32_t n, const ctd_balloon_row* balloon_rows_dev,
                     const uint64_t* bits_dev, const ctd_layout_params* params, ctd_layout_row* rows_dev, void* stream);

/* ---- shaped fit: text lines that follow each balloon's outline (added within ABI v10) -------------------------------- */

/* An addition to ABI v10 like the ones above: one entry point, five structs, nothing existing changes.
 * The layout section's rectangle holds about 64 % of an elliptic balloon.  A typesetter sets short-long-short lines that
 * follow the outline instead.  This is that step for every block of a batch and every candidate size of its run, this
 * library's own rule, integers only.  Restated in numpy in tests/fit_ref.py.  It builds on the layout section's job (window,
 * word0, anchor (ax, ay) in page coordinates) and its E_b: B_b eroded by a (2m + 1)-square and clipped at the window, inset
 * m in 0 .. CTD_LAYOUT_MAX_INSET.  The caller adds the stroke radius of the text to the inset.
 * Inputs, per block b: the layout job; a run of G_b glyphs (0 .. CTD_FIT_MAX_GLYPHS); C_b candidates (0 ..
 *   CTD_FIT_MAX_CANDS) in ascending order of size, consecutive rows of the candidate table; optionally a break byte per
 *   glyph (non-zero: a line may end after this glyph); without a break table a line may end after every glyph.
 * Inputs, per candidate c: a line height h >= 1, a gap g >= 0 and the run's cumulative advances at that size, G_b + 1
 *   non-decreasing int32 of which the first is 0 (the host makes the prefix sums).
 *   axis run   of window row y: where pixel (ax, y) is in E_b, [l(y), r(y)), the maximal run of ones of that row of E_b that
 *           contains column ax; otherwise the row has none.  (The run that contains ax of an AND of rows is the
 *           intersection of the rows' own axis runs.)
 *   slot    of top row t at height h: it exists where rows t .. t + h - 1 all lie in the window and all have an axis run.
 *           L = max l and R = min r over those rows, half = min(ax - L, R - ax); the slot is [ax - half, ax + half): 2 half
 *           wide and symmetric about the axis.
 *   stack   of n lines for (h, g): total = n h + (n - 1) g, top = ay - (total >> 1), line k has the top row
 *           top + k (h + g).  The stack is admissible where every line has a slot.
 *   break   glyphs.flow's horizontal greedy breaker with the slot's width for the box's: line k starts at glyph s_k
 *           (s_0 = 0) and ends before the first glyph whose advance summed from s_k would pass the slot's width; where that
 *           is not the run's end and there is a break table, it ends after the last allowed break in s_k .. end - 1 where
 *           there is one, and stays where it is otherwise (a hard break).  A line whose first glyph does not fit its slot
 *           makes the stack FAIL (flow lets that glyph stand alone; here the text would leave the balloon).
 *   fit     stack n fits where it is admissible and the breaker places all G_b glyphs in exactly n lines, none of them
 *           empty.  A candidate's n is the smallest n in 1 .. CTD_FIT_MAX_LINES that fits; the block's answer is the
 *           candidate of the largest index that has one.  Every (candidate, n) is evaluated: nothing is assumed monotone.
 * status, the first that applies:
 *   CTD_FIT_NO_REGION  as CTD_LAYOUT_NO_REGION (no balloon row, a balloon row that is not OK, more than max_words words)
 *   CTD_FIT_NO_TEXT    G_b = 0 or C_b = 0
 *   CTD_FIT_NO_ANCHOR  (ax, ay) is no pixel of E_b (or lies outside the window)
 *   CTD_FIT_NO_FIT     no candidate has a stack that fits
 *   CTD_FIT_OK
 * In every status but OK all other fields of the row are 0.
 * Row per block, 656 bytes of int32, no padding: status; cand, the candidate's index among the block's; n_lines; n_inner =
 * |E_b|; CTD_FIT_MAX_LINES line records of five int32 (the start glyph, the slot's x1 and the line's top row in page
 * coordinates, the slot's width, the length of the line's advances <= width); the records beyond n_lines are 0.
 * PRECONDITION: a candidate's cumulative advances do not decrease.  The entry point sees no device array of that size; where
 * they do decrease the lines are some function of the table, and nothing outside the tables is read.
 * Limits: the order of the glyphs is kept; this entry point moves no word down to balance the lines, so a last line may be
 * short (ctd_layout_fit_balanced below does); horizontal lines only; a region whose anchor column leaves the region is cut there (a comb's teeth, the far side of a
 * ring); one axis per block, so an L-shaped balloon still gets the arm of its anchor. */
#define CTD_FIT_OK 0
#define CTD_FIT_NO_REGION 1
#define CTD_FIT_NO_TEXT 2
#define CTD_FIT_NO_ANCHOR 3
#define CTD_FIT_NO_FIT 4
#define CTD_FIT_MAX_CANDS 16
#define CTD_FIT_MAX_LINES 32
#define CTD_FIT_MAX_GLYPHS 4096

/* One block's text (a row of the device fit job table, beside row i of the layout job table), 24 bytes. */
typedef struct ctd_fit_job {
  int32_t n_glyphs; /* G_b                                                                                  */
  int32_t n_cands;  /* C_b                                                                                  */
  int32_t cand0;    /* the block's first row of the candidate table                                         */
  int32_t pad_;
  int64_t break0;   /* the run's first byte of breaks_dev (n_glyphs bytes), or -1: a break after every glyph */
} ctd_fit_job;

/* One candidate size of one block (a row of the device candidate table), 16 bytes. */
typedef struct ctd_fit_cand {
  int32_t line; /* h, the line height                                                      */
  int32_t gap;  /* g, the rows between two lines                                           */
  int64_t cum0; /* the first of the run's n_glyphs + 1 cumulative advances in cum_dev      */
} ctd_fit_cand;

typedef struct ctd_fit_params {
  int32_t inset;
  int32_t max_words; /* as ctd_layout_params                                               */
  int32_t n_rows;    /* as ctd_layout_params                                               */
  int32_t n_cands;   /* the rows of cands_dev                                              */
  int64_t n_cum;     /* the int32 of cum_dev                                               */
  int64_t n_breaks;  /* the bytes of breaks_dev                                            */
} ctd_fit_params;

/* One line of a fitted stack. */
typedef struct ctd_fit_line {
  int32_t start;  /* the line's first glyph                                                */
  int32_t x1;     /* the slot's left column, page coordinates                              */
  int32_t y;      /* the line's top row, page coordinates                                  */
  int32_t width;  /* the slot's width                                                      */
  int32_t length; /* the sum of the line's advances                                        */
} ctd_fit_line;

/* One row of the result. */
typedef struct ctd_fit_row {
  int32_t status; /* CTD_FIT_* */
  int32_t cand;
  int32_t n_lines;
  int32_t n_inner;
  ctd_fit_line lines[CTD_FIT_MAX_LINES];
} ctd_fit_row;

/* The rule above for n blocks in ONE launch on `stream`, one workgroup per block: rows_dev[i] is the row of jobs_dev[i] and
 * fit_jobs_dev[i].  jobs_dev, balloon_rows_dev and bits_dev are ctd_layout_boxes' (bits_dev is read only; rows_dev needs
 * 4-byte alignment, cum_dev too).  `params` is read on the host during the call, and so are fit_jobs_dev and cands_dev: the two
 * small tables are fetched from the device behind whatever `stream` holds, before the launch, so that every offset is checked
 * before a kernel uses it.  n = 0 launches nothing.  An error rc, and no launch, for: a negative n, n_rows, n_cands, n_cum or
 * n_breaks; inset outside 0 .. 16; max_words outside 0 .. 8192; a missing table with n > 0 (bits_dev may be NULL where
 * max_words is 0, cands_dev, cum_dev and breaks_dev where their counts are 0); a job with n_glyphs outside 0 ..
 * CTD_FIT_MAX_GLYPHS, n_cands outside 0 .. CTD_FIT_MAX_CANDS, candidate rows beyond n_cands, or a break0 that is neither -1
 * nor leaves n_glyphs bytes inside n_breaks; a candidate of a job with line < 1, gap < 0, or a cum0 that does not leave
 * n_glyphs + 1 int32 inside n_cum. */
int ctd_layout_fit(const ctd_layout_job* jobs_dev, const ctd_fit_job* fit_jobs_dev, int32_t n,
                   const ctd_balloon_row* balloon_rows_dev, const uint64_t* bits_dev, const ctd_fit_cand* cands_dev,
                   const int32_t* cum_dev, const uint8_t* breaks_dev, const ctd_fit_params* params, ctd_fit_row* rows_dev,
                   void* stream);

/* ---- shaped fit, balanced lines (added within ABI v10) ------------------------------------------------------------------ */

/* An addition to ABI v10: two entry points, one struct; ctd_layout_fit, its structs and its results do not change.
 * The greedy breaker above fills every line and leaves what remains to the last one, which may then stand far off the
 * outline.  This is the same fit with the slack spread evenly over the lines.  Integers only.  Restated in numpy in
 * tests/balance_ref.py.
 *   start     everything up to the block's answer is the shaped-fit rule unchanged: the status, the candidate c*, its n*
 *             lines, and the slots of that stack with their widths w_0 .. w_(n* - 1).  The balanced breaker changes neither
 *             the size nor the line count: for a fixed stack, filling each line to the furthest allowed break is optimal for
 *             feasibility.  cum is c*'s cumulative advances, G the run's glyphs.
 *   boundary  a line may end in front of glyph e, 1 <= e <= G, where e = G, or there is no break table, or the break byte of
 *             glyph e - 1 is non-zero.
 *   vector    0 = s_0 < s_1 < ... < s_n* = G is admissible where every s_1 .. s_(n* - 1) is a boundary and
 *             cum[s_(k+1)] - cum[s_k] <= w_k for every k.  Lines are non-empty by glyph count; advances of 0 are legal.
 *   cost      the sum over k of (w_k - (cum[s_(k+1)] - cum[s_k]))^2 in int64: at most 32 x 32766^2 < 2^35.  The sum of the
 *             slacks is fixed by c* and n*, so the cost measures only how evenly the slack is spread.
 *   answer    the admissible vector of least cost; among equals the lexicographically largest (s_1, .., s_(n* - 1)): what a
 *             backward table g(k, s) gives when a forward pass takes the largest end that attains it.
 *   fallback  where no admissible vector exists the greedy lines stand: the greedy stack needed a hard break and no other
 *             vector avoids one.
 * The row is ctd_fit_row as above; against ctd_layout_fit's row only `start` and `length` of the line records may differ.
 * A second row per block, ctd_fit_balance, 16 bytes: balanced, 1 where the answer was written and 0 where the greedy lines
 * stand; cost, the cost of the lines written.  Every field is 0 in any status but OK.
 * Limits: squares of the slack in pixels, so a narrow slot at the top and a wide one in the middle are drawn to the same
 * slack, not to the same share of their width; the last line is treated like every other (no allowance for a short last
 * line); horizontal lines only, and the limits of the shaped fit above other than its first. */
typedef struct ctd_fit_balance {
  int32_t balanced; /* 1: the balanced lines were written, 0: the greedy lines stand      */
  int32_t pad_;
  int64_t cost;     /* the sum of the squared slacks of the lines written                 */
} ctd_fit_balance;

/* The bytes of work_dev that ctd_layout_fit_balanced needs for the n jobs of the HOST copy of a fit job table: a function
 * of the table alone, 8 x 32 x (n_glyphs + 1) bytes for every job with n_glyphs in 1 .. CTD_FIT_MAX_GLYPHS (a block's table
 * of states where it does not fit the block's LDS), 0 for any other job.  -1 for a negative n or a missing table with n > 0. */
int64_t ctd_layout_fit_work_bytes(const ctd_fit_job* fit_jobs_host, int32_t n);

/* ctd_layout_fit with the balanced breaker, ONE launch, one workgroup per block: the block that has found the winning stack
 * runs the dynamic program and writes rows_dev[i] and bal_dev[i] (4-byte alignment each; every int32 of both written once).
 * All of ctd_layout_fit's arguments, reads and refusals apply.  work_dev: work_bytes bytes of scratch, 8-byte aligned, its
 * contents do not matter before and mean nothing after; nothing behind work_bytes is written.  An error rc, and no launch and
 * no row written, too for: a NULL bal_dev with n > 0; a negative work_bytes; a work_bytes below
 * ctd_layout_fit_work_bytes of the job table; a work_dev that is NULL or not 8-byte aligned where that is more than 0. */
int ctd_layout_fit_balanced(const ctd_layout_job* jobs_dev, const ctd_fit_job* fit_jobs_dev, int32_t n,
                            const ctd_balloon_row* balloon_rows_dev, const uint64_t* bits_dev, const ctd_fit_cand* cands_dev,
                            const int32_t* cum_dev, const uint8_t* breaks_dev, const ctd_fit_params* params,
                            ctd_fit_row* rows_dev, ctd_fit_balance* bal_dev, void* work_dev, int64_t work_bytes, void* stream);

/* ---- typeset: text layers with outlines composited into pages (added within ABI v10) ---------------------------------- */

/* An addition to ABI v10 like the five above: one entry point, six structs, nothing existing changes.
 * The layout section ends at the box; the translated text, rendered by any font engine into 8-bit coverage bitmaps, goes
 * back into the device pages here, with the outline that is the standard manga treatment.  This library's own rule,
 * integers only, so a result is a function of its inputs to the byte.  Restated in numpy in tests/typeset_ref.py.
 *   page    P, H x W x 3 u8 at any pitch and any byte alignment, sides 1 .. CTD_TYPESET_MAX_SIDE; modified in place.
 *   layer   a coverage bitmap cov, h x w u8 (h and w 1 .. CTD_TYPESET_MAX_SIDE), rows cov_pitch >= 0 bytes apart from byte
 *           cov0 >= 0 of ONE packed coverage buffer; its page; the page coordinates (x0, y0) of the bitmap's top-left pixel
 *           (any int32 with |x0|, |y0| <= 2^29); a fill colour f[3] and a stroke colour s[3] in the page's channel order; a
 *           stroke radius r, 0 .. CTD_TYPESET_MAX_RADIUS; a clip rectangle cx1, cy1, cx2, cy2, exclusive, page coordinates.
 *   F(p)    cov(p - (x0, y0)), and 0 outside the bitmap.
 *   S(p)    for r > 0 the max of F(q) over all q with (qx - px)^2 + (qy - py)^2 <= r^2: a grey-scale dilation by a disk
 *           of 5, 13, 29, 49, 81, 113, 149, 197, 253, 317, 377, 441 pixels for r = 1 .. 12.  For r = 0, S = 0.
 *   blend   blend(c, k, a) = (c (255 - a) + k a + 127) / 255, integer division, per channel: a = 0 gives c, a = 255 gives
 *           k, and the result always lies between c and k.
 *   one layer   every pixel p inside the page, the clip and the bitmap's rectangle grown by r on every side becomes
 *           blend(blend(P(p), s, S(p)), f, F(p)): the stroke goes on first and the fill over it.  No other pixel changes.
 *   several layers   the layers of one call are applied in the order of the layer table.  Where they overlap the later one
 *           sees the earlier one's result, so swapping two overlapping layers changes bytes.
 *   row     per layer two int32: n_fill, the pixels written with F > 0, and n_stroke, the pixels written with S > 0.  Sums
 *           of integers: they depend on no order.
 *   invalid a layer draws nothing and counts nothing, and none of its coverage is read, when its page is not one of
 *           0 .. n_pages - 1, w or h is 0 or above CTD_TYPESET_MAX_SIDE, r is above CTD_TYPESET_MAX_RADIUS, cov0 or
 *           cov_pitch is negative, or cov0 + (h - 1) cov_pitch + w is more than params.cov_bytes.
 * The launch works on page tiles of CTD_TYPESET_TILE_W x CTD_TYPESET_TILE_H pixels, one workgroup per tile of the tile
 * table, which walks the tile's entries (layer indices) in table order.  The caller lists the touched tiles only (tile
 * (tx, ty) of a page covers x in tx TILE_W .. and y in ty TILE_H ..) and, per tile, in ascending order every layer whose
 * grown rectangle, cut to page and clip, meets it.
 * PRECONDITION: a page tile appears at most once in the tile table, and the pages of one call do not overlap in memory.
 * The entry point cannot see device tables; typeset.typeset_tables is their producer.  Short of that the tables are free:
 * a tile that is no tile of its page, an entry that names no layer, a layer of another page or one that does not meet the
 * tile contribute nothing, and entry ranges are cut to 0 .. n_entries.  A wrong table costs pixels and never faults.
 * Limits: the radius is a whole number of pixels, and a max over an anti-aliased bitmap gives an outline whose edge is as
 * smooth as the glyph's and no smoother; no resampling and no rotation, the caller renders at the final size and angle; no
 * gamma; a layer is opaque text, there is no per-layer opacity. */
#define CTD_TYPESET_MAX_SIDE 8192
#define CTD_TYPESET_MAX_RADIUS 12
#define CTD_TYPESET_TILE_W 64
#define CTD_TYPESET_TILE_H 32

/* One page of a typeset call (a row of the device page table), 24 bytes. */
typedef struct ctd_typeset_page {
  void* page_dev; /* H x W x 3 u8, written in place                                */
  int32_t H, W;
  int64_t pitch;  /* bytes from a row to the next, at least 3 W                    */
} ctd_typeset_page;

/* One layer (a row of the device layer table), 56 bytes. */
typedef struct ctd_typeset_layer {
  int64_t cov0;      /* the bitmap's first byte of cov_dev                         */
  int32_t page;
  int32_t x0, y0;    /* page coordinates of the bitmap's top-left pixel            */
  int32_t w, h;
  int32_t cov_pitch;
  int32_t clip[4];   /* x1, y1, x2, y2, exclusive, page coordinates                */
  uint8_t fill[3];   /* page channel order                                         */
  uint8_t stroke[3];
  uint8_t radius;
  uint8_t pad_;
} ctd_typeset_layer;

/* One touched tile (a row of the device tile table, n_tiles + 1 rows), 16 bytes.  The tile's entries are
 * entries_dev[first .. the next row's first); the last row's `first` is the entry count, its other fields are unused. */
typedef struct ctd_typeset_tile {
  int32_t page, tx, ty;
  int32_t first;
} ctd_typeset_tile;

typedef struct ctd_typeset_params {
  int32_t n_layers, n_pages, n_tiles, n_entries;
  int64_t cov_bytes; /* the size of cov_dev: no layer reads beyond it                */
  int64_t pad_;
} ctd_typeset_params;

/* One row of the result. */
typedef struct ctd_typeset_row {
  int32_t n_fill, n_stroke;
} ctd_typeset_row;

/* The rule above for all pages of a batch in ONE launch on `stream`, one workgroup per row of the tile table: a workgroup
 * reads its tile of the page once, applies the tile's layers in table order on chip (the coverage patch of each in LDS) and
 * writes the tile once, so a page byte is read once and written once whatever the number of layers, and the order of
 * overlapping layers is exact without an atomic on a pixel.  There is no cap on the layers of a tile.  All tables are on the
 * device (entries_dev: int32 layer indices; rows_dev: n_layers rows, 4-byte aligned, cleared by the call before the launch,
 * summed into by integer atomics); `params` is read on the host during the call.  n_layers = 0 or n_tiles = 0 launches
 * nothing (the rows are still cleared).  A negative count or cov_bytes, a missing table where its count is positive
 * (pages_dev: n_pages; layers_dev and rows_dev: n_layers; tiles_dev: n_tiles; entries_dev: n_entries), or cov_dev NULL with
 * cov_bytes > 0 is an error rc and launches nothing. */
int ctd_typeset(const ctd_typeset_page* pages_dev, const ctd_typeset_layer* layers_dev, const ctd_typeset_tile* tiles_dev,
                const int32_t* entries_dev, const uint8_t* cov_dev, const ctd_typeset_params* params,
                ctd_typeset_row* rows_dev, void* stream);

/* ---- typeset from a glyph atlas: glyph runs composited into pages (added within ABI v10) ------------------------------- */

/* An addition to ABI v10 like the ones above: one entry point, four structs, nothing existing changes.
 * The section above takes one coverage bitmap per layer; a font engine gives one bitmap per GLYPH plus metrics.  Here every
 * distinct glyph lies once in an atlas on the device, a layer is a run of placements, and the layer's coverage is assembled
 * on chip.  Everything but the coverage is the typeset rule above, unchanged.  Restated in tests/glyph_ref.py.
 *   glyph   an atlas record (off, w, h): dense rows of w bytes from byte off of the atlas, sides 0 .. CTD_TYPESET_MAX_SIDE.
 *           A side of 0 is legal (a space) and draws nothing.
 *   layer   a page, a fill colour, a stroke colour, a stroke radius r of 0 .. CTD_TYPESET_MAX_RADIUS and a clip rectangle:
 *           the bitmap layer's fields minus the bitmap.
 *   placement   (layer, glyph, x, y): (x, y) the page coordinates of the glyph bitmap's top-left pixel.
 *   F(p)    the MAX over the layer's placements of the glyph's coverage at p, and 0 where no glyph lies.  A max, not a
 *           saturating sum: it needs no order and is idempotent, so a glyph placed twice at one position counts once.
 *   S, blend, one layer, several layers, row   as above, with this F: S is the disk max of F, a pixel inside the page and the
 *           clip becomes blend(blend(P, s, S), f, F), layers apply in table order, the row counts the pixels with F > 0 and
 *           with S > 0.  (Where F = S = 0 the blend returns the pixel, so "the rectangle grown by r" needs no statement.)
 * The result is by definition what ctd_typeset gives for the block bitmap that the max-paste of the glyphs produces.
 *   invalid a placement contributes nothing, and none of its coverage is read, when its layer or its glyph index is out of
 *           range, its layer is on another page than the tile (or has r above CTD_TYPESET_MAX_RADIUS), its glyph record has
 *           a side above CTD_TYPESET_MAX_SIDE or a negative one, off < 0 or off + w h > params.atlas_bytes, or |x| or |y|
 *           is above 2^29.
 * The launch is ctd_typeset's: one workgroup per row of the tile table (ctd_typeset_tile, the same tiles).  A tile's entries
 * are int32 PLACEMENT indices, ascending, so the placements of one layer are consecutive and layers ascend; the workgroup
 * groups consecutive entries of equal layer.  The caller lists, per touched tile, every placement whose rectangle grown by
 * its layer's r, cut to page and clip, meets it.  The PRECONDITION above holds here too (a page tile at most once, pages do
 * not overlap in memory); glyphs.glyph_tables is the producer.  Short of that the tables are free: a tile that is none of its
 * page returns, an entry that names no placement or a placement that misses the tile contributes nothing, entry ranges are
 * cut to 0 .. n_entries, and entries of one layer that are not consecutive merely apply that layer twice.  A wrong table
 * costs pixels and never faults.
 * Limits beyond those above: overlap within a layer is max, not sum; one colour per layer, so a coloured word is a layer of
 * its own; no kerning or shaping, which stay a font engine's (rasterisation: the section after this one). */

/* One glyph layer (a row of the device layer table), 32 bytes. */
typedef struct ctd_glyph_layer {
  int32_t page;
  int32_t clip[4];   /* x1, y1, x2, y2, exclusive, page coordinates                */
  uint8_t fill[3];   /* page channel order                                         */
  uint8_t stroke[3];
  uint8_t radius;
  uint8_t pad_;
  int32_t pad2_;
} ctd_glyph_layer;

/* One placement (a row of the device placement table), 16 bytes. */
typedef struct ctd_glyph_place {
  int32_t layer, glyph;
  int32_t x, y;      /* page coordinates of the glyph bitmap's top-left pixel      */
} ctd_glyph_place;

/* One glyph of the atlas (a row of the device record table), 16 bytes. */
typedef struct ctd_glyph_record {
  int64_t off;       /* the glyph's first byte of atlas_dev; rows are w bytes apart */
  int32_t w, h;
} ctd_glyph_record;

typedef struct ctd_glyph_params {
  int32_t n_layers, n_pages, n_tiles, n_entries;
  int32_t n_places, n_glyphs;
  int64_t atlas_bytes; /* the size of atlas_dev: no placement reads beyond it        */
} ctd_glyph_params;

/* The rule above for all pages of a batch in ONE launch on `stream`, one workgroup per row of the tile table, which reads
 * its tile of the page once, assembles each layer's coverage patch in LDS from the atlas, runs the outline and the blend of
 * ctd_typeset on it and writes the tile once.  There is no cap on the placements of a tile or of a layer.  All tables are on
 * the device (pages_dev: ctd_typeset_page; tiles_dev: ctd_typeset_tile, n_tiles + 1 rows; entries_dev: int32 placement
 * indices; rows_dev: n_layers ctd_typeset_row, 4-byte aligned, cleared by the call before the launch, summed into by integer
 * atomics); `params` is read on the host during the call.  n_tiles = 0 or n_layers = 0 does nothing at all: no launch, and
 * the rows are not touched.  A negative count or atlas_bytes, a missing table where its count is positive (pages_dev:
 * n_pages; layers_dev and rows_dev: n_layers; places_dev: n_places; glyphs_dev: n_glyphs; tiles_dev: n_tiles; entries_dev:
 * n_entries), or atlas_dev NULL with atlas_bytes > 0 is an error rc and launches nothing. */
int ctd_typeset_glyphs(const ctd_typeset_page* pages_dev, const ctd_glyph_layer* layers_dev, const ctd_glyph_place* places_dev,
                       const ctd_glyph_record* glyphs_dev, const ctd_typeset_tile* tiles_dev, const int32_t* entries_dev,
                       const uint8_t* atlas_dev, const ctd_glyph_params* params, ctd_typeset_row* rows_dev, void* stream);

/* ---- glyph outlines rasterised into the atlas (added within ABI v10) ------------------------------------------------------ */

/* An addition to ABI v10 like the ones above: one entry point, one struct, nothing existing changes.
 * The section above composites glyphs that already lie in the atlas.  This one puts them there: quadratic outlines are kept
 * on the device, and any number of (glyph, size) instances are rasterised straight into the atlas's own buffer in ONE
 * launch.  All integers, so the kernel and the restatement (tests/raster_ref.py) agree on every byte.
 *   outline   a glyph is n segments, each a row of 6 int32 in font units, y up: (x0, y0, cx, cy, x1, y1), |v| <= 2^15 (the
 *             kernel clamps a value beyond that).  A segment whose control point equals either end point (in font units) is
 *             a straight line; any other is a quadratic Bezier.  Contours are closed by the caller's segments; the rule
 *             never adds an edge.  Cubic curves are not accepted.
 *   instance  a glyph at scale S, 16.16 pixels per font unit, 0 < S <= CTD_RASTER_MAX_SCALE = 2^22.  A point maps to 26.6
 *             fixed point, y down: X = (x S + 512) >> 10, Y = (-y S + 512) >> 10, arithmetic shifts on int64.
 *   box       from ALL transformed points, controls included: bx = floor(minX / 64), by = floor(minY / 64),
 *             w = ceil(maxX / 64) - bx, h = ceil(maxY / 64) - by.  A glyph without segments has w = h = 0.  Sides above
 *             CTD_RASTER_MAX_SIDE are refused.
 *   flatten   for a curve, dd = max(|X0 - 2 X1 + X2|, |Y0 - 2 Y1 + Y2|), L the smallest of 0 .. 5 with (dd >> 2L) <= 16 (5 if
 *             none), N = 1 << L, Q_k = ((N-k)^2 P0 + 2 k (N-k) P1 + k^2 P2 + (N^2 >> 1)) >> 2L for k = 0 .. N, the edges
 *             Q_k -> Q_k+1.  A line is one edge.  Rounded convex combinations of integers stay inside the control box, so
 *             no edge leaves the box.
 *   coverage  a pixel row py has 16 sample rows at Ys = 64 (by + py) + 4 k + 2, k = 0 .. 15.  An edge with ends lo, hi
 *             ordered by Y, lo.Y != hi.Y, crosses a sample row iff lo.Y <= Ys < hi.Y; its direction d is +1 if the edge runs
 *             down (its first point is lo), else -1; its crossing, in 1/256 pixel from the box's left, is
 *             Xc = floor(4 (lo.X (hi.Y - Ys) + hi.X (Ys - lo.Y)) / (hi.Y - lo.Y)) - 256 bx (int64; 0 <= Xc <= 256 w always).
 *             A_k(px) = sum over edges of d clamp(256 (px + 1) - Xc, 0, 256), and the byte is
 *             c(px, py) = (255 sum_k min(|A_k(px)|, 256) + 2048) >> 12.
 * |.| makes the two contour orientations equal.  The clamp is how overlapping contours are handled: exact where the winding
 * is 0 or +-1 on a sample row, saturating elsewhere.
 * What the rule cannot do: no hinting (stems are not moved to the pixel grid; it is an unhinted rasteriser of ordinary
 * quality); no sub-pixel positioning (an instance is rasterised at the origin's pixel phase only); no cubics (convert them
 * first, e.g. with cu2qu); 16 vertical samples, so a horizontal edge is placed to 1/16 pixel (horizontally the area is exact
 * to 1/256); overlapping contours saturate instead of following a fill rule.
 * A job is one instance: the host computes off, w, h, bx, by with the rule above (it must, to lay out the atlas) and the
 * kernel trusts none of it.  Status per job, the first that applies:
 *   CTD_RASTER_REFUSED  the segment range leaves 0 .. n_segs, the record off .. off + w h leaves 0 .. atlas_bytes, a side is
 *                       negative or above CTD_RASTER_MAX_SIDE, or the scale is not in 1 .. CTD_RASTER_MAX_SCALE.  Nothing is
 *                       written.
 *   CTD_RASTER_EMPTY    w or h is 0, or there are no segments.  Nothing is written.
 *   CTD_RASTER_OK       the w h bytes of the record are written, dense rows of w bytes, every one of them.
 * A crossing outside 0 .. 256 w is clamped, and X - 64 bx is clamped to +-2^30: a wrong table costs pixels and never faults.
 * Records of different jobs must not overlap (the caller's to see to, as for the pages of ctd_typeset). */
#define CTD_RASTER_MAX_SIDE 1024
#define CTD_RASTER_MAX_SCALE (1 << 22)
#define CTD_RASTER_OK 0
#define CTD_RASTER_EMPTY 1
#define CTD_RASTER_REFUSED 2

/* One instance (a row of the device job table), 40 bytes. */
typedef struct ctd_raster_job {
  int64_t off;       /* the record's first byte of atlas_dev; rows are w bytes apart */
  int32_t w, h;      /* the box, pixels                                            */
  int32_t bx, by;    /* the box's top-left pixel relative to the glyph's origin    */
  int32_t seg_first, seg_count; /* the glyph's rows of segs_dev                    */
  int32_t scale;     /* S, 16.16 pixels per font unit                              */
  int32_t pad_;
} ctd_raster_job;

/* The rule above for all jobs in ONE launch on `stream`.  segs_dev: n_segs rows of 6 int32; jobs_dev: n_jobs rows;
 * status_dev: n_jobs int32, every one written; atlas_dev: atlas_bytes bytes, of which only the records of the OK jobs are
 * written.  n_jobs = 0 does nothing at all.  A negative count or atlas_bytes, jobs_dev or status_dev NULL, segs_dev NULL with
 * n_segs > 0 or atlas_dev NULL with atlas_bytes > 0 is an error rc (plus ctd_last_error) and launches nothing. */
int ctd_rasterise_glyphs(const int32_t* segs_dev, int64_t n_segs, const ctd_raster_job* jobs_dev, int32_t n_jobs,
                         uint8_t* atlas_dev, int64_t atlas_bytes, int32_t* status_dev, void* stream);

/* ---- tilted text: regions and typeset in a block's own frame (added within ABI v10) ------------------------------------------ */

/* An addition to ABI v10 like the ones above: two entry points, three structs, one flag, nothing existing changes.
 * The detector gives every block an integer angle in degrees; the layout section's limit "rotated text gets an axis-aligned
 * box" is lifted here WITHOUT a new layout or fit kernel.  ctd_layout_boxes, ctd_layout_fit and ctd_layout_fit_balanced read
 * a window, a bit plane, an anchor and a balloon row: given the region plane turned into the block's frame they run as they
 * stand, and the compositor turns the frame back into the page.  Integers only, every product in 64 bits; image coordinates
 * are x right, y down.  Restated in numpy in tests/tilt_ref.py.
 *   frame   a pivot (ax, ay), an integer page pixel, and a pair (c, s) of 16.16 integers.  The HOST makes them from an
 *           integer angle t in -180 .. 180 degrees: c = rint(cos(t) 65536), s = rint(sin(t) 65536); the device sees no
 *           trigonometry.  (65536, 0) is the identity.
 *   frame -> page   for frame pixel q with d = q - pivot: PX = (ax << 16) + c dx - s dy, PY = (ay << 16) + s dx + c dy.
 *   page -> frame   for page pixel p with d = p - pivot:  u = (ax << 16) + c dx + s dy,  v = (ay << 16) - s dx + c dy.
 *           With t the block's angle, page -> frame turns the block's text lines axis-parallel.
 * Tilted region (ctd_balloon_tilt).  Job i belongs to row i of the source balloon rows; it names the block's window (wx1,
 * wy1, ww, wh, nw and word0 exactly as the balloon section lays them out), the frame, and the page's W and H.  T_b lives in
 * the SAME window and the same word layout, in a second bit buffer of the same size:
 *   T_b     frame pixel q of the window is set iff page pixel ((PX + 32768) >> 16, (PY + 32768) >> 16) lies in the window
 *           and in B_b.  The pivot need not lie in the window or in the region.
 *   row     status is the source row's.  A source row that is not CTD_BALLOON_OK is copied as it stands and the block's
 *           owned words are written 0; a window of more than min(params.max_words, CTD_BALLOON_MAX_WORDS) words (or one
 *           with x2 <= x1 or y2 <= y1) owns no words and an OK source row there comes back TOO_LARGE, all else 0; a job
 *           with |c| or |s| above 65537 or |ax| or |ay| above 2^29 has no frame: NOT_PLAIN, all else 0, words 0.  For an
 *           OK row: area, bbox, sum_x and sum_y are taken over T_b (frame coordinates), n_seed is the source row's, and
 *           flags = the eight cut bits computed on T_b, bit 8 copied from the source, bit 9 CTD_BALLOON_TILTED set.
 *           (c, s) = (65536, 0) gives the source plane and the source row plus bit 9.
 * Tilted coverage (ctd_typeset_tilted).  A layer is ctd_glyph_layer plus its frame; its placements' (x, y) are FRAME
 * coordinates.
 *   U(q)    the glyph section's F over frame pixels: the max over the layer's placements, 0 outside every glyph.
 *   F(p)    for page pixel p: x0 = u >> 16, fx = (u >> 8) & 255, y0 = v >> 16, fy = (v >> 8) & 255, Uij = U(x0 + i, y0 + j):
 *           F = ((U00 (256 - fx) + U10 fx) (256 - fy) + (U01 (256 - fx) + U11 fx) fy + 32768) >> 16.
 *   S, blend, layers, clip, row   the typeset rule, unchanged, in PAGE space: S is the disk max of F, r <= 12, the pixel is
 *           blend(blend(P, stroke, S), fill, F), layers apply in table order, clips are page rectangles, n_fill and n_stroke
 *           count the pixels written with F > 0 and S > 0.  With (65536, 0), F = U and the result is ctd_typeset_glyphs' to
 *           the byte.
 *   invalid as the glyph section, and: a layer whose frame maps the tile's coverage patch (CTD_TYPESET_TILE_W + 24 by
 *           CTD_TYPESET_TILE_H + 24 pixels) onto more than 106 frame columns or rows draws nothing.  c^2 + s^2 <=
 *           65537^2 never does: the patch's diagonal is under 103 pixels.
 * The tile table is ctd_typeset_glyphs': the caller lists, per touched tile, every placement whose rectangle, grown by one
 * pixel, turned into the page and grown by r, cut to page and clip, can meet it (glyphs.tilt_tables is the producer and
 * computes that box conservatively in integers).
 * Limits: nearest-neighbour turning is no bijection of the pixel grid, so T_b is contained in the turned B_b only up to a
 * pixel (add a pixel of inset); the window is kept, so a large angle cuts the corners of a long window, and the cut flags
 * say so; the outline is a page-space disk; glyphs are resampled, not re-rasterised, so tilted text is slightly softer. */
#define CTD_BALLOON_TILTED 512 /* flags, bit 9: the row and the plane are in the block's frame */

/* One block of a ctd_balloon_tilt call (a row of the device job table), 48 bytes. */
typedef struct ctd_tilt_job {
  int32_t win[4]; /* the block's window x1, y1, x2, y2 in page coordinates, as the balloon call's caller laid it out */
  int32_t ax, ay; /* the pivot, page coordinates                                                                       */
  int32_t c, s;   /* 16.16 cosine and sine                                                                             */
  int32_t W, H;   /* the page's size: which window sides are page edges                                                */
  int64_t word0;  /* the block's first word of bits_dev and of bits_out_dev                                            */
} ctd_tilt_job;

typedef struct ctd_tilt_params {
  int32_t max_words; /* the largest nw * wh <= CTD_BALLOON_MAX_WORDS among the call's blocks: sizes the launch's LDS */
  int32_t pad_[3];
} ctd_tilt_params;

/* The tilted-region rule for n blocks in ONE launch on `stream`, one workgroup per block: rows_out_dev[i] and the owned
 * words of bits_out_dev are job i's.  balloon_rows_dev and bits_dev may be the results of a balloon call earlier on the same
 * stream; both are read only, and the outputs must not overlap them.  `params` is read on the host during the call.
 * n = 0 launches nothing.  A negative n, max_words outside 0 .. 8192 or a missing table with n > 0 is an error rc and
 * launches nothing (bits_dev and bits_out_dev may be NULL where max_words is 0). */
int ctd_balloon_tilt(const ctd_tilt_job* jobs_dev, int32_t n, const ctd_balloon_row* balloon_rows_dev, const uint64_t* bits_dev,
                     const ctd_tilt_params* params, ctd_balloon_row* rows_out_dev, uint64_t* bits_out_dev, void* stream);

/* One tilted glyph layer (a row of the device layer table), 48 bytes: ctd_glyph_layer's fields, then the frame. */
typedef struct ctd_tilt_layer {
  int32_t page;
  int32_t clip[4];   /* x1, y1, x2, y2, exclusive, page coordinates                */
  uint8_t fill[3];   /* page channel order                                         */
  uint8_t stroke[3];
  uint8_t radius;
  uint8_t pad_;
  int32_t ax, ay;    /* the pivot, page coordinates, |ax|, |ay| <= 2^29            */
  int32_t c, s;      /* 16.16 cosine and sine                                      */
  int32_t pad2_;
} ctd_tilt_layer;

/* ctd_typeset_glyphs with tilted layers: the same page, placement, record, tile, entry and atlas tables, the same params and
 * rows, the same launch shape (one workgroup of 256 threads per row of the tile table, no cap on the placements of a tile or
 * a layer) and the same refusals. */
int ctd_typeset_tilted(const ctd_typeset_page* pages_dev, const ctd_tilt_layer* layers_dev, const ctd_glyph_place* places_dev,
                       const ctd_glyph_record* glyphs_dev, const ctd_typeset_tile* tiles_dev, const int32_t* entries_dev,
                       const uint8_t* atlas_dev, const ctd_glyph_params* params, ctd_typeset_row* rows_dev, void* stream);

/* ---- the detector tail ------------------------------------------------------ */

/* Everything `TextDetector.__call__` does after `self.net(img_in)` (reference inference.py:148-178) for a
 * whole batch of pages, driven natively: NMS + `postprocess_yolo` (inference.py:101-114), the DB
 * text-line stage (`SegDetectorRepresenter`, utils/db_utils.py:32-211: two labelling passes and contour
 * tables on the GPU, hull / min-area rectangle / unclip on the host), the mask crop + resize
 * (inference.py:164-165), `group_output` (utils/textblock.py:421-508), `refine_mask` and
 * `refine_undetected_mask` (utils/textmask.py:135-169: histograms, xor distances, candidate masks,
 * labelling, merge rounds, dilation, hole filling and the final OR on the GPU; colour / threshold picks
 * on the host).  A `ctd_tail` owns a HIP stream and its buffers; different objects may run concurrently
 * from different host threads.  All calls are synchronous: results are complete on return. */
typedef struct ctd_tail ctd_tail;

typedef struct ctd_tail_page {
  const uint8_t* img_dev; /* the page as the caller passed it: BGR u8 (im_h, im_w, 3) on the device      */
  int32_t im_h, im_w;     /* page size                                                                    */
  int32_t dw, dh;         /* right / bottom letterbox padding of the network input (inference.py:143)     */
} ctd_tail_page;

typedef struct ctd_tail_params {
  float conf_thresh, nms_thresh; /* reference inference.py:121 defaults 0.4 / 0.35                        */
  float box_thresh;              /* DB line score threshold, 0.6 (inference.py:159)                       */
  int32_t max_candidates;        /* 1000 (utils/db_utils.py:33)                                           */
  double unclip_ratio;           /* 1.5                                                                   */
  int32_t refine;                /* 0: stop after group_output                                            */
  int32_t refine_mode;           /* REFINEMASK_INPAINT 0 / REFINEMASK_ANNOTATION 1 (utils/textmask.py:13) */
  int32_t keep_undetected_mask;  /* run refine_undetected_mask (inference.py:175-176)                     */
  int32_t pad_;
} ctd_tail_params;

int ctd_tail_create(ctd_tail** out, int32_t device);
void ctd_tail_destroy(ctd_tail* t);
void* ctd_tail_stream(ctd_tail* t); /* the hipStream_t the tail's kernels run on */

/* Network outputs of a batch (all on the device): blks (B,rows,no) f32, mask_u8 (B,Hn,Wn) u8 =
 * `postprocess_mask` (fused in the engine), prob = plane 0 of lines_map (page b at prob_dev +
 * b * prob_stride floats), bitmap (B,Hn,Wn) u8 = prob > 0.3.  mask_out[b] / refined_out[b]: host arrays of
 * im_h * im_w bytes (the `mask` and `mask_refined` the reference returns; entries or the arrays may be NULL).
 * ready_event: a hipEvent_t recorded after the network on its stream (waited for on the tail's stream), or
 * NULL if the outputs are already complete.  Blocks: ctd_tail_page_counts / ctd_tail_page_fetch. */
int ctd_tail_run(ctd_tail* t, int32_t B, int32_t Hn, int32_t Wn, const float* blks_dev, int32_t rows, int32_t no,
                 const uint8_t* mask_u8_dev, const float* prob_dev, int64_t prob_stride, const uint8_t* bitmap_dev,
                 const ctd_tail_page* pages, const ctd_tail_params* prm, uint8_t* const* mask_out,
                 uint8_t* const* refined_out, void* ready_event);

/* Host wall clock of the stages of the last ctd_tail_run in ms: [0] enqueue of NMS / labelling / contour tables /
 * page masks, [1] wait for them, [2] table download + contour geometry, [3] yolo unpack + group_output,
 * [4] refine: wait for the histograms, [5] refine: wait for the xor sums, [6] refine: host decisions + enqueue,
 * [7] refine_undetected_mask, [8] final wait + copies, [9] total, [10] the part of [2] spent waiting for the
 * table download, [11]-[13] parts of [0]: NMS + buffers, labelling + contour tables, page-mask copies, [14] the part
 * of [8] spent waiting for the refine stage's kernels, [15] refine: wait for the window-local merge kernel's overflow
 * flags.  ms must hold 16 doubles. */
int ctd_tail_timings(const ctd_tail* t, double* ms);

/* Which path the refine windows of the last ctd_tail_run / ctd_tail_refine took (reference utils/textmask.py:73-132,
 * merge_mask_list per window): counts3 = [windows merged by the window-local kernel (one block per window on bit planes in
 * LDS), windows merged through the packed canvases (too large for the LDS, or re-done after an overflow), run-table
 * overflows of the window-local kernel].  Same results on every path; ABI v6. */
int ctd_tail_refine_paths(const ctd_tail* t, int32_t* counts3);

/* The DB text-line stage alone (`SegDetectorRepresenter.__call__`, reference utils/db_utils.py:40-69): boxes and
 * scores of every contour of every page, read back with ctd_tail_page_counts / ctd_tail_page_fetch. */
int ctd_tail_db_boxes(ctd_tail* t, int32_t B, int32_t Hn, int32_t Wn, const float* prob_dev, int64_t prob_stride,
                      const uint8_t* bitmap_dev, int32_t max_candidates, double unclip_ratio);

/* `refine_mask` (+ `refine_undetected_mask`) alone for given pages, page-size masks (HOST) and block boxes
 * (blk_xyxy: all pages' (x1,y1,x2,y2) concatenated, blk_counts[b] per page).  mask_out receives the masks
 * as `refine_undetected_mask` edits them in place (may be NULL). */
int ctd_tail_refine(ctd_tail* t, int32_t n_pages, const ctd_tail_page* pages, const uint8_t* const* masks_host,
                    const int32_t* blk_xyxy, const int32_t* blk_counts, int32_t refine_mode, int32_t keep_undetected_mask,
                    uint8_t* const* mask_out, uint8_t* const* refined_out);

/* Results of the last ctd_tail_run for one page: grouped blocks (ctd_blk, below) with their line and distance
 * pools, every DB contour box (n,4,2) i16 + score as `SegDetectorRepresenter.__call__` returns them, and the
 * NMS blocks (xyxy i32, class, confidence) as `postprocess_yolo` returns them.  Any output may be NULL. */
int ctd_tail_page_counts(const ctd_tail* t, int32_t page, int32_t* n_blocks, int32_t* n_lines, int32_t* n_dist,
                         int32_t* n_db_boxes, int32_t* n_yolo);
struct ctd_blk;
int ctd_tail_page_fetch(const ctd_tail* t, int32_t page, struct ctd_blk* blocks, int32_t* lines, double* dist,
                        int16_t* db_boxes, float* db_scores, int32_t* yolo_xyxy, int32_t* yolo_cls, float* yolo_conf);

/* The same grouped blocks for the WHOLE batch of the last ctd_tail_run in two calls (the per-page pair above costs the
 * Python host side two foreign calls and three allocations per page, under the interpreter lock its tail workers share):
 * counts (B,5) i32 = per page n_blocks, n_lines, n_dist, n_db_boxes, n_yolo; then the pages' ctd_blk records, line
 * quads (n,8) i32 and distance triples (m,3) f64 back to back in page order (a block's line_off / dist_off stay
 * relative to ITS page's first line / triple).  Any output may be NULL.  Pure host code. */
int ctd_tail_batch_counts(const ctd_tail* t, int32_t* counts);
int ctd_tail_batch_fetch(const ctd_tail* t, struct ctd_blk* blocks, int32_t* lines, double* dist);

/* The grouped blocks of EVERY page of the last ctd_tail_run as fixed-capacity f64 records, the unit of the multi-GPU
 * record gather (comic-text-detector_amd/dist.py): per page
 *   [n_blocks, n_lines (true counts), cap_blk, cap_line,
 *    cap_blk x 12: x1, y1, x2, y2, language, vertical, angle, font_size, n_lines, norm, vec_x, vec_y,
 *    cap_line x 8: the line quads in block order]
 * truncated (counts stay true) when a page has more blocks / lines than the capacities.  `out` holds
 * B * (4 + 12 cap_blk + 8 cap_line) doubles, zero filled where unused.  Pure host code. */
int ctd_tail_pack_records(const ctd_tail* t, int32_t cap_blk, int32_t cap_line, double* out);

/* Host threads the per-page / per-window host loops of this tail object may use (default 8; >= 1).  A node running one
 * process per GPU divides its cores between the ranks' tail workers. */
int ctd_tail_set_threads(ctd_tail* t, int32_t n);

/* ---- trace of the tail's device-made tables (ABI v9; for tests, off by default) ---------------------------------------
 * With the trace on, a tail object keeps host copies of what its refine and DB stages download from the device anyway:
 * no extra kernel, no extra device work; with it off (the default) each stage takes one untaken branch.  Per object.
 * ctd_tail_set_trace also drops what was recorded. */
int ctd_tail_set_trace(ctd_tail* t, int32_t on);

/* One refine window (reference utils/textmask.py:159-169), in the order the refine stage saw them: the windows of the
 * blocks first (pass 0), then those of `refine_undetected_mask` (pass 1).  Cleared at the start of every ctd_tail_run /
 * ctd_tail_refine. */
typedef struct ctd_trace_win {
  int32_t page, x1, y1, w, h; /* page index of the call, window in the page                                           */
  int32_t pass;               /* 0: a block's window, 1: a window of refine_undetected_mask                           */
  int32_t path;               /* merge stage: 0 window-local kernel, 1 canvases, 2 canvases after a run-table overflow */
  int32_t n_cand;             /* candidates `merge_mask_list` walks, 1..4                                             */
  uint32_t hist[4 * 256];     /* as downloaded: grey of pixels whose 3x3-eroded mask > 127 | B | G | R of the window  */
  int32_t rules[6 * 3];       /* (kind, lo, hi): kind -1 unused, 0 grey range [lo, hi], 1..3 channel B/G/R > lo       */
  int32_t cand_rule[4];       /* the candidates in merge order: rule index 0..5,                                      */
  int32_t cand_invert[4];     /*   1 = the rule's negative was closer,                                                */
  uint64_t sums[6];           /* as downloaded: sum of xor(rule's mask, predicted mask) per rule, 0 for an unused one */
  uint64_t cand_dist[4];      /*   and their xor distances                                                            */
} ctd_trace_win;

/* Windows recorded since the last run / refine; pages of the last DB stage (ctd_tail_run, ctd_tail_db_boxes) recorded. */
int ctd_tail_trace_counts(const ctd_tail* t, int32_t* n_windows, int32_t* n_db_pages);
int ctd_tail_trace_windows(const ctd_tail* t, ctd_trace_win* out); /* n_windows records */

/* An addition within ABI v10 (one new entry point, nothing existing changes, so CTD_ABI_VERSION stays): the launches of the
 * window-local merge kernel (one block per window on bit planes in LDS) in the refine stage of the last ctd_tail_run /
 * ctd_tail_refine, in launch order, recorded while the trace is on.  *n_launches = their number; out6 (may be NULL: the
 * count alone) receives per launch six values as the LAUNCHER used them, after its own clamping, not as the tuning keys
 * said: [windows (= blocks), max_words (plane words of the LDS layout), rcap (runs a labelling may have), threads per block,
 * dynamic LDS bytes, 1 if the launch was refused its LDS (nothing enqueued: its windows took the canvases) else 0]. */
int ctd_tail_trace_lds_launches(const ctd_tail* t, int32_t* n_launches, int32_t* out6);

/* The device-made contour tables of one page exactly as the host geometry (ctd_db_boxes_compact, below) received them.
 * hdr4 = [n_f, n_b, row-table entries used, overflow flag]; sizes3 = [nf, nb, nr] rows of the tables kept (all 0 on an
 * overflowed page, which takes the label-image path).  ctd_tail_trace_db_fetch fills
 *   i32: st_f (nf,5) | first_f | par_f | off_f (nf each) | st_b (nb,5) | first_b | par_b | off_b | ring_cnt (nb each) |
 *        row_lo | row_hi (nr each)                                   = 8 nf + 9 nb + 2 nr values
 *   f64: sum_f (nf) | sum_b | ring_sum (nb each)                     = nf + 2 nb values */
int ctd_tail_trace_db_sizes(const ctd_tail* t, int32_t page, int32_t* hdr4, int32_t* sizes3);
int ctd_tail_trace_db_fetch(const ctd_tail* t, int32_t page, int32_t* i32, double* f64);

/* ---- host-side input staging ---------------------------------------------------------------- */

/* Copies `n` host buffers (the caller's page images, reference inference.py:141 `img`) back to back into
 * `dst` (page-locked memory the caller then uploads with ONE asynchronous copy), on up to `threads` host
 * threads.  Pure host code; called through an FFI it runs without the caller's interpreter lock. */
int ctd_host_gather(void* dst, const void* const* srcs, const size_t* sizes, int32_t n, int32_t threads);

/* ---- host-side contour geometry of the DB text-line stage -------------- */

/* `SegDetectorRepresenter.boxes_from_bitmap` (reference utils/db_utils.py:134-211) downstream of
 * the two labelling passes: all pointers are HOST memory, no device work (scalar O(#contours)
 * double arithmetic).  prob (H,W) f32 = shrink map; lab_f / st_f / n_f = labels,
 * [x,y,w,h,area] stats and count of `ctd_ccl(bitmap, connectivity 8)`; lab_b / st_b / n_b =
 * those of `ctd_ccl(1 - bitmap, connectivity 4)`.  The contour set of
 * cv2.findContours(RETR_LIST) (db_utils.py:142) = one outer border per foreground component + one
 * hole border per background component that does not touch the frame, newest first.  Per
 * contour: get_mini_boxes (:177-194), the min-side test (:146-147), box_score_fast (:196-211),
 * unclip (:168-174), second get_mini_boxes (:154) and the rescale/clip of :158-163 with dest
 * size == bitmap size.  Outputs: boxes (n,4,2) i16 and scores (n) f32 with n = min(#contours,
 * max_candidates) in *n_out; rejected contours keep all-zero rows, like the reference's
 * preallocated arrays (:143-144).  boxes / scores must hold max_candidates entries. */
int ctd_db_boxes(const float* prob, const int32_t* lab_f, const int32_t* st_f, int32_t n_f, const int32_t* lab_b,
                 const int32_t* st_b, int32_t n_b, int32_t W, int32_t H, int32_t max_candidates,
                 double unclip_ratio, int16_t* boxes, float* scores, int32_t* n_out);

/* The same stage (`boxes_from_bitmap`, reference utils/db_utils.py:123-211) from tables compacted on the
 * DEVICE, so that no label image or probability map is downloaded (csrc/kernels_tail.hip `launch_dbc`, driven
 * by `ctd_tail_run`).  HOST memory only.  Per polarity (f = 8-connected foreground components, b =
 * 4-connected background components; labels 1..n in first-pixel order, row l-1 of every table):
 *   st_*    (n,5) [x,y,w,h,area]            first_* (n) linear index of the component's first pixel
 *   par_f   (n_f) background label left of the first pixel (0 at the page edge)
 *   par_b   (n_b) foreground label left of the first pixel if the component is a HOLE (does not touch the
 *                 page frame), else 0
 *   off_f   (n_f) first entry of the component's h rows in row_lo / row_hi (leftmost / rightmost x per row)
 *   off_b   (n_b) first entry of the h + 2 rows of a hole's border ring (the ringing component's pixels that
 *                 4-touch the hole), rows y - 1 .. y + h
 *   sum_f / sum_b  sum of the probability map over the component / the hole
 *   ring_sum / ring_cnt  sum of the probability map over the border ring / its pixel count
 * Outputs as `ctd_db_boxes`. */
int ctd_db_boxes_compact(int32_t W, int32_t H, int32_t n_f, const int32_t* st_f, const int32_t* first_f,
                         const int32_t* par_f, const int32_t* off_f, const double* sum_f, int32_t n_b,
                         const int32_t* st_b, const int32_t* first_b, const int32_t* par_b, const int32_t* off_b,
                         const double* sum_b, const double* ring_sum, const int32_t* ring_cnt, const int32_t* row_lo,
                         const int32_t* row_hi, int32_t max_candidates, double unclip_ratio, int16_t* boxes,
                         float* scores, int32_t* n_out);

/* ---- host-side block / line grouping ------------------------------------- */

/* One grouped text block: the detection fields of the reference's `TextBlock` record (reference
 * utils/textblock.py:45-56).  Lines and distances live in pools: lines (n,4,2) i32 at line_off;
 * `TextBlock.distance` at dist_off as triples (distance, c, d) with distance = |sin(arccos(c)) * d|
 * (utils/textblock.py:327-328; c and d let the caller re-evaluate that expression with its own math
 * library).  n_dist is NOT always n_lines: `split_textblk` hands every part the whole array of the
 * block it came from (:395-396). */
typedef struct ctd_blk {
  int32_t xyxy[4];
  int32_t language;      /* 0 eng, 1 ja, 2 unknown (reference utils/textblock.py:9) */
  int32_t vertical;
  int32_t angle;
  int32_t font_is_float; /* Python type of font_size in the reference: int (0), float after a merge (1) */
  double font_size;
  double vec[2];
  double norm;
  double weight;
  int32_t merged;
  int32_t line_off, n_lines;
  int32_t dist_off, n_dist;
  int32_t pad_;
} ctd_blk;

/* `group_output` (reference utils/textblock.py:421-508, sort_blklist=True) for one page.  HOST memory
 * only, no device work.  blines (n_blk,4) i32 / cls (n_blk) i32 = `postprocess_yolo`'s blocks (reference
 * inference.py:101-114); lines (n_lines,4,2) i32 = the rescaled DB boxes (inference.py:166-172);
 * mask (im_h rows of mask_pitch bytes) = the page-size u8 mask, or NULL (mask=None).
 * Outputs: blocks in reading order; capacities blk_cap >= n_blk + n_lines, line_cap >= n_blk + n_lines,
 * dist_cap >= (n_blk + n_lines) * max(1, n_lines) are always enough (CTD_ERR_NOMEM otherwise). */
int ctd_group_output(const int32_t* blines, const int32_t* cls, int32_t n_blk, const int32_t* lines, int32_t n_lines,
                     int32_t im_w, int32_t im_h, const uint8_t* mask, int32_t mask_pitch, ctd_blk* blks_out,
                     int32_t blk_cap, int32_t* lines_out, int32_t line_cap, double* dist_out, int32_t dist_cap,
                     int32_t* n_blk_out, int32_t* n_lines_out, int32_t* n_dist_out);

/* ---- host decisions of the mask refinement (exposed for tests; HOST memory, no device work) ---- */

/* np.histogram(px, bins=255) + get_topk_color(k=3, color_var=10, bin_tol=0.001) (reference
 * utils/textmask.py:16-27,61-62) from the 256-bin histogram of the selected grey pixels; writes up to 3
 * colours (left bin edges, float64) and returns how many. */
int ctd_topk_colors(const int64_t* hist256, double* colors3);
/* Threshold picked by cv2.threshold(.., THRESH_OTSU) (reference utils/textmask.py:47) from a 256-bin histogram. */
int ctd_otsu_from_hist(const int64_t* hist256);
/* Integer bounds cv2.inRange(u8, lo, hi) derives from double scalars (reference utils/textmask.py:68);
 * lb > ub on return = the empty range. */
void ctd_inrange_bounds(double lo, double hi, int32_t* lb, int32_t* ub);

/* ---- misc -------------------------------------------------------------- */
const char* ctd_last_error(void);
int32_t ctd_abi_version(void);
/* Fills name (<=255 chars) and returns the gfx arch number (950 on MI355X), or <0. */
int ctd_device_info(int32_t device, char* name, int32_t* cu_count, int64_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CTD_HIP_H */
