/*
 * fpm.h — C ABI of the MI355X-native NCC template matcher (libfpm_hip.so).
 *
 * Drop-in boundary for the reference's `TemplateMatcher` (lrm2017/Fastest_Image_Pattern_Matching,
 * include/TemplateMatcher.h:9-90, src/TemplateMatcher.cpp:1-1239).  Every entry point below names the
 * reference interface it replaces.  Plain pointers and sizes only: no torch / OpenCV / Qt types.
 *
 * Conventions
 *   - Images are 8-bit single-channel (CV_8UC1) row-major with an explicit row stride in bytes, exactly
 *     what `cv::imread(..., IMREAD_GRAYSCALE)` yields (src/MatchToolDialog.cpp:314, 341).
 *   - Host image pointers are copied to device memory inside the call; the library never retains them.
 *     (fpm_stage_sources_device / fpm_match_device take images that already lie in device memory, gray or colour.)
 *   - Every function returns an `int` status: FPM_OK (0) or a negative FPM_E_* code.  "No match" is
 *     FPM_OK with *n_results == 0, mirroring the reference's empty vector (TemplateMatcher.cpp:99-114, 398).
 *   - One context per host thread; a context is bound to one HIP device and owns one HIP stream.
 *   - fpm_last_error() returns a human-readable message for the last failing call on a context.
 */
#ifndef FPM_H_
#define FPM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPM_ABI_VERSION 11

/* status codes */
#define FPM_OK 0
#define FPM_E_INVALID_ARG (-1)   /* null pointer, non-positive size, bad stride            */
#define FPM_E_NOT_LEARNED (-2)   /* match() before learnPattern() (TemplateMatcher.cpp:99)   */
#define FPM_E_SIZE (-3)          /* source smaller than template (TemplateMatcher.cpp:107-114)*/
#define FPM_E_DEVICE (-4)        /* HIP runtime error / no gfx950 device                     */
#define FPM_E_CAPACITY (-5)      /* caller-provided result buffer too small                 */
#define FPM_E_INTERNAL (-6)

/* Result semantics (fpm_params.semantics).  The drop-in target is the Qt TemplateMatcher (src/TemplateMatcher.cpp);
 * the README's published numbers come from the MFC tool (MatchTool/MatchToolDlg.cpp), whose search differs in
 * a few places.  FPM_SEMANTICS_MFC reproduces those:
 *   - s_BlockMax blocks of 2x the template, right + bottom strips without a corner block, the last block on
 *     equal maxima, and a full-map minMaxLoc when the map holds no whole block (MatchToolDlg.h:108-210);
 *   - the angle list from the tolerance ranges when tolerance_range is set (MatchToolDlg.cpp:805-815);
 *   - corners and centre in f64, the reported angle negated and wrapped to [-180, 180], at most max_pos
 *     results (MatchToolDlg.cpp:1080-1116). */
#define FPM_SEMANTICS_QT 0
#define FPM_SEMANTICS_MFC 1

/* Search parameters: the 7 public setters of TemplateMatcher (TemplateMatcher.h:22-28) plus the hidden
 * fixed members m_bToleranceRange / m_dTolerance1..4 (TemplateMatcher.h:88-89, TemplateMatcher.cpp:38).
 * Defaults (fpm_params_default) equal the reference constructor (TemplateMatcher.cpp:28-39). */
typedef struct fpm_params {
    int32_t max_pos;          /* setMaxPositions      (default 70)   */
    int32_t min_reduce_area;  /* setMinReduceArea     (default 256)  */
    double max_overlap;       /* setMaxOverlap        (default 0.0)  */
    double score;             /* setScore             (default 0.7)  */
    double tolerance_angle;   /* setToleranceAngle    (default 0.0)  */
    int32_t use_simd;         /* setUseSIMD           (default 1): lower layers use the per-row int32 ->
                                 float fold of IM_Conv_SIMD (TemplateMatcher.cpp:487-512); 0 = TM_CCORR */
    int32_t subpixel;         /* setSubPixelEstimation(default 0)    */
    int32_t tolerance_range;  /* m_bToleranceRange    (fixed false in the Qt class; MFC toggles it,
                                 MatchToolDlg.cpp:2137): 3 refinement angles always; with FPM_SEMANTICS_MFC
                                 also the top-layer angle list from tolerance[0..3]                   */
    int32_t semantics;        /* FPM_SEMANTICS_QT (default) or FPM_SEMANTICS_MFC                       */
    double tolerance[4];      /* m_dTolerance1..4: the MFC ranges [t1, t2] and [t3, t4] (MatchToolDlg.cpp:812-815) */
    double top_angle_step;    /* extension, no reference knob: the top-layer angle step in degrees replacing the
                                 derived atan(2 / max(w, h)) of TemplateMatcher.cpp:130 when > 0 (BASELINE
                                 configs[3] "1 degree step"); 0 = the reference's step (default)     */
    int32_t stop_layer;       /* m_bStopLayer1, the MFC tool's fast mode (MatchToolDlg.cpp:936; default 0): nonzero stops
                                 the pyramid descent at layer 1 instead of layer 0 (:949-956, :1033-1037).  The layer-1
                                 ptLT is doubled in float (:951, :1035), no sub-pixel fit runs (:1013), the overlap
                                 filter's rectangle is the layer-1 template size times two (:1053-1054) and the result
                                 corners keep the level-0 size (:1080).  A coarse match: layer-1 precision for speed.
                                 With a top layer of 0 the reference indexes vecPyramid[1] out of bounds; here that
                                 case is the normal search (the stop layer is min(1, top layer))               */
    int32_t bitwise_not;      /* m_ckBitwiseNot (MatchToolDlg.cpp:788-796; default 0): nonzero searches 255 - source,
                                 the template as learned (patterns of inverted polarity).  The pyramid is built from
                                 the inverted source (:790-791).  Both switches are honoured under both
                                 semantics values, as tolerance_range is                                        */
} fpm_params;

/* One result; POD-identical to s_SingleTargetMatch (DataStructures.h:97-115): five cv::Point2d then two
 * doubles, 12 f64 in total, same order. */
typedef struct fpm_result {
    double lt_x, lt_y;        /* ptLT     */
    double rt_x, rt_y;        /* ptRT     */
    double rb_x, rb_y;        /* ptRB     */
    double lb_x, lb_y;        /* ptLB     */
    double cx, cy;            /* ptCenter */
    double angle;             /* dMatchedAngle (Qt: +dMatchAngle, TemplateMatcher.cpp:428; MFC: negated and
                                 wrapped, MatchToolDlg.cpp:1093-1099) */
    double score;             /* dMatchScore */
} fpm_result;

typedef struct fpm_ctx fpm_ctx;

/* --- lifecycle -------------------------------------------------------------------------------------- */
void fpm_params_default(fpm_params* p);                 /* TemplateMatcher::TemplateMatcher (:28-39) */
int fpm_create(int device, fpm_ctx** out);               /* TemplateMatcher::TemplateMatcher          */
int fpm_destroy(fpm_ctx* ctx);                           /* TemplateMatcher::~TemplateMatcher (:41)   */
const char* fpm_last_error(const fpm_ctx* ctx);
int fpm_abi_version(void);

/* --- parameters ------------------------------------------------------------------------------------- */
int fpm_set_params(fpm_ctx* ctx, const fpm_params* p);   /* the 7 setters (TemplateMatcher.h:22-28)   */
int fpm_get_params(const fpm_ctx* ctx, fpm_params* p);   /* the 7 getters (TemplateMatcher.h:31-37)   */

/* --- template ----------------------------------------------------------------------------------------*/
/* TemplateMatcher::learnPattern (TemplateMatcher.cpp:45-95).  Returns FPM_E_INVALID_ARG on an empty image
 * (the reference returns false, :47-49). */
int fpm_learn(fpm_ctx* ctx, const uint8_t* gray, int32_t width, int32_t height, size_t stride);
int fpm_clear_pattern(fpm_ctx* ctx);                     /* clearPattern (:439-443)                   */
int fpm_is_learned(const fpm_ctx* ctx);                  /* isPatternLearned (TemplateMatcher.h:43)   */

/* --- search ------------------------------------------------------------------------------------------*/
/* TemplateMatcher::match (TemplateMatcher.cpp:97-437).  Writes at most `cap` results (sorted by
 * descending score, exactly the reference's vector order) and the count to *n_results.
 * *seconds receives getLastExecutionTime() semantics: the pyramid->filter wall time; left unchanged when
 * there is no result (the reference returns before updating it, :398-404).  seconds may be NULL. */
int fpm_match(fpm_ctx* ctx, const uint8_t* gray, int32_t width, int32_t height, size_t stride,
              fpm_result* out, int32_t cap, int32_t* n_results, double* seconds);

/* Batched / device-resident search (no reference equivalent: the UI calls match() once per image).
 * Sources are staged into context-owned HBM once (fpm_stage_sources), then fpm_match_staged runs the
 * whole search for all staged sources layer-synchronously with one device->host copy at the end.
 * out is [count][cap_per_source]; n_results is [count]. */
int fpm_stage_sources(fpm_ctx* ctx, const uint8_t* const* grays, int32_t count, int32_t width,
                      int32_t height, size_t stride);
int fpm_match_staged(fpm_ctx* ctx, fpm_result* out, int32_t cap_per_source, int32_t* n_results);
/* fpm_match_staged split in two: _launch enqueues the whole device pass on the context's stream and returns;
 * _finish waits for it and runs the host post-processing.  Several contexts (one stream each) on one device
 * can have searches in flight at once; the staged sources must not be re-staged in between. */
int fpm_match_staged_launch(fpm_ctx* ctx);
/* out == NULL skips the host tail (sort, filters, conversion; n_results[s] = 0): for an angle-sharded context whose
 * candidate records (fpm_last_candidates) are merged elsewhere. */
int fpm_match_staged_finish(fpm_ctx* ctx, fpm_result* out, int32_t cap_per_source, int32_t* n_results);
/* The results of the last fpm_match / fpm_match_staged(_finish) call once more, laid out as fpm_match_staged's
 * output ([sources][cap_per_source], counts in n_results[sources]; one source after fpm_match).  No reference
 * equivalent (match() returns a growing std::vector): after FPM_E_CAPACITY the caller grows its buffer and fetches
 * the results already computed instead of searching again. */
int fpm_last_results(const fpm_ctx* ctx, fpm_result* out, int32_t cap_per_source, int32_t* n_results);

/* --- sources already in device memory (no reference equivalent: match() takes a host cv::Mat,
 * TemplateMatcher.cpp:97-104) -------------------------------------------------------------------------------
 * Frames a GPU decoder, a torch pipeline or a camera SDK left in HBM go straight into the context's source slab: one
 * kernel (k_stage_gray) reads the caller's device images and writes the 8-bit gray plane the search runs on; nothing
 * crosses the host.  Added without a change of FPM_ABI_VERSION: the entries are additive, no existing entry or struct
 * changes, so callers built against the earlier header are unaffected.
 *
 * Pixel formats.  Colour is converted as cv::imread(IMREAD_GRAYSCALE) converts a decoded colour file (the way the
 * reference loads its images, src/MatchToolDialog.cpp:314, 341): gray = (1868 B + 9617 G + 4899 R + 8192) >> 14 in
 * exact integers.  This is deliberately NOT cv::cvtColor's 15-bit formula
 * ((3735 B + 19235 G + 9798 R + 16384) >> 15), whose rounding differs on some pixels: a colour frame staged
 * from device memory gives the gray plane of the same frame saved as a BMP and loaded by the reference. */
#define FPM_FMT_GRAY8 0         /* 1 B per pixel                                                        */
#define FPM_FMT_BGR8 1          /* 3 B per pixel, interleaved B G R (cv::Mat CV_8UC3 order)             */
#define FPM_FMT_RGB8 2          /* 3 B per pixel, interleaved R G B                                     */
#define FPM_FMT_BGRA8 3         /* 4 B per pixel, interleaved B G R A, alpha ignored                    */
#define FPM_FMT_RGBA8 4         /* 4 B per pixel, interleaved R G B A, alpha ignored                    */
#define FPM_FMT_BGR8_PLANAR 5   /* three w x h planes, B then G then R, plane_stride bytes apart        */
#define FPM_FMT_RGB8_PLANAR 6   /* three w x h planes, R then G then B, plane_stride bytes apart        */
#define FPM_FMT_COUNT 7
/* fpm_stage_sources for `count` images in device memory.  d_images is a HOST array of `count` device pointers; every
 * image is width x height pixels of `format` with `stride` bytes between rows (>= width x bytes per pixel; any value,
 * any base alignment: views into larger buffers are fine) and, for the planar formats, plane_stride bytes between
 * planes (>= stride x height; ignored otherwise).  With fpm_params.bitwise_not set at the time of the call the kernel
 * writes 255 - gray and the search launches no k_bitwise_not; the polarity is tracked as for fpm_stage_sources, so
 * the parameter may be flipped between searches of the staged batch.
 * producer_stream is the hipStream_t on which the images were, or are being, written (NULL = the null stream).  The
 * context's own stream is non-blocking, so it is ordered neither after the caller's stream nor after the null stream
 * by itself: the call records a context-owned event on producer_stream and makes its stream wait for it.  The caller
 * needs no host synchronisation before the call; the call returns once the images have been read, so the caller may
 * overwrite them afterwards.
 * Every pointer must be device memory of the context's device, or memory that device can access (managed or
 * registered host memory): FPM_E_INVALID_ARG otherwise, as for a bad size, stride or format.  The image's byte extent
 * is also checked against its allocation -- a best-effort guard, not a guarantee: a caching allocator's blocks are
 * larger than the tensors carved from them. */
int fpm_stage_sources_device(fpm_ctx* ctx, const void* const* d_images, int32_t count, int32_t width, int32_t height,
                             size_t stride, size_t plane_stride, int32_t format, void* producer_stream);
/* fpm_match on one image in device memory: arguments as fpm_stage_sources_device (d_image is the device pointer
 * itself), results, capacity handling and *seconds as fpm_match.  The staging is the reference's deep copy of the
 * source (TemplateMatcher.cpp:104), so the clock of *seconds starts once it has landed (:117). */
int fpm_match_device(fpm_ctx* ctx, const void* d_image, int32_t width, int32_t height, size_t stride,
                     size_t plane_stride, int32_t format, void* producer_stream, fpm_result* out, int32_t cap,
                     int32_t* n_results, double* seconds);

/* --- match patches: the pixels behind the results, upright and cropped, from the sources in device memory ------------
 * The reference's tools show what a caller wants after a search: the MFC tool's "Output ROI" switch saves the matched
 * region of every result (MatchToolDlg.cpp:1114, :1223-1236), the Qt tool carries a rectangle drawn on the template onto
 * every match (MatchToolDialog.cpp:1216-1328).  A patch is getRotatedROI (TemplateMatcher.cpp:1074-1090) with a
 * caller-chosen rectangle (x, y, w, h) in template coordinates in place of its fixed 3-pixel margin: for a pose (ptLT
 * as f32, angle in degrees) on a source of src_w x src_h with centre c = ((src_w - 1) / 2.f, (src_h - 1) / 2.f),
 *     ltr = ptRotatePt2f(ptLT, c, angle * D2R);  M = getRotationMatrix2D(c, angle, 1);
 *     M[2] -= (float)(ltr.x + (float)x);  M[5] -= (float)(ltr.y + (float)y);
 *     patch = cv::warpAffine(source, M, (w, h), INTER_LINEAR, BORDER_CONSTANT 0)
 * so (-3, -3, tw + 6, th + 6) is getRotatedROI itself, bit for bit, and NULL = (0, 0, tw, th) is the template's frame.
 * The rectangle may reach outside the template; pixels outside the source are 0.  w and h are 1 .. 8192.
 *
 * Pose.  fpm_last_patches* use the pose of the vecAllResult entry each result came from -- its f32 point and its
 * dMatchAngle, as the search left them (sub-pixel estimate applied; with stop_layer the doubled layer-1 point and the
 * layer-1 angle) -- not the converted fpm_result fields: under FPM_SEMANTICS_MFC the reported angle is negated and
 * wrapped, and the trigonometry of a +- 360 differs in its last bits.
 * Pixels.  The level-0 plane the last search ran on, as it lies in the context's source slab.  With
 * fpm_params.bitwise_not in force for that search the plane is 255 - source, so the patch looks like the template,
 * not like the caller's image.
 * Additive entries: FPM_ABI_VERSION is unchanged, as for the device-memory entries above. */
typedef struct fpm_patch_rect { int32_t x, y, w, h; } fpm_patch_rect;   /* template coordinates; NULL = whole template */

/* host only, no context: the forward 2x3 matrix (row-major) of one patch, by the rule above */
int fpm_patch_matrix(int32_t src_w, int32_t src_h, float lt_x, float lt_y, double angle,
                     int32_t rect_x, int32_t rect_y, double m[6]);

/* Patches of the last search's results, in result order (fpm_match, fpm_match_device, fpm_match_staged*); source = -1:
 * the patches of all sources, concatenated in source order (the per-source counts are fpm_last_results').  One device
 * launch for all of them.  Patch i is written at out + i * patch_stride, its rows row_stride apart (w <= row_stride
 * < 2^31, patch_stride >= row_stride * h); the bytes of a row past w are left untouched.  *n_patches receives the number of
 * patches; with cap below it the call returns FPM_E_CAPACITY and writes no pixel (cap = 0 with out = NULL asks for the
 * count).  matrices (may be NULL) receives the forward matrix of every patch, [cap][6].
 * FPM_E_INVALID_ARG while a search is in flight, when no search has run since the sources were staged, when nothing is
 * staged, and for a bad rectangle; FPM_E_NOT_LEARNED without a template.  After fpm_match_staged_finish(out = NULL)
 * there are no results: *n_patches = 0, FPM_OK.  Returns when the pixels have landed in `out`. */
int fpm_last_patches(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, uint8_t* out, size_t row_stride,
                     size_t patch_stride, int32_t cap, int32_t* n_patches, double* matrices);
/* The same into device memory, for a consumer on the device (a torch model): nothing crosses the host.  d_out is
 * checked as fpm_stage_sources_device checks its images (memory the context's device can access, byte extent inside
 * its allocation); any alignment and any strides are fine (views into larger buffers).  consumer_stream is the
 * hipStream_t that owns d_out (NULL = the null stream): the call makes the context's stream wait for the work already
 * enqueued there (the buffer's allocation or clearing), enqueues the launch on the context's stream, records a
 * context-owned event and makes consumer_stream wait for it, then returns -- without a host synchronisation.  Work
 * enqueued on consumer_stream afterwards sees the patches; the host must not read d_out before synchronising with that
 * stream. */
int fpm_last_patches_device(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, void* d_out, size_t row_stride,
                            size_t patch_stride, int32_t cap, int32_t* n_patches, void* consumer_stream);
/* Patches at caller-supplied poses on the staged sources (results merged elsewhere: an angle-sharded search leaves no
 * results in any context): lt [n][2] f32 ptLT, angles [n] degrees, src_index [n] source of each pose.  Needs staged
 * sources (fpm_stage_sources*, or the source of the last fpm_match), not a search.  out, strides and matrices ([n][6])
 * as fpm_last_patches. */
int fpm_patches_at(fpm_ctx* ctx, const fpm_patch_rect* rect, const int32_t* src_index, const float* lt,
                   const double* angles, int32_t n, uint8_t* out, size_t row_stride, size_t patch_stride,
                   double* matrices);
/* Which kernel samples the patches: k_patch_warp (LDS-tiled, 4 pixels per lane; default) or k_warp, the parity
 * operator of fpm_op_warp_affine, over the same job list (the comparison, and the fallback).  Both give the same
 * bytes.  Takes effect at the next patch call. */
#define FPM_PATCH_FORM_TILED 0
#define FPM_PATCH_FORM_WARP 1
int fpm_set_patch_form(fpm_ctx* ctx, int32_t form);

/* --- patch comparison: every hit against the learned template, on the device ---------------------------------------
 * Locate, rectify, inspect: what a caller does with a patch is compare it with the template it was found by.  These
 * entries do that where the pixels are -- level 0 of the sources and of the template are both in device memory after a
 * search -- and return a few numbers per hit; no patch is written.
 * Rectangle.  (x, y, w, h) in template coordinates, and unlike a patch rectangle inside the template: 0 <= x, 0 <= y,
 * x + w <= tw, y + h <= th, 1 <= w * h <= 2^22; NULL = the whole template.  Anything else is FPM_E_INVALID_ARG.
 * Pixels.  I(u, v) is the pixel (u, v) of the patch fpm_last_patches gives for that rectangle and pose (same matrix,
 * same fixed-point bilinear arithmetic, border 0, the inverted plane under bitwise_not); T(u, v) is template level 0
 * at (x + u, y + v).
 * Sums, exact integers: n = w * h, sum_i = sum I, sum_ii = sum I^2, sum_t = sum T, sum_tt = sum T^2, sum_it = sum I T.
 * With Di = n sum_ii - sum_i^2, Dt = n sum_tt - sum_t^2, N = n sum_it - sum_i sum_t (exact in int64 under the area cap):
 *     zncc = (double)N / (sqrt((double)Di) * sqrt((double)Dt)), or 0.0 when Di == 0 or Dt == 0.
 * Normalisation (FPM_COMPARE_NORMALIZE) fits the hit's gain and offset to the template's, so that a change of lighting
 * is no deviation:
 *     gain = sqrt((double)Dt) / sqrt((double)Di), or 1.0 when Di == 0
 *     offset = ((double)sum_t - gain * (double)sum_i) / (double)n
 *     LUT[v] = (uint8) min(255, max(0, rint(gain * (double)v + offset))), v = 0 .. 255
 * in f64, the product and the sum rounded separately (no fused multiply-add), rint in the default rounding mode (ties
 * to even).  Without the flag LUT is the identity, gain = 1, offset = 0.
 * Deviations.  d(u, v) = |LUT[I(u, v)] - T(u, v)|: sum_abs = sum d, max_abs = max d, n_over = the number of pixels with
 * d > threshold (threshold 0 .. 255), (x0, y0, x1, y1) = the inclusive bounding box of those pixels in rectangle
 * coordinates; with n_over == 0: x0 = w, y0 = h, x1 = y1 = -1.
 * Difference image (diff, may be NULL): d as u8, one w x h image per hit, image i at diff + i * patch_stride, rows
 * row_stride apart (the rules of fpm_last_patches; the bytes of a row past w are left untouched).
 * A call without the flag is one launch of k_patch_compare; with it two, with a copy of the sums to the host between
 * them, where the tables are built.  Additive entries: FPM_ABI_VERSION is unchanged. */
typedef struct fpm_compare_stats {
    int64_t n, sum_i, sum_ii, sum_t, sum_tt, sum_it, sum_abs;
    int32_t n_over, max_abs, x0, y0, x1, y1;
    double zncc, gain, offset;
} fpm_compare_stats;
#define FPM_COMPARE_NORMALIZE 1   /* flags */

/* The hits of the last search, in result order; source, cap, *n and every state rule as fpm_last_patches (source = -1:
 * all sources in source order; cap below the count: FPM_E_CAPACITY with the count in *n, nothing written; cap = 0
 * with out = NULL asks for the count).  Returns when out (and diff) are filled. */
int fpm_last_compare(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, int32_t threshold, int32_t flags,
                     fpm_compare_stats* out, int32_t cap, int32_t* n, uint8_t* diff, size_t row_stride,
                     size_t patch_stride);
/* The same at caller-supplied poses on the staged sources; poses as fpm_patches_at. */
int fpm_compare_at(fpm_ctx* ctx, const fpm_patch_rect* rect, const int32_t* src_index, const float* lt,
                   const double* angles, int32_t n_poses, int32_t threshold, int32_t flags, fpm_compare_stats* out,
                   uint8_t* diff, size_t row_stride, size_t patch_stride);
/* host only, no context: what the engine derives from the sums by the rules above.  zncc, gain and offset must not be
 * NULL; lut may be.  normalize = 0: gain 1, offset 0, the identity table.  FPM_E_INVALID_ARG for n outside 1 .. 2^22
 * and for sums that are those of no n bytes (negative, above 255 n or 65025 n, or Di < 0 or Dt < 0). */
int fpm_compare_derive(int64_t n, int64_t sum_i, int64_t sum_ii, int64_t sum_t, int64_t sum_tt, int64_t sum_it,
                       int32_t normalize, double* zncc, double* gain, double* offset, uint8_t lut[256]);

/* --- learning on the device: the template from a device image, a pose or a hit (no reference equivalent: learnPattern
 * takes a host cv::Mat, TemplateMatcher.cpp:45) ---------------------------------------------------------------------
 * fpm_learn uploads the image, builds the pyramid on the device, copies every level back and walks it on the host.
 * These entries learn where the pixels are: level 0 of the template slab is written by a kernel (k_stage_gray for an
 * image, k_patch_warp for a pose), the pyramid kernels build the levels, one launch of k_tmpl_prep makes what the
 * search needs of them (the i8 operand, the per-row sums, the exact sum of T and of T^2 per level), and the host derives
 * the level statistics from those sums after one stream synchronisation.  The learned template equals what fpm_learn
 * learns from the same pixels in every byte and every double (fpm_template_info, fpm_template_level,
 * fpm_template_operands).
 * State after a successful call: the template is learned, and the poses of the last search are dropped
 * (fpm_last_patches*, fpm_last_compare and fpm_learn_hit return FPM_E_INVALID_ARG until the next search).  Unlike
 * fpm_learn the entries KEEP the staged sources when the source slab's layout still fits the new template -- its top
 * layer (getTopLayer at the current min_reduce_area) equals the one the sources were staged for and the size rules of
 * fpm_match still hold -- so fpm_match_staged*, fpm_patches_at and fpm_compare_at work without restaging: teach from
 * frame 0 of a batch, search the batch, one upload.  Otherwise the sources are invalidated as fpm_learn invalidates
 * them.
 * Errors.  FPM_E_INVALID_ARG while a search is in flight and for what the argument and state rules reject (sides above
 * 65536 and pyramids of more than 16 levels included); such a call leaves the context untouched.  A failure once the
 * template slab has been touched (a device error) leaves the context as after fpm_clear_pattern, not half-learned.
 * Additive entries: FPM_ABI_VERSION is unchanged, as for the device-memory entries above. */
/* learnPattern on an image in device memory; arguments as fpm_match_device's image.  fpm_params.bitwise_not is not looked
 * at: the template is learned as given */
int fpm_learn_device(fpm_ctx* ctx, const void* d_image, int32_t width, int32_t height, size_t stride,
                     size_t plane_stride, int32_t format, void* producer_stream);
/* learnPattern on the patch fpm_patches_at gives for (rect, source, lt, angle): sampled by k_patch_warp (k_warp under
 * FPM_PATCH_FORM_WARP) straight into level 0 of the template slab.  rect NULL = the frame of the template learned now
 * (FPM_E_NOT_LEARNED without one).  Rectangle, pose and state rules as fpm_patches_at: staged sources are needed, and
 * with fpm_params.bitwise_not in force for them the plane sampled is 255 - source, the plane the search correlates with */
int fpm_learn_at(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, float lt_x, float lt_y, double angle);
/* the same at the raw pose of result `index` of `source` of the last search (the pose fpm_last_patches uses); state rules
 * as fpm_last_patches, FPM_E_INVALID_ARG for an index outside the source's results */
int fpm_learn_hit(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, int32_t index);
/* host only, no context: what learning derives for a level from its pixel count and the exact sums of its pixels and of
 * their squares -- cv::meanStdDev's mean, then norm, inv_area and vecResultEqual1 by TemplateMatcher.cpp:66-91, in
 * fpm_learn's own f64 expressions and order.  FPM_E_INVALID_ARG for n outside 1 .. 2^32 and for sums that are those of
 * no n bytes (negative, above 255 n or 65025 n, or n sum_sq < sum^2) */
int fpm_learn_derive(int64_t n, int64_t sum, int64_t sum_sq, double* mean, double* norm, double* inv_area,
                     int32_t* equal1);
/* introspection for parity tests: the whole i8 operand slab (T ^ 0x80 per level, zero padded, the 256 bytes of slack
 * behind the last level included) and the row-sum array as they lie in device memory.  *t8_bytes and *tsum_count always
 * receive the sizes; t8 and tsum (each may be NULL) must hold that many bytes / entries */
int fpm_template_operands(const fpm_ctx* ctx, int8_t* t8, size_t* t8_bytes, int32_t* tsum, size_t* tsum_count);

/* --- variation model: per-pixel tolerances trained from hits, inspection on the device (no reference equivalent) -----
 * fpm_last_compare holds every pixel of a hit against one taught image with one threshold; an edge pixel of a good part
 * moves by tens of gray levels under a quarter-pixel pose residue while a flat one moves by two.  A variation model is
 * trained from many good samples instead: it keeps a per-pixel mean and a per-pixel spread, and a pixel is a defect only
 * where it leaves mean +- max(a, k sigma).  Everything it needs is resident after a staged search (level 0 of every
 * source, the raw poses, the template), so training and inspection write no crop.
 * Model.  One per context: a rectangle (x, y, w, h) in template coordinates under the comparison's rules (inside the
 * template, 1 <= w * h <= 2^22, NULL = the whole template), a sample count n, and two w x h planes of uint32 in device
 * memory, S = sum v and Q = sum v^2 over the samples.  v is the pixel fpm_last_patches gives for that rectangle and
 * pose (same matrix, same fixed-point bilinear arithmetic, border 0, the inverted plane under bitwise_not); with
 * FPM_COMPARE_NORMALIZE v is LUT[that pixel], the hit's table built exactly as fpm_last_compare builds it (the sums
 * launch against the template, fpm_compare_derive's rule, the tables to the device).  n <= 65535, so Q <= 65535 * 65025
 * < 2^32: a training call that would exceed it returns FPM_E_CAPACITY.  A training call that fails adds nothing.
 * The first training call after a clear fixes the rectangle; a later one with another rectangle is FPM_E_INVALID_ARG.
 * The model is dropped by fpm_model_clear, by every learn entry but fpm_model_learn (fpm_learn, fpm_learn_device,
 * fpm_learn_at, fpm_learn_hit), by fpm_clear_pattern and by fpm_destroy.  Restaging sources keeps it: training over
 * several batches is the point.
 * Derived per pixel, in exact integers (one function, run by the device and by fpm_model_derive), for an absolute
 * threshold a = 0 .. 255 and a sigma multiple kq = 0 .. 255 in sixteenths:
 *     V = n Q - S^2                                   (<= 2^46)
 *     B = max(n a, isqrt((kq^2 V) >> 8))              (isqrt = the exact floor square root; the product is < 2^62)
 *     mean = (2 S + n) / (2 n)                        (integer division: the mean rounded half up)
 *     lo = max(0, ceil((S - B) / n)),  hi = min(255, floor((S + B) / n))
 * B / n = max(a, (kq / 16) sigma) with sigma = sqrt(V) / n.  A value u = 0 .. 255 is inside iff |n u - S| <= B, which is
 * iff lo <= u <= hi; lo = hi + 1 is the empty interval and can occur (n = 2, S = 21, a = 0, kq = 0: lo 11, hi 10).
 * Excess: e(u) = lo - u for u < lo (low), else u - hi for u > hi (high), else 0.
 * Inspection record per hit: n = w * h; sum_excess = sum e; n_low, n_high = the pixels below and above their interval;
 * max_excess = max e; (x0, y0, x1, y1) = the inclusive bounding box of the pixels with e > 0 in rectangle coordinates,
 * x0 = w, y0 = h, x1 = y1 = -1 when there is none; gain and offset of the hit's table (1 and 0 without the flag).  u is
 * v as above, so with FPM_COMPARE_NORMALIZE a change of lighting is no excess.
 * Excess image (img, may be NULL): e as u8, one w x h image per hit, image i at img + i * patch_stride, rows row_stride
 * apart (the rules of fpm_last_patches; the bytes of a row past w are left untouched).
 * Launches.  Training: k_model_accum, one per call.  The u8 planes mean / lo / hi: k_model_prepare, once per (a, kq,
 * state of the sums); the inspection entries and fpm_model_images prepare only when that key changed.  Inspection:
 * k_model_inspect, one per call.  With FPM_COMPARE_NORMALIZE the sums launch of k_patch_compare and a copy of the sums
 * to the host come first, as in fpm_last_compare.
 * State.  While a search is in flight every entry below is FPM_E_INVALID_ARG except fpm_model_info,
 * fpm_model_set_chunk, fpm_model_derive and fpm_model_profile.  Additive entries: FPM_ABI_VERSION is unchanged. */
typedef struct fpm_inspect_stats {
    int64_t n, sum_excess;
    int32_t n_low, n_high, max_excess, x0, y0, x1, y1;
    double gain, offset;
} fpm_inspect_stats;

int fpm_model_clear(fpm_ctx* ctx);
/* Training's work split: a workgroup of k_model_accum takes one 64 x 16 tile and `jobs` consecutive samples.  0 (the
 * default) lets the engine choose: all samples of a call when the rectangle's tiles alone fill the device (one owner
 * per pixel, plain adds), else as many chunks as bring the grid to 12 workgroups per compute unit, of at least 4 samples
 * each (integer atomic adds).
 * The sums are the same integers for every value; the entry is there for parity tests and measurements, as seg_chunks
 * is in fpm_op_pyr_down2. */
int fpm_model_set_chunk(fpm_ctx* ctx, int32_t jobs);
/* Adds the hits of the last search (source = -1: of all sources) to the model; *n_added receives how many were added
 * (0 when the call fails).  State and source rules as fpm_last_compare; rect as described above. */
int fpm_model_train_last(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, int32_t flags, int32_t* n_added);
/* The same at caller-supplied poses on the staged sources; poses and state rules as fpm_compare_at. */
int fpm_model_train_at(fpm_ctx* ctx, const fpm_patch_rect* rect, const int32_t* src_index, const float* lt,
                       const double* angles, int32_t n_poses, int32_t flags);
/* *n = the sample count, 0 = no model (rect, may be NULL, then receives zeros) */
int fpm_model_info(const fpm_ctx* ctx, int32_t* n, fpm_patch_rect* rect);
/* S and Q to the host, dense w x h each (each may be NULL).  FPM_E_INVALID_ARG without a model, as for every entry below. */
int fpm_model_sums(fpm_ctx* ctx, uint32_t* sum, uint32_t* sum_sq);
/* mean, lo and hi for (a, kq) to the host as w x h images with rows row_stride (>= w) apart; each may be NULL */
int fpm_model_images(fpm_ctx* ctx, int32_t a, int32_t kq, uint8_t* mean, uint8_t* lo, uint8_t* hi, size_t row_stride);
/* The hits of the last search against the model, over the model's rectangle; source, cap, *n, state rules and the image
 * buffer as fpm_last_compare's.  flags: FPM_COMPARE_NORMALIZE or 0.  Returns when out (and img) are filled. */
int fpm_last_inspect(fpm_ctx* ctx, int32_t source, int32_t a, int32_t kq, int32_t flags, fpm_inspect_stats* out,
                     int32_t cap, int32_t* n, uint8_t* img, size_t row_stride, size_t patch_stride);
/* The same at caller-supplied poses on the staged sources; poses as fpm_patches_at. */
int fpm_inspect_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                   int32_t a, int32_t kq, int32_t flags, fpm_inspect_stats* out, uint8_t* img, size_t row_stride,
                   size_t patch_stride);
/* Learns the model's mean image as the new template through the device learn's path: k_model_prepare writes it into
 * level 0 of the template slab, then everything fpm_learn_at does after sampling.  State afterwards as after
 * fpm_learn_at (staged sources kept when the top layer is unchanged, the last poses dropped), except that the model
 * survives, with the rectangle (0, 0, w, h) -- the new template's frame: a hit of the new template and that rectangle
 * sample the region the model was trained on. */
int fpm_model_learn(fpm_ctx* ctx);
/* host only, no context: mean, lo and hi of one pixel by the rule above.  FPM_E_INVALID_ARG for n outside 1 .. 65535, a
 * or kq outside 0 .. 255, and sums that are those of no n bytes: sum outside 0 .. 255 n, sum_sq outside sum .. 255 sum
 * or of other parity than sum (v <= v^2 <= 255 v and v^2 = v mod 2 for every byte), or n sum_sq < sum^2 */
int fpm_model_derive(int32_t n, int64_t sum, int64_t sum_sq, int32_t a, int32_t kq, int32_t* mean, int32_t* lo,
                     int32_t* hi);
/* Timing of the model's kernels, collected under fpm_profile_enable and cleared by fpm_profile_reset like the FPM_K_*
 * counters (there is no FPM_K_* index for them; the normalising sums launch counts under FPM_K_COMPARE).  which: 0 =
 * k_model_accum (bytes = source pixels read + plane bytes written), 1 = k_model_prepare (plane bytes in and out), 2 =
 * k_model_inspect (source pixels + lo and hi read + excess pixels written). */
int fpm_model_profile(const fpm_ctx* ctx, int32_t which, double* ms, int64_t* launches, int64_t* bytes);

/* --- pose alignment: every hit polished by least squares against the template, on the device (no reference equivalent)
 * The pose the entries above sample at is what the search left: the layer-0 integer peak, or the 3 x 3 x 3 quadratic fit
 * of NCC scores, on an angle grid of atan(2 / max(w, h)).  A quarter-pixel residue moves an edge pixel by tens of gray
 * levels.  These entries run Gauss-Newton iterations of the pose (shift and rotation) against the template where the
 * pixels are; per iteration one launch of k_patch_align reduces every hit to eleven exact integers, the host solves a
 * 3 x 3 system per hit in f64, and no crop is written.  ("Refine" names the pyramid descent here, fpm_op_refine; this
 * is "align".)
 * Rectangle.  (x, y, w, h) in template coordinates and inside the template, as a comparison rectangle, under two
 * narrower caps: 1 <= w * h <= 2^20 and w, h <= 4096.  NULL = the whole template; a template beyond the caps with NULL
 * is FPM_E_INVALID_ARG.  The caps bound every sum: |Tx|, |Ty|, |r| <= 255, |X| <= w - 1 and |Y| <= h - 1 give |Jt| < 255
 * (w + h), and under both caps w + h <= 4096 + 256 = 4352, so the largest sum, h_tt = sum Jt^2, stays below n * 255^2 *
 * (w + h)^2 <= 2^20 * 65025 * 4352^2 < 2^62; every other sum is smaller.  Src7's 762 x 521 template fits.
 * Pixels.  I(u, v) is the pixel (u, v) of the patch fpm_last_patches gives for that rectangle and pose (same matrix,
 * same fixed-point bilinear arithmetic, border 0, the inverted plane under bitwise_not); T(u, v) is template level 0
 * at (x + u, y + v).  With FPM_COMPARE_NORMALIZE I is LUT[I], the hit's table built exactly as fpm_last_compare builds
 * it (the sums launch of k_patch_compare, fpm_compare_derive's rule, the tables to the device) -- built ONCE, at the
 * start pose, and reused by every iteration.
 * Pixels whose footprint leaves the source are 0, as in a patch, and are NOT masked: a hit cut by the frame's edge is
 * pulled towards the frame (its residual there is -T), so its aligned pose is biased.
 * Gradients, exact integers: Tx = T(u + 1, v) - T(u - 1, v), Ty = T(u, v + 1) - T(u, v - 1) -- twice the derivative, in
 * -255 .. 255 -- read from the whole template, not only from the rectangle.  A pixel is USED iff 1 <= x + u <= tw - 2 and
 * 1 <= y + v <= th - 2.
 * Per used pixel, with X = 2 u - (w - 1), Y = 2 v - (h - 1) (doubled coordinates about the rectangle's centre, integers):
 *     Jt = X Ty - Y Tx,    r = I - T.
 * Sums over the used pixels (fpm_align_sums, exact, int64):
 *     n_used, h_xx = sum Tx^2, h_xy = sum Tx Ty, h_yy = sum Ty^2, h_xt = sum Tx Jt, h_yt = sum Ty Jt, h_tt = sum Jt^2,
 *     g_x = sum Tx r, g_y = sum Ty r, g_t = sum Jt r, ssd = sum r^2.
 * Solve (fpm_align_solve).  H q = -g with H = [[h_xx, h_xy, h_xt], [h_xy, h_yy, h_yt], [h_xt, h_yt, h_tt]], every sum
 * converted to f64 first, by the symmetric adjugate in this order (no fused multiply-add):
 *     c00 = h_yy h_tt - h_yt h_yt   c01 = h_xt h_yt - h_xy h_tt   c02 = h_xy h_yt - h_xt h_yy
 *     c11 = h_xx h_tt - h_xt h_xt   c12 = h_xy h_xt - h_xx h_yt   c22 = h_xx h_yy - h_xy h_xy
 *     det = (h_xx c00 + h_xy c01) + h_xt c02
 *     q0 = -(((c00 g_x + c01 g_y) + c02 g_t) / det), q1 = -(((c01 g_x + c11 g_y) + c12 g_t) / det),
 *     q2 = -(((c02 g_x + c12 g_y) + c22 g_t) / det)
 *     du = 2 q0, dv = 2 q1 (patch pixels), dphi = 4 q2 (radians).
 * The step is SINGULAR when n_used < 3, det <= 0 or det, du, dv or dphi is not finite; it is then (0, 0, 0).
 * Update (fpm_align_update), all in f64 with glibc cos and sin.  A = the inverted patch matrix of the current pose
 * (fpm_patch_matrix, inverted as cv::warpAffine inverts it), cx = (w - 1) / 2, cy = (h - 1) / 2.  The new pose is the
 * one whose patch map is A o D, D = the rotation by dphi about the rectangle's centre followed by the shift (du, dv):
 *     angle' = angle + dphi * 180 / pi
 *     P = A (cx + du, cy + dv, 1)
 *     lt' = P - L' (x + cx, y + cy),   L' = [[cos a', -sin a'], [sin a', cos a']],  a' = angle' * pi / 180.
 * It is evaluated as a difference from the current pose, with A (cx, cy, 1) = lt + L (x + cx, y + cy) (L as L', of
 * the current angle) taken as exact, so that a zero step returns the pose bit for bit:
 *     lt' = (float) (lt + ((A00 du + A01 dv) + ((c - c') kx - (s - s') ky),  (A10 du + A11 dv) + ((s - s') kx + (c - c') ky)))
 * with kx = x + cx, ky = y + cy, c = cos a, s = sin a, c' = cos a', s' = sin a'; the sum is rounded to f32 once.
 * Iteration (fpm_align_at / fpm_align_last; iters 1 .. 8; 0 < max_step <= 1024 source pixels, 2.0 is a good value).
 * Evaluation 0 is at the start pose.  After evaluation k < iters the host solves and updates every live hit.  A hit
 * FREEZES when its step is singular (FPM_ALIGN_SINGULAR), or when the step would move a corner of the rectangle by more
 * than max_step -- for a corner at (ex, ey) from the centre, with c = cos dphi, s = sin dphi,
 *     mx = ((c ex - s ey) - ex) + du,  my = ((s ex + c ey) - ey) + dv,  mx mx + my my > max_step max_step
 * -- or the new pose would leave the samplers' range of 2^20 pixels (both FPM_ALIGN_STEP_CLAMPED).  A frozen hit takes
 * no further step; it stays in the later launches at its last pose.  Evaluation `iters` is at the last pose: iters + 1
 * launches per call, one copy of the records to the host after each.  The pose returned is the evaluated pose with the
 * lowest ssd, the earliest on ties (FPM_ALIGN_KEPT_START when that is evaluation 0): ssd <= ssd_start always.
 * evals = the poses evaluated for the hit (steps taken + 1), best_eval = the index of the returned one.
 * Launches.  k_patch_align, never part of a search or of a captured graph; one clearing of the records ahead of each.
 * With FPM_COMPARE_NORMALIZE the sums launch of k_patch_compare and a copy of the sums to the host come first.
 * Errors.  Rectangle, iters, max_step or flags out of range: FPM_E_INVALID_ARG, nothing launched.  A call that fails
 * leaves the context untouched.  Additive entries: FPM_ABI_VERSION is unchanged. */
typedef struct fpm_align_sums {
    int64_t n_used, h_xx, h_xy, h_yy, h_xt, h_yt, h_tt, g_x, g_y, g_t, ssd;
} fpm_align_sums;
typedef struct fpm_align_result {
    float lt_x, lt_y;          /* the aligned pose: ptLT as f32 */
    double angle;              /* and its angle in degrees */
    int64_t ssd_start, ssd;    /* sum r^2 at the start pose and at the returned one */
    int64_t n_used;
    int32_t evals, best_eval;
    int32_t flags;             /* FPM_ALIGN_SINGULAR | FPM_ALIGN_STEP_CLAMPED | FPM_ALIGN_KEPT_START */
    int32_t reserved;          /* 0 */
} fpm_align_result;
#define FPM_ALIGN_SINGULAR 1       /* result flags */
#define FPM_ALIGN_STEP_CLAMPED 2
#define FPM_ALIGN_KEPT_START 4
#define FPM_ALIGN_ADOPT 2          /* call flag of fpm_align_last, beside FPM_COMPARE_NORMALIZE */

/* One launch at caller-supplied poses on the staged sources: the kernel's records.  Poses and state rules as
 * fpm_compare_at; flags: FPM_COMPARE_NORMALIZE or 0. */
int fpm_align_sums_at(fpm_ctx* ctx, const fpm_patch_rect* rect, const int32_t* src_index, const float* lt,
                      const double* angles, int32_t n_poses, int32_t flags, fpm_align_sums* out);
/* The iteration from caller-supplied poses; poses and state rules as fpm_compare_at; flags: FPM_COMPARE_NORMALIZE or 0. */
int fpm_align_at(fpm_ctx* ctx, const fpm_patch_rect* rect, const int32_t* src_index, const float* lt,
                 const double* angles, int32_t n_poses, int32_t iters, double max_step, int32_t flags,
                 fpm_align_result* out);
/* The iteration from the poses of the last search's hits, in result order; source, cap, *n and every state rule as
 * fpm_last_compare.  With FPM_ALIGN_ADOPT the aligned poses replace the context's last poses: fpm_last_patches*,
 * fpm_last_compare, fpm_last_inspect, fpm_model_train_last, fpm_learn_hit and a later fpm_align_last sample at them
 * until the next search.  fpm_last_results and fpm_last_candidates are never changed.  Without the flag nothing in the
 * context changes. */
int fpm_align_last(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, int32_t iters, double max_step,
                   int32_t flags, fpm_align_result* out, int32_t cap, int32_t* n);
/* host only, no context: the step of one record by the rule above.  Returns 0, or 1 for a singular step (then du = dv =
 * dphi = 0), or FPM_E_INVALID_ARG for a null argument. */
int fpm_align_solve(const fpm_align_sums* sums, double* du, double* dv, double* dphi);
/* host only, no context: the pose after a step by the rule above; rect must not be NULL (only x, y, w, h >= 1 matter). */
int fpm_align_update(int32_t src_w, int32_t src_h, const fpm_patch_rect* rect, float lt_x, float lt_y, double angle,
                     double du, double dv, double dphi, float* lt2_x, float* lt2_y, double* angle2);
/* Timing of k_patch_align, collected under fpm_profile_enable and cleared by fpm_profile_reset as fpm_model_profile's
 * (no FPM_K_* index: FPM_K_COUNT is unchanged; the normalising sums launch counts under FPM_K_COMPARE).  bytes =
 * source pixels read + template pixels read. */
int fpm_align_profile(const fpm_ctx* ctx, double* ms, int64_t* launches, int64_t* bytes);

/* --- defect blobs: connected components of an excess image (no reference equivalent) ----------------------------------
 * fpm_last_inspect gives per hit two counts, a sum and ONE box around every pixel that left its interval: forty isolated
 * one-pixel excesses and one 40-pixel scratch are the same record, two defects in opposite corners one box the size of
 * the part.  The step after it segments the excess image into connected regions, drops those below a minimum area and
 * reports each with its area, box, centroid sums and strength.  This block states that contract and gives its host
 * entry, fpm_blobs_host, which takes the images fpm_last_inspect / fpm_inspect_at write (or any u8 images).  The entries
 * that label where the excess images lie, on the device, follow it ("defect blobs on the device").
 * Foreground.  The input is a w x h image of u8 values e(u, v) and a level t = 0 .. 254; pixel (u, v) is foreground iff
 * e(u, v) > t.
 * Connectivity.  4 (edge neighbours) or 8 (edge and corner neighbours); a component is a maximal connected set of
 * foreground pixels.
 * Name.  A component's seed is the smallest row-major index v * w + u of its pixels (w * h <= 2^22: an int32).  It is
 * unique per component and independent of any schedule.  In the label image a pixel carries seed + 1, background 0.
 * Record: fpm_blob, 56 bytes, no padding, exact integers.  Per-image summary: fpm_blob_summary, 32 bytes, no padding.
 * Filter, order, capacity.  min_area >= 1; cap_per_hit = 1 .. 65536 with n * cap_per_hit <= 2^22.  A component
 * QUALIFIES when area >= min_area.  Records come image by image in call order, those of image i from
 * out[i * cap_per_hit] on, in ascending seed; the records behind the image's n_returned are zero-filled.  When n_blobs
 * <= cap_per_hit the output is fully determined.  When it is larger the call is still FPM_OK, the image carries
 * FPM_BLOBS_TRUNCATED, n_blobs is the true count, and cap_per_hit records come back, each the exact record of a distinct
 * qualifying component, in ascending seed: fpm_blobs_host returns the first cap_per_hit by seed (an entry that draws
 * its record slots in parallel may return any cap_per_hit of them).  Components below min_area use no capacity.
 * Label image (labels, may be NULL): dense int32 [n][h][w], seed + 1 of the pixel's component for every foreground
 * pixel, filtered or not, 0 elsewhere.
 * Errors.  connectivity other than 4 or 8, level outside 0 .. 254, min_area < 1, cap_per_hit outside its range, a null
 * image, summary or record pointer, n outside 1 .. 65535, w or h < 1, w * h > 2^22, stride < w: FPM_E_INVALID_ARG,
 * nothing written.  Additive entry: FPM_ABI_VERSION is unchanged. */
typedef struct fpm_blob {
    int32_t hit;                 /* index of the image / hit within the call                         */
    int32_t seed;                /* smallest row-major index v * w + u of the component               */
    int32_t area;                /* pixels                                                           */
    int32_t x0, y0, x1, y1;      /* inclusive box, image (rectangle) coordinates                     */
    int32_t max_value;           /* max e over the component                                         */
    int64_t sum_value;           /* sum e                                                            */
    int64_t sum_x, sum_y;        /* sum u, sum v: the centroid is (sum_x / area, sum_y / area)       */
} fpm_blob;
typedef struct fpm_blob_summary {
    int64_t fg_pixels;           /* foreground pixels                                                */
    int32_t n_components;        /* all components, before the area filter                           */
    int32_t n_blobs;             /* components with area >= min_area (the true count, may exceed cap) */
    int32_t n_returned;          /* min(n_blobs, cap_per_hit)                                        */
    int32_t largest_area;        /* over all components, 0 when there is none                        */
    int32_t flags;               /* FPM_BLOBS_TRUNCATED when n_blobs > cap_per_hit                    */
    int32_t reserved;            /* 0 */
} fpm_blob_summary;
#define FPM_BLOBS_TRUNCATED 1
#define FPM_BLOBS_MAX_CAP 65536          /* cap_per_hit */
#define FPM_BLOBS_MAX_SLOTS (1 << 22)    /* n * cap_per_hit */

/* host only, no context: n u8 images of one size (image i at images + i * stride * h, rows stride >= w apart), labelled
 * by a two-pass union-find, then filtered, sorted by seed and cut to cap_per_hit. */
int fpm_blobs_host(const uint8_t* images, int32_t n, int32_t w, int32_t h, size_t stride, int32_t level,
                   int32_t connectivity, int32_t min_area, fpm_blob_summary* summary, fpm_blob* out,
                   int32_t cap_per_hit, int32_t* labels);

/* --- defect blobs on the device: the hits cut into blobs where their excess images lie (no reference equivalent) -------
 * The contract is "defect blobs" above, unchanged: foreground e > level, connectivity 4 or 8, a component named by its
 * seed, fpm_blob and fpm_blob_summary, filter, order, capacity and FPM_BLOBS_TRUNCATED.  Of a truncated image these
 * entries return cap_per_hit exact records of distinct qualifying components in ascending seed, not necessarily the
 * first by seed (the record slots are drawn in parallel); everything else is fully determined.
 * fpm_last_blobs / fpm_blobs_at run the inspection of fpm_last_inspect / fpm_inspect_at with its excess images written to
 * the context's pitched patch buffer, label them there and bring back the records: no image crosses the host.  source,
 * cap (hits), *n, a, kq, flags, the state and model rules and every error are those of fpm_last_inspect /
 * fpm_inspect_at (cap = 0 with out = NULL asks for the count; a cap below the count is FPM_E_CAPACITY with nothing
 * written); level, connectivity, min_area and cap_per_hit are checked as fpm_blobs_host checks them, with the actual
 * number of hits.  summary holds one entry per hit, out cap_per_hit records per hit; stats, when not NULL, receives what
 * fpm_last_inspect would write.  A call that fails launches nothing and writes nothing.  The calls change no search
 * state: results, poses, candidates, staged sources, template and model stay as they were.
 * fpm_op_blobs is fpm_blobs_host's signature behind a context: the labelling kernels alone on caller-supplied images
 * (parity vehicle).  It needs no template, sources or model and leaves plan, sources, results, model and the profile
 * counters as they were.  The images are uploaded with the caller's row stride (the device pitch is stride rounded up to
 * 64, all stride bytes of a row are copied), so whatever lies between w and stride lies beside the image on the device
 * too: the kernels mask by u < w.
 * Launches.  Per round of images five kernels, none part of a search or of a captured graph: k_blob_tile (a union-find
 * per 64 x 16 tile), k_blob_merge (the tile pieces united across tile borders), k_blob_flatten (every pixel to its seed,
 * the areas), k_blob_slots (counts, record slots), k_blob_features (box, maximum and sums).  Scratch is 8 bytes per
 * pixel and image; a round takes as many images as keep it within 256 MiB (fpm_blobs_set_round overrides the number,
 * for tests; the results do not depend on it).  Integer arithmetic throughout: the results are the same for every
 * schedule.  Additive entries: FPM_ABI_VERSION is unchanged. */
/* the hits of the last search against the model, cut into blobs where the excess images lie */
int fpm_last_blobs(fpm_ctx* ctx, int32_t source, int32_t a, int32_t kq, int32_t flags,
                   int32_t level, int32_t connectivity, int32_t min_area,
                   fpm_inspect_stats* stats /* may be NULL */, fpm_blob_summary* summary, fpm_blob* out,
                   int32_t cap_per_hit, int32_t cap /* hits */, int32_t* n);
/* the same at caller-supplied poses on the staged sources */
int fpm_blobs_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                 int32_t a, int32_t kq, int32_t flags, int32_t level, int32_t connectivity, int32_t min_area,
                 fpm_inspect_stats* stats, fpm_blob_summary* summary, fpm_blob* out, int32_t cap_per_hit);
/* the labelling kernels alone on caller-supplied u8 images: fpm_blobs_host's signature behind a context (parity vehicle) */
int fpm_op_blobs(fpm_ctx* ctx, const uint8_t* images, int32_t n, int32_t w, int32_t h, size_t stride, int32_t level,
                 int32_t connectivity, int32_t min_area, fpm_blob_summary* summary, fpm_blob* out,
                 int32_t cap_per_hit, int32_t* labels /* may be NULL */);
int fpm_blobs_set_round(fpm_ctx* ctx, int32_t images);   /* images per round of launches; 0 = the engine's choice */
/* Timing of the labelling kernels, collected under fpm_profile_enable and cleared by fpm_profile_reset as
 * fpm_model_profile's (no FPM_K_* index: FPM_K_COUNT is unchanged).  which: 0 = k_blob_tile, 1 = k_blob_merge, 2 =
 * k_blob_flatten, 3 = k_blob_slots, 4 = k_blob_features; bytes = the excess pixels and plane bytes read and written. */
int fpm_blobs_profile(const fpm_ctx* ctx, int32_t which, double* ms, int64_t* launches, int64_t* bytes);

/* --- edge calipers: edges measured across every hit, on the device (no reference equivalent) --------------------------
 * The entries above answer "is the part good"; a caliper answers "how big is it".  A caliper is a narrow rectangle drawn
 * on the taught image across an edge; on every hit it reports where that edge lies, to a fraction of a sample.  Widths,
 * gaps and pin positions are differences of two such numbers.  Everything a caliper needs is resident after a staged
 * search (level 0 of every source, the raw or adopted poses, the patch family's sampler), and the results are a few
 * integers per edge: no image crosses the host.
 * Caliper: fpm_caliper, 48 bytes, no padding.  (cx, cy) = the centre of the sample grid in template coordinates; phi =
 * the scan direction in degrees in the template's frame (0 = along +x); length L = 2 .. 1024 samples along the scan;
 * width W = 1 .. 256 samples across it; half s = 1 .. 16 with 2 s <= L; contrast c = 1 .. 255 gray levels; polarity +1
 * (dark to bright along the scan), -1 or 0 (both); reserved = 0.  The centre and the rectangle may lie outside the
 * template and outside the source; pixels outside the source are 0, as in a patch.
 * Sampling pose (fpm_caliper_pose), in f64 with glibc cos / sin of degrees * (pi / 180), the expression of
 * fpm_align_update.  With hl = (L - 1) / 2, hw = (W - 1) / 2, (cp, sp) = cos, sin of phi and (c, s) those of the hit's
 * angle:
 *     ox = cx - (hl cp - hw sp),  oy = cy - (hl sp + hw cp)           (the template point of sample (0, 0))
 *     lt_k = ((float)(lt_x + (ox c - oy s)), (float)(lt_y + (ox s + oy c)))      (each rounded to f32 once)
 *     angle_k = angle + phi
 * This is the header's convention for where a pose puts a template point in the source, lt + L (x, y) with L = [[cos a,
 * -sin a], [sin a, cos a]], which fpm_align_update takes as exact.
 * Pixels.  I_k(u, v) is pixel (u, v) of the patch fpm_patches_at gives for the rectangle (0, 0, L, W) at the pose (lt_k,
 * angle_k) on that source: same matrix, same fixed-point bilinear arithmetic, border 0, the inverted plane under
 * bitwise_not -- so under bitwise_not the polarities are those of the INVERTED plane: a dark-to-bright edge of the
 * image as acquired is polarity -1.
 * Profile.  P[u] = sum over v of I_k(u, v), u = 0 .. L - 1: exact integers, 0 <= P <= 255 W.
 * Step.  D[i] = (P[i] + .. + P[i + s - 1]) - (P[i - 1] + .. + P[i - s]) for i = s .. L - s, the step across the boundary
 * between samples i - 1 and i; D = 0 outside that range.  |D| <= 16 * 255 * 256 = 1,044,480.
 * Edges.  For p = +1 or -1 let A = p D.  Index i is an edge of polarity p iff A[i] >= c s W and A[i] > A[i - 1] and A[i]
 * >= A[i + 1] (the first sample of a plateau).  Polarity 0 is the union of both lists (an index cannot be in both).
 * Edges come in ascending index.
 * Capacity.  cap_per_caliper = 1 .. 64.  The true count is always reported; with more edges than capacity the first
 * cap_per_caliper by index come back and the caliper carries FPM_CALIPER_TRUNCATED.  One workgroup owns a caliper, so
 * unlike the blobs of a truncated image this is fully determined.  Records behind n_returned are zero-filled.
 * Raw record and derivation.  The device writes four exact integers per edge (fpm_edge_raw): index, d_prev = D[i - 1], d
 * = D[i], d_next = D[i + 1].  The host derives the rest in f64 (fpm_caliper_derive), integers combined first, then
 * converted, no fused multiply-add.  With g = sign(d):
 *     a- = g d_prev, a0 = g d, a+ = g d_next;  den = (a- - a0) + (a+ - a0)                (< 0 always)
 *     delta = 0.5 * (double)(a- - a+) / (double)den                                        (in (-0.5, 0.5])
 *     t = ((double)index - 0.5) + delta;  contrast = (double)|d| / (double)(s W)
 *     template point (tx, ty) = (ox + (t cp - hw sp), oy + (t sp + hw cp))
 *     source point   (sx, sy) = lt_k + ((t ck - hw sk), (t sk + hw ck)),  (ck, sk) = cos, sin of angle_k, lt_k the f32
 *                               sampling pose widened to f64
 * Record: fpm_edge, 64 bytes, no padding.  Summary: fpm_caliper_summary, 32 bytes, no padding, one per (hit, caliper):
 * strongest = the returned edge with the largest |d|, the earliest on ties, -1 when there is none; lt_x, lt_y, angle =
 * the sampling pose.  FPM_CALIPER_OUTSIDE is set on the host, in f64, when a corner sample (0, 0), (L - 1, 0), (0, W - 1)
 * or (L - 1, W - 1) maps outside [0, sw - 1] x [0, sh - 1] through the inverted patch matrix: border zeros are in the
 * profile.
 * Limits.  n_cals = 1 .. 64; hits x n_cals x cap_per_caliper <= 2^22.  Any range violation, a non-finite cx, cy or phi,
 * or a sampling pose beyond the samplers' 2^20 range: FPM_E_INVALID_ARG, nothing launched, nothing written.
 * Launch.  k_caliper, one per call, one 256-lane workgroup per (hit, caliper), never part of a search or of a captured
 * graph.  Integer arithmetic throughout: the results do not depend on any schedule.  The calls change no search state:
 * results, poses, candidates, staged sources, template and model stay as they were.  Additive entries: FPM_ABI_VERSION
 * is unchanged. */
typedef struct fpm_caliper {
    double cx, cy;               /* centre of the sample grid, template coordinates                  */
    double phi;                  /* scan direction, degrees, template frame                          */
    int32_t length, width;       /* L samples along the scan, W across it                            */
    int32_t half;                /* s: samples summed on each side of a boundary                     */
    int32_t contrast;            /* c: least step in gray levels                                     */
    int32_t polarity;            /* +1, -1 or 0 (both)                                               */
    int32_t reserved;            /* 0 */
} fpm_caliper;
typedef struct fpm_edge_raw {
    int32_t index, d_prev, d, d_next;
} fpm_edge_raw;
typedef struct fpm_edge {
    int32_t index, d_prev, d, d_next;
    double t;                    /* sub-sample position along the scan, in samples                   */
    double contrast;             /* |d| / (s W): the step in gray levels                             */
    double tx, ty;               /* the edge point in template coordinates                           */
    double sx, sy;               /* and in source coordinates                                        */
} fpm_edge;
typedef struct fpm_caliper_summary {
    int32_t n_edges;             /* the true count (may exceed cap_per_caliper)                      */
    int32_t n_returned;          /* min(n_edges, cap_per_caliper)                                    */
    int32_t strongest;           /* index into the caliper's returned records, -1 = none             */
    int32_t flags;               /* FPM_CALIPER_TRUNCATED | FPM_CALIPER_OUTSIDE                      */
    float lt_x, lt_y;            /* the sampling pose                                                */
    double angle;
} fpm_caliper_summary;
#define FPM_CALIPER_TRUNCATED 1
#define FPM_CALIPER_OUTSIDE 2
#define FPM_CALIPER_MAX_LENGTH 1024
#define FPM_CALIPER_MAX_WIDTH 256
#define FPM_CALIPER_MAX_HALF 16
#define FPM_CALIPER_MAX_CALS 64          /* n_cals */
#define FPM_CALIPER_MAX_CAP 64           /* cap_per_caliper */
#define FPM_CALIPER_MAX_SLOTS (1 << 22)  /* hits * n_cals * cap_per_caliper */

/* host only, no context: the sampling pose of a caliper on a hit at (lt, angle), by the rule above */
int fpm_caliper_pose(float lt_x, float lt_y, double angle, const fpm_caliper* cal, float* ltk_x, float* ltk_y,
                     double* angle_k);
/* host only, no context: the step and edge rules on a caller's profile of cal->length entries, each 0 .. 255 W (the
 * reference form, as fpm_blobs_host is for blobs).  out holds cap_per_caliper records: the first min(*n_edges,
 * cap_per_caliper) are written, the rest zero-filled; *flags receives FPM_CALIPER_TRUNCATED or 0. */
int fpm_caliper_edges_host(const int32_t* profile, const fpm_caliper* cal, int32_t cap_per_caliper, fpm_edge_raw* out,
                           int32_t* n_edges, int32_t* flags);
/* host only, no context: n raw records of a caliper sampled at the pose (ltk, angle_k) into n fpm_edge, by the rule
 * above.  FPM_E_INVALID_ARG also for a record that is no edge (d = 0, an index outside half .. length - half, or not
 * a- < a0 and a+ <= a0, the local-maximum rule, from which den < 0 follows); nothing is written then. */
int fpm_caliper_derive(const fpm_caliper* cal, float ltk_x, float ltk_y, double angle_k, const fpm_edge_raw* raw,
                       int32_t n, fpm_edge* out);
/* The calipers at caller-supplied poses on the staged sources.  Poses and state rules as fpm_patches_at with a non-NULL
 * rectangle, except that no template is needed: staged sources are, a search is not.  summary: [pose][caliper]; edges:
 * [pose][caliper][cap_per_caliper]; profiles (may be NULL): int32 [pose][caliper][profile_stride] with profile_stride >=
 * the largest length, the entries from a caliper's length on 0. */
int fpm_calipers_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                    const fpm_caliper* cals, int32_t n_cals, int32_t cap_per_caliper, fpm_caliper_summary* summary,
                    fpm_edge* edges, int32_t* profiles, int32_t profile_stride);
/* The calipers over the hits of the last search in result order (source = -1: of all sources), sampled at the context's
 * last poses: the raw ones, or the aligned ones after FPM_ALIGN_ADOPT, exactly as fpm_last_compare.  source, cap (hits),
 * *n, the count-only call (cap = 0 with null outputs) and every state rule are fpm_last_compare's. */
int fpm_last_calipers(fpm_ctx* ctx, int32_t source, const fpm_caliper* cals, int32_t n_cals, int32_t cap_per_caliper,
                      fpm_caliper_summary* summary, fpm_edge* edges, int32_t* profiles, int32_t profile_stride,
                      int32_t cap /* hits */, int32_t* n);
/* Timing of k_caliper, collected under fpm_profile_enable and cleared by fpm_profile_reset as fpm_align_profile's (no
 * FPM_K_* index: FPM_K_COUNT is unchanged).  bytes = L W source pixels per job + the records and profiles written. */
int fpm_caliper_profile(const fpm_ctx* ctx, double* ms, int64_t* launches, int64_t* bytes);

/* --- template masks: compare, align, inspect and cut blobs on the part only (no reference equivalent) ---
 * The tools above work on a rectangle in template coordinates; a part rarely fills its rectangle (background in the
 * corners of a round part, a date code that changes, a hole).  A template mask says which template pixels count.
 * What a mask is.  One per context: a u8 image of exactly the learned template's level-0 size, in template
 * coordinates.  A byte != 0 means "use this pixel", a byte 0 "ignore it"; every non-zero value counts alike, and the
 * mask is stored, and returned by fpm_mask_get, as 0 or 255.  A mask of all zeros is legal.  The mask is context state,
 * like the variation model: no call takes a flag for it, and no flag value changes its meaning.
 * State rules.  Every entry: FPM_E_INVALID_ARG while a search is in flight (fpm_mask_info excepted), FPM_E_NOT_LEARNED
 * without a template.  fpm_mask_set / fpm_mask_set_device: FPM_E_INVALID_ARG for a size other than the template's, a
 * stride below the width, a null pointer, or (device) memory the context's device cannot read -- the pointer, extent and
 * stream rules are fpm_learn_device's for FPM_FMT_GRAY8: any base alignment, any stride, ordered after the work queued
 * on producer_stream.  A set that fails leaves the previous mask in force; one that succeeds replaces it and starts
 * ENABLED.  fpm_mask_enable(0) keeps the mask resident but makes every tool behave as without one; fpm_mask_enable,
 * fpm_mask_get and fpm_mask_count without a mask are FPM_E_INVALID_ARG.  fpm_mask_info reports 0 x 0, count 0, enabled 0
 * when there is none; count = the used pixels of the whole mask.  fpm_mask_count: the used pixels inside a comparison
 * rectangle (NULL = the whole template; the rectangle rules are fpm_compare_at's), whether or not the mask is enabled.
 * Lifetime: the model's.  Dropped by fpm_learn, fpm_learn_device, fpm_learn_at, fpm_learn_hit, fpm_clear_pattern and
 * fpm_destroy; kept by staging, searching, fpm_model_clear and fpm_align_*.  fpm_model_learn CROPS it to the model's
 * rectangle, as it re-frames the model: the new template is that rectangle, so the mask keeps covering the same pixels
 * (and keeps its enabled state).
 * Who honours it.  With a mask set and enabled the entries below do; with none, or a disabled one, every byte of every
 * output is what it is without this block.  M(x, y) is the mask byte at template pixel (x, y).
 *   fpm_last_compare / fpm_compare_at: pixel (u, v) of the rectangle (x, y, w, h) is USED iff M(x + u, y + v) != 0.  n,
 *     the five sums, sum_abs, max_abs, n_over and the box run over the used pixels only; n = fpm_mask_count(rect); zncc,
 *     gain, offset and the table come from those sums by fpm_compare_derive's rule; the difference image is 0 at ignored
 *     pixels.  With n == 0 the call is FPM_OK: all sums 0, zncc = 0, gain = 1, offset = 0, the identity table, the empty
 *     box (w, h, -1, -1).
 *   fpm_align_sums_at / fpm_align_at / fpm_align_last: a pixel is used iff it is used by the interior rule above AND its
 *     own mask byte is non-zero.  Its four neighbours' mask bytes do not matter: the gradient is read from the template,
 *     which is complete.  n_used counts those pixels; fewer than 3 is FPM_ALIGN_SINGULAR as before.  The normalising
 *     table is the masked comparison's.
 *   fpm_last_inspect / fpm_inspect_at: e = 0 at ignored pixels; n is the used count inside the model's rectangle; the
 *     counts, the maximum, the sum, the box and the excess image follow, and gain / offset are the masked comparison's.
 *     fpm_last_blobs / fpm_blobs_at label that excess image: an ignored pixel is background.
 *   fpm_last_histogram / fpm_histogram_at / fpm_last_segment / fpm_segment_at ("gray-value tools" below): pixel (u, v) of
 *     a rectangle (x, y, w, h) is USED iff M(x + u, y + v) != 0.  A histogram counts the used pixels only, n =
 *     fpm_mask_count(rect); Otsu's threshold comes from that histogram; e = 0 at ignored pixels, which are background.
 *   fpm_model_train_last / fpm_model_train_at: the planes accumulate EVERY pixel of the rectangle, masked or not -- the
 *     mask applies when inspecting, so it may be drawn or changed after training.  Only the FPM_COMPARE_NORMALIZE table
 *     is built from the masked sums.
 * Who does not: the search, fpm_last_patches* and fpm_patches_at, the calipers, fpm_last_locate and fpm_locate_at (the
 * "sub-pattern locators" below), the fpm_learn_* entries, fpm_model_sums and fpm_model_images, fpm_op_blobs and
 * fpm_blobs_host.
 * Launches.  Setting a mask runs k_mask_stage once (normalisation and the count, in integers).  A masked call launches
 * the MASK forms of k_patch_compare, k_patch_align and k_model_inspect: as many launches as the unmasked call, counted
 * under the same profile entries, the mask bytes read added to `bytes`.  Exact integers throughout: the results do not
 * depend on any schedule.  Additive entries: FPM_ABI_VERSION and FPM_K_COUNT are unchanged. */
int fpm_mask_set(fpm_ctx* ctx, const uint8_t* mask, int32_t width, int32_t height, size_t stride);
int fpm_mask_set_device(fpm_ctx* ctx, const void* d_mask, int32_t width, int32_t height, size_t stride,
                        void* producer_stream);
int fpm_mask_clear(fpm_ctx* ctx);
int fpm_mask_enable(fpm_ctx* ctx, int32_t enable);
int fpm_mask_info(const fpm_ctx* ctx, int32_t* width, int32_t* height, int64_t* count, int32_t* enabled);
int fpm_mask_get(fpm_ctx* ctx, uint8_t* out, size_t stride);
int fpm_mask_count(fpm_ctx* ctx, const fpm_patch_rect* rect, int64_t* n);

/* --- gray-value tools: histograms, Otsu and threshold blobs of every hit (no reference equivalent) -------
 * The tools above hold a hit against the template or a trained model.  These look at the hit's OWN gray values inside a
 * region of the taught image: "is the cap present" (mean or median of a region), "is the print dark enough" (histogram,
 * percentile), "how many pins or holes, and how big" (threshold, then connected regions).  They need no model.
 * Rectangles.  A region is a comparison rectangle (x, y, w, h) in template coordinates under fpm_compare_at's rules:
 * inside the template, 1 <= w * h <= 2^22, NULL = the whole template.  A learned template is required
 * (FPM_E_NOT_LEARNED).  State, source, cap (hits), *n and the count-only call (cap = 0 with null outputs) are
 * fpm_last_compare's for the _last entries, which sample at the context's last poses (the raw ones, or the aligned ones
 * after FPM_ALIGN_ADOPT); pose and state rules are fpm_compare_at's for the _at entries.
 * Pixels.  I(u, v) is pixel (u, v) of the patch fpm_patches_at gives for that rectangle and pose: same matrix, same
 * fixed-point bilinear arithmetic, border 0, the inverted plane under bitwise_not.  With a template mask set and enabled
 * pixel (u, v) is USED iff M(x + u, y + v) != 0 (the block above); without one every pixel of the rectangle is used.
 * The used count is n = fpm_mask_count(rect), or w * h.
 * Histogram.  H[b] = the number of used pixels with I == b, b = 0 .. 255, as uint32 (n <= 2^22 fits); the sum of H is n.
 * Pixels outside the source are 0 and land in bin 0, as in a patch.  One call takes n_rects = 1 .. 64 rectangles, which
 * may differ in size and are each checked as above; the output is uint32 [hit][rect][256] with hits * n_rects <= 65536.
 * Derivation (fpm_hist_derive; host only, no context).  fpm_hist_stats, 64 bytes, no padding.  Integers first, then f64
 * in the order written, every operation rounded on its own (no fused multiply-add).  With cum(v) = H[0] + .. + H[v]:
 *     n = cum(255);  sum = sum of b H[b];  sum_sq = sum of b^2 H[b]                       (int64, exact)
 *     min, max = the smallest and largest b with H[b] != 0;  median = the smallest v with 2 cum(v) >= n
 *     mean = (double)sum / (double)n;  stddev = sqrt((double)(n sum_sq - sum sum)) / (double)n
 *   Otsu.  For t = 0 .. 254 let n0 = cum(t) and s0 = sum over b <= t of b H[b].  t is ADMISSIBLE iff 0 < n0 < n.  N = n
 *   s0 - n0 sum, exact in int64 (|N| < 2^53: exact as a double too);
 *     B(t) = ((double)N * (double)N) / ((double)n0 * (double)(n - n0))
 *   otsu = the admissible t with the largest B, the smallest such t on ties (t rising, replaced only on strictly
 *   greater).  Class 0 is I <= otsu.
 *   Degenerate.  n == 0: every field 0 and flags = FPM_HIST_EMPTY.  min == max (no admissible t): otsu = min and
 *   FPM_HIST_FLAT is set.  A histogram whose total exceeds 2^22, or a null pointer: FPM_E_INVALID_ARG, *out untouched.
 * Segmentation (one rectangle per call).  polarity = +1 (bright: foreground iff I > t, e = I - t) or -1 (dark: foreground
 * iff I < t, e = t - I): e is 1 .. 255 on the foreground, 0 elsewhere and 0 at ignored pixels.  threshold = 0 .. 255, or
 * FPM_SEG_OTSU: each hit then takes t from its own histogram of the rectangle, t = otsu for bright, t = otsu + 1 for
 * dark (so both polarities cut between the same two classes).  A hit whose histogram is empty or flat has NO foreground
 * under FPM_SEG_OTSU (e = 0 everywhere) and carries the flag; with a fixed threshold the histogram is not taken and
 * those two flags stay 0.  The image e is labelled by the blob contract ("defect blobs") unchanged, with level 0:
 * connectivity 4 or 8, seeds, min_area, cap_per_hit, FPM_BLOBS_TRUNCATED and the rule for truncated images of "defect
 * blobs on the device".  In a record max_value and sum_value are the peak and the integrated contrast beyond the
 * threshold.  Per hit the call returns fpm_segment_info (16 bytes, no padding): n = the used count, threshold = the t
 * used, flags = FPM_HIST_EMPTY | FPM_HIST_FLAT | FPM_GRAY_OUTSIDE -- the last set on the host, in f64, by the calipers'
 * four-corner rule on the rectangle's corner pixels (0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1): border zeros are in
 * the region --; one fpm_blob_summary; cap_per_hit fpm_blob records; and, when img is not NULL, e as u8 images under
 * fpm_last_inspect's image-buffer rules (row_stride >= w, patch_stride >= row_stride * h).
 * Errors.  n_rects outside 1 .. 64, hits * n_rects > 65536, a bad rectangle, polarity other than +1 / -1, threshold
 * outside -1 .. 255, the blob entries' argument rules, a null output, a pose beyond the samplers' range:
 * FPM_E_INVALID_ARG, nothing launched, nothing written.  The calls change no search state: results, poses, candidates,
 * staged sources, template, model and mask stay as they were.
 * Launches, none part of a search or of a captured graph.  A histogram call: the output cleared on the stream, one
 * k_patch_hist (k_patch_hist_masked under a mask) over all (hit, rectangle) jobs, the words back to a pinned buffer of
 * the context, each histogram checked against its n, then copied to the caller.  A segmentation with a fixed threshold:
 * one k_patch_threshold (or _masked), then the five labelling kernels per round.  Under FPM_SEG_OTSU the histogram
 * launch and one copy to the host come first, fpm_hist_derive's rule per hit gives t, and the thresholds go back with
 * the job table.  Integer arithmetic throughout: the results do not depend on any schedule, nor on fpm_gray_set_run.
 * Out of scope: FPM_COMPARE_NORMALIZE tables (Otsu is the lighting-robust form), a band lo .. hi, hysteresis, more than
 * one rectangle (size) inside one segmentation call, results left in device memory.
 * Additive entries: FPM_ABI_VERSION and FPM_K_COUNT are unchanged. */
typedef struct fpm_hist_stats {
    int64_t n;                   /* pixels counted                                                    */
    int64_t sum, sum_sq;         /* sum b H[b], sum b^2 H[b]                                          */
    int32_t min, max;            /* smallest and largest occupied bin                                 */
    int32_t median;              /* smallest v with 2 cum(v) >= n                                     */
    int32_t otsu;                /* class 0 is I <= otsu                                              */
    double mean, stddev;
    int32_t flags;               /* FPM_HIST_EMPTY | FPM_HIST_FLAT                                    */
    int32_t reserved;            /* 0 */
} fpm_hist_stats;
typedef struct fpm_segment_info {
    int64_t n;                   /* used pixels of the rectangle                                      */
    int32_t threshold;           /* the t used                                                        */
    int32_t flags;               /* FPM_HIST_EMPTY | FPM_HIST_FLAT | FPM_GRAY_OUTSIDE                 */
} fpm_segment_info;
#define FPM_HIST_EMPTY 1
#define FPM_HIST_FLAT 2
#define FPM_GRAY_OUTSIDE 4
#define FPM_SEG_OTSU (-1)                /* threshold: per hit, from its own histogram */
#define FPM_GRAY_MAX_RECTS 64            /* n_rects */
#define FPM_GRAY_MAX_JOBS 65536          /* hits * n_rects */

/* host only, no context: the statistics and Otsu's threshold of one histogram, by the rule above */
int fpm_hist_derive(const uint32_t hist[256], fpm_hist_stats* out);
/* the histograms of n_rects rectangles over the hits of the last search in result order (source = -1: of all sources);
 * hist: uint32 [hit][rect][256] */
int fpm_last_histogram(fpm_ctx* ctx, const fpm_patch_rect* rects /* NULL with n_rects = 1: the whole template */,
                       int32_t n_rects, int32_t source, uint32_t* hist, int32_t cap /* hits */, int32_t* n);
/* the same at caller-supplied poses on the staged sources */
int fpm_histogram_at(fpm_ctx* ctx, const fpm_patch_rect* rects, int32_t n_rects, const int32_t* src_index,
                     const float* lt, const double* angles, int32_t n_poses, uint32_t* hist);
/* the hits of the last search thresholded inside rect and cut into blobs; info, summary: one per hit; out: cap_per_hit
 * records per hit; img (may be NULL): the e images */
int fpm_last_segment(fpm_ctx* ctx, int32_t source, const fpm_patch_rect* rect, int32_t threshold, int32_t polarity,
                     int32_t connectivity, int32_t min_area, fpm_segment_info* info, fpm_blob_summary* summary,
                     fpm_blob* out, int32_t cap_per_hit, int32_t cap /* hits */, int32_t* n, uint8_t* img,
                     size_t row_stride, size_t patch_stride);
/* the same at caller-supplied poses on the staged sources */
int fpm_segment_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                   const fpm_patch_rect* rect, int32_t threshold, int32_t polarity, int32_t connectivity,
                   int32_t min_area, fpm_segment_info* info, fpm_blob_summary* summary, fpm_blob* out,
                   int32_t cap_per_hit, uint8_t* img, size_t row_stride, size_t patch_stride);
/* tiles per workgroup of k_patch_hist (a workgroup walks that many consecutive 64 x 16 tiles of one job before it adds
 * its 256 counts to the job's histogram); 0 = the engine's choice.  For tests and measurements: results never depend
 * on it. */
int fpm_gray_set_run(fpm_ctx* ctx, int32_t tiles);
/* Timing of the two kernels, collected under fpm_profile_enable and cleared by fpm_profile_reset as
 * fpm_caliper_profile's (no FPM_K_* index).  which: 0 = k_patch_hist, 1 = k_patch_threshold; bytes = source pixels
 * read (+ mask bytes read) + histogram words or e pixels written. */
int fpm_gray_profile(const fpm_ctx* ctx, int32_t which, double* ms, int64_t* launches, int64_t* bytes);

/* --- sub-pattern locators: find template regions on every hit (no reference equivalent) ------------------
 * The tools above treat a hit as one rigid copy of the taught image.  A locator asks where on this hit a given piece of
 * the taught image is, and how well it matches there: a label on a cap, a print on a package, a fiducial beside a pad,
 * each with a placement error of its own.  It is the project's own operation, a normalized correlation, at its smallest
 * scale: the piece is found again inside a small window around its nominal place.
 * Feature.  fpm_feature, 32 bytes, no padding.  (x, y, w, h) is a rectangle in template coordinates, inside the learned
 * template; w and h are 1 .. 128; rx and ry are the search radii in patch pixels, 0 .. 16; reserved is 0.  These caps
 * keep every sum in int32 (sum I T <= 65025 * 16384 = 1,065,369,600 < 2^31) and the window, at most 160 x 160 bytes,
 * and the template region, at most 16 KiB, inside one workgroup's LDS.
 * Window pixels.  With ww = w + 2 rx and wh = h + 2 ry, I(u, v) is pixel (u, v) of the patch fpm_patches_at gives for
 * the rectangle (x - rx, y - ry, ww, wh) at the hit's pose: same matrix, same fixed-point bilinear arithmetic, border 0,
 * the inverted plane under bitwise_not.  The window may reach outside the template and outside the source.  T(a, b) is
 * template level 0 at (x + a, y + b).
 * Sums per offset.  For dx = -rx .. rx and dy = -ry .. ry, exact integers:
 *     S_i(dx, dy)  = sum over a < w, b < h of I(a + rx + dx, b + ry + dy)
 *     S_ii(dx, dy) = the same sum of squares;  S_it(dx, dy) = the same sum of products with T(a, b)
 * n = w h, sum_t and sum_tt are constant per feature.
 * Score.  z(dx, dy) is fpm_compare_derive's zncc of (n, S_i, S_ii, sum_t, sum_tt, S_it): the expression, the order and
 * the 0 when Di == 0 or Dt == 0 are the same.  Host and device both evaluate it in f64; the device build is
 * -ffp-contract=off with correctly rounded sqrt and /.
 * Peak.  The offset with the largest z; ties go to the smallest dx^2 + dy^2, then the smallest dy, then the smallest dx.
 * The result is fully determined and does not depend on any schedule; a flat region answers "at nominal, score 0".
 * Raw record.  The device writes fpm_locate_raw, 160 bytes, no padding.  The three arrays hold the sums of the 3 x 3
 * neighbourhood of the peak: entry (j + 1) * 3 + (i + 1) is offset (dx + i, dy + j), zero where that offset lies
 * outside the search range.  c_i, c_ii, c_it are the three sums at offset (0, 0).  flags is 0 from the device and from
 * fpm_locate_host; the entries set FPM_LOCATE_OUTSIDE there, on the host (below), and nothing else.
 * Maps.  maps may be NULL.  It receives all three sums of every offset as int32 [job][3][map_stride], job = hit *
 * n_features + feature; map_stride is at least the largest (2 rx + 1)(2 ry + 1) of the call.  Offsets are row-major, dy
 * rising then dx.  Entries behind a feature's count are 0.
 * Derivation (fpm_locate_derive; host only, no context).  f64, integers combined first, no fused multiply-add.  It fills
 * fpm_locate_result, 80 bytes, no padding:
 *     score = z at the peak;  score_nominal = z(0, 0)
 *     per axis, when the peak is not on the search range's border on that axis, with z-, z0, z+ along it:
 *       den = (z- - z0) + (z+ - z0);  delta = 0.5 (z- - z+) / den when den < 0, else 0  (so |delta| <= 0.5)
 *     on the border, and for radius 0, delta = 0 and FPM_LOCATE_EDGE_X / FPM_LOCATE_EDGE_Y is set
 *     ox = dx + delta_x, oy = dy + delta_y: the displacement from nominal in template pixels
 *     tx = (x + (w - 1) / 2) + ox, ty = (y + (h - 1) / 2) + oy
 *     (sx, sy) = lt + L (tx, ty): L the matrix of the hit's angle, lt the f32 pose widened to f64 -- the convention of
 *       fpm_caliper_derive and fpm_align_update, with glibc cos and sin:
 *       sx = (double)lt_x + (tx c - ty s), sy = (double)lt_y + (tx s + ty c), c, s = cos, sin of angle * pi / 180
 *     FPM_LOCATE_FLAT is set when Dt == 0 or the peak's Di == 0
 *     FPM_LOCATE_OUTSIDE is copied from the raw record's flags.  The entries set it there by the calipers' four-corner
 *       rule on the window's corner pixels (0, 0), (ww - 1, 0), (0, wh - 1), (ww - 1, wh - 1), on the host, in f64,
 *       through the matrix the sampler takes: border zeros are in the window.
 *   A record that no search can have produced (n != w h, |dx| > rx, |dy| > ry) is FPM_E_INVALID_ARG, *out untouched.
 * Host form.  fpm_locate_host applies the same rules to a caller's u8 window (ww x wh) and template region (w x h): the
 * reference form, as fpm_blobs_host and fpm_caliper_edges_host are for their blocks.  maps there is [3][(2 rx + 1)(2 ry
 * + 1)].
 * Limits and errors.  n_features is 1 .. 64; hits * n_features <= 65536.  A bad rectangle, size or radius, a non-zero
 * reserved, a null output, map_stride below the largest offset count (with maps), or a pose beyond the samplers' 2^20
 * range: FPM_E_INVALID_ARG, nothing launched, nothing written.  FPM_E_NOT_LEARNED without a template.  State, source,
 * cap (hits), *n and the count-only call are fpm_last_compare's for fpm_last_locate, which samples at the raw poses, or
 * at the adopted ones after FPM_ALIGN_ADOPT; pose and state rules are fpm_compare_at's for fpm_locate_at.  The calls
 * change no search state: results, poses, candidates, staged sources, template, model and mask stay as they were.
 * Mask.  A template mask is not honoured (the block above).
 * Launches.  One k_patch_locate per call over all (hit, feature) jobs, never part of a search or of a captured graph;
 * the records (and maps) come back through a pinned buffer of the context, are checked, then copied to the caller.
 * Out of scope: masked correlation, a rotation or scale search of the feature, a second-best peak, results left in
 * device memory, features learned from anything but the current template.
 * Additive entries: FPM_ABI_VERSION and FPM_K_COUNT are unchanged. */
typedef struct fpm_feature {
    int32_t x, y, w, h;          /* the region in template coordinates, inside the template; w, h 1 .. 128 */
    int32_t rx, ry;              /* search radii in patch pixels, 0 .. 16                                 */
    int32_t reserved[2];         /* 0 */
} fpm_feature;
typedef struct fpm_locate_raw {
    int32_t dx, dy;              /* the peak's offset                                                     */
    int32_t flags;               /* 0 from the device; FPM_LOCATE_OUTSIDE set by the entries, on the host */
    int32_t reserved;            /* 0 */
    int64_t n, sum_t, sum_tt;    /* w h, sum T, sum T^2                                                   */
    int32_t s_i[9], s_ii[9], s_it[9];   /* the sums of the peak's 3 x 3 neighbourhood                     */
    int32_t c_i, c_ii, c_it;     /* the sums at offset (0, 0)                                             */
} fpm_locate_raw;
typedef struct fpm_locate_result {
    int32_t dx, dy;
    int32_t flags;               /* FPM_LOCATE_EDGE_X | _EDGE_Y | _FLAT | _OUTSIDE                        */
    int32_t reserved;            /* 0 */
    double score, score_nominal;
    double ox, oy;               /* displacement from nominal, template pixels                            */
    double tx, ty;               /* the found centre in template coordinates                              */
    double sx, sy;               /* and in source coordinates                                             */
} fpm_locate_result;
#define FPM_LOCATE_EDGE_X 1
#define FPM_LOCATE_EDGE_Y 2
#define FPM_LOCATE_FLAT 4
#define FPM_LOCATE_OUTSIDE 8
#define FPM_LOCATE_MAX_SIDE 128          /* w, h */
#define FPM_LOCATE_MAX_RADIUS 16         /* rx, ry */
#define FPM_LOCATE_MAX_FEATURES 64       /* n_features */
#define FPM_LOCATE_MAX_JOBS 65536        /* hits * n_features */

/* host only, no context: sums, peak and raw record of one window (ww x wh) against one template region (w x h) */
int fpm_locate_host(const uint8_t* window, size_t window_stride, const uint8_t* tmpl, size_t tmpl_stride, int32_t w,
                    int32_t h, int32_t rx, int32_t ry, fpm_locate_raw* raw, int32_t* maps /* may be NULL */);
/* host only, no context: one raw record of feature feat on a hit at (lt, angle) into *out, by the rule above */
int fpm_locate_derive(const fpm_feature* feat, float lt_x, float lt_y, double angle, const fpm_locate_raw* raw,
                      fpm_locate_result* out);
/* the features at caller-supplied poses on the staged sources; results, raw: [pose][feature] */
int fpm_locate_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                  const fpm_feature* feats, int32_t n_feats, fpm_locate_result* results, fpm_locate_raw* raw /* may be NULL */,
                  int32_t* maps /* may be NULL */, int32_t map_stride);
/* the same over the hits of the last search in result order (source = -1: of all sources) */
int fpm_last_locate(fpm_ctx* ctx, int32_t source, const fpm_feature* feats, int32_t n_feats, fpm_locate_result* results,
                    fpm_locate_raw* raw, int32_t* maps, int32_t map_stride, int32_t cap /* hits */, int32_t* n);
/* Timing of k_patch_locate, collected under fpm_profile_enable and cleared by fpm_profile_reset as fpm_caliper_profile's
 * (no FPM_K_* index).  bytes = window pixels sampled + template pixels read + records and maps written. */
int fpm_locate_profile(const fpm_ctx* ctx, double* ms, int64_t* launches, int64_t* bytes);

/* --- edge probes: thousands of short calipers per hit, with line and circle fits (no reference
 * equivalent) ---------------------------------------------------------------------------------------------------------
 * A caliper measures one edge; an outline needs a probe every pixel or two along it: a hole's diameter is a ring of
 * radial probes and a circle fit, the straightness of a side a row of probes and a line fit, a burr or a chipped rim
 * "the edge moved by d px here".  A probe is a short caliper that reports ONE edge.  All probes of a call share their
 * size and rules (fpm_probe_params); a probe itself is a point and a direction.  The job table of a call is one entry
 * per hit plus one entry per probe, 64 hits + 32 n_probes bytes, and the two are composed on the device.
 * Probe: fpm_probe, 24 bytes, no padding.  (x, y) = the nominal edge point in template coordinates and the centre of the
 * probe's sample grid; phi = the scan direction in degrees in the template's frame (0 = along +x); for a taught contour
 * the direction of the gradient.  The point and the grid may lie outside the template and outside the source; pixels
 * outside the source are 0, as in a patch.
 * Parameters: fpm_probe_params, 32 bytes, one per call.  length L = 4 .. 64 samples along the scan; width W = 1 .. 16
 * across it; half s = 1 .. 8 with 2 s <= L; contrast c = 1 .. 255 gray levels; polarity +1 (dark to bright along the
 * scan), -1 or 0 (both); select = FPM_PROBE_NEAREST, _STRONGEST, _FIRST or _LAST; two reserved ints = 0.
 * Limits.  n_probes = 1 .. 4096 (FPM_PROBE_MAX); hits x n_probes <= 2^22.  With s W 255 <= 32 640 every D fits 16 bits.
 * Any violation, a non-finite field, or a sample beyond the samplers' 2^20 range: FPM_E_INVALID_ARG, nothing launched,
 * nothing written.  The 2^20 check is made per hit on the four corners of the template-space bounding box of all
 * probes' sample grids, through that hit's inverted matrix.
 * Sampling matrix.  Per probe, once per call, in f64 with glibc cos / sin of phi * (pi / 180):
 *     (cp, sp) = cos, sin;  hl = (L - 1) / 2;  hw = (W - 1) / 2
 *     ox = x - (hl cp - hw sp);  oy = y - (hl sp + hw cp)               (the template point of sample (0, 0))
 * Per hit, once: Minv = the inverted patch matrix of the template frame, fpm_patch_matrix for the rectangle origin
 * (0, 0), inverted as cv::warpAffine inverts it -- what every per-hit tool samples the template's rectangle with.  The
 * matrix N that takes sample (u, v) of probe k on that hit to source coordinates is the composition below, every
 * product and every sum rounded once, in exactly this order (fpm_probe_matrix):
 *     N0 = Minv0 cp + Minv1 sp            N3 = Minv3 cp + Minv4 sp
 *     N1 = Minv1 cp - Minv0 sp            N4 = Minv4 cp - Minv3 sp
 *     N2 = (Minv0 ox + Minv1 oy) + Minv2  N5 = (Minv3 ox + Minv4 oy) + Minv5
 * The device evaluates the same expressions in f64 without contraction, so host, device and a restatement agree bit
 * for bit.
 * Pixels.  From N the pixels are the patch family's, kAbBits = 10, kInterBits = 5, kAbScale = 1024, kRoundDelta = 16:
 *     ad[u] = rint(N0 u kAbScale), bd[u] = rint(N3 u kAbScale)
 *     X0[v] = rint((N1 v + N2) kAbScale) + kRoundDelta, Y0[v] = rint((N4 v + N5) kAbScale) + kRoundDelta
 *     X = (X0[v] + ad[u]) >> (kAbBits - kInterBits), Y = (Y0[v] + bd[u]) >> (kAbBits - kInterBits)
 *     I(u, v) = the bilinear tap set of level 0 at (X, Y), border 0 (cv::remap's fixed-point rule, as in a patch)
 * on the inverted plane under bitwise_not, whose polarities the probes therefore see.  A probe's pixels are NOT
 * bit-equal to those of a caliper drawn at the same place: the pose convention differs on purpose (no f32 rounding of
 * a per-probe lt, no cos(angle + phi)).  A probe with phi = 0 and ox = oy = 0 has N == Minv, so its pixels are
 * fpm_patches_at's for the rectangle (0, 0, L, W).
 * Profile, step, edges: the caliper's definitions, unchanged.  P[u] = sum over v of I(u, v); D[i] = (P[i] + .. + P[i + s
 * - 1]) - (P[i - 1] + .. + P[i - s]) for i = s .. L - s and 0 elsewhere; with A = p D, index i is an edge of polarity p
 * iff A[i] >= c s W and A[i] > A[i - 1] and A[i] >= A[i + 1]; polarity 0 is the union.
 * Selection.  One edge per probe, by integers only.  NEAREST minimises |2 i - L| (boundary i lies at i - 0.5, the
 * grid's centre at (L - 1) / 2); STRONGEST maximises |D[i]|; ties in both go to the lower index.  FIRST and LAST go by
 * index.
 * Raw record: fpm_probe_raw, 24 bytes: index, n_edges, d_prev = D[i - 1], d = D[i], d_next = D[i + 1], flags.  index = 0
 * when no edge qualifies (valid indices are >= 1); the D fields are then 0.  n_edges is the true count.
 * FPM_PROBE_OUTSIDE is set by the device, iff one of the four corner samples (0, 0), (L - 1, 0), (0, W - 1), (L - 1,
 * W - 1) has its tap origin (X >> kInterBits, Y >> kInterBits) outside [0, sw - 2] x [0, sh - 2]: the sampler's border
 * path, an exact integer rule (border zeros may be in the profile; a warning, not an error).
 * Derivation (fpm_probe_derive): host only, f64, integers combined first, no fused multiply-add.  With g = sign(d):
 *     a- = g d_prev, a0 = g d, a+ = g d_next;  den = (a- - a0) + (a+ - a0)
 *     delta = 0.5 * (double)(a- - a+) / (double)den;  t = ((double)index - 0.5) + delta
 *     contrast = (double)a0 / (double)(s W);  dev = t - hl     (signed displacement from nominal along phi, template px)
 *     (tx, ty) = (ox + (t cp - hw sp), oy + (t sp + hw cp))
 *     (sx, sy) = ((double)lt_x + (tx c - ty s), (double)lt_y + (tx s + ty c)),  (c, s) = cos, sin of the hit's angle
 * the last line being the header's one convention for where a pose puts a template point.  A record that is no edge
 * (d = 0, an index outside s .. L - s, n_edges outside 1 .. L, or not a- < a0 and a+ <= a0) is rejected; a record with
 * index = 0 must have n_edges = 0 and zero D fields and gives a result whose doubles are 0.
 * Result: fpm_probe_result, 64 bytes, no padding: index, n_edges, d, flags, then dev, contrast, tx, ty, sx, sy.
 * Summary: fpm_probe_summary, 64 bytes, one per hit, from the hit's results in ascending probe index: n_found (index >=
 * 1), n_missing, n_ambiguous (n_edges > 1), n_outside, worst (the probe with the largest |dev|, the earliest on ties,
 * -1 if none is found), sum_dev, sum_dev_sq (each dev * dev rounded, then added), max_abs_dev, and the hit's pose.
 * Launch.  k_probe, one per call: one 64-lane wave per (hit, probe), four probes of a hit per workgroup, never part of a
 * search or of a captured graph.  Integer arithmetic from the pixels on: the results do not depend on any schedule.
 * The calls change no search state.  Additive entries: FPM_ABI_VERSION is unchanged. */
typedef struct fpm_probe {
    double x, y;                 /* nominal edge point = centre of the sample grid, template coordinates */
    double phi;                  /* scan direction, degrees, template frame                          */
} fpm_probe;
typedef struct fpm_probe_params {
    int32_t length, width;       /* L samples along the scan, W across it                            */
    int32_t half;                /* s: samples summed on each side of a boundary                     */
    int32_t contrast;            /* c: least step in gray levels                                     */
    int32_t polarity;            /* +1, -1 or 0 (both)                                               */
    int32_t select;              /* FPM_PROBE_NEAREST .. FPM_PROBE_LAST                              */
    int32_t reserved[2];         /* 0 */
} fpm_probe_params;
typedef struct fpm_probe_raw {
    int32_t index, n_edges, d_prev, d, d_next, flags;
} fpm_probe_raw;
typedef struct fpm_probe_result {
    int32_t index, n_edges, d, flags;
    double dev;                  /* signed displacement from nominal along phi, template pixels      */
    double contrast;             /* |d| / (s W): the step in gray levels                             */
    double tx, ty;               /* the edge point in template coordinates                           */
    double sx, sy;               /* and in source coordinates                                        */
} fpm_probe_result;
typedef struct fpm_probe_summary {
    int32_t n_found, n_missing, n_ambiguous, n_outside;
    int32_t worst;               /* probe index of the largest |dev|, -1 = none found                */
    int32_t reserved;            /* 0 */
    double sum_dev, sum_dev_sq, max_abs_dev;
    float lt_x, lt_y;            /* the hit's pose                                                   */
    double angle;
} fpm_probe_summary;
#define FPM_PROBE_NEAREST 0
#define FPM_PROBE_STRONGEST 1
#define FPM_PROBE_FIRST 2
#define FPM_PROBE_LAST 3
#define FPM_PROBE_OUTSIDE 1
#define FPM_PROBE_MIN_LENGTH 4
#define FPM_PROBE_MAX_LENGTH 64
#define FPM_PROBE_MAX_WIDTH 16
#define FPM_PROBE_MAX_HALF 8
#define FPM_PROBE_MAX 4096               /* n_probes */
#define FPM_PROBE_MAX_SLOTS (1 << 22)    /* hits * n_probes */

/* host only, no context: the composed matrix N of one probe on a hit at (lt, angle) of a src_w x src_h source */
int fpm_probe_matrix(int32_t src_w, int32_t src_h, float lt_x, float lt_y, double angle, const fpm_probe* probe,
                     const fpm_probe_params* params, double n[6]);
/* host only, no context: the step, edge and select rules on a caller's profile of params->length entries, each 0 ..
 * 255 W (the reference form); out->flags = 0 */
int fpm_probe_edges_host(const int32_t* profile, const fpm_probe_params* params, fpm_probe_raw* out);
/* host only, no context: raw record i of probe i (n of each) on a hit at (lt, angle) into out[i], by the rule above;
 * FPM_E_INVALID_ARG for a record that is no edge, nothing written then */
int fpm_probe_derive(const fpm_probe* probes, const fpm_probe_params* params, float lt_x, float lt_y, double angle,
                     const fpm_probe_raw* raw, int32_t n, fpm_probe_result* out);
/* The probes at caller-supplied poses on the staged sources.  Poses and state rules as fpm_calipers_at: staged sources
 * are needed, a template and a search are not.  summary: [pose]; results: [pose][probe]; profiles (may be NULL): int32
 * [pose][probe][profile_stride] with profile_stride >= length, the entries from length on 0. */
int fpm_probes_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                  const fpm_probe* probes, int32_t n_probes, const fpm_probe_params* params, fpm_probe_summary* summary,
                  fpm_probe_result* results, int32_t* profiles, int32_t profile_stride);
/* The probes over the hits of the last search in result order (source = -1: of all sources), at the context's last
 * poses: the raw ones, or the aligned ones after FPM_ALIGN_ADOPT, exactly as fpm_last_compare.  source, cap (hits), *n,
 * the count-only call (cap = 0 with null outputs) and every state rule are fpm_last_compare's. */
int fpm_last_probes(fpm_ctx* ctx, int32_t source, const fpm_probe* probes, int32_t n_probes, const fpm_probe_params* params,
                    fpm_probe_summary* summary, fpm_probe_result* results, int32_t* profiles, int32_t profile_stride,
                    int32_t cap /* hits */, int32_t* n);
/* Timing of k_probe, collected under fpm_profile_enable and cleared by fpm_profile_reset as fpm_caliper_profile's (no
 * FPM_K_* index: FPM_K_COUNT is unchanged).  bytes = L W source pixels per (hit, probe) + the job table read + the
 * records and profiles written. */
int fpm_probe_profile(const fpm_ctx* ctx, double* ms, int64_t* launches, int64_t* bytes);

/* Fits (host only, f64, no fused multiply-add): what turns a ring or a row of found probes into a diameter or a
 * straightness.  pts = [n][2] doubles, (sx, sy) or (tx, ty) of the found records.  trim > 0: after the first fit the
 * points with |residual| > trim are dropped and the fit is repeated once on the rest, in their order (when fewer than
 * the least number remain the first fit stands and FPM_FIT_TRIM_STARVED is set); trim = 0: no rejection.
 * FPM_E_INVALID_ARG below 2 points for the line and 3 for the circle, for a non-finite coordinate, or for a trim that is
 * negative or not finite; nothing is written then.
 * fpm_fit_line: total least squares.  mx = (x_0 + x_1 + ..) / m, my alike, sums in index order; with dx = x_i - mx, dy
 * = y_i - my: sxx = sum dx dx, sxy = sum dx dy, syy = sum dy dy, in index order.  theta = 0.5 atan2(2 sxy, sxx - syy),
 * the direction, angle = theta in degrees, in (-90, 90]; the signed residual of a point is dy cos theta - dx sin theta;
 * (px, py) = the point of the line nearest the origin, m - (mx cos theta + my sin theta) (cos theta, sin theta).
 * fpm_fit_circle: Kasa's algebraic fit on centred coordinates (u, v) = (x - mx, y - my): [suu suv; suv svv] (uc, vc) =
 * 0.5 (suuu + suvv, svvv + svuu), r^2 = uc^2 + vc^2 + (suu + svv) / m; then at most 8 Gauss-Newton steps on the
 * geometric residual d_i - r, stopped when every component of a step is at most 1e-10 in magnitude.
 * FPM_FIT_COLLINEAR when the 2 x 2 determinant is at most 1e-12 (suu + svv)^2 (centre, radius, rms and max_resid are
 * then 0); FPM_FIT_NOT_CONVERGED when the eighth step was still larger, or a step's 3 x 3 system was singular.
 * rms = sqrt(sum r_i^2 / n_used), max_resid = the largest |r_i|, both over the points used. */
typedef struct fpm_line_fit {
    double angle;                /* direction, degrees, in (-90, 90]                                 */
    double px, py;               /* the point of the line nearest the origin                         */
    double rms, max_resid;
    int32_t n_used, flags;
} fpm_line_fit;
typedef struct fpm_circle_fit {
    double cx, cy, r;
    double rms, max_resid;
    int32_t n_used, flags;
} fpm_circle_fit;
#define FPM_FIT_NOT_CONVERGED 1
#define FPM_FIT_COLLINEAR 2
#define FPM_FIT_TRIM_STARVED 4
int fpm_fit_line(const double* pts, int32_t n, double trim, fpm_line_fit* out);
int fpm_fit_circle(const double* pts, int32_t n, double trim, fpm_circle_fit* out);

/* --- angle sharding of one search (no reference equivalent: the reference loops over the
 * whole angle list on one thread, TemplateMatcher.cpp:157-211) ----------------------------------------------
 * A search splits at the reference's own seam: the top-layer sweep and every candidate's pyramid descent
 * (:157-371) are independent per angle, while the std::sort of the top candidates (:214) and the result
 * filters (:373-432) need all of them.  So: every rank runs the search restricted to its shard of the angle
 * list, exports its candidate records, the records are all-gathered in shard order (RCCL over xGMI on a node),
 * and fpm_merge_candidates runs the coupled tail.  The merged results equal the unsharded search's bit for bit.
 *
 * One top-layer candidate (an s_MatchParameter of vecMatchParameter, DataStructures.h:58-94) and the outcome of
 * its refinement. */
typedef struct fpm_candidate {
    double top_score;     /* dMatchScore at the top layer: the key of std::sort(compareScoreBig2Small) (:214) */
    double x, y;          /* refined ptLT at the stop layer, scaled to layer 0 (the vecAllResult entry's pt, :346-356;
                             fpm_params.stop_layer: MatchToolDlg.cpp:951, :1035), when kept                  */
    double score;         /* refined dMatchScore (:312), when kept                                         */
    double angle;         /* refined dMatchAngle (sub-pixel estimate applied, :334-344), when kept          */
    int32_t angle_index;  /* index of the candidate's angle in the full top-layer angle list (:130-144)    */
    int32_t peak_rank;    /* push order of the peak within its angle (0 = the minMaxLoc / s_BlockMax max)  */
    int32_t source;       /* source index within a staged batch (0 for fpm_match)                           */
    int32_t kept;         /* 1: reaches vecAllResult; 0: left the descent at a layer score (:331-332)       */
} fpm_candidate;

/* Restrict this context's searches to shard `shard` of `shards`: the contiguous block
 * [n*shard/shards, n*(shard+1)/shards) of the n top-layer angles.  (0, 1) = the whole list (default).  fpm_match /
 * fpm_match_staged on a sharded context return the results of that block alone. */
int fpm_set_angle_shard(fpm_ctx* ctx, int32_t shard, int32_t shards);
int fpm_get_angle_shard(const fpm_ctx* ctx, int32_t* shard, int32_t* shards);
/* Candidate records of source `source` of the last fpm_match / fpm_match_staged* call, in push order
 * (angle_index ascending, then peak_rank), every top-layer candidate of the context's shard included. */
int fpm_last_candidates(const fpm_ctx* ctx, int32_t source, fpm_candidate* out, int32_t cap, int32_t* n);
/* The coupled tail of TemplateMatcher::match (:214, :262-432) over the candidate records of ONE source: `cand` is
 * the concatenation of every shard's records in shard order (push order; FPM_E_INVALID_ARG otherwise).  Host
 * only, no context or device needed; tmpl_w/tmpl_h = the learned template's level-0 size.  With p->stop_layer set the
 * overlap filter's rectangle is the layer-1 template size times two (MatchToolDlg.cpp:1053-1054) when the top layer is
 * at least 1; having no context, the function derives the top layer from tmpl_w, tmpl_h and p->min_reduce_area by the
 * rule the search uses (getTopLayer, TemplateMatcher.cpp:445-455), so p must carry the search's min_reduce_area. */
int fpm_merge_candidates(const fpm_params* p, int32_t tmpl_w, int32_t tmpl_h, const fpm_candidate* cand, int32_t n,
                         fpm_result* out, int32_t cap, int32_t* n_results);

/* --- pixel operators (L1 kernels exposed for parity tests and standalone use) ----------------------- */
/* cv::pyrDown (8U, 5x5 Gaussian, reflect-101), as called by cv::buildPyramid (TemplateMatcher.cpp:55,124).
 * dst is ((w+1)/2) x ((h+1)/2) with row stride dst_stride. */
int fpm_op_pyr_down(fpm_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, size_t src_stride,
                    uint8_t* dst, size_t dst_stride);
/* Two cv::pyrDown levels in one device launch (the search's pyramid kernel, k_pyr_down2): dst1 = pyrDown(src),
 * dst2 = pyrDown(dst1), each with cv::pyrDown's own reflect-101 border at its level (buildPyramid,
 * TemplateMatcher.cpp:124).  Level 1 is walked in chunks of 16 or 32 rows: chunk_rows 16 or 32 forces that
 * height, 0 lets the kernel choose as the search does (32, or 16 where 32-row chunks would leave CUs idle).
 * seg_chunks > 0 gives each workgroup that many chunks of level 1 (runs that start mid-image, as a multi-source
 * search has them); 0 sizes the grid as the search does. */
int fpm_op_pyr_down2(fpm_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, size_t src_stride,
                     uint8_t* dst1, size_t dst1_stride, uint8_t* dst2, size_t dst2_stride, int32_t seg_chunks,
                     int32_t chunk_rows);
/* 255 - src (the MFC tool's `255 - m_matSrc`, MatchToolDlg.cpp:790) by the kernel a bitwise_not search runs over its
 * staged sources (k_bitwise_not).  dst is w x h with row stride dst_stride. */
int fpm_op_bitwise_not(fpm_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, size_t src_stride,
                       uint8_t* dst, size_t dst_stride);
/* The gray plane fpm_stage_sources_device writes for one image, host in / host out like the other operators (no
 * reference equivalent: match() takes a host cv::Mat, TemplateMatcher.cpp:97-104; the conversion is that of
 * cv::imread(IMREAD_GRAYSCALE), src/MatchToolDialog.cpp:314, 341).  src is copied to device memory byte for byte,
 * keeping its row stride and its address modulo 16, so the kernel (k_stage_gray) takes the path it would take for a
 * device image at that alignment; format, src_stride and plane_stride as fpm_stage_sources_device; invert != 0 gives
 * 255 - gray.  dst is w x h with row stride dst_stride; the bytes between w and dst_stride come back as the kernel
 * left them (untouched). */
int fpm_op_to_gray(fpm_ctx* ctx, const void* src, int32_t w, int32_t h, size_t src_stride, size_t plane_stride,
                   int32_t format, int32_t invert, uint8_t* dst, size_t dst_stride);
/* cv::warpAffine(INTER_LINEAR, BORDER_CONSTANT=border) with forward 2x3 matrix m (row-major), as called at
 * TemplateMatcher.cpp:175 (top layer) and :1089 (getRotatedROI, border 0). */
int fpm_op_warp_affine(fpm_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, size_t src_stride,
                       const double m[6], uint8_t* dst, int32_t dw, int32_t dh, size_t dst_stride,
                       int32_t border);
/* TemplateMatcher::MatchTemplate + CCOEFF_Denominator (TemplateMatcher.cpp:485-598) of `src` against
 * pyramid level `layer` of the learned template.  fold=1 selects the IM_Conv_SIMD per-row float fold
 * (:496-510), fold=0 the TM_CCORR path (:514).  out is (w-tw+1) x (h-th+1) f32, dense. */
int fpm_op_ncc_map(fpm_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, size_t src_stride,
                   int32_t layer, int32_t fold, float* out);
/* filterWithRotatedRect (TemplateMatcher.cpp:1133-1194, with sortPtWithCenter :1093-1131) on n rectangles given as
 * corners[6 i .. 6 i + 5] = ptLT, ptRT, ptRB (cv::RotatedRect(p1, p2, p3), as match() builds them, :380-390) with
 * scores[i], in the caller's order (the reference's: by descending score).  mode 0 runs the host filter, mode 1 the
 * device pair test (k_overlap_pairs, whatever n) with the host replaying its decisions and falling back to the host
 * filter where the device lists cannot hold the pairs -- the two paths of a search's tail.  keep receives the indices
 * of the surviving rectangles in order (*n_keep of them); stats (may be NULL) receives [0] the path taken (0 host,
 * 1 device, 2 device fell back to the host), [1] pairs whose point order the host decided with acos, [2] the device
 * fallback flags (1: a rectangle with more partners than the kernel keeps, 2: the pair list overflowed), [3] the
 * device pair-list entries. */
int fpm_op_overlap_filter(fpm_ctx* ctx, const float* corners, const double* scores, int32_t n, double max_overlap,
                          int32_t mode, int32_t* keep, int32_t* n_keep, int32_t* stats);
/* One refinement layer of the search (TemplateMatcher.cpp:299-328) on ROIs the caller supplies, through the search's
 * own kernels and form selection (k_roi_small for small templates, else k_roi_tables -> k_roi_warp / k_roi_warp3 ->
 * k_roi_corr -> k_roi_eval): for each ROI, getRotatedROI of a level image around a ptLT at an angle, the 7x7 map
 * against pyramid level `layer` of the learned template, and what the search keeps of it. */
typedef struct fpm_roi_record {
    float score;          /* minMaxLoc maximum of the 7x7 map (the first one in row-major order)             */
    int32_t mx, my;       /* its location                                                                    */
    int32_t on_border;    /* bPosOnBorder (TemplateMatcher.cpp:321-322)                                      */
    float vec[9];         /* vecResult[x+1][y+1] at [(x+1)*3 + (y+1)] (:323-328); zeros on the border        */
} fpm_roi_record;
/* levels: `count` level images of w x h (row stride `stride`).  lt: [count][n][2] ptLT (x, y) per candidate in the
 * level's own coordinates (the value the search passes to getRotatedROI, its `lt * 2`; |x|, |y| <= 8192, as w and h:
 * the range of the samplers' 16.16 fixed-point tables).  angles: [count][n][n3] degrees, n3 = 1 or 3.  fold as
 * fpm_op_ncc_map.  round_rois: ROIs per round of launches (a multiple of n3; 0 = all in one round), the search's
 * bounded-scratch rounds.  rec: [count][n][n3].  roi_pixels (may be NULL): [count][n][n3] dense (tw+6) x (th+6) u8
 * sampled ROIs, written where the form materialises them (the k_roi_tables .. k_roi_eval path of a non-constant
 * template; *pixels_written = 1), untouched otherwise (k_roi_small keeps the ROI in LDS; *pixels_written = 0). */
int fpm_op_refine(fpm_ctx* ctx, const uint8_t* const* levels, int32_t count, int32_t w, int32_t h, size_t stride,
                  int32_t layer, const float* lt, const double* angles, int32_t n, int32_t n3, int32_t fold,
                  int32_t round_rois, fpm_roi_record* rec, uint8_t* roi_pixels, int32_t* pixels_written);
/* The search's top-layer peak pass (getNextMaxLoc, TemplateMatcher.cpp:1196-1221, and s_BlockMax, DataStructures.h:
 * 150-246 / MatchToolDlg.h:93-210) on score maps the caller supplies, through the search's own launchers and form
 * selection (launch_nms: k_nms_blocks, k_nms_greedy, k_nms_fast, k_nms; launch_top_greedy).  No learned template is
 * needed; the plan, the staged sources, the last results, the model and the profile counters stay as they were.
 * Additive entry: FPM_ABI_VERSION is unchanged. */
typedef struct fpm_peak {
    int32_t x, y;         /* ptMaxLoc                                                                        */
    float score;          /* dMaxValue                                                                       */
} fpm_peak;
#define FPM_PEAKS_MAX_PIXELS (1 << 26)   /* total pixels of one call's maps */
#define FPM_PEAKS_MAX_SLOTS (1 << 24)    /* n_maps * cap */
#define FPM_PEAKS_STATS_CALL 8           /* call-level stats entries; then FPM_PEAKS_STATS_JOB per map */
#define FPM_PEAKS_STATS_JOB 4
/* maps: n_maps dense f32 maps of mw[i] x mh[i] (1 .. 65535 each way; n_maps <= 65535), one job each, copied to device
 * memory unchanged.  Contract: the maps hold finite values (no NaN, no infinities), as the NCC maps of a search do.
 * tw, th (1 .. 65535), cap (= max_pos + MATCH_CANDIDATE_NUM), by_block, mfc, thr (= vecLayerScore[top]) and overlap
 * (finite, |overlap| <= 16; negative values enlarge the painted rectangle) are the NmsArgs fields of a search.  form 0: the split path (one launch_nms; in block mode with
 * k_nms_blocks' candidate lists and strip scratch).  form 1: the list path of the matrix-core top layer: the op lists
 * each map's pixels with (double)v >= thr and their values, in an order shuffled by list_seed, keeps the first list_cap
 * of them (0 = the engine's capacity: 8192 in block mode, 512 plain; larger values are clamped to it) with the true
 * count, runs launch_top_greedy and then the fallback launch_nms on the maps.  form 1 takes what the search's plan
 * admits to that path: thr > 0.01, overlap >= 0, cap <= 256, at most 12288 coverage cells per map.
 * peaks: [n_maps][cap], the first counts[i] of map i written.  stats (may be NULL): FPM_PEAKS_STATS_CALL +
 * FPM_PEAKS_STATS_JOB * n_maps entries: [0] kernels launched (1 k_nms_blocks, 2 k_nms, 4 k_nms_fast, 8 k_nms_greedy),
 * [1] lds_blocks and [2] cand_lds of the k_nms_fast launch, [3] k_nms_greedy's sort capacity (0: not launched), [4]
 * k_nms carried the LDS of its plain path's block maxima, [5] the list capacity in effect, [6] max_blocks, [7]
 * max_cells; per map [0] pixels with (double)v >= thr (the list's true count), [1] the map's list count read back after
 * the launches (-1: taken by k_nms_greedy; else k_nms_blocks' count in block mode), [2] taken by k_nms_greedy, [3]
 * k_nms's plain form for the map, computed on the host from the kernel's rule (-1 block mode, 0 full scans on little work, 1 block maxima, 2 full scans on a map
 * beyond the block maxima's LDS).  An argument outside these ranges returns FPM_E_INVALID_ARG with nothing launched
 * and nothing written. */
int fpm_op_peaks(fpm_ctx* ctx, const float* const* maps, const int32_t* mw, const int32_t* mh, int32_t n_maps,
                 int32_t tw, int32_t th, int32_t cap, int32_t by_block, int32_t mfc, double thr, double overlap,
                 int32_t form, int32_t list_cap, uint32_t list_seed, fpm_peak* peaks, int32_t* counts,
                 int32_t* stats);
/* The search's own top-layer scoring over every (source, angle) job of the staged batch, and what it computed: the
 * score maps before any peak is taken, or the matrix-core form's candidate lists.  Needs a learned template
 * (FPM_E_NOT_LEARNED) and staged sources (fpm_stage_sources / fpm_stage_sources_device).  The call builds, or reuses,
 * the plan fpm_match_staged would use with the context's parameters, runs the search's pyramid launches and then only
 * the top-layer scoring, with the plan's own job tables, work units, B fragments and launchers (launch_top_mma, the
 * split launchers): no geometry or layout is restated.
 *   form 0  the split chain as the search selects it (k_warp -> k_ncc_tile / k_ncc_map): full maps
 *   form 1  k_top_map (the matrix-core form's mode 1) over every job, the list counts zeroed first so that no job is
 *           skipped: full maps
 *   form 2  k_top_mma (mode 0), the list counts zeroed first: per job the true count of outputs with (double)score >=
 *           thr (it may exceed the capacity) and the first min(count, capacity) (map index y * mw + x, score) pairs, in
 *           no particular order
 * Forms 1 and 2 return FPM_E_SIZE, with nothing launched, where the plan did not admit the matrix-core form (the
 * template level's shape, the parameters or FPM_TOP_MMA=0 keep the search on the other kernels).
 * thr <= 0: the plan's layer score of the top layer.  thr > 0.01: that value instead, for forms 1 and 2 (the list
 * threshold and the prefilter's constant follow it by the plan's own expression).  0 < thr <= 0.01 and a non-finite
 * thr are FPM_E_INVALID_ARG.
 * Sizes.  n_sources, n_angles, map_floats (the dense maps of one source: the sum of mw * mh over the angles) and
 * list_cap (the list capacity in effect) are written by every successful call (each may be NULL).  A call with geom,
 * maps and the three list outputs all NULL is the sizing call: it plans, launches nothing and writes the sizes and
 * stats.
 * Outputs.  geom: [n_angles][4] = bw, bh (the rotated canvas), mw, mh (the map; 0, 0 for an angle the search skips,
 * whose jobs have no map and an empty list); geom_cap = the angles it holds.  maps (forms 0 and 1): [source][angle]
 * dense f32, mw * mh each, n_sources * map_floats in all; maps_cap = the floats it holds.  list_count: [source][angle];
 * list_index, list_value: [source][angle][list_cap]; list_slots = the entries each of the two holds (form 2; list_count
 * holds n_sources * n_angles).  A capacity below the need: FPM_E_CAPACITY, nothing launched.  stats (may be NULL):
 * FPM_TOP_MAPS_STATS entries: [0] the plan admitted the matrix-core form, [1] list capacity, [2] strip width sw, [3]
 * rows per run (the tallest unit), [4] work units, [5] the kernel instantiation launch_top_mma takes (FPM_TOP_FORM_*),
 * [6] the grid of the mode-1 launch, [7] block mode (s_BlockMax peaks); [1] .. [6] are 0 (and [5] -1) without the
 * matrix-core form.
 * State.  FPM_E_INVALID_ARG while a search is in flight, without staged sources, for a form outside 0 .. 2 and for a
 * missing output of the form.  The learned template, the staged sources, the parameters, the last results and
 * candidates, the model and the profile counters stay as they were; a following fpm_match_staged returns what it
 * returns without the call.  Additive entry: FPM_ABI_VERSION is unchanged. */
#define FPM_TOP_MAPS_STATS 8
#define FPM_TOP_FORM_EXACT16 0   /* <8, 32>, template height 16 as a constant  */
#define FPM_TOP_FORM_EXACT14 1   /* <7, 32>, template height 14 as a constant  */
#define FPM_TOP_FORM_SMALL 2     /* <8, 32>, rows past the height masked       */
#define FPM_TOP_FORM_LARGE 3     /* <16, 64>                                   */
int fpm_op_top_maps(fpm_ctx* ctx, int32_t form, double thr, int32_t* n_sources, int32_t* n_angles, int64_t* map_floats,
                    int32_t* list_cap, int32_t* geom, int32_t geom_cap, float* maps, int64_t maps_cap,
                    int32_t* list_count, int32_t* list_index, float* list_value, int64_t list_slots, int32_t* stats);
/* The fused top layer (k_top_fused: the canvas warp, the NCC and the plain getNextMaxLoc loop of one (source, angle) job
 * in one workgroup's LDS) over every job of the staged batch, and what it computed: the peaks of the product kernel,
 * and the score maps before any peak is painted, which only a second, map-writing instantiation of the same source
 * (template parameter DUMP) stores.  Needs a learned template (FPM_E_NOT_LEARNED) and staged sources.  The call builds,
 * or reuses, the plan fpm_match_staged would use with the context's parameters, runs the search's pyramid launches and
 * then launch_top_fused twice on the plan's own job tables and job order, whatever the job count (the search itself
 * takes this form from 256 jobs on, or with FPM_TOP_FUSED=1): first the product instantiation, then the map-writing
 * one, neither with the candidate initialisation.  The threshold is the plan's layer score of the top layer, the
 * overlap the context's max_overlap, the capacity the plan's (max_pos + MATCH_CANDIDATE_NUM): nothing is restated.
 * FPM_E_SIZE, with nothing launched, where the fused form cannot run: block mode (s_BlockMax peaks), a template level
 * beyond k_ncc_tile's form (128 x 64), or a job whose canvas and map need more LDS than stats[2].
 * Sizes.  n_sources, n_angles, map_floats (as fpm_op_top_maps) and cap (peak slots per job) are written by every call
 * that planned (each may be NULL), stats too.  A call with geom, maps and the four peak outputs all NULL is the sizing
 * call: it plans, launches nothing and writes the sizes and stats.
 * Outputs.  geom, geom_cap, maps, maps_cap: as fpm_op_top_maps (the maps are the map-writing launch's; 0 x 0 and no
 * map for an angle the search skips).  peaks: [source][angle][cap], counts: [source][angle], of the product launch;
 * dump_peaks, dump_counts: the same of the map-writing launch.  All four are in/out: their contents are copied to
 * the device before the launches and back after them, so a slot no kernel wrote (every peak slot from counts on)
 * returns as the caller left it.  peak_slots = the entries each of peaks and dump_peaks holds (>= n_sources * n_angles
 * * cap).  A capacity below the need: FPM_E_CAPACITY, nothing launched.  stats (may be NULL): FPM_TOP_FUSED_STATS
 * entries: [0] the dynamic LDS of the launches in bytes (the largest job's need, also where it is refused), [1] the
 * product kernel's static LDS, [2] the dynamic LDS limit (64 KB - [1]), [3] the grid (FPM_GRID_TOP caps it; the jobs
 * loop), [4] jobs, [5] cap, [6] the search itself takes the fused form for this plan, [7] the map-writing kernel's
 * static LDS (equal to [1]; checked once per process), [8] the angles whose jobs sample from an LDS copy of the source
 * level (it lies in the job's map region, so [0] does not grow; 0: no map holds the level and every tap reads global
 * memory), [9] 1 where the product launch takes an f32 bound ahead of the exact score (top template area <= 258, layer
 * score > 0.01, not ResultEqual1).  Neither changes a peak, a count or a map.
 * State.  As fpm_op_top_maps: FPM_E_INVALID_ARG while a search is in flight, without staged sources and for a missing
 * output; the template, the sources, the parameters, the last results and candidates, the model and the profile
 * counters stay as they were; a following fpm_match_staged returns what it returns without the call.  Additive entry:
 * FPM_ABI_VERSION is unchanged. */
#define FPM_TOP_FUSED_STATS 10
int fpm_op_top_fused(fpm_ctx* ctx, int32_t* n_sources, int32_t* n_angles, int64_t* map_floats, int32_t* cap,
                     int32_t* geom, int32_t geom_cap, float* maps, int64_t maps_cap, fpm_peak* peaks, int32_t* counts,
                     fpm_peak* dump_peaks, int32_t* dump_counts, int64_t peak_slots, int32_t* stats);
/* Learned-template introspection: number of pyramid levels, per-level size and statistics
 * (s_TemplData, DataStructures.h:16-55). */
int fpm_template_info(const fpm_ctx* ctx, int32_t* levels, int32_t* border_color);
int fpm_template_level(const fpm_ctx* ctx, int32_t level, int32_t* w, int32_t* h, double* mean,
                       double* norm, double* inv_area, int32_t* result_equal1, uint8_t* pixels,
                       size_t stride);

/* --- instrumentation -------------------------------------------------------------------------------- */
/* Per-search counters of the last fpm_match / fpm_match_staged call (source 0 for staged batches):
 *   [0] top-layer angles  [1] top-layer candidates  [2..2+L-stop) live candidates entering layer L-1..stop
 * (stop = the stop layer: 0, or min(1, L) with fpm_params.stop_layer).  Returns the number of entries written. */
int fpm_search_stats(const fpm_ctx* ctx, int64_t* stats, int32_t cap);
/* SURVEY.md §8(d) algorithmic bytes of the last search, summed over its sources: B_pyr (pyramid in + out), B_top
 * (top-layer level read per angle + the f32 maps), B_ref (per live refinement ROI: the source footprint, the template
 * level and the 7x7 f32 scores).  The roofline's achieved bandwidth is these bytes over the measured time. */
int fpm_search_bytes(const fpm_ctx* ctx, int64_t* b_pyr, int64_t* b_top, int64_t* b_ref);

/* Kernel timing: when enabled, HIP events bracket every launch of each kernel on the context's stream (the
 * search then runs eagerly instead of as a replayed graph); fpm_profile_get returns total milliseconds, launch
 * count and algorithmic bytes (compulsory inputs + outputs, u8 = 1 B, f32 = 4 B) accumulated since the last
 * reset (bytes: each kernel's share of SURVEY.md §8(d)'s per-stage figures, as fpm_search_bytes; intermediate
 * scratch of this design is not counted).  One index per kernel. */
#define FPM_K_PYR 0         /* k_pyr_down     K1 pyrDown                                          */
#define FPM_K_TOP_WARP 1    /* k_warp         K2 top-layer rotation                               */
#define FPM_K_TOP_NCC 2     /* k_top_mma / k_ncc_tile / k_ncc_map  K2-K4 top-layer CCORR + norm.  */
#define FPM_K_TOP_NMS 3     /* k_nms / k_nms_greedy  K5 peak extraction                           */
#define FPM_K_CAND_INIT 4   /* k_cand_init    candidates from the top-layer peaks                 */
#define FPM_K_ROI_TABLES 5  /* k_roi_tables   K6a refinement warp tables + tile descriptors       */
#define FPM_K_ROI_WARP 6    /* k_roi_warp     K6b refinement ROI sampling                         */
#define FPM_K_ROI_CORR 7    /* k_roi_corr     K7 refinement row correlation (i8 MFMA) + windows   */
#define FPM_K_ROI_EVAL 8    /* k_roi_eval     K8 row fold, CCOEFF, argmax, 3x3, candidate step    */
#define FPM_K_ROI_SMALL 9   /* k_roi_small    K6-K8 in one kernel for small templates             */
#define FPM_K_CAND_STEP 10  /* k_cand_step    candidate step after k_roi_small                    */
#define FPM_K_TOP_MAP 11    /* k_top_map: full maps of the jobs the list path left (fallback) */
#define FPM_K_NOT 12        /* k_bitwise_not: 255 - source over the staged level 0 (fpm_params.bitwise_not) */
#define FPM_K_PATCH 13      /* k_patch_warp (or k_warp, fpm_set_patch_form): the patches of fpm_last_patches* / fpm_patches_at;
                               bytes = pixels written + as many source pixels read */
#define FPM_K_COMPARE 14    /* k_patch_compare: the launches of fpm_last_compare / fpm_compare_at (one, or two with
                               FPM_COMPARE_NORMALIZE); bytes = source pixels read + template pixels read + difference
                               pixels written */
#define FPM_K_LEARN 15      /* k_tmpl_prep: the one launch of fpm_learn_device / fpm_learn_at / fpm_learn_hit over all levels;
                               bytes = template pixels read + operand bytes (slack included) and row sums written */
#define FPM_K_COUNT 16
int fpm_profile_enable(fpm_ctx* ctx, int32_t enable);
int fpm_profile_reset(fpm_ctx* ctx);
int fpm_profile_get(const fpm_ctx* ctx, int32_t kernel, double* total_ms, int64_t* launches,
                    int64_t* bytes);
/* Timing of the last fpm_match / fpm_match_staged call (always collected): device_ms = GPU time of the search
 * (events around the whole device pass, results copy included), host_ms = host post-processing after the device
 * pass (reference-order sort, layer-0 decision, filters, conversion), call_ms = wall time of the call. */
int fpm_profile_last(const fpm_ctx* ctx, double* device_ms, double* host_ms, double* call_ms);

#ifdef __cplusplus
}
#endif

#endif /* FPM_H_ */
