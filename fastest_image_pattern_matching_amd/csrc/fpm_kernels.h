// fpm_kernels.h — device job descriptors and kernel launchers (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fpm_geom.h"

namespace fpm {

// K2 / fpm_op_warp_affine: one inverse-mapped bilinear warp (cv::warpAffine INTER_LINEAR, BORDER_CONSTANT).
struct WarpJob {
    const uint8_t* src;
    uint8_t* dst;
    int32_t sw, sh, sp;      // source size, row pitch (bytes)
    int32_t dw, dh, dp;      // destination size, row pitch
    int32_t border;
    int32_t pad;
    double M[6];             // INVERTED matrix (dst -> src)
};

// K3+K4 / fpm_op_ncc_map: full NCC map of an image against one template level.
struct NccJob {
    const uint8_t* img;
    const uint8_t* tmpl;
    float* out;              // dense (ow x oh)
    int32_t iw, ih, ip;
    int32_t tw, th, tp;
    int32_t ow, oh;
    int32_t fold;            // 1: IM_Conv_SIMD per-row float fold; 0: TM_CCORR exact sum -> f32
    int32_t equal1;          // s_TemplData::vecResultEqual1 -> map of ones
    double mean, norm, inv_area;
};

// K5: peak extraction on one top-layer map (plain getNextMaxLoc or s_BlockMax).
struct NmsJob {
    float* map;
    float* bmax;             // s_BlockMax scratch (block mode), nb entries
    int32_t* bloc;
    int32_t mw, mh;
};

struct Peak {
    int32_t x, y;
    float score;
    int32_t pad;
};

struct NmsArgs {
    const NmsJob* jobs;
    Peak* peaks;             // [job][cap]
    int32_t* counts;         // [job]
    int32_t tw, th;          // top template size
    int32_t cap;             // max_pos + MATCH_CANDIDATE_NUM
    int32_t by_block;
    int32_t mfc;             // MFC s_BlockMax semantics (fpm_params.semantics, MatchToolDlg.h:93-210)
    int32_t lds_blocks;      // block-maxima capacity in LDS (set by launch_nms; 0 = global scratch)
    int32_t* cand;           // s_BlockMax mode: indices of the map pixels >= thr, [job][cand_cap] (k_nms_blocks)
    int32_t* cand_cnt;       // [job], zeroed before the launch
    int32_t cand_cap;        // kNmsCandCap
    int32_t cand_lds;        // candidate capacity in LDS (set by launch_nms)
    double thr;              // vecLayerScore[top]
    double overlap;
    uint64_t* stamps;        // profiling only (scripts/nms_probe.hip): k_nms_fast phase cycles of job 0, else null
    uint64_t* skey;          // s_BlockMax mode: [job][3] strip-block maxima keys, zeroed before the launch
    int32_t* sdone;          // [job][3] finished chunks of each strip block, zeroed before the launch
    const float* cand_val;   // k_nms_greedy: the candidates' values (k_top_mma's lists), nullptr = read the map
    int32_t reset_untaken;   // k_nms_greedy: a map it does not take gets cand_cnt = 0 (k_nms_blocks recounts it)
    int32_t greedy_cap;      // k_nms_greedy: sort capacity in LDS (power of 2; 0 = kGreedyMax)
};

// Angle-tree node: the reference's refinement angle for one path, with glibc trig of angle*D2R.
struct AngleNode {
    double angle;
    double c, s;             // cos, sin of (angle * D2R)
    double cn, sn;           // cos, sin of -(angle * D2R)
};

// Top-layer per-angle constants (host-computed, TemplateMatcher.cpp:163-173).
struct TopAngle {
    float tx, ty;            // fTranslationX/Y
    int32_t bw, bh;          // sizeBest
};

struct CandInitArgs {
    const Peak* peaks;
    const int32_t* counts;
    const TopAngle* angles;  // [nang]
    const AngleNode* top_nodes;  // [nang] angle, cos/sin of +-angle*D2R
    CandState* state;        // [cap_total]
    int32_t* live;           // output live list (layer top-1)
    int32_t* live_count;
    int32_t nang, cap;       // per source
    int32_t total;           // sources * nang * cap
    F2 center;               // top-layer ptCenter
    int32_t refine;          // top layer > 0
};

struct RoiArgs {
    const uint8_t* level;    // source pyramid level base (source 0); + src * level_stride
    size_t level_stride;
    int32_t W, H, P;         // level size and pitch
    const uint8_t* tmpl;     // template level
    int32_t tw, th, tp;
    const int8_t* tmpl8;     // template level as i8 (T ^ 0x80), zero beyond tw / th: [round_up(th,16)][tp8]
    int32_t tp8;             // its row pitch (multiple of 64)
    int32_t nk;              // ceil(tw / 64): MFMA k-steps per row
    const int32_t* tsum;     // per template row: sum of T (u8)
    int32_t n3;              // refinement angles per candidate (1 or 3)
    int32_t fold;            // use_simd
    int32_t equal1;
    int32_t per_source;      // candidates per source (nang * cap)
    int32_t slot_base;       // this round covers live ROIs [slot_base, slot_base + slot_cap)
    int32_t slot_cap;
    double mean, norm, inv_area;
    const int32_t* live;
    const int32_t* live_count;
    CandState* state;        // read by the ROI kernels, stepped by k_roi_eval
    const AngleNode* nodes;  // level nodes; child = parent * n3 + j
    int32_t* tab;            // [slot] fixed-point warp tables: ad[tabw], bd[tabw], x0[tabh], y0[tabh]
    int32_t tabw, tabh;
    int4* tdesc;             // [slot][tdesc_stride] per 32x32 ROI tile: source footprint box + flags
    int32_t tdesc_stride;
    uint8_t* roi;            // [slot] sampled ROI, tile-major: 32 x 32 tiles of 1 KB, row of tiles by row
    int32_t roi_pitch;       // LDS row pitch of staged ROI rows (k_roi_corr)
    size_t roi_stride;
    int32_t nparts;          // the fused experiment only (scripts/roi_fused.hip): runs of bands per ROI
    uint32_t* rowsum;        // [slot][th][49] exact int32 per-row dot products
    // the window sums of the normalisation, S(dy, dx) = sum_{t < th} W[t + dy][dx] (W[r][dx]: the sum of I, or of I^2,
    // over the window [dx, dx + tw) of ROI row r), leave k_roi_corr as band totals and edge rows and are rebuilt by
    // k_roi_eval:  S(dy, dx) = sum_bands wtot[band][dx] - sum_{r < dy} W[r][dx] + sum_{r < dy} W[th + r][dx]
    // (integers throughout; holds for every th >= 1, also th < 6 where the head and tail rows overlap)
    uint32_t* wtot;          // [slot][nband][7] sum of W over the band's own template rows 32 band .. 32 band + rb - 1 (I)
    uint64_t* wtotq;         // [slot][nband][7] the same of I^2; nband = ceil(th / 32)
    uint32_t* wedge;         // [slot][2][12][7] W of ROI rows 0 .. 5 (band 0) and th .. th + 5 (the last band): I, then I^2
    RoiRecord* rec;          // [cand * n3 + j]
    // candidate step fused into k_roi_eval (TemplateMatcher.cpp:329-366) when step != 0
    int32_t step;            // 1: best of n3, early break, back-mapping, append to live_out
    int32_t mark_reached0;   // next layer is 0
    int32_t* live_out;
    int32_t* live_out_count;
    double thr;              // vecLayerScore[layer]
    // k_roi_small with prev_rec set (consecutive small layers above layer 0): the previous
    // layer's candidate step runs in each workgroup's prologue (every workgroup of a candidate computes the same
    // stepped state; jj 0 stores it to state_out and counts the survivor in *live_out_count), over the previous
    // layer's live list unchanged -- candidates that died stay in it as holes their workgroups skip.  k_cand_step
    // after the run's last layer compacts the list.  k_cand_step also writes state_out (nullptr = state).
    const RoiRecord* prev_rec;   // the previous layer's records [cand * n3 + j]
    const AngleNode* prev_nodes; // the previous layer's nodes
    double prev_thr;             // vecLayerScore of the previous layer
    int32_t prev_W, prev_H;      // the previous layer's level size
    CandState* state_out;
    // nt_tab != nullptr: the step (k_roi_eval, k_cand_step -> k_cand_step_tab) also writes the next layer's warp tables
    // and tile descriptors for each survivor at its next-list position, so that layer launches no k_roi_tables (the
    // next layer takes tables and runs as one round; tdesc / tdesc_stride / per_source are shared with it)
    int32_t* nt_tab;
    const AngleNode* nt_nodes;   // the next layer's nodes
    int32_t nt_tabw, nt_tabh, nt_tw, nt_th, nt_W, nt_H;
    uint64_t* stamps;        // profiling ablations only (scripts/roi_microbench.hip): per-phase s_memtime stamps
};


// Final pack of a search's results into pinned host memory (replaces several device -> host copies): top-peak
// counts and peaks, live counts, and for the candidates that reached layer 0 (the layer-0 live list) their ids,
// states and refinement records, compacted by live index.
struct PackArgs {
    const int32_t* counts; int32_t J;
    const Peak* peaks; int32_t C;
    int32_t cap;                   // peak slots per job (C == J * cap)
    const int32_t* livecnt; int32_t nlive;
    const int32_t* live0;          // layer-0 live list (nullptr when the top layer is layer 0)
    const int32_t* live0_count;
    const CandState* state;
    const RoiRecord* rec;
    int32_t n3;
    char* host;                    // pinned host buffer
    size_t o_counts, o_peaks, o_live, o_live0, o_state0, o_rec0;
};

// launchers (stream-ordered, no synchronisation)
// seg_chunks > 0 forces that many 32-row chunks per workgroup (the op entry point uses it so single images exercise
// the carried-window path); 0 = sized for the grid
// zero / nzero: as launch_warp (the search's first pyramid launch clears the counters when the top layer's kernel
// also writes the live list)
void launch_pyr_down(const uint8_t* src, int sw, int sh, int sp, size_t s_img, uint8_t* dst, int dw, int dh,
                     int dp, size_t d_img, int nimg, hipStream_t st, int seg_chunks = 0, int32_t* zero = nullptr,
                     int nzero = 0);
// two pyramid levels in one launch: src -> b (level l+1, written) -> c (level l+2); same arguments per level
void launch_pyr_down2(const uint8_t* src, int sw, int sh, int sp, size_t s_img, uint8_t* bdst, int bw, int bh, int bp,
                      size_t b_img, uint8_t* cdst, int cw, int ch, int cp, size_t c_img, int nimg, hipStream_t st,
                      int seg_chunks = 0, int32_t* zero = nullptr, int nzero = 0, int chunk_rows = 0);
// k_bitwise_not: 255 - x in place over the w x h pixels of nimg images (row pitch `pitch`, image stride `img_bytes`; the
// bytes between w and the pitch are left alone).  Needs 16-byte aligned rows (img, pitch and img_bytes multiples of 16,
// as level_layout gives them); returns false, launching nothing, otherwise
bool launch_bitwise_not(uint8_t* img, int w, int h, int pitch, size_t img_bytes, int nimg, hipStream_t st);
// k_stage_gray<FMT, ALIGNED>: the 8-bit gray plane of nimg caller-owned device images (d_imgs: device-side table of
// their base pointers; w x h pixels of `format`, an FPM_FMT_* of include/fpm.h; `stride` bytes between rows,
// `plane_stride` between the planes of a planar format) written to dst + image * img_bytes with row pitch `pitch`:
// exactly the w bytes of each row, the bytes between w and the pitch are left alone.  invert: 255 - gray.
// aligned: every image base, the stride and (planar) the plane stride are multiples of 16, so whole 16-pixel groups
// load as 16-byte words; otherwise the general form runs (aligned dwords + byte alignment, any base and stride).
// Needs 16-byte aligned destination rows, as launch_bitwise_not; returns false, launching nothing, otherwise or on an
// unknown format
bool launch_stage_gray(const uint8_t* const* d_imgs, int nimg, int w, int h, size_t stride, size_t plane_stride,
                       int format, bool aligned, uint8_t* dst, int pitch, size_t img_bytes, bool invert,
                       hipStream_t st);
int stage_gray_bpp(int format);   // bytes per pixel within a row (1 for the planar formats); 0 = unknown format
// zero / nzero: counters the search zeroes before its later kernels use them (block (0, 0) clears them), so the
// graph carries no memset nodes
void launch_warp(const WarpJob* jobs, int njobs, int max_pixels, hipStream_t st, int32_t* zero = nullptr,
                 int nzero = 0);
// ---- match patches (fpm_last_patches / fpm_patches_at): upright crops of level 0 of the staged
// sources, all of one size, one launch for all of them.  One descriptor per patch, built on the host.
struct PatchJob {
    double M[6];             // INVERTED matrix (patch -> source)
    int64_t out_off;         // byte offset of the patch's first pixel from PatchArgs::out
    int32_t src;             // source index in the slab
    int32_t pad;
};
struct PatchArgs {
    const PatchJob* jobs;
    int32_t njobs;
    const uint8_t* level0;   // level 0 of source 0; + src * img_stride
    size_t img_stride;
    int32_t sw, sh, sp;      // source size and row pitch (>= sw + 4: aligned dword reads of a footprint stay in the row)
    uint8_t* out;
    size_t row_stride;       // bytes between the rows of a patch
    int32_t pw, ph;          // patch size
    int32_t dword;           // out, row_stride and every out_off are multiples of 4: whole groups of 4 pixels are stored
                             // as dwords (bytes otherwise)
    int32_t tiles_x, tiles_y;   // 64 x 16 output tiles per patch (set by launch_patch_warp)
};
// k_patch_warp: one workgroup per 64 x 16 output tile.  Returns false, launching nothing, when the grid would exceed
// 2^31 - 1 workgroups.
bool launch_patch_warp(PatchArgs a, hipStream_t st);
// ---- patch comparison (fpm_last_compare / fpm_compare_at): the patches of a job table against
// the template pixels beneath them, reduced to one record per patch; the patch itself is never written.
// The fields a workgroup reduces, in the order of its LDS partials: sums first, then maxima.
enum { kCmpSumI, kCmpSumII, kCmpSumT, kCmpSumTT, kCmpSumIT, kCmpSumAbs, kCmpNOver, kCmpMaxAbs, kCmpX0, kCmpY0, kCmpX1,
       kCmpY1, kCompareFields };
// One record per patch, zero-filled before the launch.  m = n_over, max_abs, then the box of the pixels over the
// threshold as maxima: pw - x0, ph - y0, x1 + 1, y1 + 1 (all 0 = no such pixel).
struct CompareAcc {
    uint64_t s[6];           // kCmpSumI .. kCmpSumAbs
    uint32_t m[6];           // kCmpNOver .. kCmpY1
};
struct CompareArgs {
    PatchArgs p;             // jobs, sources and patch size as for k_patch_warp; out = the difference images or null
    const uint8_t* tmpl;     // template level 0, row pitch tp (a multiple of 64)
    int32_t tp;
    int32_t rx, ry;          // the rectangle's origin in the template (the rectangle lies inside it)
    int32_t threshold;       // a pixel counts as deviating when d > threshold
    const uint8_t* luts;     // [njobs][256] (kCompareDevLut), 4-byte aligned
    CompareAcc* acc;         // [njobs]
    const uint8_t* mask;     // the template mask plane (0x00 / 0xFF, the template's pitch tp) or null: the MASK forms
};
// the launches of a comparison: everything at once without a table; or the sums, then (the host having built the
// tables from them) the deviations through the tables
enum { kCompareRaw, kCompareSums, kCompareDevLut };
// k_patch_compare, k_patch_warp's grid.  Returns false, launching nothing, for a grid past 2^31 - 1 or an unknown form.
bool launch_patch_compare(CompareArgs c, int form, hipStream_t st);
// ---- variation model (fpm_model_* / fpm_last_inspect / fpm_inspect_at): the patches of a job table
// summed per pixel into two u32 planes, the planes turned into u8 mean / lo / hi planes, and patches held against lo / hi.
struct ModelAccumArgs {
    PatchArgs p;             // jobs, sources and patch size as for k_patch_warp; out unused
    uint32_t* sum;           // dense pw x ph planes: sum v and sum v^2 over the samples
    uint32_t* sum_sq;
    const uint8_t* luts;     // [njobs][256] (normalised training), 4-byte aligned; null = the pixels as sampled
    int32_t chunk;           // consecutive jobs per workgroup (set by launch_model_accum from its argument)
    int32_t nchunks;         // ceil(njobs / chunk); 1: one owner per pixel, plain adds; else atomic adds
};
// k_model_accum: one workgroup per (chunk of jobs, 64 x 16 tile).  chunk 1 .. njobs.  Returns false, launching
// nothing, for a bad chunk or a grid past 2^31 - 1.
bool launch_model_accum(ModelAccumArgs m, int chunk, hipStream_t st);
struct ModelPrepareArgs {
    const uint32_t* sum;     // dense w x h
    const uint32_t* sum_sq;
    int32_t w, h, n;         // n = samples, 1 .. 65535
    int32_t a, kq;           // absolute threshold 0 .. 255; sigma multiple in sixteenths 0 .. 255
    uint8_t* mean;           // each may be null; rows pitch bytes apart
    uint8_t* lo;
    uint8_t* hi;
    int32_t pitch;
};
void launch_model_prepare(const ModelPrepareArgs& a, hipStream_t st);
// The fields a workgroup of k_model_inspect reduces, and the hit's record (zero-filled before the launch): sums first,
// then maxima; the box of the pixels outside their interval is kept as CompareAcc keeps its own.
enum { kInsSumExcess, kInsNLow, kInsNHigh, kInsMaxExcess, kInsX0, kInsY0, kInsX1, kInsY1, kInspectFields };
struct InspectAcc {
    uint32_t f[kInspectFields];   // sum_excess <= 2^22 * 255 fits
};
struct InspectArgs {
    PatchArgs p;             // out = the excess images or null
    const uint8_t* lo;       // the model's planes in rectangle coordinates, row pitch mp (>= pw + 4, a multiple of 64)
    const uint8_t* hi;
    int32_t mp;
    const uint8_t* luts;     // [njobs][256] or null
    InspectAcc* acc;         // [njobs]
    const uint8_t* mask;     // the template mask plane (0x00 / 0xFF, row pitch mkp) or null: the MASK forms
    int32_t mkp;
    int32_t mx, my;          // the model rectangle's origin in the template, where the mask lives
};
// k_model_inspect, k_patch_warp's grid; the table form when luts is set.  Returns false for a grid past 2^31 - 1.
bool launch_model_inspect(InspectArgs c, hipStream_t st);
// ---- pose alignment (fpm_align_*): the patches of a job table against the template and its
// central-difference gradient beneath them, reduced to the eleven exact sums of one Gauss-Newton step per patch.
// The record's fields, in fpm_align_sums' order; signed ones are kept in two's complement.
enum { kAlnN, kAlnHxx, kAlnHxy, kAlnHyy, kAlnHxt, kAlnHyt, kAlnHtt, kAlnGx, kAlnGy, kAlnGt, kAlnSsd, kAlignFields };
constexpr int kAlignMaxSide = 4096;             // with the area cap every sum stays below 2^62 (include/fpm.h)
constexpr int64_t kAlignMaxArea = (int64_t)1 << 20;
struct AlignAcc {
    uint64_t f[kAlignFields];   // zero-filled before the launch
};
struct AlignArgs {
    PatchArgs p;             // jobs, sources and patch size as for k_patch_warp; out unused
    const uint8_t* tmpl;     // template level 0, row pitch tp (a multiple of 64, >= tw + 4)
    int32_t tp;
    int32_t tw, th;          // the template's size: the gradient is read from all of it, not only from the rectangle
    int32_t rx, ry;          // the rectangle's origin in the template (the rectangle lies inside it)
    const uint8_t* luts;     // [njobs][256] or null
    AlignAcc* acc;           // [njobs]
    const uint8_t* mask;     // the template mask plane (0x00 / 0xFF, the template's pitch tp) or null: the MASK forms
};
// k_patch_align, k_patch_warp's grid; the table form when luts is set.  Returns false, launching nothing, for a grid past
// 2^31 - 1 or a rectangle beyond the caps.
bool launch_patch_align(AlignArgs c, hipStream_t st);
// ---- template masks (fpm_mask_*).  k_mask_stage: the w x h bytes at src (`stride` bytes between
// rows, any base alignment; device-readable memory) normalised to 0x00 / 0xFF into dst with row pitch `pitch`, a
// multiple of 64: whole 16-byte groups are stored, zero behind a row's end.  *count (device, zeroed by the caller)
// receives the number of used pixels.  Returns false, launching nothing, for a misaligned plane or more than 2^31 pixels.
bool launch_mask_stage(const uint8_t* src, int w, int h, size_t stride, uint8_t* dst, int pitch,
                       unsigned long long* count, hipStream_t st);
// ---- edge calipers (fpm_last_calipers / fpm_calipers_at): one L x W patch per (hit, caliper), each
// of its own size, summed across its width into a profile of L integers that never leaves LDS, then the step filter,
// the local-maximum test and an ordered compaction of the edges.  One descriptor per job, built on the host.
constexpr int kCaliperMaxLength = 1024, kCaliperMaxWidth = 256, kCaliperMaxHalf = 16, kCaliperMaxCap = 64;
struct CaliperJob {
    PatchJob p;              // the inverted matrix and the source, as for k_patch_warp; out_off = the job's first record
                             // (in records) from CaliperArgs::edges
    int32_t L, W, s;         // length, width, half
    int32_t thr;             // c s W: the least |D| of an edge
    int32_t polarity;        // +1, -1, 0 = both
    int32_t pad;
    int64_t prof_off;        // the job's first profile entry (in entries) from CaliperArgs::profiles
};
struct CaliperArgs {
    const CaliperJob* jobs;
    int32_t njobs;
    const uint8_t* level0;   // as PatchArgs
    size_t img_stride;
    int32_t sw, sh, sp;
    int32_t cap;             // records per job, 1 .. kCaliperMaxCap
    int32_t prof_stride;     // entries per job of profiles: those from L on are written as 0
    int4* edges;             // [njobs][cap]: index, d_prev, d, d_next; those behind the count written as 0
    int32_t* counts;         // [njobs]: the true count
    int32_t* profiles;       // [njobs][prof_stride] or null
};
// k_caliper: one workgroup per job.  Returns false, launching nothing, for a capacity outside its range.
bool launch_caliper(const CaliperArgs& a, hipStream_t st);
// ---- edge probes (fpm_last_probes / fpm_probes_at): thousands of short calipers per hit that
// share one size and one set of rules and report one edge each.  The job table is one PatchJob head per hit (the
// inverted matrix of the template frame and the source) and one ProbeFrame per probe; k_probe composes the two.
constexpr int kProbeMaxLength = 64, kProbeMaxWidth = 16, kProbeMaxHalf = 8, kProbeMax = 4096;
constexpr int kProbeOutside = 1;                      // FPM_PROBE_OUTSIDE
enum { kProbeNearest, kProbeStrongest, kProbeFirst, kProbeLast };   // FPM_PROBE_NEAREST ..
struct ProbeFrame {
    double cp, sp;           // cos and sin of the scan direction
    double ox, oy;           // the template point of sample (0, 0)
};
struct ProbeRaw {            // fpm_probe_raw, field for field
    int32_t index, n_edges, d_prev, d, d_next, flags;
};
struct ProbeArgs {
    const PatchJob* jobs;    // [njobs]: one head per hit; out_off unused (hit h's records start at h * n_probes)
    int32_t njobs;           // hits
    const uint8_t* level0;   // as PatchArgs
    size_t img_stride;
    int32_t sw, sh, sp;
    const ProbeFrame* frames;   // [n_probes]
    int32_t n_probes;
    int32_t L, W, s;         // length, width, half
    int32_t thr;             // c s W: the least |D| of an edge
    int32_t polarity;        // +1, -1, 0 = both
    int32_t select;          // kProbeNearest ..
    ProbeRaw* records;       // [njobs][n_probes]
    int32_t* profiles;       // [njobs][n_probes][L] or null
};
// k_probe: one wave per (hit, probe), four probes of a hit per workgroup.  Returns false, launching nothing, for a
// parameter outside its range, a null output or a grid past 2^31 - 1.
bool launch_probe(const ProbeArgs& a, hipStream_t st);
// ---- gray-value tools (fpm_last_histogram / fpm_histogram_at / fpm_last_segment / fpm_segment_at, DESIGN.md section
// 23): the 256-bin histogram of a (hit, rectangle) patch that is never written, and the patch thresholded into the u8
// image e that the labelling kernels take.  One descriptor per job serves both kernels, built on the host.
struct GrayJob {
    PatchJob p;              // the inverted matrix and the source, as for k_patch_warp; out_off = byte offset of the job's
                             // e image from GrayArgs::out (k_patch_threshold)
    int32_t pw, ph;          // the rectangle's size
    int32_t rx, ry;          // and its origin in the template, where the mask lives
    int64_t hist_off;        // the job's first histogram word (in words) from GrayArgs::hist
    int32_t wg0;             // k_patch_hist: the job's first workgroup; ascending over the table, jobs[0].wg0 = 0
    int32_t t;               // k_patch_threshold: the threshold 0 .. 255
    int32_t polarity;        // +1: e = I - t where I > t; -1: e = t - I where I < t; 0: e = 0 (no foreground)
    int32_t pad;
};
struct GrayArgs {
    const GrayJob* jobs;
    int32_t njobs;
    const uint8_t* level0;   // as PatchArgs
    size_t img_stride;
    int32_t sw, sh, sp;
    const uint8_t* mask;     // the template mask plane (0x00 / 0xFF, row pitch mkp, a multiple of 64) or null: the MASK forms
    int32_t mkp;
    uint32_t* hist;          // k_patch_hist: [..][256], zero-filled before the launch
    int32_t run;             // k_patch_hist: consecutive tiles of one job per workgroup, >= 1
    int32_t grid;            // k_patch_hist: workgroups = the sum over the jobs of ceil(tiles / run)
    uint8_t* out;            // k_patch_threshold: the e images, rows row_stride apart, all of pw x ph
    size_t row_stride;
    int32_t pw, ph;
    int32_t dword;           // as PatchArgs
    int32_t tiles_x, tiles_y;   // set by launch_patch_threshold
};
// k_patch_hist: one workgroup per run of tiles of one job.  Returns false, launching nothing, for a run or grid below 1.
bool launch_patch_hist(const GrayArgs& a, hipStream_t st);
// k_patch_threshold: k_patch_warp's grid over jobs of one size.  Returns false for a grid past 2^31 - 1.
bool launch_patch_threshold(GrayArgs a, hipStream_t st);
// ---- sub-pattern locators (fpm_last_locate / fpm_locate_at): the window of a (hit, feature) job
// sampled into LDS, correlated there with the feature's template region at every offset of the search range, reduced to
// the peak's record.  One descriptor per job, built on the host.
constexpr int kLocateMaxSide = 128, kLocateMaxRadius = 16;
constexpr int kLocateWords = 40;   // an fpm_locate_raw in dwords
struct LocateJob {
    PatchJob p;              // the inverted matrix of the WINDOW rectangle and the source, as for k_patch_warp; out_off unused
    int32_t x, y, w, h;      // the feature's region in the template (inside it), w, h 1 .. kLocateMaxSide
    int32_t rx, ry;          // radii 0 .. kLocateMaxRadius
    int32_t bands;           // row bands an offset's S_it is cut into, 1 .. h (speed only: integer sums)
    int32_t pad;
};
struct LocateArgs {
    const LocateJob* jobs;
    int32_t njobs;
    const uint8_t* level0;   // as PatchArgs
    size_t img_stride;
    int32_t sw, sh, sp;
    const uint8_t* tmpl;     // template level 0, row pitch tp (a multiple of 64)
    int32_t tp;
    int32_t* raw;            // [njobs][kLocateWords]: fpm_locate_raw records
    int32_t* maps;           // [njobs][3][map_stride] or null
    int32_t map_stride;
};
// k_patch_locate: one workgroup per job.  Returns false, launching nothing, without a record buffer.
bool launch_patch_locate(const LocateArgs& a, hipStream_t st);
// ---- defect blobs on the device (fpm_last_blobs / fpm_blobs_at / fpm_op_blobs): connected
// components of n pitched u8 images of one size, by a union-find per 64 x 16 tile in LDS and a merge of the tile pieces
// in device memory.  A label is the row-major index v * w + u, within its image, of a pixel of the same component that is
// not larger than the pixel's own; after k_blob_flatten it is the component's seed.
// The device record: fpm_blob, field for field (the engine asserts the offsets).
struct BlobRec {
    int32_t hit, seed, area, x0, y0, x1, y1, max_value;
    unsigned long long sum_value, sum_x, sum_y;   // 64-bit integer atomic adds
};
static_assert(sizeof(BlobRec) == 56, "the device record is fpm_blob, field for field");
// Per image, zero-filled before the launches: foreground pixels, all components, the components of at least min_area
// pixels (the true count, also when it exceeds cap_dev) and the largest area.
struct BlobCount {
    int32_t fg, comps, qual, largest;
};
struct BlobArgs {
    const uint8_t* img;      // image i at img + i * img_stride, rows pitch bytes apart; pitch is a multiple of 64, so a
    size_t pitch;            // tile's dwords lie inside the row.  The bytes at u >= w are NOT clean: masked by u < w
    size_t img_stride;
    int32_t n, w, h;         // images of this round; w * h <= 2^22
    int32_t tiles_x, tiles_y;   // 64 x 16 tiles per image (set by the launchers)
    int32_t level;           // foreground: e > level
    int32_t conn8;           // 1: 8-connectivity, 0: 4-connectivity
    int32_t min_area;
    int32_t cap_dev;         // record slots per image
    int32_t hit0;            // BlobRec::hit of image 0 of the round
    int32_t* L;              // labels, dense [n][h][w]; -1 = background
    int32_t* A;              // areas at the roots after k_blob_flatten; the slot (or -1) at the roots after k_blob_slots
    BlobCount* cnt;          // [n]
    BlobRec* rec;            // [n][cap_dev], zero-filled before the launches
};
// One launch each, in this order, on one stream: the kernel boundaries publish the labels.  Every launcher returns
// false, launching nothing, for a grid past 2^31 - 1.
bool launch_blob_tile(BlobArgs a, hipStream_t st);
bool launch_blob_merge(BlobArgs a, hipStream_t st);
bool launch_blob_flatten(const BlobArgs& a, hipStream_t st);
bool launch_blob_slots(const BlobArgs& a, hipStream_t st);
bool launch_blob_features(const BlobArgs& a, hipStream_t st);
// ---- learning on the device (fpm_learn_device / fpm_learn_at / fpm_learn_hit): what learnPattern
// derives from a template pyramid that already lies in the template slab, in one launch over all its levels.
constexpr int kTmplPrepMaxLevels = 16;   // a 2^26-pixel template at min_reduce_area 1 has 13 levels above level 0
struct TmplPrepLevel {
    uint32_t off, off8;      // byte offsets of the level in the template slab and in the i8 operand slab
    uint32_t tsum_off;       // element offset of its row sums
    int32_t w, h;
    int32_t pitch, p8;       // row pitches: the slab's (round_up(w + 4, 64)) and the operand's (64 * ceil(w / 64) <= pitch)
    int32_t chunk0;          // the level's first workgroup; it has round_up(h, kMmaRows) / kMmaRows of them
};
struct TmplPrepArgs {
    const uint8_t* tmpl;     // the template slab
    int8_t* tmpl8;           // i8 operand slab: T ^ 0x80 at x < w, y < h, 0 in every other byte of [0, o8)
    int32_t* tsum;           // per-row sums of T, 0 for the rows h .. round_up(h, kMmaRows) - 1
    uint64_t* acc;           // [nlv][2] exact sum of T and of T^2 per level (integer atomics), zeroed before the launch
    uint32_t slack_off;      // the 256 bytes behind the last level (k_roi_corr's prefetch), zeroed by workgroup 0
    int32_t nlv, nchunks;
    TmplPrepLevel lv[kTmplPrepMaxLevels];
};
// k_tmpl_prep: one workgroup per (level, kMmaRows-row chunk).  Returns false, launching nothing, for a level table the
// kernel's 16-byte accesses do not fit (offsets and pitches are multiples of 16 in the engine's layouts, p8 <= pitch).
bool launch_tmpl_prep(const TmplPrepArgs& a, hipStream_t st);
void launch_ncc_map(const NccJob* jobs, int njobs, int max_out, int tmpl_bytes, hipStream_t st);
bool ncc_tile_fits(int tw, int th);   // LDS-tiled variant applies (templates up to 128 x 64)
void launch_ncc_tile(const NccJob* jobs, int njobs, int max_ow, int max_oh, int tw, int th, hipStream_t st);
constexpr int kNmsCandCap = 8192;   // s_BlockMax candidates (pixels >= the top-layer score) kept per map
// max_blocks: s_BlockMax blocks of the largest map (block mode); max_map_dim: largest map width or height
// max_cells: the largest ceil(mw / tw) * ceil(mh / th) over the maps (k_nms_greedy's coverage cells)
// max_items: the largest nms_block_items of the maps (k_nms_blocks' grid: strip blocks are scanned in chunks)
// ci (plain getNextMaxLoc path only, cap <= kNmsInitCap): k_nms also does k_cand_init's work for its job's
// candidate slots (one launch fewer); the live counter must have been zeroed by an earlier launch
constexpr int kNmsInitCap = 128;
// what a peak launcher decided (fpm_op_peaks reports it; the search passes null)
enum { kNmsRanBlocks = 1, kNmsRanNms = 2, kNmsRanFast = 4, kNmsRanGreedy = 8 };
struct NmsLaunchInfo {
    uint32_t kernels;        // kNmsRan* of the kernels launched
    int32_t lds_blocks;      // NmsArgs::lds_blocks of the k_nms_fast / k_nms launch
    int32_t cand_lds;        // NmsArgs::cand_lds of the k_nms_fast launch
    int32_t greedy_cap;      // k_nms_greedy's sort capacity (0: not launched)
    int32_t blk_lds;         // k_nms carried the LDS of its plain path's block maxima
};
// max_map_px: the largest map's pixel count (sizes k_nms's dynamic LDS; -1 = unknown)
void launch_nms(const NmsArgs& a, int njobs, int max_blocks, int max_map_dim, int max_cells, hipStream_t st,
                int max_items = 0, const CandInitArgs* ci = nullptr, long max_map_px = -1,
                NmsLaunchInfo* info = nullptr);
int nms_block_items(int mw, int mh, int tw, int th, int mfc);
// the launch maxima of launch_nms / launch_top_greedy over a set of top-layer maps (0 x 0: a map that does not exist)
struct NmsMaxima {
    int max_blocks = 0, max_map_dim = 0, max_cells = 0, max_items = 0;
    long max_map_px = 0;
};
// adds one map; returns its s_BlockMax block count (0 in plain mode)
int nms_maxima_add(NmsMaxima& m, int mw, int mh, int tw, int th, int by_block, int mfc);
// k_nms's plain path on a map of n pixels: 0 = full-map scans (little work), 1 = 64-pixel block maxima in LDS,
// 2 = full-map scans (more blocks than the LDS holds); blk_lds as NmsLaunchInfo
int nms_plain_form(int blk_lds, int cap, long n);
void launch_cand_init(const CandInitArgs& a, hipStream_t st);
// K2-K5 fused for small canvases (plain peak path): LDS bytes of one (source, angle) job, and the launch (one
// workgroup per job; zero / nzero as launch_warp)
size_t top_fused_lds(int bw, int bh, int tw, int th);
size_t top_fused_lds_limit();   // 64 KB minus k_top_fused's static LDS (hipFuncGetAttributes, per device)
constexpr int kTopFusedMinJobs = 256;   // fewer jobs than CUs: the three split kernels finish sooner
// What the host decides per launch of k_top_fused (the engine's plan_top_fused_opts).
struct TopFusedOpts {
    int32_t level_copy;      // 1: a job whose map region holds it samples from an LDS copy of its source level
    int32_t bound;           // 1: f32 bound before the exact f64 score (product instantiation only; area <= 258,
                             //    thr > 0.01, not equal1: k_top_mma's conditions)
    float thrK, E;           // the bound's constants, as TopMmaArgs::thrK / E (top_mma_thresholds)
    uint32_t tsum, area;     // sum of the template level's pixels, tw * th
};
// The LDS copy of a sw x sh source level holds horizontal pixel pairs: u16 entry [y + 1][x + 1] = pixel (x, y) | pixel
// (x + 1, y) << 8 for x in [-1, sw - 1], y in [-1, sh], the border value wherever a pixel lies outside the level.  Its
// row pitch in entries (a multiple of 4: four entries are staged per item) and its size in bytes
constexpr int top_fused_level_pitch(int sw) { return (sw + 1 + 3) & ~3; }
constexpr size_t top_fused_level_bytes(int sw, int sh) { return 2 * (size_t)top_fused_level_pitch(sw) * (size_t)(sh + 2); }
// whether a job with an ow x oh map samples from the copy: it lies in the map's LDS, which nothing else uses until the
// canvas is complete, so the copy adds nothing to the job's LDS (host and kernel decide by this one function)
constexpr bool top_fused_level_fits(int sw, int sh, int ow, int oh) {
    return ow > 0 && oh > 0 && top_fused_level_bytes(sw, sh) <= 4 * (size_t)ow * (size_t)oh;
}
// ci (cap <= kNmsInitCap): the candidate init fused as in k_nms; the live counter must be zero before the launch
// (zero / nzero are then 0: block 0's clearing would race with the other blocks' atomics)
// order (optional): the job each workgroup takes, costliest angles first (fewer workgroups than resident slots are
// left for the last round)
// dump: the map-writing instantiation (fpm_op_top_fused): every job's LDS map, unpainted, also goes to NccJob::out; the
// search passes false.  top_fused_static_lds: the kernel's static LDS as compiled (0 if the query fails)
// opts: the level copy and the bound (TopFusedOpts)
void launch_top_fused(const WarpJob* wjobs, const NccJob* njobs, const NmsArgs& a, int njobs_n, size_t lds,
                      int32_t* zero, int nzero, hipStream_t st, const CandInitArgs* ci, const int32_t* order,
                      bool dump, const TopFusedOpts& opts);
size_t top_fused_static_lds(bool dump);
int top_fused_grid(int njobs_n);   // the workgroups launch_top_fused starts for njobs_n jobs (FPM_GRID_TOP)
// ---- the top layer on the matrix cores (k_top_mma): warp + TM_CCORR + CCOEFF_Denominator for every (source, angle)
// job without materialising the rotated canvas or the map.  Work unit = (job, strip of output columns, run of output
// rows); the host builds the unit list (top_mma_plan).
struct TopUnit { int32_t job, x0, y0, y1; };
constexpr int kTopMmaMaxSw = 192;              // strip width cap (output columns)   // output columns [x0, x0 + sw) and rows [y0, y1) of map `job`
struct TopMmaArgs {
    const WarpJob* wjobs;    // per job: source level, canvas size (dw x dh), inverse matrix, border
    const NccJob* njobs;     // per job: map size (ow x oh) and, for mode 1, the map
    const TopUnit* units;
    int32_t nunits;
    const uint8_t* bfrag;    // [nq][64 lanes][16 B] the correlation's B fragments (T - 128 as i8, Toeplitz-banded)
    int32_t nq, R;           // MFMA slots per 16 x 16 output tile; template rows per slot (2: tw <= 17, 1: tw <= 49)
    int32_t tw, th, area;
    uint32_t tsum;           // sum of the template level's pixels
    int32_t sw;              // strip width (output columns, multiple of 16)
    int32_t cp;              // canvas ring row pitch (bytes; the kernel's compile-time TM_CP)
    int32_t rr;              // ring rows per plane (power of two >= 16 + th - 1; the kernel form's RR)
    int32_t ct, rt;          // column / row table capacity (entries)
    int32_t o_colt, o_rowt, o_bf, o_ft;   // dynamic LDS offsets (bytes)
    int32_t nqm;             // B slots staged in LDS (the kernel form's unrolled slot count; zero past nq)
    int32_t mode;            // 0: candidate lists, 1: full maps of the jobs with cand_cnt >= 0 (fallback)
    int32_t prefilter;       // 1: f32 bound before the exact f64 score (area <= 258, thr > 0)
    float thrK, E;           // prefilter: (thr (1 - 1e-5))^2 * norm^2 * area, absolute slack of the f32 terms
    double thr, mean, norm, inv_area;
    int32_t* cand;           // [job][cand_cap] map indices of the outputs with score >= thr
    float* cand_val;         // [job][cand_cap] their scores
    int32_t* cand_cnt;       // [job] (zeroed before mode 0; may exceed cand_cap)
    int32_t cand_cap;
};
size_t top_mma_lds(const TopMmaArgs& a);
// fills the layout fields of `a` (sw, cp, rr, hp, ct, rt, o_*) for a strip width and the largest unit height
void top_mma_layout(TopMmaArgs& a, int sw, int max_rows);
bool top_mma_fits(int tw, int th);   // template shapes the kernel takes (R = 2 up to 17 wide, R = 1 up to 49)
void launch_top_mma(const TopMmaArgs& a, hipStream_t st);
// what launch_top_mma takes for `a`: the kernel instantiation (FPM_TOP_FORM_* of include/fpm.h) and the grid of a.mode
enum { kTopFormExact16 = 0, kTopFormExact14 = 1, kTopFormSmall = 2, kTopFormLarge = 3 };
int top_mma_form(const TopMmaArgs& a);
int top_mma_grid(const TopMmaArgs& a);
// k_nms_greedy over k_top_mma's lists (a.cand_val set): plain getNextMaxLoc key (by_block 0) or s_BlockMax key; with ci
// (plain, cap <= kNmsInitCap) the candidate init of the jobs it takes.  Needs a.overlap >= 0, as every use of the greedy
// form (its cell lists hold a rectangle of at most twice the template): plan_top_mma keeps other searches off this path
void launch_top_greedy(const NmsArgs& a, int njobs, int max_cells, hipStream_t st, const CandInitArgs* ci,
                       NmsLaunchInfo* info = nullptr);
void launch_roi_tables(const RoiArgs& a, hipStream_t st);
void launch_roi_warp(const RoiArgs& a, hipStream_t st);
void launch_roi_corr(const RoiArgs& a, hipStream_t st);
void launch_roi_eval(const RoiArgs& a, hipStream_t st);
bool roi_small_fits(int tw, int th);   // the single-kernel small-template refinement applies
size_t roi_small_lds(int tw, int th);
void launch_roi_small(const RoiArgs& a, hipStream_t st);
void launch_cand_step(const RoiArgs& a, int max_items, hipStream_t st);
void launch_pack(const PackArgs& a, hipStream_t st);

// ---- filterWithRotatedRect's pair decisions on the device (TemplateMatcher.cpp:1133-1194) ----
// One result's rotated rectangle: its corners (rrect corners, host-computed from the cv::RotatedRect) and size; its
// corner box widened by 1 px (the host's prefilter: boxes farther apart cannot intersect) in a separate float4 array
// (x0, y0, x1, y1), which the all-pairs sweep reads.
struct OvRect { F2 c[4]; float w, h; };
constexpr int kOverlapMaxCand = 512;   // overlapping partners of one rectangle decided on the device
// For every pair i < j of the n rectangles (sorted as the filter sees them) whose boxes overlap, the exact
// rotatedRectangleIntersection + sortPtWithCenter + area test (fpm_rrect.h); the j of every pair whose overlap
// exceeds max_overlap are written, ascending, to lists[off[i] .. off[i] + cnt[i]) (offcnt[2i], offcnt[2i+1]), as ~j
// when the point order depends on acos (the host decides that pair).  meta[0] = entries written (atomic allocator,
// zeroed by the caller), meta[1] bit 0 = more than kOverlapMaxCand overlapping partners, bit 1 = list full.
// lists / offcnt may be mapped host memory (plain stores only); meta must be device memory.
void launch_overlap_pairs(const OvRect* r, const float4* box, int n, double max_overlap, int32_t* lists, int list_cap,
                          int32_t* offcnt, int32_t* meta, hipStream_t st);
int roi_pitch_for(int tw);
int roi_tab_rows(int th);   // rows of a ROI's X0 / Y0 tables: th + 6 rounded up to a 32-row tile
size_t roi_tiles_bytes(int tw, int th);
int roi_tiles_for(int tw, int th);   // 32x32 warp tiles of a (tw+6) x (th+6) ROI
size_t roi_corr_lds(int roi_pitch);
constexpr int kRoiEdgeWords = 2 * 12 * 7;   // RoiArgs::wedge per slot
int roi_bands(int th);                       // k_roi_corr's bands of template rows (RoiArgs::wtot / wtotq per slot: x 7)
constexpr int kMmaRows = 16;   // template rows per MFMA correlation chunk (M of v_mfma_i32_16x16x64_i8)

}  // namespace fpm
