// fpm_engine.hip — host orchestration of the MI355X template matcher and the C ABI (include/fpm.h).
//
// Mirrors TemplateMatcher::learnPattern / match (src/TemplateMatcher.cpp:45-437) with this split:
//   host, once per (template, params, source size):  angle list (:130-144), per-angle canvas size and
//       warp matrix (:163-173, :901-969), refinement angle tree with glibc cos/sin (:282-298), buffer layout;
//   device, per search (one stream, no host sync until the end):  pyramid (K1), top-layer rotation + NCC +
//       peak extraction for every (source, angle) (K2-K5), candidate init, and the layer loop
//       L-1 .. 0 (K6-K8 fused + best-of-3 step) over a device-compacted live-candidate list;
//   host, after ONE device->host copy:  reference-order candidate sort (:214), layer-0 decision / sub-pixel /
//       back-mapping (:331-358), filterWithScore, filterWithRotatedRect, final sort and s_SingleTargetMatch
//       conversion (:373-432).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fpm.h"
#include "fpm_host.h"
#include "fpm_kernels.h"
#include "fpm_model.h"

using namespace fpm;

namespace {

inline int round_up(int v, int a) { return (v + a - 1) / a * a; }
inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= n && p) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        if (bytes == 0) bytes = 256;
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) n = bytes;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    template <class T> T* as(size_t byte_off = 0) const { return (T*)((char*)p + byte_off); }
};

struct PinBuf {
    void* p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= n && p) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; n = 0; }
        if (bytes == 0) bytes = 256;
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocMapped);   // device-visible (k_pack writes it)
        if (e == hipSuccess) n = bytes;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
    template <class T> T* as(size_t byte_off = 0) const { return (T*)((char*)p + byte_off); }
};

struct TmplLevel {
    int w, h, pitch;
    size_t off;              // offset in the device template slab
    size_t off8;             // offset in the i8 template slab (T ^ 0x80, zero padded; MFMA A operand)
    int p8;                  // its row pitch: 64 * ceil(w / 64)
    size_t tsum_off;         // offset (elements) of the per-row sums in d_tsum
    double mean, norm, inv_area;
    bool equal1;
    // host copy (dense).  After a device learn only the top level's is filled; fpm_template_level fetches the others
    // on first use, behind its const context
    mutable std::vector<uint8_t> px;
};

struct SrcLevel {
    int w, h, pitch;
    size_t img_bytes;        // pitch * h (rounded), per source image
    size_t off;              // offset of source 0 in the device source slab
};

// Everything that depends only on (template, params, source size, batch size).
struct Plan {
    bool valid = false;
    int sw = 0, sh = 0, S = 0, L = 0;
    int stop = 0;                              // the last refined layer: min(1, L) with fpm_params.stop_layer, else 0
    fpm_params prm{};
    int nang = 0, cap = 0, n3 = 1, C = 0;      // C = S * nang * cap candidate slots
    int a0 = 0, nang_all = 0;                  // this plan's angles = [a0, a0 + nang) of the full top-layer list
    int shard = 0, shards = 1;                 // angle shard the plan was built for (fpm_set_angle_shard)
    bool by_block = false;
    uint32_t step_layers = 0;                  // bit d: the last pass launched k_cand_step for layer depth d (profiling)
    bool top_lists = false;                    // the last pass took its top-layer peaks from k_top_mma's lists
    std::vector<double> angles, layer_score;
    std::vector<TopAngle> top;
    std::vector<AngleNode> top_nodes;
    std::vector<std::vector<AngleNode>> nodes;  // [d], d = 0 <-> layer L-1
    std::vector<size_t> node_off;                // device offsets (elements)
    F2 center;
    // top-layer layout (per source)
    std::vector<size_t> canvas_off, map_off, blk_off;
    std::vector<int> canvas_pitch, map_w, map_h, nblk;
    std::vector<int32_t> order;                // k_top_fused workgroup -> job (costliest angles first)
    size_t canvas_bytes = 0, map_floats = 0, blk_count = 0;
    int max_canvas = 0, max_map = 0, max_nblk = 0, max_cells = 0, max_nitems = 0;
    NmsMaxima nmax;                            // the top-layer maps' maxima for launch_nms / launch_top_greedy
    int off_skey = 0, nzero = 0;   // d_livecnt layout: strip keys' offset, words zeroed by k_warp
    // the matrix-core top layer (k_top_mma + k_nms_greedy on its candidate lists): layout and
    // constants of the launch (pointers set at plan time), the unit list and B fragments in d_tmu, the values of the
    // lists in d_tcandv (indices in d_ncand), their counts at d_livecnt + L + 2 (zeroed by the first pyramid launch)
    bool top_mma = false;
    TopMmaArgs tma{};
    int tcand_cap = 0;
    DevBuf d_tmu, d_tcandv;
    // device buffers owned by the plan
    DevBuf d_ncand;                            // s_BlockMax candidate lists (k_nms_blocks -> k_nms_fast)
    DevBuf d_canvas, d_map, d_bmax, d_bloc, d_jobs, d_nodes, d_top, d_topn, d_peaks, d_counts, d_state,
        d_live, d_livecnt, d_rec, d_rowsum, d_wtot, d_wtotq, d_wedge, d_tab, d_roi, d_tdesc, d_state2, d_rec2;
    int tabw = 0, tabh = 0, roi_pitch = 0, tdesc_stride = 1;
    size_t roi_stride = 0;
    int slot_cap = 0;                          // ROIs per refinement round (bounded scratch)
    size_t off_warp = 0, off_ncc = 0, off_nms = 0, off_order = 0;
    PinBuf h_out;
    size_t h_counts = 0, h_peaks = 0, h_live = 0, h_live0 = 0, h_state = 0, h_rec = 0, h_total = 0;
    char* h_dev = nullptr;   // device-side address of h_out (k_pack writes it over PCIe)
    void release() {
        for (DevBuf* b : {&d_tmu, &d_tcandv, &d_ncand, &d_canvas, &d_map, &d_bmax, &d_bloc, &d_jobs, &d_nodes, &d_top, &d_topn, &d_peaks,
                          &d_counts, &d_state, &d_live, &d_livecnt, &d_rec, &d_rowsum, &d_wtot, &d_wtotq, &d_wedge, &d_tab, &d_roi, &d_tdesc, &d_state2, &d_rec2})
            b->release();
        h_out.release();
        valid = false;
    }
};

// The pose a result was built from (its vecAllResult entry: the f32 point, dMatchAngle), kept next to the results for
// fpm_last_patches: the converted fpm_result fields do not give it back under FPM_SEMANTICS_MFC.
struct RawPose {
    float x, y;
    double angle;
};

struct KProf {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t used = 0;
    double ms = 0;
    int64_t launches = 0, bytes = 0;
};
// Profiling slots: one per FPM_K_* index (fpm_profile_get), then the variation model's three (fpm_model_profile) and the
// alignment's one (fpm_align_profile), the blob labelling's five (fpm_blobs_profile), the calipers' one
// (fpm_caliper_profile), the gray-value tools' two (fpm_gray_profile), the locators' one (fpm_locate_profile) and the
// probes' one (fpm_probe_profile), which have no FPM_K_* index: FPM_K_COUNT stays what it is.
enum { kProfModelTrain = FPM_K_COUNT, kProfModelPrepare, kProfModelInspect, kProfAlign, kProfBlobTile, kProfBlobMerge,
       kProfBlobFlatten, kProfBlobSlots, kProfBlobFeatures, kProfCaliper, kProfGrayHist, kProfGrayThreshold, kProfLocate,
       kProfProbe, kProfSlots };

}  // namespace

struct fpm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    fpm_params prm{};
    std::string err;
    // template (s_TemplData)
    bool learned = false;
    int border = 0;
    std::vector<TmplLevel> tmpl;
    DevBuf d_tmpl, d_tmpl8, d_tsum;
    uint64_t tmpl_gen = 0;
    // staged sources
    int S = 0, sw = 0, sh = 0, src_L = -1;
    // angle shard (fpm_set_angle_shard): this context's slice of the top-layer angle list
    int shard = 0, shards = 1;
    std::vector<SrcLevel> src;
    DevBuf d_src;
    // sources from device memory (stage_device_sources): the images' pointer table (pinned staging + device copy) and
    // the event that orders the context's stream after the producer's (timing disabled, created on first use)
    PinBuf h_imgtab;
    DevBuf d_imgtab;
    hipEvent_t in_ev = nullptr;
    // plan
    Plan plan;
    uint64_t plan_gen = ~0ull;
    // op scratch
    DevBuf d_op_a, d_op_b, d_op_job;
    // fpm_op_refine's per-ROI scratch (the plan's d_tab .. d_wedge belong to the recorded search)
    DevBuf d_rf_tab, d_rf_tdesc, d_rf_roi, d_rf_rowsum, d_rf_wtot, d_rf_wtotq, d_rf_wedge;
    // filterWithRotatedRect on the device (overlap_filter_device): rectangles + counters; staging and mapped outputs
    DevBuf d_ov;
    PinBuf h_ov_in, h_ov_out;
    // last search stats
    std::vector<int64_t> stats;
    int64_t alg_bytes[3] = {0, 0, 0};   // SURVEY.md §8(d) algorithmic bytes of the last search: B_pyr, B_top, B_ref
    // profiling
    bool prof = false;
    KProf kp[kProfSlots];
    // the whole device-resident search captured once per (plan, source slab) and replayed as one hipGraph
    hipGraphExec_t graph = nullptr;
    uint64_t graph_plan = ~0ull;
    const void* graph_src = nullptr;
    uint64_t plan_builds = 0;
    // timing of the last search (fpm_profile_last)
    hipEvent_t t_ev[2] = {nullptr, nullptr};
    double last_device_ms = 0, last_host_ms = 0, last_call_ms = 0;
    std::chrono::steady_clock::time_point t_call0;
    bool pending = false;    // a staged search is in flight (fpm_match_staged_launch)
    bool staged = false;     // the source slab holds an fpm_stage_sources batch (fpm_match re-lays it out for one source)
    bool src_inverted = false;   // level 0 of the slab holds 255 - source (fpm_params.bitwise_not; apply_polarity)
    fpm_params run_prm{};    // parameters of the search in flight (snapshot at launch; the host tail reads these)
    // per-source candidate records of the last search (collect_candidates; fpm_match_*candidates)
    std::vector<std::vector<fpm_candidate>> cands;
    std::vector<std::vector<fpm_result>> results;   // of the last search, per source (fpm_last_results)
    std::vector<std::vector<RawPose>> poses;        // the results' raw poses, same shape (fpm_last_patches)
    // match patches (fpm_last_patches* / fpm_patches_at)
    bool src_valid = false;   // level 0 of the slab holds staged sources (not so after a new template or a failed staging)
    bool searched = false;    // a search has finished on them since they were staged
    int patch_form = FPM_PATCH_FORM_TILED;
    PinBuf h_patchtab;        // job table: pinned staging + device copy; tab_ev = the last staging copy has left h_patchtab
    DevBuf d_patchtab, d_patch;   // d_patch: the patches of the host variants, before they are copied out
    hipEvent_t tab_ev = nullptr, out_ev = nullptr;
    DevBuf d_cmpacc;          // the comparison's per-hit records (fpm_last_compare / fpm_compare_at) and their host copy
    PinBuf h_cmpacc;
    // learning on the device (fpm_learn_device / fpm_learn_at / fpm_learn_hit): k_tmpl_prep's per-level sums, and their
    // host copy followed by the pixels of the top level
    DevBuf d_tacc;
    PinBuf h_tacc;
    // variation model (fpm_model_* / fpm_last_inspect / fpm_inspect_at): model_n samples over model_rect summed in
    // d_model (two dense u32 planes, sum then sum of squares); model_n = 0: no model.  d_band = the u8 mean / lo / hi
    // planes derived for (band_a, band_kq) from generation band_gen of the sums (prepared when the key changes).
    int model_n = 0;
    fpm_patch_rect model_rect{0, 0, 0, 0};
    int model_chunk = 0;      // fpm_model_set_chunk: jobs per workgroup of k_model_accum, 0 = the engine's choice
    uint64_t model_gen = 0;
    DevBuf d_model, d_band;
    int band_a = -1, band_kq = -1;
    uint64_t band_gen = ~0ull;
    DevBuf d_insacc;          // the inspection's per-hit records and their host copy
    PinBuf h_insacc;
    DevBuf d_alnacc;          // the alignment's per-hit records (fpm_align_*) and their host copy
    PinBuf h_alnacc;
    // defect blobs on the device (fpm_last_blobs / fpm_blobs_at / fpm_op_blobs): the label and area planes of one round
    // of images, the round's counters and records with their host copy, fpm_op_blobs' images and the labels' host copy
    int blobs_round = 0;      // fpm_blobs_set_round: images per round, 0 = the engine's choice
    DevBuf d_blobplanes, d_blobrec, d_blobimg;
    PinBuf h_blobrec, h_bloblab;
    // edge calipers (fpm_last_calipers / fpm_calipers_at): the raw records, counts and profiles of a call and their host copy
    DevBuf d_calout;
    PinBuf h_calout;
    // gray-value tools (fpm_last_histogram / fpm_last_segment ..): the histograms of a call and their host copy
    int gray_run = 0;         // fpm_gray_set_run: tiles per workgroup of k_patch_hist, 0 = the engine's choice
    DevBuf d_gray;
    PinBuf h_gray;
    // sub-pattern locators (fpm_last_locate / fpm_locate_at): the raw records and maps of a call and their host copy
    DevBuf d_locout;
    PinBuf h_locout;
    // edge probes (fpm_last_probes / fpm_probes_at): the raw records and profiles of a call and their host copy
    DevBuf d_probeout;
    PinBuf h_probeout;
    // template mask (fpm_mask_*): one u8 plane of the template's level-0 size and row pitch, 0x00 /
    // 0xFF, zero behind a row's end; mask_host = its dense host copy (the counts, fpm_mask_get).  d_mask_in = the
    // staging buffer (a host mask's upload, the plane being staged, the count); a set that fails leaves d_mask alone.
    bool mask_set = false, mask_on = false;
    int64_t mask_count = 0;
    std::vector<uint8_t> mask_host;
    DevBuf d_mask, d_mask_in;
    // the used count of the rectangle asked for last (mask_count_rect): the tools ask for one rectangle call after call
    mutable bool mask_rect_known = false;
    mutable fpm_patch_rect mask_rect{0, 0, 0, 0};
    mutable int64_t mask_rect_count = 0;
};

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);               \
            return FPM_E_DEVICE;                                                        \
        }                                                                               \
    } while (0)

namespace {

// ---------------------------------------------------------------------------------------------------------
// profiling helpers
// ---------------------------------------------------------------------------------------------------------
struct ProfScope {
    fpm_ctx* ctx;
    int k;
    hipEvent_t b = nullptr, e = nullptr;
    ProfScope(fpm_ctx* c, int kk, int64_t bytes) : ctx(c), k(kk) {
        if (!ctx->prof) return;
        KProf& p = ctx->kp[k];
        if (p.used == p.ev.size()) {
            hipEvent_t x, y;
            if (hipEventCreate(&x) != hipSuccess || hipEventCreate(&y) != hipSuccess) return;
            p.ev.push_back({x, y});
        }
        b = p.ev[p.used].first;
        e = p.ev[p.used].second;
        p.used++;
        p.launches++;
        p.bytes += bytes;
        (void)hipEventRecord(b, ctx->stream);
    }
    ~ProfScope() {
        if (b) (void)hipEventRecord(e, ctx->stream);
    }
};

void prof_collect(fpm_ctx* ctx) {
    if (!ctx->prof) return;
    for (int k = 0; k < kProfSlots; ++k) {
        KProf& p = ctx->kp[k];
        for (size_t i = 0; i < p.used; ++i) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, p.ev[i].first, p.ev[i].second) == hipSuccess) p.ms += ms;
        }
        p.used = 0;
    }
}

// the fpm_*_profile getters: slot `first + which` of a tool whose slots are first .. first + last_which
int kprof_out(const fpm_ctx* ctx, int first, int32_t which, int32_t last_which, double* ms, int64_t* launches, int64_t* bytes) {
    if (!ctx || which < 0 || which > last_which || !ms || !launches || !bytes) return FPM_E_INVALID_ARG;
    const KProf& p = ctx->kp[first + which];
    *ms = p.ms;
    *launches = p.launches;
    *bytes = p.bytes;
    return FPM_OK;
}

// ---------------------------------------------------------------------------------------------------------
// host restatements of reference helpers
// ---------------------------------------------------------------------------------------------------------
int top_layer(int w, int h, int min_len) {   // getTopLayer (TemplateMatcher.cpp:445-455)
    int L = 0, mra = min_len * min_len, area = w * h;
    while (area > mra) { area /= 4; ++L; }
    return L;
}

void mean_stddev(const std::vector<uint8_t>& px, double* mean, double* sdv) {  // cv::meanStdDev, 8UC1
    int64_t s = 0, q = 0;
    for (uint8_t v : px) { s += v; q += (int64_t)v * v; }
    const double scale = px.empty() ? 0. : 1. / (double)px.size();
    const double m = (double)s * scale;
    *mean = m;
    *sdv = std::sqrt(std::max((double)q * scale - m * m, 0.));
}

// getBestRotationSize (TemplateMatcher.cpp:901-969); ptRotatePt2f with glibc trig of angle*D2R
void best_rotation_size(int sw, int sh, int dw, int dh, double ang, int* ow, int* oh) {
    const double rad = ang * kD2R, c = std::cos(rad), s = std::sin(rad);
    const F2 ctr = f2((sw - 1) / 2.0f, (sh - 1) / 2.0f);
    const F2 lt = rotate_pt(f2(0.f, 0.f), ctr, c, s);
    const F2 lb = rotate_pt(f2(0.f, (float)(sh - 1)), ctr, c, s);
    const F2 rb = rotate_pt(f2((float)(sw - 1), (float)(sh - 1)), ctr, c, s);
    const F2 rt = rotate_pt(f2((float)(sw - 1), 0.f), ctr, c, s);
    const float top = std::max(std::max(lt.y, lb.y), std::max(rb.y, rt.y));
    const float bottom = std::min(std::min(lt.y, lb.y), std::min(rb.y, rt.y));
    const float right = std::max(std::max(lt.x, lb.x), std::max(rb.x, rt.x));
    const float left = std::min(std::min(lt.x, lb.x), std::min(rb.x, rt.x));
    if (ang > 360) ang -= 360;
    else if (ang < 0) ang += 360;
    if (std::fabs(std::fabs(ang) - 90) < kVisionTol || std::fabs(std::fabs(ang) - 270) < kVisionTol) {
        *ow = sh; *oh = sw;
        return;
    }
    if (std::fabs(ang) < kVisionTol || std::fabs(std::fabs(ang) - 180) < kVisionTol) {
        *ow = sw; *oh = sh;
        return;
    }
    double a = ang;
    if (a > 90 && a < 180) a -= 90;
    else if (a > 180 && a < 270) a -= 180;
    else if (a > 270 && a < 360) a -= 270;
    const float h1 = dw * std::sin(a * kD2R) * std::cos(a * kD2R);
    const float h2 = dh * std::sin(a * kD2R) * std::cos(a * kD2R);
    const int half_h = (int)std::ceil(top - ctr.y - h1);
    const int half_w = (int)std::ceil(right - ctr.x - h2);
    int rw = half_w * 2, rh = half_h * 2;
    const bool wrong = (dw < rw && dh > rh) || ((dw > rw && dh < rh) || (int64_t)dw * dh > (int64_t)rw * rh);
    if (wrong) { rw = int(right - left + 0.5); rh = int(top - bottom + 0.5); }
    *ow = rw;
    *oh = rh;
}

AngleNode make_node(double angle) {
    AngleNode n;
    n.angle = angle;
    const double r = angle * kD2R;
    n.c = std::cos(r); n.s = std::sin(r);
    n.cn = std::cos(-r); n.sn = std::sin(-r);
    return n;
}

// ---------------------------------------------------------------------------------------------------------
// layouts the refinement kernels rely on, shared by the search (layout_sources, build_plan) and fpm_op_refine
// ---------------------------------------------------------------------------------------------------------
// One image of a source pyramid level in the device slab (off is the caller's).
SrcLevel level_layout(int w, int h) {
    SrcLevel s{};
    s.w = w; s.h = h;
    s.pitch = round_up(w + 4, 64);          // +4: aligned dword over-reads stay in the row
    s.img_bytes = round_up((size_t)s.pitch * (h + 1), (size_t)256);   // one spare row per image
    return s;
}
// Slack past the last image of a slab whose largest level has row pitch `pitch0`: the ROI sampler's footprint staging
// reads whole 16-row groups, up to 15 rows past a box (k_roi_warp3), i.e. past the last image's spare row
size_t level_slab_slack(int pitch0) { return 16 * (size_t)pitch0 + 256; }

// Per-ROI refinement scratch (tables, tile descriptors, sampled ROI, row sums, the window sums' band totals
// and edge rows) sized for the largest
// of the template levels lv[0 .. nlv).
struct RoiScratchDims {
    int tabw = 1, tabh = 1, roi_pitch = 1, tdesc_stride = 1;
    size_t roi_stride = 0, max_rows = 1, max_bands = 1;
    size_t per_roi() const {
        return sizeof(int32_t) * 2 * (tabw + tabh) + sizeof(int4) * tdesc_stride + roi_stride + max_rows * 49 * 4 +
               max_bands * 7 * 12 + kRoiEdgeWords * 4;
    }
};
RoiScratchDims roi_scratch_dims(const TmplLevel* lv, int nlv) {
    RoiScratchDims d;
    int max_w = 1;
    for (int l = 0; l < nlv; ++l) {
        d.tdesc_stride = std::max(d.tdesc_stride, roi_tiles_for(lv[l].w, lv[l].h));
        d.max_rows = std::max(d.max_rows, (size_t)lv[l].h);
        d.max_bands = std::max(d.max_bands, (size_t)roi_bands(lv[l].h));
        max_w = std::max(max_w, lv[l].w);
        d.roi_stride = std::max(d.roi_stride, roi_tiles_bytes(lv[l].w, lv[l].h));
    }
    d.roi_pitch = roi_pitch_for(max_w);
    d.tabw = d.roi_pitch;
    d.tabh = roi_tab_rows((int)d.max_rows);
    return d;
}
hipError_t roi_scratch_ensure(const RoiScratchDims& d, size_t slots, DevBuf& tab, DevBuf& tdesc, DevBuf& roi,
                              DevBuf& rowsum, DevBuf& wtot, DevBuf& wtotq, DevBuf& wedge) {
    hipError_t e = tab.ensure(slots * 2 * (d.tabw + d.tabh) * sizeof(int32_t));
    if (e == hipSuccess) e = tdesc.ensure(slots * d.tdesc_stride * sizeof(int4));
    if (e == hipSuccess) e = roi.ensure(slots * d.roi_stride);
    if (e == hipSuccess) e = rowsum.ensure(slots * round_up(d.max_rows * 49, (size_t)4) * 4);
    if (e == hipSuccess) e = wtot.ensure(slots * d.max_bands * 7 * 4);
    if (e == hipSuccess) e = wtotq.ensure(slots * d.max_bands * 7 * 8);
    if (e == hipSuccess) e = wedge.ensure(slots * kRoiEdgeWords * 4);
    return e;
}

// ---------------------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------------------
bool same_search_params(const fpm_params& a, const fpm_params& b) {
    return a.max_pos == b.max_pos && a.min_reduce_area == b.min_reduce_area && a.max_overlap == b.max_overlap &&
           a.score == b.score && a.tolerance_angle == b.tolerance_angle && a.use_simd == b.use_simd &&
           a.tolerance_range == b.tolerance_range && a.semantics == b.semantics &&
           a.top_angle_step == b.top_angle_step && std::equal(a.tolerance, a.tolerance + 4, b.tolerance) &&
           (a.stop_layer != 0) == (b.stop_layer != 0);
}

// Input guard of the angle list (TemplateMatcher.cpp:130-144 accumulates `a += step` until the tolerance): a non-finite
// tolerance or step, or a step so small that the list would exceed kMaxTopAngles, is refused up front (the oracle
// applies the same rule) instead of looping without end / growing the list until memory runs out.
constexpr double kMaxTopAngles = 100000;
static bool angle_list_ok(const fpm_params& prm, double step, bool mfc) {
    if (!std::isfinite(step) || step <= 0) return false;
    auto span = [&](double lo, double hi) { return (hi - lo) / step + 2; };
    double n;
    if (mfc && prm.tolerance_range) {
        for (double t : prm.tolerance)
            if (!std::isfinite(t)) return false;
        n = span(prm.tolerance[0], prm.tolerance[1]) + span(prm.tolerance[2], prm.tolerance[3]);
    } else {
        if (!std::isfinite(prm.tolerance_angle)) return false;
        n = prm.tolerance_angle < kVisionTol ? 1 : 2 * span(0, prm.tolerance_angle);
    }
    return n <= kMaxTopAngles;
}

// The list threshold of the matrix-core top layer and its prefilter's constants (fpm_kernels.hip, "Exactness of the
// bound"): thr = the layer score; thrK carries the 1e-5 relative margin, E the absolute slack of the two f32 terms
void top_mma_thresholds(TopMmaArgs& A, double thr, const TmplLevel& tt) {
    const double tm = thr * (1.0 - 1e-5);
    A.thrK = (float)(tm * tm * tt.norm * tt.norm * (double)A.area);
    A.E = 1024.f;
    A.thr = thr;
}

// The matrix-core top layer's plan (k_top_mma): whether it applies, its strip width and row runs
// (work units), the B fragments of the top template level and the candidate-list buffers.  Applies where the template
// level fits the kernel's two MFMA layouts, the layer score is > 0.01 (the greedy peak forms need thr > 0, and the lists
// stay short), there is a pyramid launch to zero the list counters (L >= 1), the level is not flat (ResultEqual1) and
// the greedy form can hold the maps' coverage cells; FPM_TOP_MMA=0 keeps the split / fused kernels (read when the plan is
// built).
int plan_top_mma(fpm_ctx* ctx, Plan& P, const TmplLevel& tt) {
    P.top_mma = false;
    const char* env = getenv("FPM_TOP_MMA");
    if (env && atoi(env) == 0) return FPM_OK;
    const int L = P.L, S = ctx->S, J = S * P.nang;
    const double thr = P.layer_score[L];
    int max_mw = 0, max_mh = 0;
    for (int a = 0; a < P.nang; ++a) { max_mw = std::max(max_mw, P.map_w[a]); max_mh = std::max(max_mh, P.map_h[a]); }
    // (MaxOverlap < 0: a painted rectangle of more than twice the template outgrows the 3 x 3 cells k_nms_greedy files it in)
    if (L < 1 || J <= 0 || !top_mma_fits(tt.w, tt.h) || tt.equal1 || !(thr > 0.01) || max_mw <= 0 ||
        !(ctx->prm.max_overlap >= 0.0) ||
        std::max(max_mw, max_mh) >= 65536 || P.cap > 256 || P.max_cells > 12 * 1024)
        return FPM_OK;
    // strip width: one strip up to 192 output columns, else the fewest strips of at most 192, evened out
    const int nstrip = (max_mw + kTopMmaMaxSw - 1) / kTopMmaMaxSw;
    const int sw = (((max_mw + nstrip - 1) / nstrip) + 15) / 16 * 16;
    // row runs: the longest (fewer first-band re-samplings of th - 1 rows) that still give >= 2048 units
    std::vector<TopUnit> units;
    int seg = 64;
    for (int cand : {1 << 30, 256, 128, 64}) {
        long n = 0;
        for (int a = 0; a < P.nang; ++a)
            if (P.map_w[a] > 0 && P.map_h[a] > 0)
                n += (long)((P.map_w[a] + sw - 1) / sw) * ((P.map_h[a] + std::min(cand, P.map_h[a]) - 1) /
                                                           std::min(cand, P.map_h[a]));
        seg = cand;
        if (n * S >= 2048) break;
    }
    // plain-peak searches with few work units (< 128 workgroups: a lone Src7 search's 41 small maps make 82) and few
    // peaks per map (MaxPos <= 10, the reference's own s_BlockMax threshold) run faster on the split kernels, whose
    // grids cover the chip: device 0.233 vs 0.248 ms for the lone Src7 search.  Many peaks per map keep the lists, whose
    // greedy pass beats k_nms's painted-rectangle loop even on one map (Src3 / Dst3 at 0 deg, MaxPos 38, 3 units: 0.170
    // vs 0.229 ms), and so do s_BlockMax searches and many-unit sweeps (profiles/r06_lone/); FPM_TOP_MMA=1 keeps the form
    {
        long nunits = 0;
        for (int a = 0; a < P.nang; ++a)
            if (P.map_w[a] > 0 && P.map_h[a] > 0)
                nunits += (long)((P.map_w[a] + sw - 1) / sw) * ((P.map_h[a] + std::min(seg, P.map_h[a]) - 1) /
                                                               std::min(seg, P.map_h[a]));
        if (!(env && atoi(env) == 1) && !P.by_block && ctx->prm.max_pos <= 10 && nunits * S < 128 &&
            ncc_tile_fits(tt.w, tt.h))
            return FPM_OK;
    }
    int max_rows = 0;
    for (int s = 0; s < S; ++s)
        for (int a = 0; a < P.nang; ++a) {
            const int mw = P.map_w[a], mh = P.map_h[a];
            if (mw <= 0 || mh <= 0) continue;
            const int run = std::min(seg, mh);
            for (int x0 = 0; x0 < mw; x0 += sw)
                for (int y0 = 0; y0 < mh; y0 += run) {
                    TopUnit u;
                    u.job = s * P.nang + a; u.x0 = x0; u.y0 = y0; u.y1 = std::min(mh, y0 + run);
                    units.push_back(u);
                    max_rows = std::max(max_rows, u.y1 - u.y0);
                }
        }
    TopMmaArgs& A = P.tma;
    A = TopMmaArgs{};
    A.tw = tt.w; A.th = tt.h; A.area = tt.w * tt.h;
    top_mma_layout(A, sw, max_rows);
    if (top_mma_lds(A) > 160 * 1024 - 1024) return FPM_OK;
    uint32_t tsum = 0;
    for (uint8_t v : tt.px) tsum += v;
    A.tsum = tsum;
    // B fragments: slot q, lane (n = lane & 15, g = lane >> 4), byte i is k = 16 g + i -> template row r, column c - n
    std::vector<int8_t> bf((size_t)A.nq * 64 * 16, 0);
    for (int q = 0; q < A.nq; ++q)
        for (int lane = 0; lane < 64; ++lane)
            for (int i = 0; i < 16; ++i) {
                const int n = lane & 15, g = lane >> 4;
                const int r = A.R == 2 ? 2 * q + (g >> 1) : q;
                const int c = (A.R == 2 ? 16 * (g & 1) : 16 * g) + i - n;
                if (r < tt.h && c >= 0 && c < tt.w)
                    bf[((size_t)q * 64 + lane) * 16 + i] = (int8_t)((int)tt.px[(size_t)r * tt.w + c] - 128);
            }
    const size_t ubytes = ((units.size() * sizeof(TopUnit)) + 255) & ~(size_t)255;
    HIP_TRY(P.d_tmu.ensure(ubytes + bf.size()));
    HIP_TRY(hipMemcpyAsync(P.d_tmu.p, units.data(), units.size() * sizeof(TopUnit), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(P.d_tmu.as<char>(ubytes), bf.data(), bf.size(), hipMemcpyHostToDevice, ctx->stream));
    // candidate lists: s_BlockMax maps share d_ncand with k_nms_blocks' fallback lists (kNmsCandCap per map); plain
    // maps need no more than the greedy form takes
    P.tcand_cap = P.by_block ? kNmsCandCap : 512;
    // FPM_TOP_LIST_CAP=n (tests): lists of n entries, so every map with more candidates takes the fallback path
    if (const char* lc = getenv("FPM_TOP_LIST_CAP"))
        if (atoi(lc) > 0) P.tcand_cap = std::min(P.tcand_cap, atoi(lc));
    HIP_TRY(P.d_ncand.ensure(sizeof(int32_t) * (size_t)P.tcand_cap * J));
    HIP_TRY(P.d_tcandv.ensure(sizeof(float) * (size_t)P.tcand_cap * J));
    A.wjobs = P.d_jobs.as<WarpJob>(P.off_warp);
    A.njobs = P.d_jobs.as<NccJob>(P.off_ncc);
    A.units = P.d_tmu.as<TopUnit>();
    A.nunits = (int)units.size();
    A.bfrag = P.d_tmu.as<uint8_t>(ubytes);
    A.prefilter = A.area <= 258 ? 1 : 0;
    top_mma_thresholds(A, thr, tt);
    A.mean = tt.mean; A.norm = tt.norm; A.inv_area = tt.inv_area;
    A.cand = P.d_ncand.as<int32_t>();
    A.cand_val = P.d_tcandv.as<float>();
    A.cand_cap = P.tcand_cap;
    if (!P.by_block) {   // plain maps: the list counters follow the live counts (s_BlockMax plans already zero them)
        P.nzero = L + 2 + J;
        HIP_TRY(P.d_livecnt.ensure(sizeof(int32_t) * (size_t)P.nzero));
    }
    A.cand_cnt = P.d_livecnt.as<int32_t>() + L + 2;
    P.top_mma = true;
    return FPM_OK;
}

int build_plan(fpm_ctx* ctx) {
    Plan& P = ctx->plan;
    const int L = ctx->src_L;
    if (P.valid && ctx->plan_gen == ctx->tmpl_gen && P.sw == ctx->sw && P.sh == ctx->sh && P.S == ctx->S &&
        P.L == L && same_search_params(P.prm, ctx->prm) && P.shard == ctx->shard && P.shards == ctx->shards)
        return FPM_OK;
    P.valid = false;
    P.sw = ctx->sw; P.sh = ctx->sh; P.S = ctx->S; P.L = L; P.prm = ctx->prm;
    P.shard = ctx->shard; P.shards = ctx->shards;
    const fpm_params& prm = ctx->prm;
    // fast mode (MatchToolDlg.cpp:936): with a top layer of 0 the reference reads vecPyramid[1] out of bounds; here
    // that case is the normal search
    P.stop = std::min(prm.stop_layer ? 1 : 0, L);
    const TmplLevel& tt = ctx->tmpl[L];
    // angle list (TemplateMatcher.cpp:130-144); the step override is an extension (fpm_params.top_angle_step)
    const double step = prm.top_angle_step > 0 ? prm.top_angle_step : std::atan(2.0 / std::max(tt.w, tt.h)) * kR2D;
    const bool mfc = prm.semantics == FPM_SEMANTICS_MFC;
    P.angles.clear();
    if (!angle_list_ok(prm, step, mfc)) {   // the reference would loop without end or exhaust memory on these
        ctx->err = "angle list: non-finite tolerance or step, or more than 100000 top-layer angles";
        return FPM_E_INVALID_ARG;
    }
    if (mfc && prm.tolerance_range) {   // MFC angle ranges (MatchToolDlg.cpp:805-815)
        const double* t = prm.tolerance;
        if (t[0] >= t[1] || t[2] >= t[3]) { ctx->err = "angle ranges need tolerance[0] < [1] and [2] < [3]"; return FPM_E_INVALID_ARG; }
        for (double a = t[0]; a < t[1] + step; a += step) P.angles.push_back(a);
        for (double a = t[2]; a < t[3] + step; a += step) P.angles.push_back(a);
    } else if (prm.tolerance_angle < kVisionTol) {
        P.angles.push_back(0.0);
    } else {
        for (double a = 0; a < prm.tolerance_angle + step; a += step) P.angles.push_back(a);
        for (double a = -step; a > -prm.tolerance_angle - step; a -= step) P.angles.push_back(a);
    }
    // angle shard: a contiguous block [a0, a1) of the reference's list, so the concatenation of the shards' candidate
    // lists in shard order is the reference's push order (angle-major, TemplateMatcher.cpp:157-211)
    P.nang_all = (int)P.angles.size();
    P.a0 = (int)((int64_t)P.nang_all * P.shard / P.shards);
    const int a1 = (int)((int64_t)P.nang_all * (P.shard + 1) / P.shards);
    P.angles = std::vector<double>(P.angles.begin() + P.a0, P.angles.begin() + a1);
    P.nang = (int)P.angles.size();
    P.layer_score.assign(L + 1, prm.score);
    for (int l = 1; l <= L; ++l) P.layer_score[l] = P.layer_score[l - 1] * 0.9;
    const SrcLevel& top = ctx->src[L];
    P.center = f2((top.w - 1) / 2.0f, (top.h - 1) / 2.0f);
    P.by_block = ((top.w * top.h) / (tt.w * tt.h) > 500) && prm.max_pos > 10;
    P.cap = std::max(prm.max_pos + kMatchCandidateNum, 1);
    P.n3 = (prm.tolerance_range || prm.tolerance_angle >= kVisionTol) ? 3 : 1;
    P.C = ctx->S * P.nang * P.cap;
    // per-angle canvas geometry (TemplateMatcher.cpp:163-175)
    P.top.resize(P.nang);
    P.top_nodes.resize(P.nang);
    P.canvas_off.resize(P.nang); P.map_off.resize(P.nang); P.blk_off.resize(P.nang);
    P.canvas_pitch.resize(P.nang); P.map_w.resize(P.nang); P.map_h.resize(P.nang); P.nblk.resize(P.nang);
    std::vector<std::array<double, 6>> mats(P.nang);
    size_t co = 0, mo = 0, bo = 0;
    P.max_canvas = 0; P.max_map = 0; P.nmax = NmsMaxima{};
    for (int a = 0; a < P.nang; ++a) {
        int bw, bh;
        best_rotation_size(top.w, top.h, tt.w, tt.h, P.angles[a], &bw, &bh);
        TopAngle& ta = P.top[a];
        ta.bw = bw; ta.bh = bh;
        ta.tx = (bw - 1) / 2.0f - P.center.x;
        ta.ty = (bh - 1) / 2.0f - P.center.y;
        const double r = P.angles[a] * kD2R;
        double m[6];
        rotation_matrix(P.center, std::cos(r), std::sin(r), m);
        m[2] += ta.tx;
        m[5] += ta.ty;
        invert_affine(m);
        std::copy(m, m + 6, mats[a].begin());
        P.top_nodes[a] = make_node(P.angles[a]);
        const bool ok = bw >= tt.w && bh >= tt.h && bw > 0 && bh > 0;
        P.canvas_pitch[a] = round_up(std::max(bw, 1), 64);
        P.canvas_off[a] = co;
        co += round_up((size_t)P.canvas_pitch[a] * std::max(bh, 1), (size_t)256);
        P.map_w[a] = ok ? bw - tt.w + 1 : 0;
        P.map_h[a] = ok ? bh - tt.h + 1 : 0;
        P.map_off[a] = mo;
        mo += round_up((size_t)P.map_w[a] * P.map_h[a], (size_t)64);
        // s_BlockMax blocks (BlockGeom in fpm_kernels.hip: Qt or MFC layout) and the peak launchers' maxima, by the
        // function fpm_op_peaks uses for its maps
        const int nb = nms_maxima_add(P.nmax, P.map_w[a], P.map_h[a], tt.w, tt.h, P.by_block ? 1 : 0, mfc ? 1 : 0);
        P.nblk[a] = nb;
        P.blk_off[a] = bo;
        bo += round_up((size_t)nb, (size_t)64);
        P.max_canvas = std::max(P.max_canvas, bw * bh);
        P.max_map = std::max(P.max_map, P.map_w[a] * P.map_h[a]);
    }
    P.canvas_bytes = co; P.map_floats = mo; P.blk_count = bo;
    P.max_nblk = P.nmax.max_blocks; P.max_cells = P.nmax.max_cells; P.max_nitems = P.nmax.max_items;
    // refinement angle tree: level d has nang * n3^(d+1) nodes (TemplateMatcher.cpp:282-298)
    P.nodes.assign(L, {});
    P.node_off.assign(L, 0);
    size_t noff = 0;
    for (int d = 0; d < L; ++d) {
        const int layer = L - 1 - d;
        const double astep = std::atan(2.0 / std::max(ctx->tmpl[layer].w, ctx->tmpl[layer].h)) * kR2D;
        const size_t parents = d == 0 ? (size_t)P.nang : P.nodes[d - 1].size();
        std::vector<AngleNode>& lv = P.nodes[d];
        lv.resize(parents * P.n3);
        for (size_t p = 0; p < parents; ++p) {
            const double matched = d == 0 ? P.angles[p] : P.nodes[d - 1][p].angle;
            for (int j = 0; j < P.n3; ++j) {
                double ang;
                if (P.n3 == 1) ang = 0.0;
                else ang = matched + astep * (j - 1);
                lv[p * P.n3 + j] = make_node(ang);
            }
        }
        P.node_off[d] = noff;
        noff += lv.size();
    }
    // device buffers
    const int S = ctx->S, J = S * P.nang;
    HIP_TRY(P.d_canvas.ensure(P.canvas_bytes * S));
    HIP_TRY(P.d_map.ensure(sizeof(float) * P.map_floats * S));
    HIP_TRY(P.d_bmax.ensure(sizeof(float) * std::max<size_t>(P.blk_count, 1) * S));
    HIP_TRY(P.d_bloc.ensure(sizeof(int32_t) * std::max<size_t>(P.blk_count, 1) * S));
    P.off_warp = 0;
    P.off_ncc = round_up(sizeof(WarpJob) * J, (size_t)256);
    P.off_nms = P.off_ncc + round_up(sizeof(NccJob) * J, (size_t)256);
    P.off_order = P.off_nms + round_up(sizeof(NmsJob) * J, (size_t)256);
    HIP_TRY(P.d_jobs.ensure(P.off_order + sizeof(int32_t) * J));
    HIP_TRY(P.d_nodes.ensure(sizeof(AngleNode) * std::max<size_t>(noff, 1)));
    HIP_TRY(P.d_top.ensure(sizeof(TopAngle) * P.nang));
    HIP_TRY(P.d_topn.ensure(sizeof(AngleNode) * P.nang));
    HIP_TRY(P.d_peaks.ensure(sizeof(Peak) * (size_t)P.C));
    HIP_TRY(P.d_counts.ensure(sizeof(int32_t) * J));
    if (P.by_block) HIP_TRY(P.d_ncand.ensure(sizeof(int32_t) * (size_t)kNmsCandCap * J));
    HIP_TRY(P.d_state.ensure(sizeof(CandState) * (size_t)P.C));
    HIP_TRY(P.d_live.ensure(sizeof(int32_t) * (size_t)P.C * 2));
    // live counts [L + 2], then (s_BlockMax) the per-map candidate counts [J]: zeroed together by k_warp
    // (s_BlockMax) then the strip-block keys [J][3] (u64, 8-aligned) and chunk counts [J][3] of k_nms_blocks
    P.off_skey = round_up(L + 2 + J, 2);
    P.nzero = L + 2 + (P.by_block ? P.off_skey - (L + 2) + 9 * J : 0);
    HIP_TRY(P.d_livecnt.ensure(sizeof(int32_t) * (size_t)P.nzero));
    HIP_TRY(P.d_rec.ensure(sizeof(RoiRecord) * (size_t)P.C * P.n3));
    // the prologue-stepped run of small layers (below) alternates state and records between two buffers each
    HIP_TRY(P.d_state2.ensure(sizeof(CandState) * (size_t)P.C));
    HIP_TRY(P.d_rec2.ensure(sizeof(RoiRecord) * (size_t)P.C * P.n3));
    {   // refinement scratch per ROI (tables, sampled ROI, row sums, window band totals and edge rows); bounded, rounds cover the rest
        const RoiScratchDims rd = roi_scratch_dims(ctx->tmpl.data(), L);
        P.tdesc_stride = rd.tdesc_stride;
        P.roi_pitch = rd.roi_pitch;
        P.tabw = rd.tabw;
        P.tabh = rd.tabh;
        P.roi_stride = rd.roi_stride;
        const size_t per_roi = rd.per_roi();
        // slots are sized for the worst case (every top candidate alive at every layer) so the captured graph needs
        // no host round trip; up to a sixth of the free HBM (<= 48 GB of 288; FPM_SCRATCH_MB caps it) holds them,
        // rounds only beyond that.  A floor of min(4 GB, half the free HBM) keeps a batch in few rounds when another
        // allocator in the process holds most of the device; an allocation failure halves the slots (more rounds)
        // instead of failing the search.
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)16 << 30;
        size_t budget = std::min((size_t)48 << 30, std::max(std::min((size_t)4 << 30, free_b / 2), free_b / 6));
        if (const char* e = getenv("FPM_SCRATCH_MB")) {
            const long mb = atol(e);
            if (mb > 0) budget = std::min(budget, (size_t)mb << 20);
        }
        const size_t want = (size_t)P.C * P.n3;
        // rounds hold whole candidates (k_roi_eval steps a candidate from its n3 records)
        P.slot_cap = (int)std::max<size_t>((size_t)P.n3, std::min(want, budget / per_roi) / P.n3 * P.n3);
        for (;;) {
            const hipError_t e = roi_scratch_ensure(rd, (size_t)P.slot_cap, P.d_tab, P.d_tdesc, P.d_roi, P.d_rowsum,
                                                    P.d_wtot, P.d_wtotq, P.d_wedge);
            if (e == hipSuccess) break;
            (void)hipGetLastError();   // clear the sticky allocation error
            if (e != hipErrorOutOfMemory || P.slot_cap <= P.n3) HIP_TRY(e);
            P.d_tab.release(); P.d_tdesc.release(); P.d_roi.release();
            P.d_rowsum.release(); P.d_wtot.release(); P.d_wtotq.release(); P.d_wedge.release();
            P.slot_cap = std::max(P.n3, P.slot_cap / 2 / P.n3 * P.n3);
        }
    }
    // job tables
    std::vector<WarpJob> wj(J);
    std::vector<NccJob> nj(J);
    std::vector<NmsJob> mj(J);
    const uint8_t* dsrc = ctx->d_src.as<uint8_t>();
    for (int s = 0; s < S; ++s)
        for (int a = 0; a < P.nang; ++a) {
            const int k = s * P.nang + a;
            uint8_t* canvas = P.d_canvas.as<uint8_t>() + P.canvas_bytes * s + P.canvas_off[a];
            float* map = P.d_map.as<float>() + P.map_floats * s + P.map_off[a];
            WarpJob& w = wj[k];
            w.src = dsrc + top.off + top.img_bytes * s;
            w.sw = top.w; w.sh = top.h; w.sp = top.pitch;
            w.dst = canvas;
            w.dw = P.top[a].bw; w.dh = P.top[a].bh; w.dp = P.canvas_pitch[a];
            w.border = ctx->border;
            w.pad = 0;
            std::copy(mats[a].begin(), mats[a].end(), w.M);
            NccJob& n = nj[k];
            n.img = canvas; n.iw = w.dw; n.ih = w.dh; n.ip = w.dp;
            n.tmpl = ctx->d_tmpl.as<uint8_t>() + tt.off; n.tw = tt.w; n.th = tt.h; n.tp = tt.pitch;
            n.out = map; n.ow = P.map_w[a]; n.oh = P.map_h[a];
            n.fold = 0;   // top layer: cv::matchTemplate(TM_CCORR) (:177 -> :514)
            n.equal1 = tt.equal1 ? 1 : 0;
            n.mean = tt.mean; n.norm = tt.norm; n.inv_area = tt.inv_area;
            NmsJob& m = mj[k];
            m.map = map; m.mw = P.map_w[a]; m.mh = P.map_h[a];
            m.bmax = P.d_bmax.as<float>() + P.blk_count * s + P.blk_off[a];
            m.bloc = P.d_bloc.as<int32_t>() + P.blk_count * s + P.blk_off[a];
        }
    HIP_TRY(hipMemcpyAsync(P.d_jobs.as<char>(P.off_warp), wj.data(), sizeof(WarpJob) * J, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(P.d_jobs.as<char>(P.off_ncc), nj.data(), sizeof(NccJob) * J, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(P.d_jobs.as<char>(P.off_nms), mj.data(), sizeof(NmsJob) * J, hipMemcpyHostToDevice, ctx->stream));
    {
        const int rc = plan_top_mma(ctx, P, tt);
        if (rc != FPM_OK) return rc;
    }
    {   // k_top_fused's workgroup -> job order: the angles with the largest map x template work first, every source's
        // job of an angle together (one launch covers S x nang jobs in ~1.4 rounds of resident workgroups at Src7: the
        // cheap jobs fill the last round); a scheduling choice only, every job writes its own outputs
        std::vector<int> ang(P.nang);
        for (int a = 0; a < P.nang; ++a) ang[a] = a;
        auto cost = [&](int a) {
            return (double)P.map_w[a] * P.map_h[a] * tt.w * tt.h + (double)P.top[a].bw * P.top[a].bh;
        };
        std::stable_sort(ang.begin(), ang.end(), [&](int x, int y) { return cost(x) > cost(y); });
        P.order.resize(J);
        for (int i = 0; i < P.nang; ++i)
            for (int s = 0; s < S; ++s) P.order[(size_t)i * S + s] = s * P.nang + ang[i];
        HIP_TRY(hipMemcpyAsync(P.d_jobs.as<char>(P.off_order), P.order.data(), sizeof(int32_t) * J,
                               hipMemcpyHostToDevice, ctx->stream));
    }
    for (int d = 0; d < L; ++d)
        HIP_TRY(hipMemcpyAsync(P.d_nodes.as<AngleNode>() + P.node_off[d], P.nodes[d].data(),
                               sizeof(AngleNode) * P.nodes[d].size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(P.d_top.p, P.top.data(), sizeof(TopAngle) * P.nang, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(P.d_topn.p, P.top_nodes.data(), sizeof(AngleNode) * P.nang, hipMemcpyHostToDevice, ctx->stream));
    // pinned host buffer written by k_pack: counts | peaks | live counts | layer-0 ids | states | records
    P.h_counts = 0;
    P.h_peaks = round_up(sizeof(int32_t) * J, (size_t)256);
    P.h_live = P.h_peaks + round_up(sizeof(Peak) * (size_t)P.C, (size_t)256);
    P.h_live0 = P.h_live + round_up(sizeof(int32_t) * (L + 2), (size_t)256);
    P.h_state = P.h_live0 + round_up(sizeof(int32_t) * (size_t)P.C, (size_t)256);
    P.h_rec = P.h_state + round_up(sizeof(CandState) * (size_t)P.C, (size_t)256);
    P.h_total = P.h_rec + sizeof(RoiRecord) * (size_t)P.C * P.n3;
    HIP_TRY(P.h_out.ensure(P.h_total));
    {
        void* dp = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dp, P.h_out.p, 0));
        P.h_dev = (char*)dp;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    P.valid = true;
    ctx->plan_gen = ctx->tmpl_gen;
    ctx->plan_builds++;
    return FPM_OK;
}

// ---------------------------------------------------------------------------------------------------------
// sources
// ---------------------------------------------------------------------------------------------------------
int layout_sources(fpm_ctx* ctx, int count, int w, int h) {
    const int L = top_layer(ctx->tmpl[0].w, ctx->tmpl[0].h, (int)std::sqrt((double)ctx->prm.min_reduce_area));
    if (L >= (int)ctx->tmpl.size()) {
        ctx->err = "MinReduceArea changed after learnPattern: template pyramid too shallow";
        return FPM_E_INVALID_ARG;
    }
    ctx->S = count; ctx->sw = w; ctx->sh = h; ctx->src_L = L;
    ctx->src_valid = false;   // until the pixels are on their way (upload_sources, stage_device_sources)
    ctx->searched = false;
    ctx->src.assign(L + 1, {});
    size_t off = 0;
    int lw = w, lh = h;
    for (int l = 0; l <= L; ++l) {
        SrcLevel& s = ctx->src[l];
        s = level_layout(lw, lh);
        s.off = off;
        off += s.img_bytes * count;
        lw = (lw + 1) / 2;
        lh = (lh + 1) / 2;
    }
    HIP_TRY(ctx->d_src.ensure(off + level_slab_slack(ctx->src[0].pitch)));
    return FPM_OK;
}

int check_sizes(fpm_ctx* ctx, int w, int h) {   // TemplateMatcher.cpp:99-114
    if (!ctx->learned) { ctx->err = "template not learned"; return FPM_E_NOT_LEARNED; }
    const TmplLevel& t = ctx->tmpl[0];
    if ((t.w < w && t.h > h) || (t.w > w && t.h < h)) { ctx->err = "template/source orientation mismatch"; return FPM_E_SIZE; }
    if ((int64_t)t.w * t.h > (int64_t)w * h) { ctx->err = "template larger than source"; return FPM_E_SIZE; }
    return FPM_OK;
}

// ---------------------------------------------------------------------------------------------------------
// search
// ---------------------------------------------------------------------------------------------------------
constexpr int kPrologueMaxSources = 2;            // step prologue of the small layers up to this batch size
constexpr int64_t kPyr2MaxBytes = 16ll << 20;     // two-level pyramid launches up to this many input bytes

// K1: source pyramid (all staged sources per launch).  pyr_zero: the first launch also zeroes the plan's counters
// (d_livecnt, P.nzero words) ahead of the top layer's atomics.
void enqueue_pyramid(fpm_ctx* ctx, bool pyr_zero) {
    Plan& P = ctx->plan;
    const int L = P.L, S = P.S;
    hipStream_t st = ctx->stream;
    uint8_t* dsrc = ctx->d_src.as<uint8_t>();
    // Two levels per launch (k_pyr_down2) where the pair's input is small (<= kPyr2MaxBytes over the batch:
    // launch-bound levels, e.g. every pair of a single Src7 search: 14.8 -> 11.3 us for levels 0-2), else one level per
    // launch (k_pyr_down_s keeps more workgroups in flight: 43 Src7 levels 0-2 in 197 us vs 217-258 us,
    // profiles/r04/mb32_r04g.txt).  FPM_PYR2=0 / 1 forces one form.
    const char* pyr2_env = getenv("FPM_PYR2");
    const int pyr2_mode = pyr2_env ? atoi(pyr2_env) : -1;
    for (int l = 1; l <= L;) {
        const SrcLevel& a = ctx->src[l - 1];
        const SrcLevel& b = ctx->src[l];
        int32_t* zero = l == 1 && pyr_zero ? P.d_livecnt.as<int32_t>() : nullptr;
        const int nzero = l == 1 && pyr_zero ? P.nzero : 0;
        const int64_t in_bytes = (int64_t)S * a.w * a.h;
        const bool two = l + 1 <= L && (pyr2_mode >= 0 ? pyr2_mode != 0 : in_bytes <= kPyr2MaxBytes);
        const SrcLevel& c = ctx->src[two ? l + 1 : l];
        l += two ? 2 : 1;
        if (two) {
            ProfScope ps(ctx, FPM_K_PYR, (int64_t)S * ((int64_t)a.w * a.h + (int64_t)b.w * b.h + (int64_t)c.w * c.h));
            launch_pyr_down2(dsrc + a.off, a.w, a.h, a.pitch, a.img_bytes, dsrc + b.off, b.w, b.h, b.pitch, b.img_bytes,
                             dsrc + c.off, c.w, c.h, c.pitch, c.img_bytes, S, st, 0, zero, nzero);
        } else {
            ProfScope ps(ctx, FPM_K_PYR, (int64_t)S * ((int64_t)a.w * a.h + (int64_t)b.w * b.h));
            launch_pyr_down(dsrc + a.off, a.w, a.h, a.pitch, a.img_bytes, dsrc + b.off, b.w, b.h, b.pitch, b.img_bytes, S,
                            st, 0, zero, nzero);
        }
    }
}

// The split top layer's maps: k_warp (which zeroes the plan's counters) then k_ncc_tile, or k_ncc_map for the template
// levels beyond its tile form.
void enqueue_top_split_maps(fpm_ctx* ctx) {
    Plan& P = ctx->plan;
    const int L = P.L, S = P.S, J = S * P.nang;
    hipStream_t st = ctx->stream;
    const SrcLevel& top = ctx->src[L];
    const TmplLevel& tt = ctx->tmpl[L];
    {
        const int64_t bytes = (int64_t)P.nang * top.w * top.h;
        ProfScope ps(ctx, FPM_K_TOP_WARP, bytes * S);
        launch_warp(P.d_jobs.as<WarpJob>(P.off_warp), J, P.max_canvas, st, P.d_livecnt.as<int32_t>(), P.nzero);
    }
    {
        int64_t bytes = 0;
        for (int a = 0; a < P.nang; ++a) bytes += 4LL * P.map_w[a] * P.map_h[a];
        ProfScope ps(ctx, FPM_K_TOP_NCC, bytes * S);
        if (ncc_tile_fits(tt.w, tt.h)) {
            int mw = 0, mh = 0;
            for (int a = 0; a < P.nang; ++a) { mw = std::max(mw, P.map_w[a]); mh = std::max(mh, P.map_h[a]); }
            launch_ncc_tile(P.d_jobs.as<NccJob>(P.off_ncc), J, mw, mh, tt.w, tt.h, st);
        } else {
            launch_ncc_map(P.d_jobs.as<NccJob>(P.off_ncc), J, P.max_map, tt.w * tt.h, st);
        }
    }
}

// k_top_fused's dynamic LDS for the plan (its largest canvas and map), or 0 where the fused form cannot run: block
// mode, a template level beyond k_ncc_tile's form, no job, or more LDS than the kernel's static arrays leave of the
// default 64 KB launch limit (tests/test_gpu_parity.py::test_top_fused_lds_threshold runs canvases either side of it).
// need (optional): the LDS the largest job asks for, whatever the limit
size_t plan_top_fused_lds(const fpm_ctx* ctx, size_t* need = nullptr) {
    const Plan& P = ctx->plan;
    const TmplLevel& tt = ctx->tmpl[P.L];
    if (need) *need = 0;
    if (P.by_block || !ncc_tile_fits(tt.w, tt.h) || P.S * P.nang <= 0) return 0;
    size_t lds = 0;
    for (int a = 0; a < P.nang; ++a) lds = std::max(lds, top_fused_lds(P.top[a].bw, P.top[a].bh, tt.w, tt.h));
    if (need) *need = lds;
    return lds > top_fused_lds_limit() ? 0 : lds;
}

// What a launch of k_top_fused may do beside the plain form (TopFusedOpts), decided per plan when the launch is recorded:
//   level_copy  the taps read an LDS copy of the source level in every job whose map region holds it (copy_angles, where
//               asked for: how many of the plan's angles).  The copy lies in the map's LDS, so neither the launch's
//               dynamic LDS (plan_top_fused_lds: the fused / split choice) nor the workgroups per CU change.  Needs a
//               border colour of one byte;
//   bound       k_top_mma's f32 bound ahead of the exact score, under k_top_mma's conditions (plan_top_mma: area <= 258,
//               layer score > 0.01, not ResultEqual1) and with its constants (top_mma_thresholds).
TopFusedOpts plan_top_fused_opts(const fpm_ctx* ctx, int* copy_angles = nullptr) {
    const Plan& P = ctx->plan;
    const TmplLevel& tt = ctx->tmpl[P.L];
    const SrcLevel& top = ctx->src[P.L];
    TopFusedOpts o{};
    int fits = 0;
    for (int a = 0; a < P.nang; ++a) fits += top_fused_level_fits(top.w, top.h, P.map_w[a], P.map_h[a]) ? 1 : 0;
    o.level_copy = fits > 0 && ctx->border >= 0 && ctx->border <= 255 ? 1 : 0;
    if (copy_angles) *copy_angles = o.level_copy ? fits : 0;
    const double thr = P.layer_score[P.L];
    o.area = (uint32_t)(tt.w * tt.h);
    if (o.area <= 258 && thr > 0.01 && !tt.equal1 && tt.px.size() == (size_t)o.area) {
        TopMmaArgs A{};
        A.area = (int32_t)o.area;
        top_mma_thresholds(A, thr, tt);
        o.thrK = A.thrK; o.E = A.E;
        for (uint8_t v : tt.px) o.tsum += v;
        o.bound = 1;
    }
    return o;
}

// The top layer's form as the search selects it: *fused_lds > 0 = k_top_fused with that much dynamic LDS (small
// canvases with the plain peak path and enough (source, angle) jobs to fill the chip; FPM_TOP_FUSED=0 keeps the
// three-kernel form, =1 forces the fused one whatever the job count), *use_mma = the matrix-core form (where the plan
// admits it, except where the fused kernel applies; FPM_TOP_MMA=1 takes it there too), else the split chain.  Both
// switches are read when the search is recorded (once per plan)
void plan_top_choice(const fpm_ctx* ctx, size_t* fused_lds, bool* use_mma) {
    const Plan& P = ctx->plan;
    const char* top_env = getenv("FPM_TOP_FUSED");
    const int top_mode = top_env ? atoi(top_env) : -1;
    *fused_lds = 0;
    if (top_mode != 0 && (P.S * P.nang >= kTopFusedMinJobs || top_mode == 1)) *fused_lds = plan_top_fused_lds(ctx);
    const char* mma_env = getenv("FPM_TOP_MMA");
    *use_mma = P.top_mma && (*fused_lds == 0 || (mma_env && atoi(mma_env) == 1));
    if (*use_mma) *fused_lds = 0;
}

// The top-layer peak pass's arguments as the plan gives them (the launchers' own fields are set by the callers)
NmsArgs plan_nms_args(const fpm_ctx* ctx) {
    const Plan& P = ctx->plan;
    const TmplLevel& tt = ctx->tmpl[P.L];
    NmsArgs na{};
    na.jobs = P.d_jobs.as<NmsJob>(P.off_nms);
    na.peaks = P.d_peaks.as<Peak>();
    na.counts = P.d_counts.as<int32_t>();
    na.tw = tt.w; na.th = tt.h; na.cap = P.cap; na.by_block = P.by_block ? 1 : 0;
    na.mfc = ctx->prm.semantics == FPM_SEMANTICS_MFC ? 1 : 0;
    na.thr = P.layer_score[P.L]; na.overlap = ctx->prm.max_overlap;
    na.lds_blocks = 0;
    na.cand = nullptr; na.cand_cnt = nullptr; na.cand_cap = 0; na.cand_lds = 0; na.stamps = nullptr;
    na.skey = nullptr; na.sdone = nullptr;
    return na;
}

int enqueue_search(fpm_ctx* ctx) {
    Plan& P = ctx->plan;
    const int L = P.L, S = P.S, J = S * P.nang;
    const int stop = P.stop;   // the last refined layer (the plan's copy: nothing here reads the context's parameters for it)
    hipStream_t st = ctx->stream;
    uint8_t* dsrc = ctx->d_src.as<uint8_t>();
    const SrcLevel& top = ctx->src[L];
    P.step_layers = 0;   // (set again by the launches recorded below)
    P.top_lists = false;
    // small canvases with the plain peak path: the whole top layer as one kernel (k_top_fused), canvas and map in
    // LDS, when there are enough (source, angle) jobs to fill the chip: one workgroup runs a job's warp, map and
    // peak loop serially (33 us for a single Src7 source's 41 jobs against 24 us for the three split kernels; 75.5
    // against 106.4 us at 1763 jobs, profiles/r02_z/lat_r02_z.txt).  FPM_TOP_FUSED=0 keeps the three-kernel form,
    // FPM_TOP_FUSED=1 forces the fused one whatever the job count (tests, profiling comparisons); else the matrix-core
    // top layer (k_top_mma + greedy peaks from its lists) where the plan admits it: plan_top_choice
    size_t fused_lds = 0;
    bool use_mma = false;
    plan_top_choice(ctx, &fused_lds, &use_mma);
    int32_t* live[2] = {P.d_live.as<int32_t>(), P.d_live.as<int32_t>() + P.C};
    int32_t* livecnt = P.d_livecnt.as<int32_t>();
    CandInitArgs ca;   // the top peaks -> candidate states and the first live list (k_cand_init, or fused in k_nms)
    ca.peaks = P.d_peaks.as<Peak>();
    ca.counts = P.d_counts.as<int32_t>();
    ca.angles = P.d_top.as<TopAngle>();
    ca.top_nodes = P.d_topn.as<AngleNode>();
    ca.state = P.d_state.as<CandState>();
    ca.live = live[0];
    ca.live_count = livecnt + 0;
    ca.nang = P.nang; ca.cap = P.cap; ca.total = P.C;
    ca.center = P.center;
    ca.refine = L > stop ? (L - 1 == stop ? 2 : 1) : 0;   // (no refinement at all when L == stop: MatchToolDlg.cpp:949-953)
    bool cand_fused = false;
    // the fused top layer also initialises the candidates (cand_init_job) when the peaks fit its LDS list; its
    // live-list atomics then need the counters zeroed by an earlier launch: the first pyramid level's
    const bool top_init = fused_lds > 0 && P.cap <= kNmsInitCap && (size_t)J * P.cap == (size_t)P.C;
    // L >= 1: the first pyrDown launch zeroes the counters before the top kernel's live-list atomics.  L == 0: no
    // pyramid launch precedes it, so its block 0 zeroes them -- safe only because the candidate init then runs in
    // mode 1 (refine == 0: states and live list written directly, no live-count atomics); launch_top_fused checks it
    // (L == stop == 1 also runs mode 1, behind the pyramid launch's zeroing)
    const bool pyr_zero = (top_init && L >= 1) || use_mma;   // (use_mma implies L >= 1: plan_top_mma)
    enqueue_pyramid(ctx, pyr_zero);
    NmsArgs na = plan_nms_args(ctx);
    if (fused_lds > 0) {
        int64_t bytes = (int64_t)P.nang * top.w * top.h;
        for (int a = 0; a < P.nang; ++a) bytes += 4LL * P.map_w[a] * P.map_h[a];
        ProfScope ps(ctx, FPM_K_TOP_NCC, bytes * S);
        launch_top_fused(P.d_jobs.as<WarpJob>(P.off_warp), P.d_jobs.as<NccJob>(P.off_ncc), na, J, fused_lds,
                         pyr_zero ? nullptr : P.d_livecnt.as<int32_t>(), pyr_zero ? 0 : P.nzero, st,
                         top_init ? &ca : nullptr, P.d_jobs.as<int32_t>(P.off_order), false, plan_top_fused_opts(ctx));
        cand_fused = top_init;
    }
    if (use_mma) {
        const int mdim = P.nmax.max_map_dim;
        const long mpx = P.nmax.max_map_px;
        TopMmaArgs ta = P.tma;
        {   // canvases, correlation, scores and the lists of outputs >= the layer score; profiling bytes: the top level
            // read per angle (its share of B_top; the map is never written)
            ProfScope ps(ctx, FPM_K_TOP_NCC, (int64_t)S * P.nang * top.w * top.h);
            ta.mode = 0;
            launch_top_mma(ta, st);
        }
        const bool ci_ok = !P.by_block && P.cap <= kNmsInitCap && (size_t)J * P.cap == (size_t)P.C;
        NmsArgs ga = na;
        ga.cand = P.d_ncand.as<int32_t>(); ga.cand_val = P.d_tcandv.as<float>();
        ga.cand_cnt = ta.cand_cnt; ga.cand_cap = P.tcand_cap;
        ga.reset_untaken = P.by_block ? 1 : 0;
        {   // (its bytes, the map term of B_top the lists stand in for, are added when the pass completes)
            ProfScope ps(ctx, FPM_K_TOP_NMS, 0);
            launch_top_greedy(ga, J, P.max_cells, st, ci_ok ? &ca : nullptr);
        }
        P.top_lists = true;
        {   // the maps the lists could not give (overflow, or a shape the greedy form does not take): full maps
            ProfScope ps(ctx, FPM_K_TOP_MAP, 0);
            ta.mode = 1;
            launch_top_mma(ta, st);
        }
        {   // ... and their peaks by the split kernels, which skip the maps the greedy form took (cand_cnt < 0)
            ProfScope ps(ctx, FPM_K_TOP_NMS, 0);
            NmsArgs fa = na;
            fa.cand = ga.cand; fa.cand_cnt = ga.cand_cnt; fa.cand_cap = P.tcand_cap;
            if (P.by_block) {
                fa.skey = (uint64_t*)(P.d_livecnt.as<int32_t>() + P.off_skey);
                fa.sdone = P.d_livecnt.as<int32_t>() + P.off_skey + 6 * J;
            }
            launch_nms(fa, J, P.max_nblk, mdim, P.max_cells, st, P.max_nitems, ci_ok ? &ca : nullptr, mpx);
        }
        cand_fused = ci_ok;
    }
    // profiling bytes: each kernel's share of §8(d)'s B_top = sum_angles (W_L H_L + 4 |R_a|): the rotation reads the
    // top level, the correlation writes the map (the rotated canvases are this design's scratch)
    if (fused_lds == 0 && !use_mma) enqueue_top_split_maps(ctx);
    if (fused_lds == 0 && !use_mma) {
        ProfScope ps(ctx, FPM_K_TOP_NMS, 0);   // (reads the maps counted once in B_top)
        if (P.by_block) {   // (the counts and strip keys were zeroed by k_warp)
            na.cand = P.d_ncand.as<int32_t>(); na.cand_cnt = P.d_livecnt.as<int32_t>() + L + 2; na.cand_cap = kNmsCandCap;
            na.skey = (uint64_t*)(P.d_livecnt.as<int32_t>() + P.off_skey);
            na.sdone = P.d_livecnt.as<int32_t>() + P.off_skey + 6 * J;
        }
        const int mdim = P.nmax.max_map_dim;
        const long mpx = P.nmax.max_map_px;
        // plain path: k_nms also initialises the candidates (the live counter was zeroed by k_warp)
        cand_fused = !P.by_block && P.cap <= kNmsInitCap && (size_t)J * P.cap == (size_t)P.C;
        launch_nms(na, J, P.max_nblk, mdim, P.max_cells, st, P.max_nitems, cand_fused ? &ca : nullptr, mpx);
    }
    if (!cand_fused) {
        ProfScope ps(ctx, FPM_K_CAND_INIT, 0);
        launch_cand_init(ca, st);
    }
    // the prologue-stepped run: layers L-1 .. run_end, the leading small layers above the stop layer (none of them a
    // matResult = 1 layer).  From its second layer on, a layer's k_roi_small steps the previous layer's candidates in
    // its prologue over the unchanged live list (k_cand_step launches saved: run length - 1); one k_cand_step after
    // the run's last layer steps and compacts.  FPM_STEP_PROLOGUE=0 keeps one k_cand_step per layer (result-neutral).
    // Used for batches of at most kPrologueMaxSources sources, where the saved launches outweigh the prologue's
    // dependent loads on every workgroup's critical path (single Src7 search: 23 dispatches, 236.8 us of kernels vs
    // 25 and 244.6; a 43-source batch: k_roi_small 181 -> 218 us per pass, profiles/r04/gpu_r04g).
    // FPM_STEP_PROLOGUE=1 forces it, =0 disables it (read when the search is recorded, once per plan).
    const char* prol_env = getenv("FPM_STEP_PROLOGUE");
    const bool step_prologue = prol_env ? atoi(prol_env) != 0 : S <= kPrologueMaxSources;
    int run_end = L;
    if (step_prologue)
        for (int l = L - 1; l > stop; --l) {
            if (!roi_small_fits(ctx->tmpl[l].w, ctx->tmpl[l].h) || ctx->tmpl[l].equal1) break;
            run_end = l;
        }
    if (L - run_end < 2) run_end = L;   // a run of one layer has no prologue to fuse
    CandState* const state_buf[2] = {P.d_state.as<CandState>(), P.d_state2.as<CandState>()};
    RoiRecord* const rec_buf[2] = {P.d_rec.as<RoiRecord>(), P.d_rec2.as<RoiRecord>()};
    int cur_list = 0;   // live[cur_list]: the list the layer's ROIs come from; its count is livecnt[list_cnt]
    int list_cnt = 0;
    int run_k = 0;      // layers of the run done
    // the next layer's warp tables written by the step of this layer (RoiArgs::nt_tab): where that layer takes tables
    // (not small, not equal1) and every layer runs as one round; FPM_STEP_TABLES=0 keeps the k_roi_tables launches
    // (result-neutral: the same pure functions of the stepped state)
    const char* stab_env = getenv("FPM_STEP_TABLES");
    const bool step_tables = (stab_env ? atoi(stab_env) != 0 : true) && (size_t)P.C * P.n3 <= (size_t)P.slot_cap;
    bool tables_done = false;   // this layer's tables were written by the previous layer's step
    for (int l = L - 1; l >= stop; --l) {
        const int d = L - 1 - l;
        const SrcLevel& lv = ctx->src[l];
        const TmplLevel& tl = ctx->tmpl[l];
        const bool in_run = l >= run_end;
        RoiArgs ra{};
        ra.level = dsrc + lv.off; ra.level_stride = lv.img_bytes;
        ra.W = lv.w; ra.H = lv.h; ra.P = lv.pitch;
        ra.tmpl = ctx->d_tmpl.as<uint8_t>() + tl.off; ra.tw = tl.w; ra.th = tl.h; ra.tp = tl.pitch;
        ra.tmpl8 = ctx->d_tmpl8.as<int8_t>() + tl.off8; ra.tp8 = tl.p8; ra.nk = (tl.w + 63) / 64;
        ra.tsum = ctx->d_tsum.as<int32_t>() + tl.tsum_off;
        ra.n3 = P.n3;
        ra.fold = ctx->prm.use_simd ? 1 : 0;
        ra.equal1 = tl.equal1 ? 1 : 0;
        ra.per_source = P.nang * P.cap;
        ra.mean = tl.mean; ra.norm = tl.norm; ra.inv_area = tl.inv_area;
        ra.live = live[cur_list];
        ra.live_count = livecnt + list_cnt;
        ra.state = P.d_state.as<CandState>();
        ra.nodes = P.d_nodes.as<AngleNode>() + P.node_off[d];
        // per-level scratch geometry (the buffers are sized for the largest level)
        ra.tab = P.d_tab.as<int32_t>(); ra.tabw = roi_pitch_for(tl.w); ra.tabh = roi_tab_rows(tl.h);
        ra.tdesc = P.d_tdesc.as<int4>(); ra.tdesc_stride = P.tdesc_stride;
        ra.roi = P.d_roi.as<uint8_t>(); ra.roi_pitch = roi_pitch_for(tl.w); ra.roi_stride = P.roi_stride;
        ra.rowsum = P.d_rowsum.as<uint32_t>();
        ra.wtot = P.d_wtot.as<uint32_t>();
        ra.wtotq = P.d_wtotq.as<uint64_t>();
        ra.wedge = P.d_wedge.as<uint32_t>();
        ra.rec = P.d_rec.as<RoiRecord>();
        ra.step = l > stop ? 1 : 0;   // candidate step fused into k_roi_eval (the stop layer is decided on the host)
        ra.mark_reached0 = l - 1 == stop ? 1 : 0;
        ra.live_out = live[cur_list ^ 1];
        ra.live_out_count = livecnt + d + 1;
        ra.thr = P.layer_score[l];
        if (in_run) {
            // run layer k reads state_buf[(k + 1) & 1] (k = 0: the initial states, buffer 0) and records of layer k - 1
            // from rec_buf[(k + 1) & 1], writes state_buf[k & 1] and records to rec_buf[k & 1]
            ra.rec = rec_buf[run_k & 1];
            if (run_k > 0) {
                ra.state = state_buf[(run_k + 1) & 1];
                ra.state_out = state_buf[run_k & 1];
                ra.prev_rec = rec_buf[(run_k + 1) & 1];
                ra.prev_nodes = P.d_nodes.as<AngleNode>() + P.node_off[d - 1];
                ra.prev_thr = P.layer_score[l + 1];
                ra.prev_W = ctx->src[l + 1].w;
                ra.prev_H = ctx->src[l + 1].h;
                ra.live_out_count = livecnt + d;   // the survivors entering this layer (counted, not listed)
            }
        }
        if (step_tables && l - 1 >= stop && ra.step && !roi_small_fits(ctx->tmpl[l - 1].w, ctx->tmpl[l - 1].h) &&
            !ctx->tmpl[l - 1].equal1) {
            const TmplLevel& nt = ctx->tmpl[l - 1];
            ra.nt_tab = P.d_tab.as<int32_t>();
            ra.nt_nodes = P.d_nodes.as<AngleNode>() + P.node_off[d + 1];
            ra.nt_tabw = roi_pitch_for(nt.w); ra.nt_tabh = roi_tab_rows(nt.h);
            ra.nt_tw = nt.w; ra.nt_th = nt.h;
            ra.nt_W = ctx->src[l - 1].w; ra.nt_H = ctx->src[l - 1].h;
        }
        const int total_rois = P.C * P.n3;
        const bool small = roi_small_fits(tl.w, tl.h);   // one-kernel refinement of the ROI in LDS
        for (int base = 0; base < total_rois; base += P.slot_cap) {
            ra.slot_base = base;
            ra.slot_cap = std::min(P.slot_cap, total_rois - base);
            if (small) {
                ProfScope ps(ctx, FPM_K_ROI_SMALL, 0);
                launch_roi_small(ra, st);
                continue;
            }
            if (!tables_done) {
                ProfScope ps(ctx, FPM_K_ROI_TABLES, 0);
                launch_roi_tables(ra, st);
            }
            {
                ProfScope ps(ctx, FPM_K_ROI_WARP, 0);
                launch_roi_warp(ra, st);
            }
            {
                ProfScope ps(ctx, FPM_K_ROI_CORR, 0);
                launch_roi_corr(ra, st);
            }
            {
                ProfScope ps(ctx, FPM_K_ROI_EVAL, 0);
                launch_roi_eval(ra, st);
            }
        }
        tables_done = ra.nt_tab != nullptr;
        if (in_run && l > run_end) {   // the step runs in the next layer's prologue
            tables_done = false;
            ++run_k;
            continue;
        }
        if (small && ra.step) {
            ProfScope ps(ctx, FPM_K_CAND_STEP, 0);
            if (in_run && run_k > 0) {   // the run's last layer: step from its buffers into the canonical state
                ra.state = state_buf[run_k & 1];
                ra.state_out = state_buf[0];
                ra.rec = rec_buf[run_k & 1];
                ra.live_out_count = livecnt + d + 1;
            }
            launch_cand_step(ra, P.C, st);
            P.step_layers |= 1u << d;
        }
        if (ra.step) {
            cur_list ^= 1;
            list_cnt = d + 1;
        }
    }
    HIP_TRY(hipGetLastError());
    // results into pinned host memory (one kernel; only the stop-layer candidates' states and records)
    {
        PackArgs pa;
        pa.counts = P.d_counts.as<int32_t>(); pa.J = J;
        pa.peaks = P.d_peaks.as<Peak>(); pa.C = P.C;
        pa.cap = P.cap;
        if ((size_t)J * P.cap != (size_t)P.C) { ctx->err = "plan layout: C != J * cap"; return FPM_E_INTERNAL; }
        pa.livecnt = livecnt; pa.nlive = L + 2;
        pa.live0 = L > stop ? live[cur_list] : nullptr;   // the stop layer's list
        pa.live0_count = livecnt + (L > stop ? L - 1 - stop : 0);
        pa.state = P.d_state.as<CandState>();
        pa.rec = P.d_rec.as<RoiRecord>();
        pa.n3 = P.n3;
        pa.host = P.h_dev;
        pa.o_counts = P.h_counts; pa.o_peaks = P.h_peaks; pa.o_live = P.h_live;
        pa.o_live0 = P.h_live0; pa.o_state0 = P.h_state; pa.o_rec0 = P.h_rec;
        launch_pack(pa, st);
        HIP_TRY(hipGetLastError());
    }
    return FPM_OK;
}

// Host half of the search, split at the one point where a search can be sharded by angle:
//   collect_candidates: every top-layer candidate of source s in the reference's push order (angle-major, then
//     peak order, TemplateMatcher.cpp:157-211) with its own refinement outcome (:262-371) — each candidate's
//     descent is independent of every other candidate's, so a shard of the angle list yields exactly the
//     records of its angles;
//   merge_candidates: everything after that which couples candidates — the std::sort of the top list (:214),
//     vecAllResult in sorted order, filterWithScore, filterWithRotatedRect, the final sort and the
//     s_SingleTargetMatch conversion (:373-432).  It needs the complete push-order sequence, i.e. the shards'
//     records concatenated in shard order.
// pos[id] = index of candidate id in the stop layer's live list (k_pack's compact states / records), -1 if absent.
// The stop layer is layer 0, or layer 1 in fast mode (fpm_params.stop_layer, MatchToolDlg.cpp:936-1037): the same
// decision from that layer's records, no sub-pixel fit (:1013), the back-mapped ptLT doubled in float (:1035).
void collect_candidates(fpm_ctx* ctx, int s, const std::vector<int>& pos, std::vector<fpm_candidate>& out) {
    Plan& P = ctx->plan;
    const int L = P.L, stop = P.stop;
    out.clear();
    if (P.nang == 0) return;
    const char* h = P.h_out.as<char>();
    const int32_t* counts = (const int32_t*)(h + P.h_counts);
    const Peak* peaks = (const Peak*)(h + P.h_peaks);
    const CandState* state = (const CandState*)(h + P.h_state);
    const RoiRecord* rec = (const RoiRecord*)(h + P.h_rec);
    const TmplLevel& t0 = ctx->tmpl[0];
    const double astep = std::atan(2.0 / std::max(t0.w, t0.h)) * kR2D;   // layer 0's angle step (:283)
    const SrcLevel& lv = ctx->src[stop];
    const F2 sc = f2((lv.w - 1) / 2.0f, (lv.h - 1) / 2.0f);
    // each angle's candidates go to their place in push order (angle-major): the angles run on the host pool when
    // there are many candidates
    std::vector<int> first(P.nang + 1, 0);
    for (int a = 0; a < P.nang; ++a) first[a + 1] = first[a] + counts[s * P.nang + a];
    out.resize(first[P.nang]);
    auto angle = [&](int a) {
        const int job = s * P.nang + a;
        HostMatch nm[3];   // one candidate's n3 (1 or 3) angle results
        int o = first[a];
        for (int r = 0; r < counts[job]; ++r) {
            const int id = job * P.cap + r;
            const Peak& pk = peaks[id];
            fpm_candidate c{};
            c.top_score = (double)pk.score;
            c.angle_index = P.a0 + a;
            c.peak_rank = r;
            c.source = s;
            if (L <= stop) {   // iTopLayer <= iStopLayer (:272-276; MatchToolDlg.cpp:949-953: ptLT * 2 when L == 1)
                const F2 pt = f2((float)pk.x - P.top[a].tx, (float)pk.y - P.top[a].ty);
                const double rad = -P.angles[a] * kD2R;
                const F2 lt = rotate_pt(f2(pt.x, pt.y), P.center, std::cos(rad), std::sin(rad));
                const F2 up_lt = L == 0 ? lt : f2(lt.x * 2, lt.y * 2);
                c.x = up_lt.x; c.y = up_lt.y; c.score = pk.score; c.angle = P.angles[a]; c.kept = 1;
                out[o++] = c;
                continue;
            }
            const int li = pos[id];
            if (li < 0) { out[o++] = c; continue; }   // broke out at a layer > 0 (:331-332)
            const CandState& cs = state[li];
            // the stop layer (:282-358) from the device's ROI records
            const int d = L - 1 - stop;
            int imax = 0;
            double big = -1;
            for (int j = 0; j < P.n3; ++j) {
                const RoiRecord& rr = rec[(size_t)li * P.n3 + j];
                HostMatch m{};
                m.ptx = rr.mx; m.pty = rr.my;
                m.score = rr.score;
                m.angle = P.nodes[d][(size_t)cs.node * P.n3 + j].angle;
                m.on_border = rr.on_border != 0;
                for (int x = 0; x < 3; ++x)
                    for (int y = 0; y < 3; ++y) m.vec[x][y] = rr.vec[x * 3 + y];
                nm[j] = m;
                if (nm[j].score > big) { imax = j; big = nm[j].score; }
            }
            if (nm[imax].score < P.layer_score[stop]) { out[o++] = c; continue; }
            if (ctx->run_prm.subpixel && stop == 0 && !nm[imax].on_border && imax != 0 && imax != 2) {
                double nx = 0, ny = 0, na = 0;
                subpix_estimation(nm, &nx, &ny, &na, astep, imax);
                nm[imax].ptx = nx; nm[imax].pty = ny;
                nm[imax].angle = na;
            }
            const double nang = nm[imax].angle;
            const double rad = nang * kD2R;
            const F2 r0 = rotate_pt(f2(cs.lt.x * 2, cs.lt.y * 2), sc, std::cos(rad), std::sin(rad));
            const F2 pad = f2(r0.x - 3, r0.y - 3);
            F2 p = f2((float)(nm[imax].ptx + pad.x), (float)(nm[imax].pty + pad.y));
            const double nrad = -nang * kD2R;
            p = rotate_pt(p, sc, std::cos(nrad), std::sin(nrad));
            if (stop) p = f2(p.x * 2, p.y * 2);   // to layer 0's coordinates, in float before it widens (MatchToolDlg.cpp:1035)
            c.x = p.x; c.y = p.y; c.score = nm[imax].score; c.angle = nang; c.kept = 1;
            out[o++] = c;
        }
    };
    if (first[P.nang] < 1024) {
        for (int a = 0; a < P.nang; ++a) angle(a);
    } else {
        host_parallel(P.nang, angle);
    }
}

// vecAllResult after filterWithScore (:214, :262-358, :373-378) when that needs no sort emulation: if the kept
// candidates scoring at least the threshold have pairwise distinct scores (and none is NaN), the sorted order after
// filterWithScore is the unique descending order, whatever the push order and the first std::sort did with equal
// top scores.  LSD radix sort on order-preserving 64-bit keys; false (nothing decided) on a tie or a NaN, and the
// caller replays both std::sorts.
static bool select_distinct_scores(const fpm_params& prm, const fpm_candidate* cand, int n, std::vector<int>& src) {
    struct SK { uint64_t k; int32_t i; };
    std::vector<SK> a, b;
    a.reserve(n);
    for (int i = 0; i < n; ++i) {
        const fpm_candidate& c = cand[i];
        if (!c.kept) continue;
        if (std::isnan(c.score)) return false;
        if (c.score < prm.score) continue;
        uint64_t u;
        std::memcpy(&u, &c.score, 8);
        u = (u >> 63) ? ~u : (u | (1ULL << 63));   // ascending key = ascending score
        a.push_back({~u, i});                        // ascending ~key = descending score
    }
    const size_t m = a.size();
    b.resize(m);
    uint64_t diff = 0;
    for (size_t t = 1; t < m; ++t) diff |= a[t].k ^ a[0].k;
    for (int sh = 0; sh < 64; sh += 8) {
        if (!((diff >> sh) & 0xFF)) continue;   // every key shares this byte
        size_t cnt[257] = {};
        for (const SK& e : a) cnt[((e.k >> sh) & 0xFF) + 1]++;
        for (int d = 0; d < 256; ++d) cnt[d + 1] += cnt[d];
        for (const SK& e : a) b[cnt[(e.k >> sh) & 0xFF]++] = e;
        a.swap(b);
    }
    for (size_t t = 1; t < m; ++t)
        if (cand[a[t].i].score == cand[a[t - 1].i].score) return false;   // equal scores (+0 == -0 included)
    src.resize(m);
    for (size_t t = 0; t < m; ++t) src[t] = a[t].i;
    return true;
}

// filterWithRotatedRect (:1133-1194) with its pair tests on the device: k_overlap_pairs decides every pair i < j
// whose boxes overlap (the exact test of fpm_rrect.h, bit-identical to the host's), and the host replays the
// reference's loop on those decisions -- for i in order, skipped once deleted, each listed j not yet deleted
// deletes the lower-scored of the two (j, as v is sorted by descending score) -- evaluating itself only the pairs
// whose point order needs acos.  The same deletions as filter_with_rotated_rect.  Returns false (nothing done, the
// caller runs the host filter) without a context, for short lists, or when a rectangle has more overlapping
// partners than the kernel keeps.
constexpr int kOverlapDeviceMin = 1024;   // FPM_OVERLAP_DEVICE_MIN overrides (tests force small lists through it)
struct OverlapStats {
    int host_pairs = 0, flags = 0, entries = 0;
};
static bool overlap_filter_device(fpm_ctx* ctx, std::vector<HostMatch>& v, double max_overlap, int min_n = 0,
                                  OverlapStats* st = nullptr) {
    const int n = (int)v.size();
    if (min_n <= 0) {
        min_n = kOverlapDeviceMin;
        if (const char* e = getenv("FPM_OVERLAP_DEVICE_MIN")) min_n = std::max(1, atoi(e));
    }
    if (!ctx || n < min_n) return false;
    const int cap = 48 * n;
    const size_t boff = (sizeof(OvRect) * (size_t)n + 15) / 16 * 16;
    const size_t rbytes = boff + sizeof(float4) * (size_t)n;   // rects, then boxes
    if (ctx->h_ov_in.ensure(rbytes) != hipSuccess || ctx->d_ov.ensure(rbytes + 64) != hipSuccess ||
        ctx->h_ov_out.ensure(sizeof(int32_t) * ((size_t)cap + 2 * (size_t)n + 16)) != hipSuccess)
        return false;
    OvRect* rin = ctx->h_ov_in.as<OvRect>();
    float4* bin = ctx->h_ov_in.as<float4>(boff);
    static const bool tail_times = [] { const char* e = getenv("FPM_TAIL_TIMES"); return e && *e == '1'; }();
    using clk = std::chrono::steady_clock;
    const clk::time_point q0 = clk::now();
    auto geom = [&](int i0, int i1) {   // corners and boxes exactly as filter_with_rotated_rect computes them
        for (int i = i0; i < i1; ++i) {
            OvRect& o = rin[i];
            rrect_corners(v[i].rect, o.c);
            float x0 = o.c[0].x, x1 = o.c[0].x, y0 = o.c[0].y, y1 = o.c[0].y;
            for (int k = 1; k < 4; ++k) {
                x0 = std::min(x0, o.c[k].x); x1 = std::max(x1, o.c[k].x);
                y0 = std::min(y0, o.c[k].y); y1 = std::max(y1, o.c[k].y);
            }
            o.w = v[i].rect.w; o.h = v[i].rect.h;
            bin[i] = make_float4(x0 - 1.f, y0 - 1.f, x1 + 1.f, y1 + 1.f);
        }
    };
    host_parallel((n + 511) / 512, [&](int t) { geom(t * 512, std::min(n, t * 512 + 512)); });
    const clk::time_point q1 = clk::now();
    int32_t* hout = ctx->h_ov_out.as<int32_t>();   // [meta 16][offcnt 2n][lists cap]
    int32_t* dout = nullptr;
    if (hipHostGetDevicePointer((void**)&dout, ctx->h_ov_out.p, 0) != hipSuccess) return false;
    OvRect* drects = ctx->d_ov.as<OvRect>();
    int32_t* dmeta = (int32_t*)((char*)ctx->d_ov.p + rbytes);
    if (hipMemcpyAsync(drects, rin, rbytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemsetAsync(dmeta, 0, 2 * sizeof(int32_t), ctx->stream) != hipSuccess)
        return false;
    launch_overlap_pairs(drects, ctx->d_ov.as<float4>(boff), n, max_overlap, dout + 16 + 2 * n, cap, dout + 16, dmeta,
                         ctx->stream);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(hout, dmeta, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return false;
    const clk::time_point q2 = clk::now();
    if (st) { st->flags = hout[1]; st->entries = hout[0]; }
    if (hout[1] != 0) return false;   // a rectangle with too many partners, or the list overflowed
    // the outputs, written by the device into mapped host memory, read once into ordinary memory
    std::vector<int32_t> local((size_t)2 * n + hout[0]);
    std::memcpy(local.data(), hout + 16, sizeof(int32_t) * local.size());
    const clk::time_point q3 = clk::now();
    const int32_t* offcnt = local.data();
    const int32_t* lists = local.data() + 2 * n;
    std::vector<char> del(n, 0);
    int host_pairs = 0;
    // v is sorted by descending score, so "the lower-scored of the two" is j; a NaN score breaks that order, and then
    // the scores are compared as the reference does
    bool monotone = true;
    for (int i = 0; i + 1 < n && monotone; ++i) monotone = v[i].score >= v[i + 1].score;
    for (int i = 0; i < n; ++i) {
        if (del[i]) continue;
        const int32_t* L = lists + offcnt[2 * i];
        for (int k = 0; k < offcnt[2 * i + 1]; ++k) {
            const int32_t e = L[k];
            const int j = e >= 0 ? e : ~e;
            if (del[j]) continue;
            if (e < 0 && (++host_pairs, !rrect_pair_drops(v[i].rect, v[j].rect, max_overlap))) continue;
            if (monotone || v[i].score >= v[j].score) del[j] = 1;
            else del[i] = 1;
        }
    }
    size_t w = 0;
    for (int i = 0; i < n; ++i)
        if (!del[i]) v[w++] = v[i];
    v.resize(w);
    if (st) st->host_pairs = host_pairs;
    if (tail_times) {
        auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "overlap-dev n=%d geom %.3f device %.3f read %.3f replay %.3f ms, %d pair entries, %d decided on the host\n",
                n, ms(q0, q1), ms(q1, q2), ms(q2, q3), ms(q3, clk::now()), hout[0], host_pairs);
    }
    return true;
}

// Returns false when `cand` is not in push order (angle_index ascending, peak_rank 0, 1, ... within an angle).
// stop: the search's stop layer (the plan's), or -1 to derive it from prm (fpm_merge_candidates has no plan).
// poses (optional): the raw pose of every result, in result order.
bool merge_candidates(const fpm_params& prm, int t0w, int t0h, const fpm_candidate* cand, int n,
                      std::vector<fpm_result>& out, fpm_ctx* dev_ctx, int stop = -1,
                      std::vector<RawPose>* poses = nullptr) {
    out.clear();
    if (poses) poses->clear();
    for (int i = 0; i < n; ++i) {
        const bool first = i == 0 || cand[i].angle_index != cand[i - 1].angle_index;
        if (first ? (cand[i].peak_rank != 0 || (i > 0 && cand[i].angle_index < cand[i - 1].angle_index))
                  : cand[i].peak_rank != cand[i - 1].peak_rank + 1)
            return false;
    }
    // FPM_TAIL_TIMES=1: per-stage wall clocks of this tail on stderr (profiling aid)
    static const bool tail_times = [] { const char* e = getenv("FPM_TAIL_TIMES"); return e && *e == '1'; }();
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = clk::now();
    clk::time_point t1 = t0;
    std::vector<HostMatch> all;
    // the overlap filter's rectangle: the stop layer's template size scaled to layer 0 (MatchToolDlg.cpp:1053-1054) --
    // with fast mode and a top layer >= 1 the layer-1 size times two, which exceeds an odd level-0 size by one.
    // Without a plan the top layer comes from the level-0 size and MinReduceArea by the search's own rule.
    if (stop < 0) stop = std::min(prm.stop_layer ? 1 : 0, top_layer(t0w, t0h, (int)std::sqrt((double)prm.min_reduce_area)));
    const int rw = stop ? (t0w + 1) / 2 * 2 : t0w, rh = stop ? (t0h + 1) / 2 * 2 : t0h;
    // vecAllResult entry from a candidate record, with its rotated rectangle (:380-390)
    auto fill = [&](HostMatch& m, const fpm_candidate& c) {
        m = HostMatch{};
        m.ptx = c.x; m.pty = c.y; m.score = c.score; m.angle = c.angle;
        const double rad = -m.angle * kD2R;
        const float cs = (float)std::cos(rad), sn = (float)std::sin(rad);
        const F2 lt = f2((float)m.ptx, (float)m.pty);
        const F2 rt = f2(lt.x + rw * cs, lt.y - rw * sn);
        const F2 rb = f2(rt.x + rh * sn, rt.y + rh * cs);
        m.rect = rrect_from3(lt, rt, rb);
        m.del = false;
    };
    std::vector<int> src;   // candidate index of each vecAllResult entry after filterWithScore
    if (select_distinct_scores(prm, cand, n, src)) {
        t1 = clk::now();
    } else {
        // std::sort(vecMatchParameter, compareScoreBig2Small) (:214) over the push-order sequence.  The permutation
        // std::sort produces depends only on the sequence of comparison results, so sorting light (score, index)
        // keys with the same comparator reproduces the reference's order of equal scores exactly.
        struct Key { double score; int i; };
        auto by_score = [](const Key& l, const Key& r) { return l.score > r.score; };
        std::vector<Key> order(n);
        for (int i = 0; i < n; ++i) order[i] = {cand[i].top_score, i};
        std::sort(order.begin(), order.end(), by_score);
        // vecAllResult in sorted-candidate order (:262-358) is the kept candidates' sequence; filterWithScore's
        // std::sort (:373-378) sees exactly their scores in that order, so it runs on (score, candidate) keys too
        std::vector<Key> ks;
        ks.reserve(n);
        for (const Key& k : order)
            if (cand[k.i].kept) ks.push_back({cand[k.i].score, k.i});
        t1 = clk::now();
        std::sort(ks.begin(), ks.end(), by_score);
        size_t m = 0;   // the sorted list ends at the first score below the threshold (filter_with_score)
        while (m < ks.size() && !(ks[m].score < prm.score)) ++m;
        src.resize(m);
        for (size_t t = 0; t < m; ++t) src[t] = ks[t].i;
    }
    const clk::time_point t2 = clk::now();
    const int na = (int)src.size();
    all.resize(na);
    if (na <= 512) {
        for (int i = 0; i < na; ++i) fill(all[i], cand[src[i]]);
    } else {
        host_parallel((na + 255) / 256, [&](int t) {
            for (int i = t * 256; i < std::min(na, t * 256 + 256); ++i) fill(all[i], cand[src[i]]);
        });
    }
    const clk::time_point t3 = clk::now();
    if (!overlap_filter_device(dev_ctx, all, prm.max_overlap)) filter_with_rotated_rect(all, prm.max_overlap);
    const clk::time_point t4 = clk::now();
    std::sort(all.begin(), all.end(), score_big2small);
    if (tail_times) {
        auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "tail n=%d sort1+collect %.3f score %.3f rects %.3f overlap %.3f final %.3f ms -> %zu\n", n,
                ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, clk::now()), all.size());
    }
    if (prm.semantics == FPM_SEMANTICS_MFC) {   // MatchToolDlg.cpp:1080-1116
        for (const HostMatch& m : all) {
            const double rad = -m.angle * kD2R;
            fpm_result o;
            o.lt_x = m.ptx; o.lt_y = m.pty;   // f64 corners from the f64 point (the Qt class rounds to Point2f)
            o.rt_x = o.lt_x + t0w * std::cos(rad); o.rt_y = o.lt_y - t0w * std::sin(rad);
            o.lb_x = o.lt_x + t0h * std::sin(rad); o.lb_y = o.lt_y + t0h * std::cos(rad);
            o.rb_x = o.rt_x + t0h * std::sin(rad); o.rb_y = o.rt_y + t0h * std::cos(rad);
            o.cx = (o.lt_x + o.rt_x + o.rb_x + o.lb_x) / 4;
            o.cy = (o.lt_y + o.rt_y + o.rb_y + o.lb_y) / 4;
            o.angle = -m.angle;   // negated, wrapped to [-180, 180]
            if (o.angle < -180) o.angle += 360;
            if (o.angle > 180) o.angle -= 360;
            o.score = m.score;
            out.push_back(o);
            if (poses) poses->push_back({(float)m.ptx, (float)m.pty, m.angle});
            if ((int)out.size() == prm.max_pos) break;   // at most MaxPos rows (:1115-1116)
        }
        return true;
    }
    for (const HostMatch& m : all) {   // :406-432
        const double rad = -m.angle * kD2R;
        const float cs = (float)std::cos(rad), sn = (float)std::sin(rad);
        const F2 lt = f2((float)m.ptx, (float)m.pty);
        const F2 rt = f2(lt.x + t0w * cs, lt.y - t0w * sn);
        const F2 lb = f2(lt.x + t0h * sn, lt.y + t0h * cs);
        const F2 rb = f2(rt.x + t0h * sn, rt.y + t0h * cs);
        const F2 c = f2((lt.x + rt.x + lb.x + rb.x) / 4.0f, (lt.y + rt.y + lb.y + rb.y) / 4.0f);
        fpm_result o;
        o.lt_x = lt.x; o.lt_y = lt.y; o.rt_x = rt.x; o.rt_y = rt.y;
        o.rb_x = rb.x; o.rb_y = rb.y; o.lb_x = lb.x; o.lb_y = lb.y;
        o.cx = c.x; o.cy = c.y; o.angle = m.angle; o.score = m.score;
        out.push_back(o);
        if (poses) poses->push_back({lt.x, lt.y, m.angle});
    }
    return true;
}

// Launch the search: replay the captured graph (every pointer and launch shape is fixed by the plan and the
// source slab; data-dependent work sizes live in device counters), or enqueue it eagerly when profiling.
int launch_search(fpm_ctx* ctx) {
    if (ctx->prof) return enqueue_search(ctx);   // per-launch HIP events need the eager path
    if (!ctx->graph || ctx->graph_plan != ctx->plan_builds || ctx->graph_src != ctx->d_src.p) {
        if (ctx->graph) { (void)hipGraphExecDestroy(ctx->graph); ctx->graph = nullptr; }
        hipGraph_t g = nullptr;
        HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue_search(ctx);
        const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
        if (rc != FPM_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
        HIP_TRY(e);
        const hipError_t ie = hipGraphInstantiate(&ctx->graph, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        HIP_TRY(ie);
        ctx->graph_plan = ctx->plan_builds;
        ctx->graph_src = ctx->d_src.p;
    }
    HIP_TRY(hipGraphLaunch(ctx->graph, ctx->stream));
    return FPM_OK;
}

// fpm_params.bitwise_not (MatchToolDlg.cpp:788-796): bring level 0 of the source slab to the polarity the search
// asks for, on the context's stream ahead of the search graph.  The inversion is an involution, so switching the
// option off over a batch that is still staged restores the uploaded bytes; the upper levels are rebuilt from level
// 0 by every pass.
int apply_polarity(fpm_ctx* ctx) {
    const bool want = ctx->prm.bitwise_not != 0;
    if (want == ctx->src_inverted) return FPM_OK;
    const SrcLevel& l0 = ctx->src[0];
    ProfScope ps(ctx, FPM_K_NOT, 2 * (int64_t)ctx->S * l0.w * l0.h);
    if (!launch_bitwise_not(ctx->d_src.as<uint8_t>() + l0.off, l0.w, l0.h, l0.pitch, l0.img_bytes, ctx->S, ctx->stream)) {
        ctx->err = "source slab layout: level-0 rows not 16-byte aligned";
        return FPM_E_INTERNAL;
    }
    HIP_TRY(hipGetLastError());
    ctx->src_inverted = want;
    return FPM_OK;
}

// First half of a staged search: plan, then the whole device pass enqueued on the context's stream (no wait).
int start_staged(fpm_ctx* ctx) {
    ctx->t_call0 = std::chrono::steady_clock::now();
    ctx->cands.clear();
    ctx->stats.clear();
    int rc = build_plan(ctx);
    if (rc != FPM_OK) return rc;
    if (!ctx->t_ev[0]) {
        HIP_TRY(hipEventCreate(&ctx->t_ev[0]));
        HIP_TRY(hipEventCreate(&ctx->t_ev[1]));
    }
    HIP_TRY(hipEventRecord(ctx->t_ev[0], ctx->stream));
    rc = apply_polarity(ctx);   // (inside the timed pass, as the reference inverts inside its timer, :783-791)
    if (rc != FPM_OK) return rc;
    if (ctx->plan.nang > 0) {   // an angle shard with no angles has no device work (and no candidates)
        rc = launch_search(ctx);
        if (rc != FPM_OK) return rc;
    }
    HIP_TRY(hipEventRecord(ctx->t_ev[1], ctx->stream));
    ctx->run_prm = ctx->prm;
    ctx->pending = true;
    return FPM_OK;
}

// Second half: wait for the device pass, then the host's reference-order post-processing per source.
int complete_staged(fpm_ctx* ctx, std::vector<std::vector<fpm_result>>& results, bool merge = true) {
    if (!ctx->pending) { ctx->err = "no search in flight"; return FPM_E_INVALID_ARG; }
    ctx->pending = false;
    const auto c0 = ctx->t_call0;
    {   // a large host tail follows (thousands of top-layer candidates per source): wake the host pool now, so its
        // workers are spinning, not asleep, when the tail's parallel regions start after the device wait
        const Plan& P = ctx->plan;
        if ((size_t)P.nang * P.cap >= 2048)
            host_pool_warm((int)std::min(10000.0, 1000.0 * std::max(1.0, (double)ctx->last_device_ms) + 1000.0));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const auto c1 = std::chrono::steady_clock::now();
    {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ctx->t_ev[0], ctx->t_ev[1]) == hipSuccess) ctx->last_device_ms = ms;
    }
    prof_collect(ctx);
    Plan& P = ctx->plan;
    results.assign(P.S, {});
    std::vector<int> pos;
    if (P.L > P.stop && P.nang > 0) {   // the stop layer's live list
        const char* hb = P.h_out.as<char>();
        const int n0 = ((const int32_t*)(hb + P.h_live))[P.L - 1 - P.stop];
        const int32_t* ids = (const int32_t*)(hb + P.h_live0);
        pos.assign(P.C, -1);
        for (int li = 0; li < n0; ++li) pos[ids[li]] = li;
    }
    ctx->cands.assign(P.S, {});
    ctx->poses.assign(P.S, {});
    ctx->searched = true;
    for (int s = 0; s < P.S; ++s) {
        collect_candidates(ctx, s, pos, ctx->cands[s]);
        if (merge)
            merge_candidates(ctx->run_prm, ctx->tmpl[0].w, ctx->tmpl[0].h, ctx->cands[s].data(), (int)ctx->cands[s].size(),
                             results[s], ctx, P.stop, &ctx->poses[s]);
    }
    // stats: [angles, top candidates, live entering layer L-1 .. stop] (totals over the batch)
    const char* h = P.h_out.as<char>();
    const int32_t* counts = (const int32_t*)(h + P.h_counts);
    int64_t topc = 0;
    for (int k = 0; k < P.S * P.nang; ++k) topc += counts[k];
    ctx->stats.assign({(int64_t)P.nang, topc});
    static const int32_t zeros[64] = {};
    const int32_t* lc = P.nang > 0 ? (const int32_t*)(h + P.h_live) : zeros;
    const int nref = P.L - P.stop;   // refinement layers that ran
    for (int d = 0; d < nref; ++d) ctx->stats.push_back(lc[d]);
    // SURVEY.md §8(d) algorithmic bytes (compulsory input + output of each stage, u8 = 1 B, f32 = 4 B; scratch
    // between the stages of this design is not counted), summed over the batch:
    //   B_pyr = sum_{l<L} (W_l H_l + W_{l+1} H_{l+1});  B_top = sum_angles (W_L H_L + 4 |R_a|);
    //   B_ref = sum_{stop<=l<L} sum_{live ROIs at l} ((w_l + 6)(h_l + 6) + w_l h_l + 49 * 4)
    // (the pyramid is built down from level 0 whatever the stop layer; the layers below it add nothing to B_ref)
    {
        int64_t bp = 0, bt = 0, br = 0;
        for (int l = 0; l < P.L; ++l)
            bp += (int64_t)ctx->src[l].w * ctx->src[l].h + (int64_t)ctx->src[l + 1].w * ctx->src[l + 1].h;
        for (int a = 0; a < P.nang; ++a)
            bt += (int64_t)ctx->src[P.L].w * ctx->src[P.L].h + 4LL * P.map_w[a] * P.map_h[a];
        for (int d = 0; d < nref && P.nang > 0; ++d) {
            const TmplLevel& t = ctx->tmpl[P.L - 1 - d];
            br += (int64_t)lc[d] * P.n3 * ((int64_t)(t.w + 6) * (t.h + 6) + (int64_t)t.w * t.h + 49 * 4);
        }
        ctx->alg_bytes[0] = bp * P.S;
        ctx->alg_bytes[1] = bt * P.S;
        ctx->alg_bytes[2] = br;
    }
    if (ctx->prof && P.nang > 0) {   // per-kernel share of B_ref (the live counts are known only now)
        // the matrix-core top layer never writes its maps: the peak extraction over them (the greedy form on the
        // lists) is charged the map term of B_top, 4 |R_a| per source and angle
        if (P.top_lists)
            for (int a = 0; a < P.nang; ++a) ctx->kp[FPM_K_TOP_NMS].bytes += 4LL * P.map_w[a] * P.map_h[a] * P.S;
        for (int d = 0; d < nref; ++d) {
            const int l = P.L - 1 - d;
            const TmplLevel& t = ctx->tmpl[l];
            const int64_t rois = (int64_t)lc[d] * P.n3;
            const int64_t foot = (int64_t)(t.w + 6) * (t.h + 6), tmpl = (int64_t)t.w * t.h;
            if (P.step_layers & (1u << d))   // the step: its candidates' records and state (design state, not §8(d))
                ctx->kp[FPM_K_CAND_STEP].bytes +=
                    (int64_t)lc[d] * (P.n3 * (int64_t)sizeof(RoiRecord) + 2 * (int64_t)sizeof(CandState) + 4);
            if (roi_small_fits(t.w, t.h)) {   // one kernel: footprint + template in, the 7x7 scores out
                ctx->kp[FPM_K_ROI_SMALL].bytes += rois * (foot + tmpl + 49 * 4);
                continue;
            }
            // the sampled ROI, row sums and window band totals are this design's scratch, not §8(d) traffic: the
            // sampling kernel is charged the footprint read, the correlation the template, the evaluation the scores
            ctx->kp[FPM_K_ROI_WARP].bytes += rois * foot;
            ctx->kp[FPM_K_ROI_CORR].bytes += rois * tmpl;
            ctx->kp[FPM_K_ROI_EVAL].bytes += rois * 49 * 4;
        }
    }
    const auto c2 = std::chrono::steady_clock::now();
    ctx->last_host_ms = std::chrono::duration<double, std::milli>(c2 - c1).count();
    ctx->last_call_ms = std::chrono::duration<double, std::milli>(c2 - c0).count();
    return FPM_OK;
}

int run_staged(fpm_ctx* ctx, std::vector<std::vector<fpm_result>>& results) {
    const int rc = start_staged(ctx);
    if (rc != FPM_OK) return rc;
    return complete_staged(ctx, results);
}

int upload_sources(fpm_ctx* ctx, const uint8_t* const* grays, int count, int w, int h, size_t stride) {
    int rc = layout_sources(ctx, count, w, h);
    if (rc != FPM_OK) return rc;
    ctx->src_inverted = false;   // the slab holds the sources as given
    const SrcLevel& l0 = ctx->src[0];
    for (int s = 0; s < count; ++s)
        HIP_TRY(hipMemcpy2DAsync(ctx->d_src.as<uint8_t>() + l0.off + l0.img_bytes * s, l0.pitch, grays[s], stride, w, h,
                                 hipMemcpyHostToDevice, ctx->stream));
    ctx->src_valid = true;
    return FPM_OK;
}

// ---- sources already in device memory (fpm_stage_sources_device, fpm_match_device, fpm_op_to_gray) ----
inline bool fmt_planar(int format) { return format == FPM_FMT_BGR8_PLANAR || format == FPM_FMT_RGB8_PLANAR; }

// sizes, format and strides of a device-image description; no device call
int check_image_desc(fpm_ctx* ctx, int count, int w, int h, size_t stride, size_t plane_stride, int format) {
    if (count <= 0 || w <= 0 || h <= 0) { ctx->err = "bad sources: count, width and height must be positive"; return FPM_E_INVALID_ARG; }
    const int bpp = stage_gray_bpp(format);
    if (!bpp) { ctx->err = "unknown pixel format " + std::to_string(format); return FPM_E_INVALID_ARG; }
    if (stride < (size_t)w * bpp) { ctx->err = "stride below width x bytes per pixel"; return FPM_E_INVALID_ARG; }
    if (fmt_planar(format) && plane_stride < stride * (size_t)h) {
        ctx->err = "plane stride below stride x height";
        return FPM_E_INVALID_ARG;
    }
    return FPM_OK;
}

// bytes from an image's base to one past its last pixel
size_t image_extent(int w, int h, size_t stride, size_t plane_stride, int format) {
    const size_t plane = (size_t)(h - 1) * stride + (size_t)w * stage_gray_bpp(format);
    return fmt_planar(format) ? 2 * plane_stride + plane : plane;
}

// Every image must be memory the context's device can read: device memory of that device, managed memory or
// registered (pinned) host memory.  An unregistered host pointer makes hipPointerGetAttributes fail or report
// hipMemoryTypeUnregistered, depending on the runtime; either way it is rejected and the sticky error cleared.  The
// extent check against the allocation is best effort (a caching allocator's blocks are larger than its tensors), and
// skipped where the runtime cannot name the allocation.
int check_device_images(fpm_ctx* ctx, const void* const* imgs, int count, size_t extent, const char* what = "source") {
    for (int i = 0; i < count; ++i) {
        const std::string who = std::string(what) + " " + std::to_string(i);
        if (!imgs[i]) { ctx->err = who + ": null pointer"; return FPM_E_INVALID_ARG; }
        hipPointerAttribute_t at{};
        const hipError_t e = hipPointerGetAttributes(&at, imgs[i]);
        (void)hipGetLastError();
        const bool ok = e == hipSuccess && ((at.type == hipMemoryTypeDevice && at.device == ctx->device) ||
                                            at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeHost);
        if (!ok) {
            ctx->err = who + ": not memory the context's device can access (device " + std::to_string(ctx->device) +
                       " memory, managed or registered host memory expected)";
            return FPM_E_INVALID_ARG;
        }
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)imgs[i]) != hipSuccess) {
            (void)hipGetLastError();
            continue;
        }
        const size_t at_off = (size_t)((const char*)imgs[i] - (const char*)base);
        if (at_off > size || extent > size - at_off) {
            ctx->err = who + ": the image's byte extent leaves its allocation";
            return FPM_E_INVALID_ARG;
        }
    }
    return FPM_OK;
}

// upload_sources for images in device memory: checks, slab layout, ordering after the producer, pointer table, one
// k_stage_gray launch on the context's stream (no wait).  Everything is checked before anything is enqueued or the
// slab is re-laid out.  With fpm_params.bitwise_not set the kernel writes 255 - gray and the slab counts as inverted,
// so apply_polarity has nothing to do for a search under the same setting.
int stage_device_sources(fpm_ctx* ctx, const void* const* imgs, int count, int w, int h, size_t stride,
                         size_t plane_stride, int format, hipStream_t producer) {
    int rc = check_image_desc(ctx, count, w, h, stride, plane_stride, format);
    if (rc != FPM_OK) return rc;
    rc = check_device_images(ctx, imgs, count, image_extent(w, h, stride, plane_stride, format));
    if (rc != FPM_OK) return rc;
    rc = layout_sources(ctx, count, w, h);
    if (rc != FPM_OK) return rc;
    const bool invert = ctx->prm.bitwise_not != 0;
    ctx->src_inverted = invert;
    if (!ctx->in_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->in_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ctx->in_ev, producer));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->in_ev, 0));
    const size_t tab = sizeof(void*) * (size_t)count;
    HIP_TRY(ctx->h_imgtab.ensure(tab));
    HIP_TRY(ctx->d_imgtab.ensure(tab));
    bool aligned = (stride & 15) == 0 && (!fmt_planar(format) || (plane_stride & 15) == 0);
    for (int i = 0; i < count; ++i) {
        ctx->h_imgtab.as<const void*>()[i] = imgs[i];
        aligned = aligned && ((uintptr_t)imgs[i] & 15) == 0;
    }
    HIP_TRY(hipMemcpyAsync(ctx->d_imgtab.p, ctx->h_imgtab.p, tab, hipMemcpyHostToDevice, ctx->stream));
    const SrcLevel& l0 = ctx->src[0];
    if (!launch_stage_gray(ctx->d_imgtab.as<const uint8_t*>(), count, w, h, stride, plane_stride, format, aligned,
                           ctx->d_src.as<uint8_t>() + l0.off, l0.pitch, l0.img_bytes, invert, ctx->stream)) {
        ctx->err = "source slab layout: level-0 rows not 16-byte aligned";
        return FPM_E_INTERNAL;
    }
    HIP_TRY(hipGetLastError());
    ctx->src_valid = true;
    return FPM_OK;
}

// ---- match patches (fpm_last_patches*, fpm_patches_at) ----
struct PatchPose {
    int32_t src;
    RawPose pose;
};

// the forward matrix of one patch: glibc trig of angle * D2R on the host, as for every other matrix of the search
void patch_forward(int sw, int sh, const RawPose& p, int rx, int ry, double M[6]) {
    const double rad = p.angle * kD2R;
    patch_matrix(sw, sh, f2(p.x, p.y), std::cos(rad), std::sin(rad), rx, ry, M);
}

int patch_state(fpm_ctx* ctx, bool need_search) {
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    if (!ctx->learned) { ctx->err = "template not learned"; return FPM_E_NOT_LEARNED; }
    if (!ctx->src_valid || ctx->S <= 0 || ctx->src.empty() || !ctx->d_src.p) {
        ctx->err = "no staged sources to take patches from";
        return FPM_E_INVALID_ARG;
    }
    if (need_search && !ctx->searched) {
        ctx->err = "no search has run since the sources were staged";
        return FPM_E_INVALID_ARG;
    }
    return FPM_OK;
}

int patch_rect(fpm_ctx* ctx, const fpm_patch_rect* rect, fpm_patch_rect* r) {
    *r = rect ? *rect : fpm_patch_rect{0, 0, ctx->tmpl[0].w, ctx->tmpl[0].h};
    constexpr int kMaxOrigin = 1 << 20;
    if (r->w < 1 || r->h < 1 || r->w > 8192 || r->h > 8192 || r->x < -kMaxOrigin || r->x > kMaxOrigin ||
        r->y < -kMaxOrigin || r->y > kMaxOrigin) {
        ctx->err = "bad patch rectangle: width and height must be 1 .. 8192, |x| and |y| at most 2^20";
        return FPM_E_INVALID_ARG;
    }
    return FPM_OK;
}

// the poses of the last search's results: of one source, or of all in source order
int last_poses(fpm_ctx* ctx, int source, std::vector<PatchPose>& poses) {
    if (source < -1 || source >= ctx->S) { ctx->err = "bad source index"; return FPM_E_INVALID_ARG; }
    for (int s = 0; s < (int)ctx->poses.size() && s < ctx->S; ++s)
        if (source < 0 || s == source)
            for (const RawPose& p : ctx->poses[s]) poses.push_back({s, p});
    return FPM_OK;
}

// Where the poses of a per-hit call come from: the last search's results of `source`, with the
// caller's capacity `cap` and count `*n` (fpm_last_X), or the caller's own poses (fpm_X_at).
struct HitQuery {
    bool from_last = false;
    int32_t source = 0, cap = 0;
    int32_t* n = nullptr;
    const int32_t* src_index = nullptr;
    const float* lt = nullptr;
    const double* angles = nullptr;
    int32_t n_poses = 0;

    static HitQuery last(int32_t source, int32_t cap, int32_t* n) {
        HitQuery q;
        q.from_last = true; q.source = source; q.cap = cap; q.n = n;
        return q;
    }
    static HitQuery at(const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses) {
        HitQuery q;
        q.src_index = src_index; q.lt = lt; q.angles = angles; q.n_poses = n_poses;
        return q;
    }
    bool need_search() const { return from_last; }   // for patch_state

    // The call's own pointers, before anything else is looked at; a last call's count starts at 0.
    int check(fpm_ctx* ctx) const {
        if (!ctx || (from_last && !n)) return FPM_E_INVALID_ARG;
        if (from_last) { *n = 0; return FPM_OK; }
        if (n_poses < 0 || (n_poses > 0 && (!src_index || !lt || !angles))) { ctx->err = "bad poses"; return FPM_E_INVALID_ARG; }
        return FPM_OK;
    }

    // The poses.  A last call also gets its count and the capacity check, under the tool's own text.  FPM_OK with
    // `poses` empty: the caller has nothing to do and returns FPM_OK.
    int resolve(fpm_ctx* ctx, const char* too_small, std::vector<PatchPose>& poses) const {
        if (!from_last) {
            poses.resize((size_t)n_poses);
            for (int i = 0; i < n_poses; ++i) poses[i] = {src_index[i], {lt[2 * i], lt[2 * i + 1], angles[i]}};
            return FPM_OK;
        }
        const int rc = last_poses(ctx, source, poses);
        if (rc != FPM_OK) return rc;
        *n = (int32_t)poses.size();
        if ((int)poses.size() > cap) { ctx->err = too_small; return FPM_E_CAPACITY; }
        return FPM_OK;
    }
};

const char* kPatchCap = "patch buffer too small";
using RectRule = int (*)(fpm_ctx*, const fpm_patch_rect*, fpm_patch_rect*);   // patch_rect, compare_rect, align_rect, model_rect

// State, rectangle and poses of a call with one rectangle, in this order; FPM_OK with poses empty = nothing to do.
int hits_begin(fpm_ctx* ctx, const HitQuery& q, RectRule rule, const fpm_patch_rect* rect, fpm_patch_rect* r,
               std::vector<PatchPose>& poses) {
    int rc = patch_state(ctx, q.need_search());
    if (rc == FPM_OK) rc = rule(ctx, rect, r);
    if (rc == FPM_OK) rc = q.resolve(ctx, kPatchCap, poses);
    return rc;
}

int check_patch_out(fpm_ctx* ctx, const void* out, const fpm_patch_rect& r, size_t row_stride, size_t patch_stride) {
    if (!out) { ctx->err = "null patch buffer"; return FPM_E_INVALID_ARG; }
    if (row_stride < (size_t)r.w || row_stride > (size_t)INT32_MAX || patch_stride / (size_t)r.h < row_stride) {
        ctx->err = "bad patch strides: row_stride >= width and patch_stride >= row_stride x height expected";
        return FPM_E_INVALID_ARG;
    }
    return FPM_OK;
}

// The checks of pose i of a job list and its matrices: fwd (optional) the forward one, M the inverted one the samplers take.
int patch_pose_matrix(fpm_ctx* ctx, const fpm_patch_rect& r, const PatchPose& p, int i, double* fwd, double M[6]) {
    if (p.src < 0 || p.src >= ctx->S) { ctx->err = "pose " + std::to_string(i) + ": bad source index"; return FPM_E_INVALID_ARG; }
    if (!std::isfinite(p.pose.x) || !std::isfinite(p.pose.y) || !std::isfinite(p.pose.angle)) {
        ctx->err = "pose " + std::to_string(i) + ": not finite";
        return FPM_E_INVALID_ARG;
    }
    patch_forward(ctx->sw, ctx->sh, p.pose, r.x, r.y, M);
    if (fwd) std::copy(M, M + 6, fwd);
    invert_affine(M);
    // the samplers' coordinates are AB_BITS fixed point in 32 bits: the patch's corners bound every pixel's
    for (int k = 0; k < 4; ++k) {
        const double x = (k & 1) ? r.w - 1 : 0, y = (k & 2) ? r.h - 1 : 0;
        const double sx = M[0] * x + M[1] * y + M[2], sy = M[3] * x + M[4] * y + M[5];
        if (!(std::fabs(sx) < 1048576.0 && std::fabs(sy) < 1048576.0)) {
            ctx->err = "pose " + std::to_string(i) + ": farther than 2^20 pixels from the source";
            return FPM_E_INVALID_ARG;
        }
    }
    return FPM_OK;
}

size_t patch_tab_bytes(int n) { return round_up(std::max(sizeof(PatchJob), sizeof(WarpJob)) * (size_t)n, (size_t)256); }

// ---- the job table of a per-hit tool: h_patchtab filled on the host, sent to d_patchtab ----
// begin: the pinned table is free again (an earlier call's copy out of it is long done as a rule), both buffers hold
// `bytes`; *jobs = the pinned table.
template <class Job>
int tab_begin(fpm_ctx* ctx, size_t bytes, Job** jobs) {
    if (!ctx->tab_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->tab_ev, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(ctx->tab_ev));
    HIP_TRY(ctx->h_patchtab.ensure(bytes));
    HIP_TRY(ctx->d_patchtab.ensure(bytes));
    *jobs = ctx->h_patchtab.as<Job>();
    return FPM_OK;
}

// head: pose i of the call checked (patch_pose_matrix), its sampler matrix, output offset and source into a job's head
int tab_head(fpm_ctx* ctx, PatchJob& j, const fpm_patch_rect& r, const PatchPose& p, int i, int64_t out_off, double* fwd = nullptr) {
    const int rc = patch_pose_matrix(ctx, r, p, i, fwd, j.M);
    if (rc != FPM_OK) return rc;
    j.out_off = out_off;
    j.src = p.src;
    j.pad = 0;
    return FPM_OK;
}

// send: the first `bytes` of the pinned table to the device, on the context's stream (no wait)
int tab_send(fpm_ctx* ctx, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(ctx->d_patchtab.p, ctx->h_patchtab.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->tab_ev, ctx->stream));
    return FPM_OK;
}

// outside: border zeros in a w x h region -- a corner sample outside the source, through the matrix the sampler takes
bool corners_outside(const fpm_ctx* ctx, const double M[6], int w, int h) {
    bool o = false;
    for (int e = 0; e < 4; ++e) {
        const double x = (e & 1) ? w - 1 : 0, y = (e & 2) ? h - 1 : 0;
        const double sx = M[0] * x + M[1] * y + M[2], sy = M[3] * x + M[4] * y + M[5];
        o = o || !(sx >= 0.0 && sx <= (double)(ctx->sw - 1) && sy >= 0.0 && sy <= (double)(ctx->sh - 1));
    }
    return o;
}

// source fields: the sent table and level 0 of the staged sources, as PatchArgs, CaliperArgs, GrayArgs and LocateArgs
// name them; every other field zero
template <class Args>
Args source_args(fpm_ctx* ctx, int njobs) {
    const SrcLevel& l0 = ctx->src[0];
    Args a{};
    a.jobs = ctx->d_patchtab.as<std::remove_pointer_t<decltype(a.jobs)>>();
    a.njobs = njobs;
    a.level0 = ctx->d_src.as<uint8_t>() + l0.off;
    a.img_stride = l0.img_bytes;
    a.sw = l0.w; a.sh = l0.h; a.sp = l0.pitch;
    return a;
}

// The job table of `poses` (PatchJob when tiled, else WarpJob), built in h_patchtab and sent to d_patchtab on the
// context's stream (no wait): patch i goes to d_out + i * patch_stride.  matrices (optional): the forward matrices,
// [n][6].  extra: bytes kept free in both buffers behind the table, from patch_tab_bytes(n) on (the comparison's tables).
int stage_patch_jobs(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, uint8_t* d_out,
                     size_t row_stride, size_t patch_stride, double* matrices, bool tiled, size_t extra = 0) {
    const int n = (int)poses.size();
    const SrcLevel& l0 = ctx->src[0];
    uint8_t* tab = nullptr;
    int rc = tab_begin(ctx, patch_tab_bytes(n) + extra, &tab);
    if (rc != FPM_OK) return rc;
    const uint8_t* level0 = ctx->d_src.as<uint8_t>() + l0.off;
    for (int i = 0; i < n; ++i) {
        const PatchPose& p = poses[i];
        double* fwd = matrices ? matrices + 6 * (size_t)i : nullptr;
        const size_t off = (size_t)i * patch_stride;
        if (tiled) {
            rc = tab_head(ctx, ((PatchJob*)tab)[i], r, p, i, (int64_t)off, fwd);
            if (rc != FPM_OK) return rc;
        } else {
            WarpJob& j = ((WarpJob*)tab)[i];
            rc = patch_pose_matrix(ctx, r, p, i, fwd, j.M);
            if (rc != FPM_OK) return rc;
            j.src = level0 + l0.img_bytes * (size_t)p.src;
            j.dst = d_out + off;
            j.sw = l0.w; j.sh = l0.h; j.sp = l0.pitch;
            j.dw = r.w; j.dh = r.h; j.dp = (int32_t)row_stride;
            j.border = 0;
            j.pad = 0;
        }
    }
    return tab_send(ctx, patch_tab_bytes(n));
}

// the arguments of the tiled kernels (k_patch_warp, k_patch_compare) for a staged PatchJob table
PatchArgs patch_args(fpm_ctx* ctx, const fpm_patch_rect& r, int n, uint8_t* d_out, size_t row_stride, size_t patch_stride) {
    PatchArgs a = source_args<PatchArgs>(ctx, n);
    a.out = d_out;
    a.row_stride = row_stride;
    a.pw = r.w; a.ph = r.h;
    a.dword = (((uintptr_t)d_out | row_stride | patch_stride) & 3) == 0;
    return a;
}

// Job table and the one launch for `poses` on the context's stream (no wait).
int enqueue_patches(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, uint8_t* d_out,
                    size_t row_stride, size_t patch_stride, double* matrices) {
    const int n = (int)poses.size();
    const bool tiled = ctx->patch_form == FPM_PATCH_FORM_TILED;
    const int rc = stage_patch_jobs(ctx, r, poses, d_out, row_stride, patch_stride, matrices, tiled);
    if (rc != FPM_OK) return rc;
    // bytes: the patch pixels written + as many source pixels read (the footprint of a scale-1 warp)
    ProfScope ps(ctx, FPM_K_PATCH, 2 * (int64_t)n * r.w * r.h);
    if (tiled) {
        const PatchArgs a = patch_args(ctx, r, n, d_out, row_stride, patch_stride);
        if (!launch_patch_warp(a, ctx->stream)) { ctx->err = "too many patch tiles for one launch"; return FPM_E_INVALID_ARG; }
    } else {
        constexpr int kMaxJobs = 65535;   // k_warp takes its job from blockIdx.y
        for (int i0 = 0; i0 < n; i0 += kMaxJobs)
            launch_warp(ctx->d_patchtab.as<WarpJob>() + i0, std::min(kMaxJobs, n - i0), r.w * r.h, ctx->stream);
    }
    HIP_TRY(hipGetLastError());
    return FPM_OK;
}

// n images of r.w x r.h from the context's pitched buffer d to the caller's host buffer, on the context's stream (no wait)
int copy_patches_out(fpm_ctx* ctx, const fpm_patch_rect& r, size_t n, const uint8_t* d, size_t pitch, size_t pbytes,
                     uint8_t* out, size_t row_stride, size_t patch_stride) {
    if (patch_stride == row_stride * (size_t)r.h) {   // the caller's patches are one run of rows
        HIP_TRY(hipMemcpy2DAsync(out, row_stride, d, pitch, r.w, (size_t)r.h * n, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        for (size_t i = 0; i < n; ++i)
            HIP_TRY(hipMemcpy2DAsync(out + i * patch_stride, row_stride, d + i * pbytes, pitch, r.w, r.h,
                                     hipMemcpyDeviceToHost, ctx->stream));
    }
    return FPM_OK;
}

// The host variants: the patches into the context's own buffer (row pitch a multiple of 64), then out to the caller's.
int patches_to_host(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, uint8_t* out,
                    size_t row_stride, size_t patch_stride, double* matrices) {
    const size_t n = poses.size();
    const size_t pitch = round_up((size_t)r.w, (size_t)64), pbytes = pitch * (size_t)r.h;
    HIP_TRY(ctx->d_patch.ensure(pbytes * n));
    uint8_t* d = ctx->d_patch.as<uint8_t>();
    int rc = enqueue_patches(ctx, r, poses, d, pitch, pbytes, matrices);
    if (rc == FPM_OK) rc = copy_patches_out(ctx, r, n, d, pitch, pbytes, out, row_stride, patch_stride);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return FPM_OK;
}

// ---- patch comparison (fpm_last_compare, fpm_compare_at, fpm_compare_derive) ----
constexpr int64_t kCompareMaxArea = (int64_t)1 << 22;   // n * sum_ii, sum_i^2 and n * sum_it stay below 2^62

// Unlike a patch rectangle, a comparison rectangle lies inside the template: every patch pixel has one beneath it.
int compare_rect(fpm_ctx* ctx, const fpm_patch_rect* rect, fpm_patch_rect* r) {
    const int tw = ctx->tmpl[0].w, th = ctx->tmpl[0].h;
    *r = rect ? *rect : fpm_patch_rect{0, 0, tw, th};
    if (r->x < 0 || r->y < 0 || r->w < 1 || r->h < 1 || r->w > tw - r->x || r->h > th - r->y ||
        (int64_t)r->w * r->h > kCompareMaxArea) {
        ctx->err = "bad comparison rectangle: it must lie inside the template and hold 1 .. 2^22 pixels";
        return FPM_E_INVALID_ARG;
    }
    return FPM_OK;
}

// ---- template masks (fpm_mask_*) ----
void mask_drop(fpm_ctx* ctx) {
    ctx->mask_set = ctx->mask_on = false;
    ctx->mask_count = 0;
    ctx->mask_host.clear();
    ctx->mask_rect_known = false;
}

// the plane the masked kernel forms read, or null: no mask, or a disabled one
const uint8_t* mask_plane(const fpm_ctx* ctx) { return ctx->mask_set && ctx->mask_on ? ctx->d_mask.as<uint8_t>() : nullptr; }

// pixels of rectangle r (inside the template) the stored mask keeps, from the host copy; counted once per rectangle
// and mask, then remembered
int64_t mask_count_rect(const fpm_ctx* ctx, const fpm_patch_rect& r) {
    if (ctx->mask_rect_known && ctx->mask_rect.x == r.x && ctx->mask_rect.y == r.y && ctx->mask_rect.w == r.w &&
        ctx->mask_rect.h == r.h)
        return ctx->mask_rect_count;
    const int tw = ctx->tmpl[0].w;
    int64_t n = 0;
    for (int y = r.y; y < r.y + r.h; ++y) {
        const uint8_t* row = ctx->mask_host.data() + (size_t)y * tw + r.x;
        for (int x = 0; x < r.w; ++x) n += row[x] != 0;
    }
    ctx->mask_rect = r;
    ctx->mask_rect_count = n;
    ctx->mask_rect_known = true;
    return n;
}

// the pixels of r a masked tool uses: all of them without an active mask
int64_t mask_used(const fpm_ctx* ctx, const fpm_patch_rect& r) {
    return mask_plane(ctx) ? mask_count_rect(ctx, r) : (int64_t)r.w * r.h;
}

// A mask of the template's size staged into a fresh plane by k_mask_stage, which then replaces the context's: from
// `host` (uploaded beside the plane first) or from device-readable memory at `dev`.  The context's mask is untouched
// until everything has succeeded.  The new mask starts enabled.  Synchronises the stream.
int mask_install(fpm_ctx* ctx, const uint8_t* host, const uint8_t* dev, size_t stride) {
    const TmplLevel& t0 = ctx->tmpl[0];
    const int w = t0.w, h = t0.h;
    const size_t plane = round_up((size_t)t0.pitch * (h + 1), (size_t)256), px = (size_t)w * h;
    HIP_TRY(ctx->d_mask_in.ensure(plane + 256 + (host ? px : 0)));
    uint8_t* base = ctx->d_mask_in.as<uint8_t>();
    HIP_TRY(hipMemsetAsync(base, 0, plane + 256, ctx->stream));   // the rows' padding, which the kernels read, and the count
    if (host) {
        HIP_TRY(hipMemcpy2DAsync(base + plane + 256, w, host, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
        dev = base + plane + 256;
        stride = (size_t)w;
    }
    if (!launch_mask_stage(dev, w, h, stride, base, t0.pitch, (unsigned long long*)(base + plane), ctx->stream)) {
        ctx->err = "mask plane layout: rows not 64-byte aligned";
        return FPM_E_INTERNAL;
    }
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> hm(px);
    unsigned long long count = 0;
    HIP_TRY(hipMemcpy2DAsync(hm.data(), w, base, t0.pitch, w, h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&count, base + plane, sizeof(count), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::swap(ctx->d_mask, ctx->d_mask_in);
    ctx->mask_host = std::move(hm);
    ctx->mask_rect_known = false;
    ctx->mask_count = (int64_t)count;
    ctx->mask_set = ctx->mask_on = true;
    return FPM_OK;
}

// state shared by the mask entries: no search in flight, a template
int mask_state(fpm_ctx* ctx, bool need_mask) {
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    if (!ctx->learned) { ctx->err = "template not learned"; return FPM_E_NOT_LEARNED; }
    if (need_mask && !ctx->mask_set) { ctx->err = "no template mask (fpm_mask_set / fpm_mask_set_device first)"; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

int mask_dims(fpm_ctx* ctx, const void* mask, int w, int h, size_t stride) {
    if (!mask) { ctx->err = "null mask"; return FPM_E_INVALID_ARG; }
    if (w != ctx->tmpl[0].w || h != ctx->tmpl[0].h) {
        ctx->err = "the mask must have the learned template's size, " + std::to_string(ctx->tmpl[0].w) + " x " +
                   std::to_string(ctx->tmpl[0].h);
        return FPM_E_INVALID_ARG;
    }
    if (stride < (size_t)w) { ctx->err = "stride below the mask's width"; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

// What the sums give (include/fpm.h states the operation order; the file is built with -ffp-contract=off, so the
// product and the sum of a table entry are two roundings).  lut may be null.
void compare_derive(int64_t n, int64_t si, int64_t sii, int64_t st, int64_t stt, int64_t sit, bool normalize,
                    double* zncc, double* gain, double* offset, uint8_t* lut) {
    const int64_t Di = n * sii - si * si, Dt = n * stt - st * st, N = n * sit - si * st;
    const double sdi = std::sqrt((double)Di), sdt = std::sqrt((double)Dt);
    *zncc = Di == 0 || Dt == 0 ? 0.0 : (double)N / (sdi * sdt);
    double g = 1.0, o = 0.0;
    if (normalize) {
        g = Di == 0 ? 1.0 : sdt / sdi;
        const double gi = g * (double)si;
        o = ((double)st - gi) / (double)n;
    }
    *gain = g;
    *offset = o;
    if (!lut) return;
    for (int v = 0; v < 256; ++v) {
        const double gv = g * (double)v;
        const double q = std::nearbyint(gv + o);   // the default rounding mode: ties to even
        lut[v] = (uint8_t)std::min(255.0, std::max(0.0, q));
    }
}

// compare_derive over the n used pixels of a masked rectangle; with none (the mask misses the rectangle) the neutral
// values: zncc 0, gain 1, offset 0, the identity table.
void compare_derive_used(int64_t n, const CompareAcc& a, bool normalize, double* zncc, double* gain, double* offset,
                         uint8_t* lut) {
    if (n == 0) {
        *zncc = 0.0; *gain = 1.0; *offset = 0.0;
        if (lut) for (int v = 0; v < 256; ++v) lut[v] = (uint8_t)v;
        return;
    }
    compare_derive(n, (int64_t)a.s[kCmpSumI], (int64_t)a.s[kCmpSumII], (int64_t)a.s[kCmpSumT], (int64_t)a.s[kCmpSumTT],
                   (int64_t)a.s[kCmpSumIT], normalize, zncc, gain, offset, lut);
}

// The first half of a normalised comparison (and of normalised training and inspection of the variation model): the
// sums launch into c.acc = d_cmpacc (zero-filled by the caller), the sums to h_cmpacc, a table per hit from them, the
// tables to the device beside the job table (stage_patch_jobs' `extra` bytes: 256 n), their address in *d_luts.
// Synchronises the stream once, between the sums and the tables.
int compare_norm_tables(fpm_ctx* ctx, CompareArgs c, const fpm_patch_rect& r, int n, const uint8_t** d_luts) {
    const size_t accb = sizeof(CompareAcc) * (size_t)n, lut_off = patch_tab_bytes(n);
    c.p.out = nullptr;
    {
        // source pixels read + template pixels read (+ mask bytes read)
        ProfScope ps(ctx, FPM_K_COMPARE, (2 + (c.mask ? 1 : 0)) * (int64_t)n * r.w * r.h);
        if (!launch_patch_compare(c, kCompareSums, ctx->stream)) {
            ctx->err = "too many patch tiles for one launch";
            return FPM_E_INVALID_ARG;
        }
    }
    HIP_TRY(hipGetLastError());
    CompareAcc* h = ctx->h_cmpacc.as<CompareAcc>();
    HIP_TRY(hipMemcpyAsync(h, ctx->d_cmpacc.p, accb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // also: the job table has left h_patchtab
    const int64_t used = c.mask ? mask_count_rect(ctx, r) : (int64_t)r.w * r.h;
    uint8_t* luts = ctx->h_patchtab.as<uint8_t>(lut_off);
    for (int i = 0; i < n; ++i) {
        double z, g, o;
        compare_derive_used(used, h[i], true, &z, &g, &o, luts + (size_t)256 * i);
    }
    HIP_TRY(hipMemcpyAsync(ctx->d_patchtab.as<uint8_t>(lut_off), luts, (size_t)256 * n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->tab_ev, ctx->stream));
    *d_luts = ctx->d_patchtab.as<uint8_t>(lut_off);
    return FPM_OK;
}

// The comparison of `poses` (n >= 1): one launch, or with FPM_COMPARE_NORMALIZE the sums, the tables built here from
// them, and the deviations through the tables.  Returns when out (and diff) are filled.
int compare_to_host(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, int threshold, int flags,
                    fpm_compare_stats* out, uint8_t* diff, size_t row_stride, size_t patch_stride) {
    const int n = (int)poses.size();
    const bool norm = (flags & FPM_COMPARE_NORMALIZE) != 0;
    const size_t pitch = round_up((size_t)r.w, (size_t)64), pbytes = pitch * (size_t)r.h;
    uint8_t* d = nullptr;   // the difference images: the context's pitched buffer, as for the host patches
    if (diff) {
        HIP_TRY(ctx->d_patch.ensure(pbytes * (size_t)n));
        d = ctx->d_patch.as<uint8_t>();
    }
    const size_t accb = sizeof(CompareAcc) * (size_t)n;
    int rc = stage_patch_jobs(ctx, r, poses, d, pitch, pbytes, nullptr, true, norm ? (size_t)256 * n : 0);
    if (rc != FPM_OK) return rc;
    HIP_TRY(ctx->d_cmpacc.ensure(accb));
    HIP_TRY(ctx->h_cmpacc.ensure(accb));
    HIP_TRY(hipMemsetAsync(ctx->d_cmpacc.p, 0, accb, ctx->stream));   // also "no pixel over the threshold" (CompareAcc)
    const TmplLevel& t0 = ctx->tmpl[0];
    CompareArgs c{};
    c.p = patch_args(ctx, r, n, norm ? nullptr : d, pitch, pbytes);
    c.tmpl = ctx->d_tmpl.as<uint8_t>() + t0.off;
    c.tp = t0.pitch;
    c.rx = r.x; c.ry = r.y;
    c.threshold = threshold;
    c.acc = ctx->d_cmpacc.as<CompareAcc>();
    c.mask = mask_plane(ctx);
    const int64_t used = mask_used(ctx, r);
    // bytes: source pixels read + template pixels read (+ mask bytes read) (+ difference pixels written), per launch
    const int64_t px = (int64_t)n * r.w * r.h;
    const int rd = 2 + (c.mask ? 1 : 0);
    const char* too_many = "too many patch tiles for one launch";
    CompareAcc* h = ctx->h_cmpacc.as<CompareAcc>();
    if (!norm) {
        ProfScope ps(ctx, FPM_K_COMPARE, (rd + (c.p.out ? 1 : 0)) * px);
        if (!launch_patch_compare(c, kCompareRaw, ctx->stream)) { ctx->err = too_many; return FPM_E_INVALID_ARG; }
    }
    HIP_TRY(hipGetLastError());
    if (norm) {
        // the sums and the tables, then the second launch, which samples the footprints again
        rc = compare_norm_tables(ctx, c, r, n, &c.luts);
        if (rc != FPM_OK) return rc;
        c.p = patch_args(ctx, r, n, d, pitch, pbytes);
        {
            ProfScope ps(ctx, FPM_K_COMPARE, (rd + (d ? 1 : 0)) * px);
            if (!launch_patch_compare(c, kCompareDevLut, ctx->stream)) { ctx->err = too_many; return FPM_E_INVALID_ARG; }
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(h, ctx->d_cmpacc.p, accb, hipMemcpyDeviceToHost, ctx->stream));
    if (d) {
        rc = copy_patches_out(ctx, r, (size_t)n, d, pitch, pbytes, diff, row_stride, patch_stride);
        if (rc != FPM_OK) return rc;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    for (int i = 0; i < n; ++i) {
        fpm_compare_stats& s = out[i];
        s.n = used;
        s.sum_i = (int64_t)h[i].s[kCmpSumI]; s.sum_ii = (int64_t)h[i].s[kCmpSumII];
        s.sum_t = (int64_t)h[i].s[kCmpSumT]; s.sum_tt = (int64_t)h[i].s[kCmpSumTT];
        s.sum_it = (int64_t)h[i].s[kCmpSumIT]; s.sum_abs = (int64_t)h[i].s[kCmpSumAbs];
        const uint32_t* m = h[i].m;
        s.n_over = (int32_t)m[kCmpNOver - kCmpNOver]; s.max_abs = (int32_t)m[kCmpMaxAbs - kCmpNOver];
        s.x0 = r.w - (int32_t)m[kCmpX0 - kCmpNOver]; s.y0 = r.h - (int32_t)m[kCmpY0 - kCmpNOver];
        s.x1 = (int32_t)m[kCmpX1 - kCmpNOver] - 1; s.y1 = (int32_t)m[kCmpY1 - kCmpNOver] - 1;
        compare_derive_used(used, h[i], norm, &s.zncc, &s.gain, &s.offset, nullptr);
    }
    return FPM_OK;
}

// ---- learning on the device (fpm_learn_device, fpm_learn_at, fpm_learn_hit, fpm_learn_derive) ----
constexpr int kLearnMaxSide = 65536;   // k_tmpl_prep keeps a row's sum of squares in 32 bits: 65025 * 65536 < 2^32

// What fpm_learn derives per level, from the level's pixel count and exact sums: mean_stddev's expressions, then those
// of fpm_learn's statistics block, in their order (the file is built with -ffp-contract=off), so the doubles are the
// ones fpm_learn gives for the same pixels.  1 / ((double)h * w) there is 1 / (double)n here: the product is exact.
void learn_derive(int64_t n, int64_t s, int64_t q, double* mean_out, double* norm_out, double* inv_area_out, bool* equal1) {
    const double scale = 1. / (double)n;
    const double m = (double)s * scale;
    const double sdv = std::sqrt(std::max((double)q * scale - m * m, 0.));
    const double inv_area = 1.0 / (double)n;
    double norm = sdv * sdv;
    *equal1 = norm < DBL_EPSILON;
    norm = std::sqrt(norm);
    norm /= std::sqrt(inv_area);
    *mean_out = m; *norm_out = norm; *inv_area_out = inv_area;
}

// bytes of the i8 operand slab and entries of the row-sum array of a learned template (fpm_learn's o8 and os)
void operand_sizes(const std::vector<TmplLevel>& lv, size_t* o8, size_t* os) {
    const TmplLevel& t = lv.back();
    *o8 = t.off8 + (size_t)t.p8 * round_up(t.h, kMmaRows) + 256;
    *os = t.tsum_off + round_up(t.h, kMmaRows);
}

// size limits of a template learned on the device; nothing is touched
int learn_size(fpm_ctx* ctx, int w, int h) {
    if (w <= 0 || h <= 0) { ctx->err = "empty template"; return FPM_E_INVALID_ARG; }
    const int L = top_layer(w, h, (int)std::sqrt((double)ctx->prm.min_reduce_area));
    if (w > kLearnMaxSide || h > kLearnMaxSide || L + 1 > kTmplPrepMaxLevels) {
        ctx->err = "template too large to learn on the device: sides up to 65536, at most 16 pyramid levels";
        return FPM_E_INVALID_ARG;
    }
    return FPM_OK;
}

// A failed device learn leaves the context as after fpm_clear_pattern, not half-learned.
int learn_fail(fpm_ctx* ctx, int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->learned = false;
    ctx->staged = false;
    ctx->src_valid = false;
    ctx->tmpl.clear();
    ctx->tmpl_gen++;
    ctx->model_n = 0;
    mask_drop(ctx);
    return rc;
}

// First half of a device learn: fpm_learn's layouts for a w x h template in lv, the buffers, and the slab cleared on
// the context's stream (its padding stays 0, as after fpm_learn; level 0 is written next, by the caller).  The context
// holds no template from here until learn_finish.
int learn_begin(fpm_ctx* ctx, int w, int h, std::vector<TmplLevel>& lv) {
    ctx->learned = false;
    ctx->tmpl.clear();
    ctx->tmpl_gen++;
    const int L = top_layer(w, h, (int)std::sqrt((double)ctx->prm.min_reduce_area));
    lv.assign(L + 1, {});
    size_t off = 0, o8 = 0, os = 0;
    int lw = w, lh = h;
    for (int l = 0; l <= L; ++l) {
        lv[l].w = lw; lv[l].h = lh;
        lv[l].pitch = round_up(lw + 4, 64);
        lv[l].off = off;
        off += round_up((size_t)lv[l].pitch * (lh + 1), (size_t)256);
        lv[l].p8 = 64 * ((lw + 63) / 64);
        lv[l].off8 = o8;
        o8 += (size_t)lv[l].p8 * round_up(lh, kMmaRows);
        lv[l].tsum_off = os;
        os += round_up(lh, kMmaRows);
        lw = (lw + 1) / 2;
        lh = (lh + 1) / 2;
    }
    o8 += 256;   // slack: k_roi_corr prefetches up to 2 64-byte blocks past a row's last
    if (off > UINT32_MAX || o8 > UINT32_MAX) { ctx->err = "template too large to learn on the device"; return FPM_E_INVALID_ARG; }
    HIP_TRY(ctx->d_tmpl.ensure(off));
    HIP_TRY(ctx->d_tmpl8.ensure(o8));
    HIP_TRY(ctx->d_tsum.ensure(os * sizeof(int32_t)));
    HIP_TRY(ctx->d_tacc.ensure(2 * sizeof(uint64_t) * kTmplPrepMaxLevels));
    HIP_TRY(ctx->h_tacc.ensure(2 * sizeof(uint64_t) * kTmplPrepMaxLevels + (size_t)lv[L].w * lv[L].h));
    HIP_TRY(hipMemsetAsync(ctx->d_tmpl.p, 0, off, ctx->stream));
    return FPM_OK;
}

// Second half, level 0 of the slab holding the pixels (written on the context's stream): the pyramid, k_tmpl_prep, the
// sums and the top level to pinned memory, one synchronisation, the statistics on the host.  The staged sources
// survive when the slab's layout still fits the new template (same top layer, sizes still allowed): a search, a patch
// or a comparison then needs no restaging; otherwise they are invalidated as fpm_learn invalidates them.
int learn_finish(fpm_ctx* ctx, std::vector<TmplLevel>& lv) {
    const int L = (int)lv.size() - 1;
    uint8_t* base = ctx->d_tmpl.as<uint8_t>();
    for (int l = 1; l <= L; ++l)   // cv::buildPyramid (:55) on the device
        launch_pyr_down(base + lv[l - 1].off, lv[l - 1].w, lv[l - 1].h, lv[l - 1].pitch, 0, base + lv[l].off, lv[l].w,
                        lv[l].h, lv[l].pitch, 0, 1, ctx->stream);
    HIP_TRY(hipGetLastError());
    constexpr size_t kAccBytes = 2 * sizeof(uint64_t) * kTmplPrepMaxLevels;
    HIP_TRY(hipMemsetAsync(ctx->d_tacc.p, 0, kAccBytes, ctx->stream));
    TmplPrepArgs a{};
    a.tmpl = base;
    a.tmpl8 = ctx->d_tmpl8.as<int8_t>();
    a.tsum = ctx->d_tsum.as<int32_t>();
    a.acc = ctx->d_tacc.as<uint64_t>();
    a.nlv = L + 1;
    int64_t bytes = 0;   // template pixels read + operand bytes and row sums written
    for (int l = 0; l <= L; ++l) {
        TmplPrepLevel& v = a.lv[l];
        const int rows = round_up(lv[l].h, kMmaRows);
        v.off = (uint32_t)lv[l].off; v.off8 = (uint32_t)lv[l].off8; v.tsum_off = (uint32_t)lv[l].tsum_off;
        v.w = lv[l].w; v.h = lv[l].h; v.pitch = lv[l].pitch; v.p8 = lv[l].p8;
        v.chunk0 = a.nchunks;
        a.nchunks += rows / kMmaRows;
        bytes += (int64_t)lv[l].w * lv[l].h + (int64_t)lv[l].p8 * rows + (int64_t)sizeof(int32_t) * rows;
    }
    a.slack_off = (uint32_t)(lv[L].off8 + (size_t)lv[L].p8 * round_up(lv[L].h, kMmaRows));
    {
        ProfScope ps(ctx, FPM_K_LEARN, bytes + 256);
        if (!launch_tmpl_prep(a, ctx->stream)) { ctx->err = "template slab layout: rows not 16-byte aligned"; return FPM_E_INTERNAL; }
    }
    HIP_TRY(hipGetLastError());
    const TmplLevel& top = lv[L];
    HIP_TRY(hipMemcpyAsync(ctx->h_tacc.p, ctx->d_tacc.p, kAccBytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(ctx->h_tacc.as<uint8_t>(kAccBytes), top.w, base + top.off, top.pitch, top.w, top.h,
                             hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    const uint64_t* acc = ctx->h_tacc.as<uint64_t>();
    for (int l = 0; l <= L; ++l)
        learn_derive((int64_t)lv[l].w * lv[l].h, (int64_t)acc[2 * l], (int64_t)acc[2 * l + 1], &lv[l].mean, &lv[l].norm,
                     &lv[l].inv_area, &lv[l].equal1);
    // the top level's pixels: plan_top_mma builds its B fragments from them; the others come on demand (fpm_template_level)
    lv[L].px.assign(ctx->h_tacc.as<uint8_t>(kAccBytes), ctx->h_tacc.as<uint8_t>(kAccBytes) + (size_t)top.w * top.h);
    ctx->border = lv[0].mean < 128 ? 255 : 0;   // :58-59
    ctx->tmpl = std::move(lv);
    ctx->learned = true;
    ctx->tmpl_gen++;
    ctx->searched = false;   // the last search's poses belong to the template before
    const std::string err = ctx->err;
    const bool keep = ctx->src_valid && ctx->S > 0 && ctx->src_L == L && check_sizes(ctx, ctx->sw, ctx->sh) == FPM_OK;
    ctx->err = err;
    if (!keep) {
        ctx->staged = false;
        ctx->src_valid = false;   // the slab's layout follows the template's pyramid depth
    }
    return FPM_OK;
}

// fpm_learn_device after its checks: the image staged into level 0 by k_stage_gray, ordered after the producer's stream
int learn_from_image(fpm_ctx* ctx, const void* d_image, int w, int h, size_t stride, size_t plane_stride, int format,
                     hipStream_t producer) {
    std::vector<TmplLevel> lv;
    ctx->model_n = 0;   // the variation model belongs to the template before
    mask_drop(ctx);     // and so does the mask
    int rc = learn_begin(ctx, w, h, lv);
    if (rc != FPM_OK) return rc;
    if (!ctx->in_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->in_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ctx->in_ev, producer));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->in_ev, 0));
    HIP_TRY(ctx->h_imgtab.ensure(sizeof(void*)));
    HIP_TRY(ctx->d_imgtab.ensure(sizeof(void*)));
    ctx->h_imgtab.as<const void*>()[0] = d_image;
    HIP_TRY(hipMemcpyAsync(ctx->d_imgtab.p, ctx->h_imgtab.p, sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    const bool aligned = (stride & 15) == 0 && (!fmt_planar(format) || (plane_stride & 15) == 0) &&
                         ((uintptr_t)d_image & 15) == 0;
    // the slab's level offsets are multiples of 256 and its pitches of 64: the launcher's alignment rule holds.  The
    // template is learned as given: no inversion, whatever fpm_params.bitwise_not says
    const TmplLevel& l0 = lv[0];
    if (!launch_stage_gray(ctx->d_imgtab.as<const uint8_t*>(), 1, w, h, stride, plane_stride, format, aligned,
                           ctx->d_tmpl.as<uint8_t>() + l0.off, l0.pitch, round_up((size_t)l0.pitch * (h + 1), (size_t)256),
                           false, ctx->stream)) {
        ctx->err = "template slab layout: level-0 rows not 16-byte aligned";
        return FPM_E_INTERNAL;
    }
    HIP_TRY(hipGetLastError());
    return learn_finish(ctx, lv);
}

// fpm_learn_at / fpm_learn_hit after their checks: the patch of `pose` sampled straight into level 0 (the patch
// entries' job table and launch, with the template slab as the output)
int learn_from_pose(fpm_ctx* ctx, const fpm_patch_rect& r, const PatchPose& pose) {
    std::vector<TmplLevel> lv;
    ctx->model_n = 0;   // the variation model belongs to the template before
    mask_drop(ctx);     // and so does the mask
    int rc = learn_begin(ctx, r.w, r.h, lv);
    if (rc != FPM_OK) return rc;
    const TmplLevel& l0 = lv[0];
    rc = enqueue_patches(ctx, r, std::vector<PatchPose>(1, pose), ctx->d_tmpl.as<uint8_t>() + l0.off, (size_t)l0.pitch,
                         (size_t)l0.pitch * r.h, nullptr);
    if (rc != FPM_OK) return rc;
    return learn_finish(ctx, lv);
}

// state, rectangle and pose checks shared by fpm_learn_at and fpm_learn_hit; nothing is touched before they pass
int learn_pose_entry(fpm_ctx* ctx, const fpm_patch_rect* rect, bool need_search, int source, int index, const RawPose* given) {
    int rc = patch_state(ctx, need_search);
    fpm_patch_rect r;
    if (rc == FPM_OK) rc = patch_rect(ctx, rect, &r);
    if (rc == FPM_OK) rc = learn_size(ctx, r.w, r.h);
    if (rc != FPM_OK) return rc;
    if (source < 0 || source >= ctx->S) { ctx->err = "bad source index"; return FPM_E_INVALID_ARG; }
    PatchPose pose{source, {}};
    if (given) {
        pose.pose = *given;
    } else {
        if (source >= (int)ctx->poses.size() || index < 0 || index >= (int)ctx->poses[source].size()) {
            ctx->err = "bad result index";
            return FPM_E_INVALID_ARG;
        }
        pose.pose = ctx->poses[source][index];
    }
    double M[6];
    rc = patch_pose_matrix(ctx, r, pose, 0, nullptr, M);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = learn_from_pose(ctx, r, pose);
    return rc == FPM_OK ? rc : learn_fail(ctx, rc);
}

// ---- variation model (fpm_model_*, fpm_last_inspect, fpm_inspect_at) ----
const char* kInFlight = "a search is in flight (fpm_match_staged_finish first)";

bool same_rect(const fpm_patch_rect& a, const fpm_patch_rect& b) { return a.x == b.x && a.y == b.y && a.w == b.w && a.h == b.h; }

int model_pitch(int w) { return round_up(w + 4, 64); }   // the template slab's rule: k_model_inspect reads dword pairs

// Jobs per workgroup of k_model_accum for n jobs over `tiles` tiles.  With enough tiles to fill the device every tile
// takes all its jobs (one owner per pixel: plain adds, no atomics); with fewer the jobs are cut into as many chunks as
// bring the grid to kModelWgPerCu workgroups per compute unit, each chunk adding to the planes with atomics -- but no
// chunk below kModelMinChunk jobs, where the atomics cost more than the idle compute units (DESIGN.md section 17 has
// the sweep both constants come from).
constexpr int kModelWgPerCu = 12;
constexpr int kModelMinChunk = 4;
int model_chunk_for(fpm_ctx* ctx, int n, int64_t tiles) {
    if (ctx->model_chunk > 0) return std::min(ctx->model_chunk, n);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0) cus = 256;
    const int64_t want = (int64_t)kModelWgPerCu * cus;
    const int64_t nchunks = std::min<int64_t>(n, std::max<int64_t>(1, (want + tiles - 1) / tiles));
    return std::min(n, std::max((int)((n + nchunks - 1) / nchunks), kModelMinChunk));
}

// The arguments of the sums launch of a normalised call over the model's rectangle, with d_cmpacc sized and cleared.
int model_norm_args(fpm_ctx* ctx, const fpm_patch_rect& r, int n, CompareArgs* c) {
    const size_t accb = sizeof(CompareAcc) * (size_t)n;
    HIP_TRY(ctx->d_cmpacc.ensure(accb));
    HIP_TRY(ctx->h_cmpacc.ensure(accb));
    HIP_TRY(hipMemsetAsync(ctx->d_cmpacc.p, 0, accb, ctx->stream));
    const TmplLevel& t0 = ctx->tmpl[0];
    *c = CompareArgs{};
    c->p = patch_args(ctx, r, n, nullptr, 0, 0);
    c->tmpl = ctx->d_tmpl.as<uint8_t>() + t0.off;
    c->tp = t0.pitch;
    c->rx = r.x; c->ry = r.y;
    c->acc = ctx->d_cmpacc.as<CompareAcc>();
    c->mask = mask_plane(ctx);   // the tables of a normalised call come from the used pixels
    return FPM_OK;
}

// Adds `poses` (n >= 1) to the model.  Everything that can reject the call comes before the first launch, so a call
// that fails adds nothing.
int model_train(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, int flags) {
    const int n = (int)poses.size();
    const bool norm = (flags & FPM_COMPARE_NORMALIZE) != 0;
    if (ctx->model_n > 0 && !same_rect(r, ctx->model_rect)) {
        ctx->err = "the variation model was trained on another rectangle (fpm_model_clear first)";
        return FPM_E_INVALID_ARG;
    }
    if (n > kModelMaxSamples - ctx->model_n) { ctx->err = "the variation model holds at most 65535 samples"; return FPM_E_CAPACITY; }
    int rc = stage_patch_jobs(ctx, r, poses, nullptr, 0, 0, nullptr, true, norm ? (size_t)256 * n : 0);
    if (rc != FPM_OK) return rc;
    const size_t px = (size_t)r.w * r.h, plane = px * sizeof(uint32_t);
    HIP_TRY(ctx->d_model.ensure(2 * plane));
    if (ctx->model_n == 0) HIP_TRY(hipMemsetAsync(ctx->d_model.p, 0, 2 * plane, ctx->stream));
    ModelAccumArgs m{};
    m.p = patch_args(ctx, r, n, nullptr, 0, 0);
    m.sum = ctx->d_model.as<uint32_t>();
    m.sum_sq = m.sum + px;
    if (norm) {
        CompareArgs c;
        rc = model_norm_args(ctx, r, n, &c);
        if (rc == FPM_OK) rc = compare_norm_tables(ctx, c, r, n, &m.luts);
        if (rc != FPM_OK) return rc;
    }
    const int64_t tiles = (int64_t)((r.w + 63) / 64) * ((r.h + 15) / 16);
    {
        // bytes: source pixels read + plane bytes written
        ProfScope ps(ctx, kProfModelTrain, (int64_t)n * r.w * r.h + 2 * (int64_t)plane);
        if (!launch_model_accum(m, model_chunk_for(ctx, n, tiles), ctx->stream)) {
            ctx->err = "too many patch tiles for one launch";
            return FPM_E_INVALID_ARG;
        }
    }
    HIP_TRY(hipGetLastError());
    ctx->model_rect = r;
    ctx->model_n += n;
    ctx->model_gen++;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return FPM_OK;
}

// the model's rectangle; FPM_E_INVALID_ARG without a model.  It lies inside the template: every entry that changes the
// template drops the model, except fpm_model_learn, which makes the rectangle the new template's frame.
int model_need(fpm_ctx* ctx, fpm_patch_rect* r) {
    if (ctx->model_n <= 0) { ctx->err = "no variation model (fpm_model_train_last / fpm_model_train_at first)"; return FPM_E_INVALID_ARG; }
    *r = ctx->model_rect;
    return FPM_OK;
}

// the RectRule of the inspection and the blobs: the model's rectangle under the comparison's rules; no rectangle is passed
int model_rect(fpm_ctx* ctx, const fpm_patch_rect*, fpm_patch_rect* r) {
    fpm_patch_rect mr;
    const int rc = model_need(ctx, &mr);
    return rc != FPM_OK ? rc : compare_rect(ctx, &mr, r);
}

int model_args(fpm_ctx* ctx, int a, int kq) {
    if (a < 0 || a > 255 || kq < 0 || kq > 255) {
        ctx->err = "abs threshold must be 0 .. 255 and the sigma multiple 0 .. 255 sixteenths";
        return FPM_E_INVALID_ARG;
    }
    return FPM_OK;
}

// mean / lo / hi for (a, kq) in d_band, prepared on the context's stream when the key changed (no wait)
int model_band_ensure(fpm_ctx* ctx, int a, int kq) {
    const fpm_patch_rect& r = ctx->model_rect;
    const int pitch = model_pitch(r.w);
    const size_t plane = (size_t)pitch * r.h;
    if (ctx->band_a == a && ctx->band_kq == kq && ctx->band_gen == ctx->model_gen) return FPM_OK;
    ctx->band_gen = ~0ull;
    HIP_TRY(ctx->d_band.ensure(3 * plane));
    HIP_TRY(hipMemsetAsync(ctx->d_band.p, 0, 3 * plane, ctx->stream));   // the padding of the rows is read (and masked off)
    const size_t px = (size_t)r.w * r.h;
    ModelPrepareArgs p{};
    p.sum = ctx->d_model.as<uint32_t>();
    p.sum_sq = p.sum + px;
    p.w = r.w; p.h = r.h; p.n = ctx->model_n;
    p.a = a; p.kq = kq;
    p.mean = ctx->d_band.as<uint8_t>();
    p.lo = p.mean + plane;
    p.hi = p.lo + plane;
    p.pitch = pitch;
    {
        ProfScope ps(ctx, kProfModelPrepare, (int64_t)px * (2 * (int64_t)sizeof(uint32_t) + 3));   // planes in and out
        launch_model_prepare(p, ctx->stream);
    }
    HIP_TRY(hipGetLastError());
    ctx->band_a = a; ctx->band_kq = kq; ctx->band_gen = ctx->model_gen;
    return FPM_OK;
}

// The inspection of `poses` (n >= 1) against the model: the planes for (a, kq), one launch of k_model_inspect (after
// the sums launch and the tables with FPM_COMPARE_NORMALIZE).  Returns when out (and img) are filled.  keep_device: the
// excess images are written to the pitched patch buffer also without img, and stay there (the blob entries label them).
int inspect_to_host(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, int a, int kq, int flags,
                    fpm_inspect_stats* out, uint8_t* img, size_t row_stride, size_t patch_stride,
                    bool keep_device = false) {
    const int n = (int)poses.size();
    const bool norm = (flags & FPM_COMPARE_NORMALIZE) != 0;
    const size_t pitch = round_up((size_t)r.w, (size_t)64), pbytes = pitch * (size_t)r.h;
    uint8_t* d = nullptr;   // the excess images: the context's pitched buffer, as for the host patches
    if (img || keep_device) {
        HIP_TRY(ctx->d_patch.ensure(pbytes * (size_t)n));
        d = ctx->d_patch.as<uint8_t>();
    }
    int rc = stage_patch_jobs(ctx, r, poses, d, pitch, pbytes, nullptr, true, norm ? (size_t)256 * n : 0);
    if (rc == FPM_OK) rc = model_band_ensure(ctx, a, kq);
    if (rc != FPM_OK) return rc;
    const size_t accb = sizeof(InspectAcc) * (size_t)n;
    HIP_TRY(ctx->d_insacc.ensure(accb));
    HIP_TRY(ctx->h_insacc.ensure(accb));
    HIP_TRY(hipMemsetAsync(ctx->d_insacc.p, 0, accb, ctx->stream));   // also "no pixel outside its interval"
    const int mp = model_pitch(r.w);
    InspectArgs c{};
    c.p = patch_args(ctx, r, n, d, pitch, pbytes);
    c.lo = ctx->d_band.as<uint8_t>() + (size_t)mp * r.h;
    c.hi = c.lo + (size_t)mp * r.h;
    c.mp = mp;
    c.acc = ctx->d_insacc.as<InspectAcc>();
    c.mask = mask_plane(ctx);
    c.mkp = ctx->tmpl[0].pitch;
    c.mx = r.x; c.my = r.y;
    const int64_t used = mask_used(ctx, r);
    if (norm) {
        CompareArgs s;
        rc = model_norm_args(ctx, r, n, &s);
        if (rc == FPM_OK) rc = compare_norm_tables(ctx, s, r, n, &c.luts);
        if (rc != FPM_OK) return rc;
    }
    {
        // bytes: source pixels read + lo and hi read (+ mask bytes read) (+ excess pixels written)
        ProfScope ps(ctx, kProfModelInspect, (3 + (c.mask ? 1 : 0) + (d ? 1 : 0)) * (int64_t)n * r.w * r.h);
        if (!launch_model_inspect(c, ctx->stream)) { ctx->err = "too many patch tiles for one launch"; return FPM_E_INVALID_ARG; }
    }
    HIP_TRY(hipGetLastError());
    InspectAcc* h = ctx->h_insacc.as<InspectAcc>();
    HIP_TRY(hipMemcpyAsync(h, ctx->d_insacc.p, accb, hipMemcpyDeviceToHost, ctx->stream));
    if (img) {
        rc = copy_patches_out(ctx, r, (size_t)n, d, pitch, pbytes, img, row_stride, patch_stride);
        if (rc != FPM_OK) return rc;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    const CompareAcc* sums = ctx->h_cmpacc.as<CompareAcc>();
    for (int i = 0; i < n; ++i) {
        fpm_inspect_stats& s = out[i];
        const uint32_t* f = h[i].f;
        s.n = used;
        s.sum_excess = (int64_t)f[kInsSumExcess];
        s.n_low = (int32_t)f[kInsNLow]; s.n_high = (int32_t)f[kInsNHigh]; s.max_excess = (int32_t)f[kInsMaxExcess];
        s.x0 = r.w - (int32_t)f[kInsX0]; s.y0 = r.h - (int32_t)f[kInsY0];
        s.x1 = (int32_t)f[kInsX1] - 1; s.y1 = (int32_t)f[kInsY1] - 1;
        s.gain = 1.0; s.offset = 0.0;
        if (norm) {
            double z;
            compare_derive_used(used, sums[i], true, &z, &s.gain, &s.offset, nullptr);
        }
    }
    return FPM_OK;
}

// ---- defect blobs on the device (fpm_last_blobs / fpm_blobs_at / fpm_op_blobs) ----
static_assert(sizeof(BlobRec) == sizeof(fpm_blob) && offsetof(BlobRec, hit) == offsetof(fpm_blob, hit) &&
                  offsetof(BlobRec, seed) == offsetof(fpm_blob, seed) && offsetof(BlobRec, area) == offsetof(fpm_blob, area) &&
                  offsetof(BlobRec, x0) == offsetof(fpm_blob, x0) && offsetof(BlobRec, y1) == offsetof(fpm_blob, y1) &&
                  offsetof(BlobRec, max_value) == offsetof(fpm_blob, max_value) &&
                  offsetof(BlobRec, sum_value) == offsetof(fpm_blob, sum_value) &&
                  offsetof(BlobRec, sum_x) == offsetof(fpm_blob, sum_x) && offsetof(BlobRec, sum_y) == offsetof(fpm_blob, sum_y),
              "the kernels' record is fpm_blob, field for field");
static_assert(sizeof(BlobCount) == sizeof(BlobCounters) && offsetof(BlobCount, fg) == offsetof(BlobCounters, fg_pixels) &&
                  offsetof(BlobCount, comps) == offsetof(BlobCounters, n_components) &&
                  offsetof(BlobCount, qual) == offsetof(BlobCounters, n_qualifying) &&
                  offsetof(BlobCount, largest) == offsetof(BlobCounters, largest_area),
              "the kernels' counters are blobs_gather's");

// Design constants, not measurements: the label and area planes of a round stay within 256 MiB (8 bytes per pixel and
// image), its records within 64 MiB.
constexpr size_t kBlobPlaneBudget = (size_t)256 << 20;
constexpr size_t kBlobRecBudget = (size_t)64 << 20;

struct BlobRun {
    int n = 0, w = 0, h = 0, round = 0, cap_dev = 0;
    size_t npx = 0, rec_off = 0;   // the records' offset behind the counters in d_blobrec / h_blobrec
    bool labels = false;
};

// Everything a labelling call allocates, sized for its largest round.  It comes before the call's first launch: ensure()
// frees and reallocates, so no buffer may grow between rounds, and pointers are taken only afterwards (blobs_run).
int blobs_reserve(fpm_ctx* ctx, int n, int w, int h, int min_area, int cap_per_hit, bool labels, BlobRun* b) {
    b->n = n; b->w = w; b->h = h; b->labels = labels;
    b->npx = (size_t)w * h;
    b->cap_dev = blobs_cap_dev(w, h, min_area, cap_per_hit);
    size_t round = std::max<size_t>(1, kBlobPlaneBudget / (2 * sizeof(int32_t) * b->npx));
    round = std::min(round, std::max<size_t>(1, kBlobRecBudget / (sizeof(BlobRec) * (size_t)b->cap_dev)));
    if (ctx->blobs_round > 0) round = std::min(round, (size_t)ctx->blobs_round);
    b->round = (int)std::min<size_t>(round, (size_t)std::min(n, 65535));
    b->rec_off = round_up(sizeof(BlobCount) * (size_t)b->round, (size_t)256);
    const size_t rec_bytes = b->rec_off + sizeof(BlobRec) * (size_t)b->round * b->cap_dev;
    HIP_TRY(ctx->d_blobplanes.ensure(2 * sizeof(int32_t) * b->npx * b->round));
    HIP_TRY(ctx->d_blobrec.ensure(rec_bytes));
    HIP_TRY(ctx->h_blobrec.ensure(rec_bytes));
    if (labels) HIP_TRY(ctx->h_bloblab.ensure(sizeof(int32_t) * b->npx * b->round));
    return FPM_OK;
}

// Labels the n images at d_img (image i at d_img + i * img_stride, rows pitch apart) round by round after
// blobs_reserve: counters and records cleared on the stream, the five launches, one copy of counters and records (and
// of the labels) into the context's pinned buffers, then blobs_gather into the caller's memory.  Device results never go
// straight into caller memory.
int blobs_run(fpm_ctx* ctx, const BlobRun& b, const uint8_t* d_img, size_t pitch, size_t img_stride, int level,
              int connectivity, int min_area, int cap_per_hit, fpm_blob_summary* summary, fpm_blob* out, int32_t* labels) {
    hipStream_t st = ctx->stream;
    int32_t* dL = ctx->d_blobplanes.as<int32_t>();
    char* drec = ctx->d_blobrec.as<char>();
    char* hrec = ctx->h_blobrec.as<char>();
    const int32_t* hlab = b.labels ? ctx->h_bloblab.as<int32_t>() : nullptr;
    for (int i0 = 0; i0 < b.n; i0 += b.round) {
        const int nr = std::min(b.round, b.n - i0);
        const size_t used = b.rec_off + sizeof(BlobRec) * (size_t)nr * b.cap_dev;
        const int64_t px = (int64_t)nr * (int64_t)b.npx;
        HIP_TRY(hipMemsetAsync(drec, 0, used, st));
        BlobArgs a{};
        a.img = d_img + (size_t)i0 * img_stride;
        a.pitch = pitch; a.img_stride = img_stride;
        a.n = nr; a.w = b.w; a.h = b.h;
        a.level = level; a.conn8 = connectivity == 8 ? 1 : 0; a.min_area = min_area;
        a.cap_dev = b.cap_dev; a.hit0 = i0;
        a.L = dL;
        a.A = dL + (size_t)b.round * b.npx;
        a.cnt = (BlobCount*)drec;
        a.rec = (BlobRec*)(drec + b.rec_off);
        const int64_t tiles = (int64_t)nr * ((b.w + 63) / 64) * ((b.h + 15) / 16);
        bool ok = true;
        {   // the excess pixels read, L and A written
            ProfScope ps(ctx, kProfBlobTile, 9 * px);
            ok = launch_blob_tile(a, st);
        }
        if (ok) {   // the labels of the border pixels and of their neighbours beyond the border
            ProfScope ps(ctx, kProfBlobMerge, tiles * (64 + 15 + 15) * 2 * (int64_t)sizeof(int32_t));
            ok = launch_blob_merge(a, st);
        }
        if (ok) {   // L read and written (the area adds go to the roots)
            ProfScope ps(ctx, kProfBlobFlatten, 8 * px);
            ok = launch_blob_flatten(a, st);
        }
        if (ok) {   // L read (A at the roots)
            ProfScope ps(ctx, kProfBlobSlots, 4 * px);
            ok = launch_blob_slots(a, st);
        }
        if (ok) {   // L and the excess pixels read, A at the roots
            ProfScope ps(ctx, kProfBlobFeatures, 5 * px);
            ok = launch_blob_features(a, st);
        }
        if (!ok) { ctx->err = "too many tiles for one labelling launch"; return FPM_E_INVALID_ARG; }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(hrec, drec, used, hipMemcpyDeviceToHost, st));
        if (hlab) HIP_TRY(hipMemcpyAsync((void*)hlab, dL, sizeof(int32_t) * (size_t)px, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        prof_collect(ctx);
        blobs_gather((const BlobCounters*)hrec, (fpm_blob*)(hrec + b.rec_off), nr, b.cap_dev, min_area, cap_per_hit,
                     out + (size_t)i0 * cap_per_hit, summary + i0);
        if (hlab) {
            int32_t* lab = labels + (size_t)i0 * b.npx;
            for (int64_t k = 0; k < px; ++k) lab[k] = hlab[k] + 1;   // seed + 1, background 0
        }
    }
    return FPM_OK;
}

// The inspection with its excess images kept in the pitched patch buffer, then the labelling of those images.
int blobs_of_poses(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, int a, int kq, int flags,
                   int level, int connectivity, int min_area, int cap_per_hit, fpm_inspect_stats* stats,
                   fpm_blob_summary* summary, fpm_blob* out) {
    const int n = (int)poses.size();
    BlobRun b;
    int rc = blobs_reserve(ctx, n, r.w, r.h, min_area, cap_per_hit, false, &b);
    if (rc != FPM_OK) return rc;
    std::vector<fpm_inspect_stats> st((size_t)n);
    rc = inspect_to_host(ctx, r, poses, a, kq, flags, st.data(), nullptr, 0, 0, true);
    if (rc != FPM_OK) return rc;
    const size_t pitch = round_up((size_t)r.w, (size_t)64);
    rc = blobs_run(ctx, b, ctx->d_patch.as<uint8_t>(), pitch, pitch * (size_t)r.h, level, connectivity, min_area,
                   cap_per_hit, summary, out, nullptr);
    if (rc != FPM_OK) return rc;
    if (stats) std::copy(st.begin(), st.end(), stats);
    return FPM_OK;
}

// ---- pose alignment (fpm_align_*) ----
static_assert(sizeof(fpm_align_sums) == sizeof(AlignAcc), "the kernel's record is fpm_align_sums, field for field");
static_assert(sizeof(fpm_align_result) == 56, "fpm_align_result has no padding");

// A comparison rectangle under the alignment's narrower caps (include/fpm.h derives the sums' bound from them).
int align_rect(fpm_ctx* ctx, const fpm_patch_rect* rect, fpm_patch_rect* r) {
    const int rc = compare_rect(ctx, rect, r);
    if (rc != FPM_OK) return rc;
    if (r->w > kAlignMaxSide || r->h > kAlignMaxSide || (int64_t)r->w * r->h > kAlignMaxArea) {
        ctx->err = "bad alignment rectangle: at most 2^20 pixels and sides of at most 4096";
        return FPM_E_INVALID_ARG;
    }
    return FPM_OK;
}

// The step of one record (include/fpm.h states the expression order; -ffp-contract=off).  true = singular, step 0.
bool align_solve(const fpm_align_sums& m, double* du, double* dv, double* dphi) {
    *du = *dv = *dphi = 0.0;
    if (m.n_used < 3) return true;
    const double hxx = (double)m.h_xx, hxy = (double)m.h_xy, hyy = (double)m.h_yy, hxt = (double)m.h_xt,
                 hyt = (double)m.h_yt, htt = (double)m.h_tt, gx = (double)m.g_x, gy = (double)m.g_y, gt = (double)m.g_t;
    const double c00 = hyy * htt - hyt * hyt, c01 = hxt * hyt - hxy * htt, c02 = hxy * hyt - hxt * hyy;
    const double c11 = hxx * htt - hxt * hxt, c12 = hxy * hxt - hxx * hyt, c22 = hxx * hyy - hxy * hxy;
    const double det = (hxx * c00 + hxy * c01) + hxt * c02;
    if (!(det > 0.0) || !std::isfinite(det)) return true;
    const double q0 = -(((c00 * gx + c01 * gy) + c02 * gt) / det);
    const double q1 = -(((c01 * gx + c11 * gy) + c12 * gt) / det);
    const double q2 = -(((c02 * gx + c12 * gy) + c22 * gt) / det);
    const double u = 2.0 * q0, v = 2.0 * q1, p = 4.0 * q2;
    if (!std::isfinite(u) || !std::isfinite(v) || !std::isfinite(p)) return true;
    *du = u; *dv = v; *dphi = p;
    return false;
}

// The pose whose patch map is A o D (include/fpm.h), as a difference from the current pose: a zero step returns it.
RawPose align_update(int sw, int sh, const fpm_patch_rect& r, const RawPose& p, double du, double dv, double dphi) {
    double A[6];
    patch_forward(sw, sh, p, r.x, r.y, A);
    invert_affine(A);
    const double kx = r.x + (r.w - 1) / 2.0, ky = r.y + (r.h - 1) / 2.0;
    const double angle2 = p.angle + dphi * kR2D;
    const double ra = p.angle * kD2R, rb = angle2 * kD2R;
    const double dc = std::cos(ra) - std::cos(rb), ds = std::sin(ra) - std::sin(rb);
    const double mx = (A[0] * du + A[1] * dv) + (dc * kx - ds * ky);
    const double my = (A[3] * du + A[4] * dv) + (ds * kx + dc * ky);
    return RawPose{(float)((double)p.x + mx), (float)((double)p.y + my), angle2};
}

// Would the step move a corner of the rectangle by more than max_step?  (Patch pixels are source pixels: scale 1.)
bool align_step_too_far(const fpm_patch_rect& r, double du, double dv, double dphi, double max_step) {
    const double c = std::cos(dphi), s = std::sin(dphi), hx = (r.w - 1) / 2.0, hy = (r.h - 1) / 2.0;
    const double lim = max_step * max_step;
    for (int k = 0; k < 4; ++k) {
        const double ex = (k & 1) ? hx : -hx, ey = (k & 2) ? hy : -hy;
        const double mx = ((c * ex - s * ey) - ex) + du, my = ((s * ex + c * ey) - ey) + dv;
        if (mx * mx + my * my > lim) return true;
    }
    return false;
}

// The job table of the start poses and, with FPM_COMPARE_NORMALIZE, the hits' tables built there as fpm_last_compare
// builds them (*luts stays null otherwise).  The tables lie behind the job table and survive its later restaging.
int align_begin(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, bool norm, const uint8_t** luts) {
    const int n = (int)poses.size();
    *luts = nullptr;
    int rc = stage_patch_jobs(ctx, r, poses, nullptr, 0, 0, nullptr, true, norm ? (size_t)256 * n : 0);
    if (rc != FPM_OK || !norm) return rc;
    CompareArgs c;
    rc = model_norm_args(ctx, r, n, &c);
    if (rc == FPM_OK) rc = compare_norm_tables(ctx, c, r, n, luts);
    return rc;
}

// One evaluation: the job table of `poses` (restaged unless the caller has just staged it), the records cleared, one
// launch of k_patch_align, the records to `out`.  Synchronises the stream.
int align_launch(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, bool restage, bool norm,
                 const uint8_t* luts, fpm_align_sums* out) {
    const int n = (int)poses.size();
    const size_t accb = sizeof(AlignAcc) * (size_t)n;
    if (restage) {
        const int rc = stage_patch_jobs(ctx, r, poses, nullptr, 0, 0, nullptr, true, norm ? (size_t)256 * n : 0);
        if (rc != FPM_OK) return rc;
    }
    HIP_TRY(ctx->d_alnacc.ensure(accb));
    HIP_TRY(ctx->h_alnacc.ensure(accb));
    HIP_TRY(hipMemsetAsync(ctx->d_alnacc.p, 0, accb, ctx->stream));
    const TmplLevel& t0 = ctx->tmpl[0];
    AlignArgs c{};
    c.p = patch_args(ctx, r, n, nullptr, 0, 0);
    c.tmpl = ctx->d_tmpl.as<uint8_t>() + t0.off;
    c.tp = t0.pitch;
    c.tw = t0.w; c.th = t0.h;
    c.rx = r.x; c.ry = r.y;
    c.luts = luts;
    c.acc = ctx->d_alnacc.as<AlignAcc>();
    c.mask = mask_plane(ctx);
    {
        // source pixels read + template pixels read (+ mask bytes read)
        ProfScope ps(ctx, kProfAlign, (2 + (c.mask ? 1 : 0)) * (int64_t)n * r.w * r.h);
        if (!launch_patch_align(c, ctx->stream)) { ctx->err = "too many patch tiles for one launch"; return FPM_E_INVALID_ARG; }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_alnacc.p, ctx->d_alnacc.p, accb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    std::memcpy(out, ctx->h_alnacc.p, accb);   // two's complement: the u64 records are the int64 sums
    return FPM_OK;
}

int align_sums_to_host(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, int flags,
                       fpm_align_sums* out) {
    const bool norm = (flags & FPM_COMPARE_NORMALIZE) != 0;
    const uint8_t* luts = nullptr;
    const int rc = align_begin(ctx, r, poses, norm, &luts);
    return rc != FPM_OK ? rc : align_launch(ctx, r, poses, false, norm, luts, out);
}

// The iteration from `start` (n >= 1): iters + 1 evaluations, the host's solve and update between them.  out and
// aligned (the returned poses, may be null) are written only when the whole call succeeds.
int align_iterate(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& start, int iters, double max_step,
                  int flags, fpm_align_result* out, std::vector<PatchPose>* aligned) {
    const int n = (int)start.size();
    const bool norm = (flags & FPM_COMPARE_NORMALIZE) != 0;
    const uint8_t* luts = nullptr;
    int rc = align_begin(ctx, r, start, norm, &luts);
    if (rc != FPM_OK) return rc;
    std::vector<PatchPose> cur = start, best = start;
    std::vector<fpm_align_sums> sums((size_t)n);
    std::vector<fpm_align_result> res((size_t)n);
    std::vector<char> frozen((size_t)n, 0), moved((size_t)n, 0);
    for (int k = 0; k <= iters; ++k) {
        rc = align_launch(ctx, r, cur, k > 0, norm, luts, sums.data());
        if (rc != FPM_OK) return rc;
        for (int i = 0; i < n; ++i) {
            fpm_align_result& o = res[i];
            const fpm_align_sums& s = sums[i];
            if (k == 0) {
                o = fpm_align_result{};
                o.ssd_start = o.ssd = s.ssd;
                o.n_used = s.n_used;
                o.evals = 1;
            } else if (moved[i]) {
                o.evals = k + 1;
                if (s.ssd < o.ssd) { o.ssd = s.ssd; o.n_used = s.n_used; o.best_eval = k; best[i] = cur[i]; }
            }
            moved[i] = 0;
            if (k == iters || frozen[i]) continue;
            double du, dv, dphi;
            if (align_solve(s, &du, &dv, &dphi)) { frozen[i] = 1; o.flags |= FPM_ALIGN_SINGULAR; continue; }
            bool far = align_step_too_far(r, du, dv, dphi, max_step);
            PatchPose next = cur[i];
            if (!far) {
                // the samplers' range, by the check the next staging makes
                next.pose = align_update(ctx->sw, ctx->sh, r, cur[i].pose, du, dv, dphi);
                const std::string err = ctx->err;
                double M[6];
                far = patch_pose_matrix(ctx, r, next, i, nullptr, M) != FPM_OK;
                ctx->err = err;
            }
            if (far) { frozen[i] = 1; o.flags |= FPM_ALIGN_STEP_CLAMPED; continue; }
            cur[i] = next;
            moved[i] = 1;
        }
    }
    for (int i = 0; i < n; ++i) {
        fpm_align_result& o = res[i];
        o.lt_x = best[i].pose.x; o.lt_y = best[i].pose.y; o.angle = best[i].pose.angle;
        if (o.best_eval == 0) o.flags |= FPM_ALIGN_KEPT_START;
        out[i] = o;
    }
    if (aligned) *aligned = best;
    return FPM_OK;
}

// ---- edge calipers (fpm_last_calipers, fpm_calipers_at) ----
static_assert(sizeof(fpm_caliper) == 48 && sizeof(fpm_edge) == 64 && sizeof(fpm_caliper_summary) == 32,
              "the caliper structs have no padding");
static_assert(sizeof(fpm_edge_raw) == sizeof(int4), "the kernel's record is fpm_edge_raw, field for field");
static_assert(kCaliperMaxLength == FPM_CALIPER_MAX_LENGTH && kCaliperMaxWidth == FPM_CALIPER_MAX_WIDTH &&
              kCaliperMaxHalf == FPM_CALIPER_MAX_HALF && kCaliperMaxCap == FPM_CALIPER_MAX_CAP, "one set of caps");

// Staged sources, no search in flight; unlike patch_state no template: a caliper reads level 0 alone.
int caliper_state(fpm_ctx* ctx) {
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    if (!ctx->src_valid || ctx->S <= 0 || ctx->src.empty() || !ctx->d_src.p) {
        ctx->err = "no staged sources to measure on";
        return FPM_E_INVALID_ARG;
    }
    return FPM_OK;
}

// the rules of a call's calipers and capacity that do not depend on the number of hits
int caliper_args(fpm_ctx* ctx, const fpm_caliper* cals, int32_t n_cals, int32_t cap_per) {
    if (!cals || n_cals < 1 || n_cals > FPM_CALIPER_MAX_CALS) { ctx->err = "1 .. 64 calipers expected"; return FPM_E_INVALID_ARG; }
    if (cap_per < 1 || cap_per > FPM_CALIPER_MAX_CAP) { ctx->err = "cap_per_caliper must be 1 .. 64"; return FPM_E_INVALID_ARG; }
    for (int k = 0; k < n_cals; ++k)
        if (const char* bad = caliper_bad(cals[k])) { ctx->err = bad; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

// and those that do: the outputs and the slots
int caliper_outputs(fpm_ctx* ctx, size_t hits, const fpm_caliper* cals, int32_t n_cals, int32_t cap_per,
                    const fpm_caliper_summary* summary, const fpm_edge* edges, const int32_t* profiles, int32_t stride) {
    if (!summary || !edges) { ctx->err = "null summary or edge buffer"; return FPM_E_INVALID_ARG; }
    if ((int64_t)hits * n_cals * cap_per > FPM_CALIPER_MAX_SLOTS) {
        ctx->err = "hits x calipers x cap_per_caliper above 2^22";
        return FPM_E_INVALID_ARG;
    }
    int max_len = 0;
    for (int k = 0; k < n_cals; ++k) max_len = std::max(max_len, cals[k].length);
    if (profiles && stride < max_len) { ctx->err = "profile_stride below the largest length"; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

// The calipers of `poses` (n >= 1), every argument checked: the job table, one launch of k_caliper, the raw records,
// counts and profiles to pinned memory, then the derivation into the caller's buffers.  Caller memory is written only
// after the device pass has succeeded.
int calipers_to_host(fpm_ctx* ctx, const std::vector<PatchPose>& poses, const fpm_caliper* cals, int n_cals, int cap_per,
                     fpm_caliper_summary* summary, fpm_edge* edges, int32_t* profiles, int32_t stride) {
    const int njobs = (int)poses.size() * n_cals;
    int max_len = 0;
    for (int k = 0; k < n_cals; ++k) max_len = std::max(max_len, cals[k].length);
    const size_t tab = round_up(sizeof(CaliperJob) * (size_t)njobs, (size_t)256);
    CaliperJob* jobs = nullptr;
    int rc = tab_begin(ctx, tab, &jobs);
    if (rc != FPM_OK) return rc;
    // the device output: records, counts, then the profiles at the largest length (the caller's stride is the host's)
    const size_t rec_b = sizeof(int4) * (size_t)njobs * cap_per, cnt_b = round_up(sizeof(int32_t) * (size_t)njobs, (size_t)16);
    const size_t prof_b = profiles ? sizeof(int32_t) * (size_t)njobs * max_len : 0;
    HIP_TRY(ctx->d_calout.ensure(rec_b + cnt_b + prof_b));
    HIP_TRY(ctx->h_calout.ensure(rec_b + cnt_b + prof_b));
    std::vector<fpm_caliper_summary> sm((size_t)njobs);
    int64_t bytes = (int64_t)(rec_b + sizeof(int32_t) * (size_t)njobs + prof_b);
    for (int i = 0, j = 0; i < (int)poses.size(); ++i)
        for (int k = 0; k < n_cals; ++k, ++j) {
            const fpm_caliper& c = cals[k];
            PatchPose q{poses[i].src, poses[i].pose};
            if (!std::isfinite(q.pose.x) || !std::isfinite(q.pose.y) || !std::isfinite(q.pose.angle)) {
                ctx->err = "pose " + std::to_string(i) + ": not finite";
                return FPM_E_INVALID_ARG;
            }
            caliper_pose(poses[i].pose.x, poses[i].pose.y, poses[i].pose.angle, c, &q.pose.x, &q.pose.y, &q.pose.angle);
            const fpm_patch_rect r{0, 0, c.length, c.width};
            CaliperJob& job = jobs[j];
            rc = tab_head(ctx, job.p, r, q, i, (int64_t)j * cap_per);
            if (rc != FPM_OK) return rc;
            job.L = c.length; job.W = c.width; job.s = c.half;
            job.thr = c.contrast * c.half * c.width;
            job.polarity = c.polarity;
            job.pad = 0;
            job.prof_off = (int64_t)j * max_len;
            bytes += (int64_t)c.length * c.width;
            const bool outside = corners_outside(ctx, job.p.M, c.length, c.width);   // border zeros in the profile
            sm[j] = fpm_caliper_summary{0, 0, -1, outside ? FPM_CALIPER_OUTSIDE : 0, q.pose.x, q.pose.y, q.pose.angle};
        }
    rc = tab_send(ctx, tab);
    if (rc != FPM_OK) return rc;
    CaliperArgs a = source_args<CaliperArgs>(ctx, njobs);
    a.cap = cap_per;
    a.prof_stride = max_len;
    a.edges = ctx->d_calout.as<int4>();
    a.counts = ctx->d_calout.as<int32_t>(rec_b);
    a.profiles = profiles ? ctx->d_calout.as<int32_t>(rec_b + cnt_b) : nullptr;
    {
        ProfScope ps(ctx, kProfCaliper, bytes);   // L W source pixels per job + the records, counts and profiles written
        if (!launch_caliper(a, ctx->stream)) { ctx->err = "bad caliper launch"; return FPM_E_INTERNAL; }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_calout.p, ctx->d_calout.p, rec_b + cnt_b + prof_b, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    const fpm_edge_raw* raw = ctx->h_calout.as<fpm_edge_raw>();
    const int32_t* counts = ctx->h_calout.as<int32_t>(rec_b);
    const int32_t* prof = ctx->h_calout.as<int32_t>(rec_b + cnt_b);
    for (int j = 0; j < njobs; ++j) {   // what the device wrote is checked before anything of it reaches the caller
        const fpm_caliper& c = cals[j % n_cals];
        const int32_t n = counts[j], nret = std::min(n, (int32_t)cap_per);
        fpm_edge e;
        bool ok = n >= 0 && n <= c.length;
        for (int32_t i = 0; ok && i < nret; ++i)
            ok = caliper_derive(c, sm[j].lt_x, sm[j].lt_y, sm[j].angle, raw[(size_t)j * cap_per + i], &e);
        if (!ok) { ctx->err = "k_caliper returned a record that is no edge"; return FPM_E_INTERNAL; }
    }
    for (int j = 0; j < njobs; ++j) {
        const fpm_caliper& c = cals[j % n_cals];
        const fpm_edge_raw* rj = raw + (size_t)j * cap_per;
        fpm_edge* ej = edges + (size_t)j * cap_per;
        fpm_caliper_summary& s = sm[j];
        s.n_edges = counts[j];
        s.n_returned = std::min(s.n_edges, (int32_t)cap_per);
        if (s.n_edges > cap_per) s.flags |= FPM_CALIPER_TRUNCATED;
        s.strongest = caliper_strongest(rj, s.n_returned);
        for (int32_t i = 0; i < s.n_returned; ++i) (void)caliper_derive(c, s.lt_x, s.lt_y, s.angle, rj[i], ej + i);
        if (s.n_returned < cap_per) std::memset(ej + s.n_returned, 0, sizeof(fpm_edge) * (size_t)(cap_per - s.n_returned));
        summary[j] = s;
        if (profiles) {
            int32_t* pj = profiles + (size_t)j * stride;
            std::memcpy(pj, prof + (size_t)j * max_len, sizeof(int32_t) * (size_t)max_len);
            if (stride > max_len) std::memset(pj + max_len, 0, sizeof(int32_t) * (size_t)(stride - max_len));
        }
    }
    return FPM_OK;
}

// ---- gray-value tools (fpm_last_histogram, fpm_histogram_at, fpm_last_segment, fpm_segment_at) ----
static_assert(sizeof(fpm_hist_stats) == 64 && sizeof(fpm_segment_info) == 16, "the gray-value structs have no padding");
static_assert(sizeof(GrayJob) % 8 == 0, "a table of GrayJob keeps its doubles aligned");

// Tiles per workgroup of k_patch_hist for `tiles` tiles in all: k_model_accum's rule turned round -- as many tiles as
// bring the grid down to kGrayWgPerCu workgroups per compute unit, so that a workgroup's 256 global adds are shared by a
// run of tiles; fpm_gray_set_run overrides it.  k_model_accum's own 12 per compute unit was measured too (DESIGN.md
// section 23): a compute unit holds 8 of these workgroups at once, so 12 is one full round and a half-empty one, and the
// launch was 15 % slower than at 74.
constexpr int kGrayWgPerCu = 64;
int gray_run_for(fpm_ctx* ctx, int64_t tiles) {
    if (ctx->gray_run > 0) return ctx->gray_run;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0) cus = 256;
    const int64_t want = (int64_t)kGrayWgPerCu * cus;
    return (int)std::min<int64_t>(std::max<int64_t>(1, (tiles + want - 1) / want), 1 << 20);
}

// the rectangles of a histogram call, each under the comparison rectangle's rules
int gray_rects(fpm_ctx* ctx, const fpm_patch_rect* rects, int32_t n_rects, std::vector<fpm_patch_rect>& out) {
    if (n_rects < 1 || n_rects > FPM_GRAY_MAX_RECTS || (!rects && n_rects != 1)) {
        ctx->err = "1 .. 64 rectangles expected (NULL with one: the whole template)";
        return FPM_E_INVALID_ARG;
    }
    out.resize((size_t)n_rects);
    for (int k = 0; k < n_rects; ++k) {
        const int rc = compare_rect(ctx, rects ? rects + k : nullptr, &out[(size_t)k]);
        if (rc != FPM_OK) return rc;
    }
    return FPM_OK;
}

struct GrayCall {
    int njobs = 0, run = 1, grid = 0;
    size_t tab = 0;          // bytes of the job table
    int64_t px = 0;          // pixels of all jobs
};

// The GrayJob table of poses x rects ([pose][rect]) in the pinned patch table, every pose checked; nothing is sent.
// Job j's histogram is words 256 j .., its e image (one rectangle) patch_stride bytes behind the one before.  outside
// (optional, [njobs]): FPM_GRAY_OUTSIDE or 0 by the calipers' four-corner rule.
int gray_jobs(fpm_ctx* ctx, const std::vector<fpm_patch_rect>& rects, const std::vector<PatchPose>& poses,
              size_t patch_stride, int t, int polarity, GrayCall* g, std::vector<int32_t>* outside) {
    const int K = (int)rects.size();
    g->njobs = (int)poses.size() * K;
    g->tab = round_up(sizeof(GrayJob) * (size_t)g->njobs, (size_t)256);
    GrayJob* jobs = nullptr;
    int rc = tab_begin(ctx, g->tab, &jobs);
    if (rc != FPM_OK) return rc;
    int64_t tiles = 0;
    g->px = 0;
    for (const fpm_patch_rect& r : rects) {
        tiles += (int64_t)poses.size() * ((r.w + 63) / 64) * ((r.h + 15) / 16);
        g->px += (int64_t)poses.size() * r.w * r.h;
    }
    g->run = gray_run_for(ctx, tiles);
    if (outside) outside->assign((size_t)g->njobs, 0);
    int64_t wg = 0;
    for (int i = 0, j = 0; i < (int)poses.size(); ++i)
        for (int k = 0; k < K; ++k, ++j) {
            const fpm_patch_rect& r = rects[(size_t)k];
            GrayJob& job = jobs[j];
            rc = tab_head(ctx, job.p, r, poses[(size_t)i], i, (int64_t)((size_t)j * patch_stride));
            if (rc != FPM_OK) return rc;
            job.pw = r.w; job.ph = r.h; job.rx = r.x; job.ry = r.y;
            job.hist_off = (int64_t)j * 256;
            job.wg0 = (int32_t)wg;
            job.t = t; job.polarity = polarity; job.pad = 0;
            const int64_t jt = (int64_t)((r.w + 63) / 64) * ((r.h + 15) / 16);
            wg += (jt + g->run - 1) / g->run;
            if (wg > INT_MAX) { ctx->err = "too many patch tiles for one launch"; return FPM_E_INVALID_ARG; }
            if (outside && corners_outside(ctx, job.p.M, r.w, r.h)) (*outside)[(size_t)j] = FPM_GRAY_OUTSIDE;   // border zeros
        }
    g->grid = (int)wg;
    return FPM_OK;
}

GrayArgs gray_args(fpm_ctx* ctx, const GrayCall& g) {
    GrayArgs a = source_args<GrayArgs>(ctx, g.njobs);
    a.mask = mask_plane(ctx);
    a.mkp = ctx->tmpl[0].pitch;
    a.run = g.run;
    a.grid = g.grid;
    return a;
}

// The histograms of a staged job table into h_gray: d_gray cleared on the stream, one launch of k_patch_hist, the words
// to pinned memory, the stream synchronised, then every histogram checked against its job's used count (used: one per
// rectangle).  d_gray and h_gray are sized by the caller.
int gray_hist_run(fpm_ctx* ctx, const GrayCall& g, const std::vector<int64_t>& used) {
    const size_t hb = sizeof(uint32_t) * 256 * (size_t)g.njobs;
    HIP_TRY(hipMemsetAsync(ctx->d_gray.p, 0, hb, ctx->stream));
    GrayArgs a = gray_args(ctx, g);
    a.hist = ctx->d_gray.as<uint32_t>();
    {
        // bytes: source pixels read (+ mask bytes read) + the histogram words
        ProfScope ps(ctx, kProfGrayHist, (1 + (a.mask ? 1 : 0)) * g.px + (int64_t)hb);
        if (!launch_patch_hist(a, ctx->stream)) { ctx->err = "bad histogram launch"; return FPM_E_INTERNAL; }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_gray.p, ctx->d_gray.p, hb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    const uint32_t* h = ctx->h_gray.as<uint32_t>();
    const size_t K = used.size();
    for (int j = 0; j < g.njobs; ++j) {   // what the device wrote is checked before anything of it reaches the caller
        int64_t s = 0;
        for (int b = 0; b < 256; ++b) s += (int64_t)h[(size_t)j * 256 + b];
        if (s != used[(size_t)j % K]) { ctx->err = "k_patch_hist returned a histogram that misses its pixel count"; return FPM_E_INTERNAL; }
    }
    return FPM_OK;
}

// The histograms of poses x rects (both non-empty), every argument checked before the one launch; caller memory is
// written only after the device pass has succeeded.
int gray_to_host(fpm_ctx* ctx, const std::vector<fpm_patch_rect>& rects, const std::vector<PatchPose>& poses, uint32_t* hist) {
    GrayCall g;
    int rc = gray_jobs(ctx, rects, poses, 0, 0, 0, &g, nullptr);
    if (rc != FPM_OK) return rc;
    const size_t hb = sizeof(uint32_t) * 256 * (size_t)g.njobs;
    HIP_TRY(ctx->d_gray.ensure(hb));
    HIP_TRY(ctx->h_gray.ensure(hb));
    std::vector<int64_t> used(rects.size());
    for (size_t k = 0; k < rects.size(); ++k) used[k] = mask_used(ctx, rects[k]);
    rc = tab_send(ctx, g.tab);
    if (rc == FPM_OK) rc = gray_hist_run(ctx, g, used);
    if (rc != FPM_OK) return rc;
    std::memcpy(hist, ctx->h_gray.p, hb);
    return FPM_OK;
}

// The segmentation of `poses` (n >= 1) inside r: with a fixed threshold one launch of k_patch_threshold into the pitched
// patch buffer and the labelling of those images; under FPM_SEG_OTSU the histogram launch, one copy to the host,
// hist_derive per hit and the thresholds into the job table come first.  blobs_reserve comes before the first launch.
int segment_of_poses(fpm_ctx* ctx, const fpm_patch_rect& r, const std::vector<PatchPose>& poses, int threshold, int polarity,
                     int connectivity, int min_area, int cap_per_hit, fpm_segment_info* info, fpm_blob_summary* summary,
                     fpm_blob* out, uint8_t* img, size_t row_stride, size_t patch_stride) {
    const int n = (int)poses.size();
    const bool otsu = threshold == FPM_SEG_OTSU;
    BlobRun b;
    int rc = blobs_reserve(ctx, n, r.w, r.h, min_area, cap_per_hit, false, &b);
    if (rc != FPM_OK) return rc;
    const size_t pitch = round_up((size_t)r.w, (size_t)64), pbytes = pitch * (size_t)r.h;
    HIP_TRY(ctx->d_patch.ensure(pbytes * (size_t)n));
    if (otsu) {
        HIP_TRY(ctx->d_gray.ensure(sizeof(uint32_t) * 256 * (size_t)n));
        HIP_TRY(ctx->h_gray.ensure(sizeof(uint32_t) * 256 * (size_t)n));
    }
    GrayCall g;
    std::vector<int32_t> flags;
    rc = gray_jobs(ctx, {r}, poses, pbytes, otsu ? 0 : threshold, polarity, &g, &flags);
    if (rc == FPM_OK) rc = tab_send(ctx, g.tab);
    if (rc != FPM_OK) return rc;
    const int64_t used = mask_used(ctx, r);
    std::vector<int32_t> ts((size_t)n, threshold);
    if (otsu) {
        rc = gray_hist_run(ctx, g, {used});
        if (rc != FPM_OK) return rc;
        // the stream is idle: the table has left the pinned buffer, which takes the thresholds and goes again
        GrayJob* jobs = ctx->h_patchtab.as<GrayJob>();
        for (int i = 0; i < n; ++i) {
            fpm_hist_stats s;
            if (!hist_derive(ctx->h_gray.as<uint32_t>() + (size_t)i * 256, &s)) { ctx->err = "histogram beyond 2^22 pixels"; return FPM_E_INTERNAL; }
            ts[(size_t)i] = polarity > 0 ? s.otsu : s.otsu + 1;
            flags[(size_t)i] |= s.flags;
            jobs[i].t = ts[(size_t)i];
            jobs[i].polarity = s.flags ? 0 : polarity;   // empty or flat: no foreground
        }
        rc = tab_send(ctx, g.tab);
        if (rc != FPM_OK) return rc;
    }
    GrayArgs a = gray_args(ctx, g);
    a.out = ctx->d_patch.as<uint8_t>();
    a.row_stride = pitch;
    a.pw = r.w; a.ph = r.h;
    a.dword = 1;   // the buffer's base, the pitch and every image offset are multiples of 64
    {
        // bytes: source pixels read (+ mask bytes read) + e pixels written
        ProfScope ps(ctx, kProfGrayThreshold, (2 + (a.mask ? 1 : 0)) * g.px);
        if (!launch_patch_threshold(a, ctx->stream)) { ctx->err = "too many patch tiles for one launch"; return FPM_E_INVALID_ARG; }
    }
    HIP_TRY(hipGetLastError());
    if (img) {
        rc = copy_patches_out(ctx, r, (size_t)n, a.out, pitch, pbytes, img, row_stride, patch_stride);
        if (rc != FPM_OK) return rc;
    }
    rc = blobs_run(ctx, b, a.out, pitch, pbytes, 0, connectivity, min_area, cap_per_hit, summary, out, nullptr);
    if (rc != FPM_OK) return rc;
    for (int i = 0; i < n; ++i) info[i] = fpm_segment_info{used, ts[(size_t)i], flags[(size_t)i]};
    return FPM_OK;
}

// ---- sub-pattern locators (fpm_last_locate, fpm_locate_at) ----
static_assert(sizeof(fpm_feature) == 32 && sizeof(fpm_locate_raw) == 160 && sizeof(fpm_locate_result) == 80,
              "the locator structs have no padding");
static_assert(sizeof(fpm_locate_raw) == sizeof(int32_t) * kLocateWords, "k_patch_locate writes the record as dwords");
static_assert(sizeof(LocateJob) % 8 == 0, "a table of LocateJob keeps its doubles aligned");
static_assert(kLocateMaxSide == FPM_LOCATE_MAX_SIDE && kLocateMaxRadius == FPM_LOCATE_MAX_RADIUS, "one set of caps");

// the rules of a call's features that do not depend on the number of hits; *max_off = the largest offset count
int locate_args(fpm_ctx* ctx, const fpm_feature* feats, int32_t n_feats, const int32_t* maps, int32_t map_stride, int* max_off) {
    if (!feats || n_feats < 1 || n_feats > FPM_LOCATE_MAX_FEATURES) { ctx->err = "1 .. 64 features expected"; return FPM_E_INVALID_ARG; }
    const int tw = ctx->tmpl[0].w, th = ctx->tmpl[0].h;
    *max_off = 0;
    for (int k = 0; k < n_feats; ++k) {
        const fpm_feature& f = feats[k];
        if (const char* bad = feature_bad(f)) { ctx->err = bad; return FPM_E_INVALID_ARG; }
        if (f.x < 0 || f.y < 0 || f.w > tw - f.x || f.h > th - f.y) {
            ctx->err = "feature: the rectangle must lie inside the template";
            return FPM_E_INVALID_ARG;
        }
        *max_off = std::max(*max_off, (2 * f.rx + 1) * (2 * f.ry + 1));
    }
    if (maps && map_stride < *max_off) { ctx->err = "map_stride below the largest (2 rx + 1)(2 ry + 1)"; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

// Row bands of one offset's S_it (LocateJob::bands): the count, up to 16, that leaves the 256 lanes the fewest rows to
// walk, rounds x rows per band; the smallest such count.  Speed only: the sums are integers.
int locate_bands(int noff, int h) {
    int best = 1;
    int64_t cost = INT64_MAX;
    for (int nb = 1; nb <= std::min(h, 16); ++nb) {
        const int64_t c = (int64_t)((noff * nb + 255) / 256) * ((h + nb - 1) / nb);
        if (c < cost) { cost = c; best = nb; }
    }
    return best;
}

// The features of `poses` (n >= 1), every argument checked: the job table, one launch of k_patch_locate, the raw records
// and maps to pinned memory, the records checked, then the derivation into the caller's buffers.  Caller memory is
// written only after the device pass has succeeded.
int locate_to_host(fpm_ctx* ctx, const std::vector<PatchPose>& poses, const fpm_feature* feats, int n_feats, int max_off,
                   fpm_locate_result* results, fpm_locate_raw* raw, int32_t* maps, int32_t map_stride) {
    const int njobs = (int)poses.size() * n_feats;
    const TmplLevel& t0 = ctx->tmpl[0];
    const size_t tab = round_up(sizeof(LocateJob) * (size_t)njobs, (size_t)256);
    LocateJob* jobs = nullptr;
    int rc = tab_begin(ctx, tab, &jobs);
    if (rc != FPM_OK) return rc;
    // the device output: records, then the maps at the largest offset count (the caller's stride is the host's)
    const size_t rec_b = sizeof(fpm_locate_raw) * (size_t)njobs;
    const size_t map_b = maps ? sizeof(int32_t) * 3 * (size_t)max_off * (size_t)njobs : 0;
    HIP_TRY(ctx->d_locout.ensure(rec_b + map_b));
    HIP_TRY(ctx->h_locout.ensure(rec_b + map_b));
    std::vector<int32_t> outside((size_t)njobs, 0);
    int64_t bytes = (int64_t)(rec_b + map_b);
    for (int i = 0, j = 0; i < (int)poses.size(); ++i)
        for (int k = 0; k < n_feats; ++k, ++j) {
            const fpm_feature& f = feats[k];
            const fpm_patch_rect r{f.x - f.rx, f.y - f.ry, f.w + 2 * f.rx, f.h + 2 * f.ry};   // the window
            LocateJob& job = jobs[j];
            rc = tab_head(ctx, job.p, r, poses[(size_t)i], i, 0);
            if (rc != FPM_OK) return rc;
            job.x = f.x; job.y = f.y; job.w = f.w; job.h = f.h; job.rx = f.rx; job.ry = f.ry;
            job.bands = locate_bands((2 * f.rx + 1) * (2 * f.ry + 1), f.h);
            job.pad = 0;
            bytes += (int64_t)r.w * r.h + (int64_t)f.w * f.h;
            outside[(size_t)j] = corners_outside(ctx, job.p.M, r.w, r.h) ? FPM_LOCATE_OUTSIDE : 0;   // border zeros in the window
        }
    rc = tab_send(ctx, tab);
    if (rc != FPM_OK) return rc;
    LocateArgs a = source_args<LocateArgs>(ctx, njobs);
    a.tmpl = ctx->d_tmpl.as<uint8_t>() + t0.off;
    a.tp = t0.pitch;
    a.raw = ctx->d_locout.as<int32_t>();
    a.maps = maps ? ctx->d_locout.as<int32_t>(rec_b) : nullptr;
    a.map_stride = max_off;
    {
        ProfScope ps(ctx, kProfLocate, bytes);   // window pixels sampled + template pixels read + records and maps written
        if (!launch_patch_locate(a, ctx->stream)) { ctx->err = "bad locate launch"; return FPM_E_INTERNAL; }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_locout.p, ctx->d_locout.p, rec_b + map_b, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    fpm_locate_raw* hr = ctx->h_locout.as<fpm_locate_raw>();
    std::vector<fpm_locate_result> res((size_t)njobs);
    for (int j = 0; j < njobs; ++j) {   // what the device wrote is checked before anything of it reaches the caller
        const RawPose& p = poses[(size_t)(j / n_feats)].pose;
        if (hr[j].flags != 0 || hr[j].reserved != 0) { ctx->err = "k_patch_locate returned a record with flags"; return FPM_E_INTERNAL; }
        hr[j].flags = outside[(size_t)j];
        if (!locate_derive(feats[j % n_feats], p.x, p.y, p.angle, hr[j], &res[(size_t)j])) {
            ctx->err = "k_patch_locate returned a record that is no peak of its feature";
            return FPM_E_INTERNAL;
        }
    }
    std::memcpy(results, res.data(), sizeof(fpm_locate_result) * (size_t)njobs);
    if (raw) std::memcpy(raw, hr, rec_b);
    if (maps) {
        const int32_t* hm = ctx->h_locout.as<int32_t>(rec_b);
        for (size_t q = 0; q < (size_t)njobs * 3; ++q) {
            int32_t* mq = maps + q * (size_t)map_stride;
            std::memcpy(mq, hm + q * (size_t)max_off, sizeof(int32_t) * (size_t)max_off);
            if (map_stride > max_off) std::memset(mq + max_off, 0, sizeof(int32_t) * (size_t)(map_stride - max_off));
        }
    }
    return FPM_OK;
}

// ---- edge probes (fpm_last_probes, fpm_probes_at) ----
static_assert(sizeof(fpm_probe) == 24 && sizeof(fpm_probe_params) == 32 && sizeof(fpm_probe_raw) == 24 &&
              sizeof(fpm_probe_result) == 64 && sizeof(fpm_probe_summary) == 64, "the probe structs have no padding");
static_assert(sizeof(ProbeRaw) == sizeof(fpm_probe_raw) && sizeof(ProbeFrame) == 32 && sizeof(PatchJob) == 64,
              "the kernel's record is fpm_probe_raw, field for field; the job table is 64 hits + 32 n_probes bytes");
static_assert(kProbeMaxLength == FPM_PROBE_MAX_LENGTH && kProbeMaxWidth == FPM_PROBE_MAX_WIDTH &&
              kProbeMaxHalf == FPM_PROBE_MAX_HALF && kProbeMax == FPM_PROBE_MAX && kProbeOutside == FPM_PROBE_OUTSIDE &&
              kProbeNearest == FPM_PROBE_NEAREST && kProbeLast == FPM_PROBE_LAST, "one set of caps and codes");

// the rules of a call's probes and parameters that do not depend on the number of hits
int probe_args(fpm_ctx* ctx, const fpm_probe* probes, int32_t n_probes, const fpm_probe_params* params) {
    if (!probes || n_probes < 1 || n_probes > FPM_PROBE_MAX) { ctx->err = "1 .. 4096 probes expected"; return FPM_E_INVALID_ARG; }
    if (!params) { ctx->err = "null probe parameters"; return FPM_E_INVALID_ARG; }
    if (const char* bad = probe_params_bad(*params)) { ctx->err = bad; return FPM_E_INVALID_ARG; }
    for (int k = 0; k < n_probes; ++k)
        if (const char* bad = probe_bad(probes[k])) { ctx->err = bad; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

// and those that do: the outputs and the slots
int probe_outputs(fpm_ctx* ctx, size_t hits, int32_t n_probes, const fpm_probe_params& p, const fpm_probe_summary* summary,
                  const fpm_probe_result* results, const int32_t* profiles, int32_t stride) {
    if (!summary || !results) { ctx->err = "null summary or result buffer"; return FPM_E_INVALID_ARG; }
    if ((int64_t)hits * n_probes > FPM_PROBE_MAX_SLOTS) { ctx->err = "hits x probes above 2^22"; return FPM_E_INVALID_ARG; }
    if (profiles && stride < p.length) { ctx->err = "profile_stride below the length"; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

// The probes of `poses` (n >= 1), every argument checked: the job table -- one head per hit, then one frame per probe,
// in the same pinned buffer -- one launch of k_probe, the raw records and profiles to pinned memory, every record
// checked by probe_derive, then results, summaries and profiles into the caller's buffers.  Caller memory is written
// only after the device pass has succeeded.  The host's work per (hit, probe) is the derivation of its one record.
int probes_to_host(fpm_ctx* ctx, const std::vector<PatchPose>& poses, const fpm_probe* probes, int n_probes,
                   const fpm_probe_params& prm, fpm_probe_summary* summary, fpm_probe_result* results, int32_t* profiles,
                   int32_t stride) {
    const int hits = (int)poses.size(), L = prm.length, W = prm.width;
    const size_t njobs = (size_t)hits * (size_t)n_probes;
    const size_t heads_b = sizeof(PatchJob) * (size_t)hits;
    const size_t tab = round_up(heads_b + sizeof(ProbeFrame) * (size_t)n_probes, (size_t)256);
    uint8_t* base = nullptr;
    int rc = tab_begin(ctx, tab, &base);
    if (rc != FPM_OK) return rc;
    PatchJob* heads = (PatchJob*)base;
    ProbeFrame* frames = (ProbeFrame*)(base + heads_b);
    // the frames, and the box of every probe's sample grid in template coordinates
    std::vector<ProbeGeom> geom((size_t)n_probes);
    double bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
    for (int k = 0; k < n_probes; ++k) {
        const ProbeGeom g = probe_geom(probes[k], prm);
        geom[(size_t)k] = g;
        frames[k] = ProbeFrame{g.cp, g.sp, g.ox, g.oy};
        for (int e = 0; e < 4; ++e) {
            const double u = (e & 1) ? L - 1 : 0, v = (e & 2) ? W - 1 : 0;
            const double x = g.ox + (u * g.cp - v * g.sp), y = g.oy + (u * g.sp + v * g.cp);
            if (k == 0 && e == 0) { bx0 = bx1 = x; by0 = by1 = y; }
            bx0 = std::min(bx0, x); bx1 = std::max(bx1, x);
            by0 = std::min(by0, y); by1 = std::max(by1, y);
        }
    }
    const fpm_patch_rect origin{0, 0, 1, 1};
    for (int i = 0; i < hits; ++i) {
        rc = tab_head(ctx, heads[i], origin, poses[(size_t)i], i, (int64_t)i * n_probes);
        if (rc != FPM_OK) return rc;
        const double* M = heads[i].M;
        for (int e = 0; e < 4; ++e) {   // the samplers' 2^20 range: the box's corners bound every sample of every probe
            const double x = (e & 1) ? bx1 : bx0, y = (e & 2) ? by1 : by0;
            const double sx = M[0] * x + M[1] * y + M[2], sy = M[3] * x + M[4] * y + M[5];
            if (!(std::fabs(sx) < 1048576.0 && std::fabs(sy) < 1048576.0)) {
                ctx->err = "pose " + std::to_string(i) + ": farther than 2^20 pixels from the source";
                return FPM_E_INVALID_ARG;
            }
        }
    }
    // the device output: records, then the profiles at stride L (the caller's stride is the host's)
    const size_t rec_b = round_up(sizeof(fpm_probe_raw) * njobs, (size_t)16);
    const size_t prof_b = profiles ? sizeof(int32_t) * njobs * (size_t)L : 0;
    HIP_TRY(ctx->d_probeout.ensure(rec_b + prof_b));
    HIP_TRY(ctx->h_probeout.ensure(rec_b + prof_b));
    rc = tab_send(ctx, tab);
    if (rc != FPM_OK) return rc;
    ProbeArgs a = source_args<ProbeArgs>(ctx, hits);
    a.frames = (const ProbeFrame*)(ctx->d_patchtab.as<uint8_t>() + heads_b);
    a.n_probes = n_probes;
    a.L = L; a.W = W; a.s = prm.half;
    a.thr = prm.contrast * prm.half * prm.width;
    a.polarity = prm.polarity;
    a.select = prm.select;
    a.records = ctx->d_probeout.as<ProbeRaw>();
    a.profiles = profiles ? ctx->d_probeout.as<int32_t>(rec_b) : nullptr;
    {
        // L W source pixels per (hit, probe) + the job table + the records and profiles written
        ProfScope ps(ctx, kProfProbe, (int64_t)njobs * L * W + (int64_t)tab + (int64_t)(rec_b + prof_b));
        if (!launch_probe(a, ctx->stream)) { ctx->err = "bad probe launch"; return FPM_E_INTERNAL; }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_probeout.p, ctx->d_probeout.p, rec_b + prof_b, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    const fpm_probe_raw* raw = ctx->h_probeout.as<fpm_probe_raw>();
    std::vector<fpm_probe_result> res(njobs);
    for (int i = 0; i < hits; ++i) {   // what the device wrote is checked before anything of it reaches the caller
        const RawPose& p = poses[(size_t)i].pose;
        const double rad = p.angle * kD2R, ca = std::cos(rad), sa = std::sin(rad);
        for (int k = 0; k < n_probes; ++k) {
            const size_t j = (size_t)i * n_probes + k;
            if ((raw[j].flags & ~FPM_PROBE_OUTSIDE) != 0 ||
                !probe_derive(geom[(size_t)k], prm, p.x, p.y, ca, sa, raw[j], &res[j])) {
                ctx->err = "k_probe returned a record that is no edge";
                return FPM_E_INTERNAL;
            }
        }
    }
    std::memcpy(results, res.data(), sizeof(fpm_probe_result) * njobs);
    for (int i = 0; i < hits; ++i) {
        const RawPose& p = poses[(size_t)i].pose;
        probe_summarise(res.data() + (size_t)i * n_probes, n_probes, p.x, p.y, p.angle, summary + i);
    }
    if (profiles) {
        const int32_t* prof = ctx->h_probeout.as<int32_t>(rec_b);
        for (size_t j = 0; j < njobs; ++j) {
            int32_t* pj = profiles + j * (size_t)stride;
            std::memcpy(pj, prof + j * (size_t)L, sizeof(int32_t) * (size_t)L);
            if (stride > L) std::memset(pj + L, 0, sizeof(int32_t) * (size_t)(stride - L));
        }
    }
    return FPM_OK;
}

// fpm_model_learn after its checks: the mean image written into level 0 of the template slab by k_model_prepare, then
// the device learn's second half
int learn_from_model(fpm_ctx* ctx) {
    const fpm_patch_rect r = ctx->model_rect;
    std::vector<TmplLevel> lv;
    int rc = learn_begin(ctx, r.w, r.h, lv);
    if (rc != FPM_OK) return rc;
    const size_t px = (size_t)r.w * r.h;
    ModelPrepareArgs p{};
    p.sum = ctx->d_model.as<uint32_t>();
    p.sum_sq = p.sum + px;
    p.w = r.w; p.h = r.h; p.n = ctx->model_n;
    p.mean = ctx->d_tmpl.as<uint8_t>() + lv[0].off;
    p.pitch = lv[0].pitch;
    {
        ProfScope ps(ctx, kProfModelPrepare, (int64_t)px * (2 * (int64_t)sizeof(uint32_t) + 1));
        launch_model_prepare(p, ctx->stream);
    }
    HIP_TRY(hipGetLastError());
    return learn_finish(ctx, lv);
}

}  // namespace

// =========================================================================================================
// C ABI
// =========================================================================================================
extern "C" {

void fpm_params_default(fpm_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->max_pos = 70;            // TemplateMatcher.cpp:29
    p->max_overlap = 0.0;       // :30
    p->score = 0.7;             // :31
    p->tolerance_angle = 0.0;   // :32
    p->min_reduce_area = 256;   // :33
    p->use_simd = 1;            // :34
    p->subpixel = 0;            // :35
    p->tolerance_range = 0;     // :38
    p->semantics = FPM_SEMANTICS_QT;
    p->top_angle_step = 0.0;    // extension: the reference's derived step
    p->stop_layer = 0;          // m_bStopLayer1 off (MatchToolDlg.cpp:936)
    p->bitwise_not = 0;         // m_ckBitwiseNot off (MatchToolDlg.cpp:788)
}

int fpm_abi_version(void) { return FPM_ABI_VERSION; }

int fpm_create(int device, fpm_ctx** out) {
    if (!out) return FPM_E_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return FPM_E_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return FPM_E_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FPM_E_DEVICE;
    fpm_ctx* ctx = new (std::nothrow) fpm_ctx();
    if (!ctx) return FPM_E_INTERNAL;
    ctx->device = device;
    fpm_params_default(&ctx->prm);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return FPM_E_DEVICE;
    }
    *out = ctx;
    return FPM_OK;
}

int fpm_destroy(fpm_ctx* ctx) {
    if (!ctx) return FPM_E_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->graph) (void)hipGraphExecDestroy(ctx->graph);
    for (hipEvent_t e : ctx->t_ev)
        if (e) (void)hipEventDestroy(e);
    ctx->plan.release();
    ctx->d_tmpl.release(); ctx->d_tmpl8.release(); ctx->d_tsum.release(); ctx->d_src.release();
    ctx->d_op_a.release(); ctx->d_op_b.release(); ctx->d_op_job.release();
    for (DevBuf* b : {&ctx->d_rf_tab, &ctx->d_rf_tdesc, &ctx->d_rf_roi, &ctx->d_rf_rowsum, &ctx->d_rf_wtot, &ctx->d_rf_wtotq, &ctx->d_rf_wedge})
        b->release();
    ctx->d_ov.release(); ctx->h_ov_in.release(); ctx->h_ov_out.release();
    ctx->d_imgtab.release(); ctx->h_imgtab.release();
    if (ctx->in_ev) (void)hipEventDestroy(ctx->in_ev);
    ctx->d_patchtab.release(); ctx->h_patchtab.release(); ctx->d_patch.release();
    ctx->d_cmpacc.release(); ctx->h_cmpacc.release();
    ctx->d_tacc.release(); ctx->h_tacc.release();
    ctx->d_model.release(); ctx->d_band.release(); ctx->d_insacc.release(); ctx->h_insacc.release();
    ctx->d_alnacc.release(); ctx->h_alnacc.release();
    ctx->d_blobplanes.release(); ctx->d_blobrec.release(); ctx->d_blobimg.release();
    ctx->h_blobrec.release(); ctx->h_bloblab.release();
    ctx->d_calout.release(); ctx->h_calout.release();
    ctx->d_gray.release(); ctx->h_gray.release();
    ctx->d_locout.release(); ctx->h_locout.release();
    ctx->d_probeout.release(); ctx->h_probeout.release();
    ctx->d_mask.release(); ctx->d_mask_in.release();
    for (hipEvent_t e : {ctx->tab_ev, ctx->out_ev})
        if (e) (void)hipEventDestroy(e);
    for (auto& k : ctx->kp)
        for (auto& e : k.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return FPM_OK;
}

const char* fpm_last_error(const fpm_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int fpm_set_params(fpm_ctx* ctx, const fpm_params* p) {
    if (!ctx || !p) return FPM_E_INVALID_ARG;
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    ctx->prm = *p;
    return FPM_OK;
}

int fpm_get_params(const fpm_ctx* ctx, fpm_params* p) {
    if (!ctx || !p) return FPM_E_INVALID_ARG;
    *p = ctx->prm;
    return FPM_OK;
}

// TemplateMatcher::learnPattern (TemplateMatcher.cpp:45-95)
int fpm_learn(fpm_ctx* ctx, const uint8_t* gray, int32_t w, int32_t h, size_t stride) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!gray || w <= 0 || h <= 0 || stride < (size_t)w) { ctx->err = "empty template"; return FPM_E_INVALID_ARG; }
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->learned = false;
    ctx->staged = false;
    ctx->src_valid = false;   // the slab's layout follows the template's pyramid depth
    ctx->model_n = 0;         // the variation model belongs to the template before
    mask_drop(ctx);           // and so does the mask
    ctx->tmpl.clear();
    const int L = top_layer(w, h, (int)std::sqrt((double)ctx->prm.min_reduce_area));
    std::vector<TmplLevel> lv(L + 1);
    size_t off = 0;
    int lw = w, lh = h;
    for (int l = 0; l <= L; ++l) {
        lv[l].w = lw; lv[l].h = lh;
        lv[l].pitch = round_up(lw + 4, 64);
        lv[l].off = off;
        off += round_up((size_t)lv[l].pitch * (lh + 1), (size_t)256);
        lw = (lw + 1) / 2;
        lh = (lh + 1) / 2;
    }
    HIP_TRY(ctx->d_tmpl.ensure(off));
    uint8_t* base = ctx->d_tmpl.as<uint8_t>();
    HIP_TRY(hipMemsetAsync(base, 0, off, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(base + lv[0].off, lv[0].pitch, gray, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
    for (int l = 1; l <= L; ++l)   // cv::buildPyramid (:55) on the device
        launch_pyr_down(base + lv[l - 1].off, lv[l - 1].w, lv[l - 1].h, lv[l - 1].pitch, 0, base + lv[l].off, lv[l].w,
                        lv[l].h, lv[l].pitch, 0, 1, ctx->stream);
    HIP_TRY(hipGetLastError());
    for (int l = 0; l <= L; ++l) {
        lv[l].px.resize((size_t)lv[l].w * lv[l].h);
        HIP_TRY(hipMemcpy2DAsync(lv[l].px.data(), lv[l].w, base + lv[l].off, lv[l].pitch, lv[l].w, lv[l].h,
                                 hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    double m0, s0;
    mean_stddev(lv[0].px, &m0, &s0);
    ctx->border = m0 < 128 ? 255 : 0;   // :58-59
    for (int l = 0; l <= L; ++l) {      // :66-91
        const double inv_area = 1.0 / ((double)lv[l].h * lv[l].w);
        double mean, sdv;
        mean_stddev(lv[l].px, &mean, &sdv);
        double norm = sdv * sdv;
        lv[l].equal1 = norm < DBL_EPSILON;
        norm = std::sqrt(norm);
        norm /= std::sqrt(inv_area);
        lv[l].mean = mean; lv[l].norm = norm; lv[l].inv_area = inv_area;
    }
    {   // MFMA operand copies: T ^ 0x80 (= T - 128 as i8), zero beyond the template; per-row sums of T
        size_t o8 = 0, os = 0;
        for (int l = 0; l <= L; ++l) {
            lv[l].p8 = 64 * ((lv[l].w + 63) / 64);
            lv[l].off8 = o8;
            o8 += (size_t)lv[l].p8 * round_up(lv[l].h, kMmaRows);
            lv[l].tsum_off = os;
            os += round_up(lv[l].h, kMmaRows);
        }
        o8 += 256;   // slack: k_roi_corr prefetches up to 2 64-byte blocks past a row's last
        std::vector<int8_t> h8(o8, 0);
        std::vector<int32_t> hs(os, 0);
        for (int l = 0; l <= L; ++l)
            for (int y = 0; y < lv[l].h; ++y) {
                int32_t sum = 0;
                for (int x = 0; x < lv[l].w; ++x) {
                    const uint8_t v = lv[l].px[(size_t)y * lv[l].w + x];
                    h8[lv[l].off8 + (size_t)y * lv[l].p8 + x] = (int8_t)(v ^ 0x80);
                    sum += v;
                }
                hs[lv[l].tsum_off + y] = sum;
            }
        HIP_TRY(ctx->d_tmpl8.ensure(o8));
        HIP_TRY(ctx->d_tsum.ensure(os * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(ctx->d_tmpl8.p, h8.data(), o8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ctx->d_tsum.p, hs.data(), os * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    ctx->tmpl = std::move(lv);
    ctx->learned = true;
    ctx->tmpl_gen++;
    return FPM_OK;
}

int fpm_clear_pattern(fpm_ctx* ctx) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    ctx->learned = false;
    ctx->staged = false;
    ctx->src_valid = false;
    ctx->tmpl.clear();
    ctx->tmpl_gen++;
    ctx->model_n = 0;
    mask_drop(ctx);
    return FPM_OK;
}

int fpm_is_learned(const fpm_ctx* ctx) { return ctx && ctx->learned ? 1 : 0; }

int fpm_stage_sources(fpm_ctx* ctx, const uint8_t* const* grays, int32_t count, int32_t w, int32_t h, size_t stride) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!grays || count <= 0 || w <= 0 || h <= 0 || stride < (size_t)w) { ctx->err = "bad sources"; return FPM_E_INVALID_ARG; }
    for (int i = 0; i < count; ++i)
        if (!grays[i]) { ctx->err = "null source"; return FPM_E_INVALID_ARG; }
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    int rc = check_sizes(ctx, w, h);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->staged = false;
    rc = upload_sources(ctx, grays, count, w, h, stride);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->staged = true;
    return FPM_OK;
}

static int copy_results(const std::vector<std::vector<fpm_result>>& res, fpm_result* out, int32_t cap,
                        int32_t* n_results) {
    int status = FPM_OK;
    for (size_t s = 0; s < res.size(); ++s) {
        n_results[s] = (int32_t)res[s].size();
        for (int i = 0; i < (int)res[s].size(); ++i) {
            if (i < cap && out) out[s * (size_t)cap + i] = res[s][i];
            else status = FPM_E_CAPACITY;
        }
    }
    return status;
}

int fpm_match_staged_launch(fpm_ctx* ctx) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!ctx->learned) { ctx->err = "template not learned"; return FPM_E_NOT_LEARNED; }
    if (ctx->S <= 0 || !ctx->staged) { ctx->err = "no staged sources (fpm_match replaces a staged batch)"; return FPM_E_INVALID_ARG; }
    if (ctx->pending) { ctx->err = "a search is already in flight"; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    return start_staged(ctx);
}

int fpm_match_staged_finish(fpm_ctx* ctx, fpm_result* out, int32_t cap, int32_t* n_results) {
    if (!ctx || !n_results) return FPM_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->results.clear();
    ctx->poses.clear();
    const int rc = complete_staged(ctx, ctx->results, out != nullptr);
    if (rc != FPM_OK) return rc;
    return copy_results(ctx->results, out, cap, n_results);
}

int fpm_match_staged(fpm_ctx* ctx, fpm_result* out, int32_t cap, int32_t* n_results) {
    if (!n_results) return FPM_E_INVALID_ARG;
    const int rc = fpm_match_staged_launch(ctx);
    if (rc != FPM_OK) return rc;
    return fpm_match_staged_finish(ctx, out, cap, n_results);
}

// TemplateMatcher::match (TemplateMatcher.cpp:97-437)
int fpm_match(fpm_ctx* ctx, const uint8_t* gray, int32_t w, int32_t h, size_t stride, fpm_result* out, int32_t cap,
              int32_t* n_results, double* seconds) {
    if (!ctx || !n_results) return FPM_E_INVALID_ARG;
    *n_results = 0;
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    // a failed call leaves no stale candidate records behind (fpm_last_candidates of a sharded search)
    ctx->cands.clear();
    ctx->stats.clear();
    ctx->results.clear();
    ctx->poses.clear();
    if (!gray || w <= 0 || h <= 0 || stride < (size_t)w) { ctx->err = "empty source"; return FPM_E_INVALID_ARG; }
    int rc = check_sizes(ctx, w, h);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->staged = false;   // the slab is re-laid out for this one source
    // the reference deep-copies the source before its clock starts (TemplateMatcher.cpp:104 then :117): the upload
    // is that copy, so getLastExecutionTime() starts once it has landed
    rc = upload_sources(ctx, &gray, 1, w, h, stride);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const auto t0 = std::chrono::high_resolution_clock::now();
    rc = run_staged(ctx, ctx->results);
    if (rc != FPM_OK) return rc;
    const auto t1 = std::chrono::high_resolution_clock::now();
    const std::vector<fpm_result>& r = ctx->results[0];
    *n_results = (int32_t)r.size();
    if (!r.empty() && seconds) *seconds = std::chrono::duration<double>(t1 - t0).count();
    for (int i = 0; i < (int)r.size() && i < cap && out; ++i) out[i] = r[i];
    return (int)r.size() > cap ? FPM_E_CAPACITY : FPM_OK;
}

// fpm_stage_sources for images already in device memory (no reference equivalent: match() takes a host cv::Mat,
// TemplateMatcher.cpp:97-104)
int fpm_stage_sources_device(fpm_ctx* ctx, const void* const* d_images, int32_t count, int32_t w, int32_t h,
                             size_t stride, size_t plane_stride, int32_t format, void* producer_stream) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!d_images) { ctx->err = "bad sources: null image table"; return FPM_E_INVALID_ARG; }
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    int rc = check_image_desc(ctx, count, w, h, stride, plane_stride, format);
    if (rc != FPM_OK) return rc;
    rc = check_sizes(ctx, w, h);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const bool was_staged = ctx->staged;
    ctx->staged = false;
    rc = stage_device_sources(ctx, d_images, count, w, h, stride, plane_stride, format, (hipStream_t)producer_stream);
    if (rc != FPM_OK) {
        if (rc == FPM_E_INVALID_ARG) ctx->staged = was_staged;   // rejected before the slab was touched
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->staged = true;
    return FPM_OK;
}

// fpm_match on an image already in device memory
int fpm_match_device(fpm_ctx* ctx, const void* d_image, int32_t w, int32_t h, size_t stride, size_t plane_stride,
                     int32_t format, void* producer_stream, fpm_result* out, int32_t cap, int32_t* n_results,
                     double* seconds) {
    if (!ctx || !n_results) return FPM_E_INVALID_ARG;
    *n_results = 0;
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    ctx->cands.clear();   // as fpm_match: a failed call leaves no stale records behind
    ctx->stats.clear();
    ctx->results.clear();
    ctx->poses.clear();
    if (!d_image) { ctx->err = "empty source"; return FPM_E_INVALID_ARG; }
    int rc = check_image_desc(ctx, 1, w, h, stride, plane_stride, format);
    if (rc != FPM_OK) return rc;
    rc = check_sizes(ctx, w, h);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const bool was_staged = ctx->staged;
    ctx->staged = false;   // the slab is re-laid out for this one source
    // the staging is the reference's deep copy of the source (TemplateMatcher.cpp:104), made before its clock starts
    // (:117), as fpm_match's upload is
    rc = stage_device_sources(ctx, &d_image, 1, w, h, stride, plane_stride, format, (hipStream_t)producer_stream);
    if (rc != FPM_OK) {
        if (rc == FPM_E_INVALID_ARG) ctx->staged = was_staged;
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const auto t0 = std::chrono::high_resolution_clock::now();
    rc = run_staged(ctx, ctx->results);
    if (rc != FPM_OK) return rc;
    const auto t1 = std::chrono::high_resolution_clock::now();
    const std::vector<fpm_result>& r = ctx->results[0];
    *n_results = (int32_t)r.size();
    if (!r.empty() && seconds) *seconds = std::chrono::duration<double>(t1 - t0).count();
    for (int i = 0; i < (int)r.size() && i < cap && out; ++i) out[i] = r[i];
    return (int)r.size() > cap ? FPM_E_CAPACITY : FPM_OK;
}

int fpm_last_results(const fpm_ctx* ctx, fpm_result* out, int32_t cap, int32_t* n_results) {
    if (!ctx || !n_results) return FPM_E_INVALID_ARG;
    if (ctx->pending) return FPM_E_INVALID_ARG;
    return copy_results(ctx->results, out, cap, n_results);
}

// --- match patches --------------------------------------------------------------------
int fpm_patch_matrix(int32_t src_w, int32_t src_h, float lt_x, float lt_y, double angle, int32_t rect_x, int32_t rect_y,
                     double m[6]) {
    if (!m || src_w <= 0 || src_h <= 0) return FPM_E_INVALID_ARG;
    const double rad = angle * kD2R;
    patch_matrix(src_w, src_h, f2(lt_x, lt_y), std::cos(rad), std::sin(rad), rect_x, rect_y, m);
    return FPM_OK;
}

int fpm_set_patch_form(fpm_ctx* ctx, int32_t form) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (form != FPM_PATCH_FORM_TILED && form != FPM_PATCH_FORM_WARP) { ctx->err = "unknown patch form"; return FPM_E_INVALID_ARG; }
    ctx->patch_form = form;
    return FPM_OK;
}

// One body per tool: query, state, rectangle or arguments, poses, outputs, run.  The public
// entries of a pair differ in their HitQuery alone unless a comment says otherwise.
static int patches_entry(fpm_ctx* ctx, const HitQuery& q, const fpm_patch_rect* rect, uint8_t* out, size_t row_stride,
                         size_t patch_stride, double* matrices) {
    int rc = q.check(ctx);
    if (rc != FPM_OK) return rc;
    fpm_patch_rect r;
    std::vector<PatchPose> poses;
    rc = hits_begin(ctx, q, patch_rect, rect, &r, poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    rc = check_patch_out(ctx, out, r, row_stride, patch_stride);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return patches_to_host(ctx, r, poses, out, row_stride, patch_stride, matrices);
}

int fpm_last_patches(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, uint8_t* out, size_t row_stride,
                     size_t patch_stride, int32_t cap, int32_t* n_patches, double* matrices) {
    return patches_entry(ctx, HitQuery::last(source, cap, n_patches), rect, out, row_stride, patch_stride, matrices);
}

int fpm_patches_at(fpm_ctx* ctx, const fpm_patch_rect* rect, const int32_t* src_index, const float* lt,
                   const double* angles, int32_t n, uint8_t* out, size_t row_stride, size_t patch_stride,
                   double* matrices) {
    return patches_entry(ctx, HitQuery::at(src_index, lt, angles, n), rect, out, row_stride, patch_stride, matrices);
}

// the device variant has no _at entry: one body, written out
int fpm_last_patches_device(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, void* d_out, size_t row_stride,
                            size_t patch_stride, int32_t cap, int32_t* n_patches, void* consumer_stream) {
    const HitQuery q = HitQuery::last(source, cap, n_patches);
    int rc = q.check(ctx);
    if (rc != FPM_OK) return rc;
    fpm_patch_rect r;
    std::vector<PatchPose> poses;
    rc = hits_begin(ctx, q, patch_rect, rect, &r, poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    rc = check_patch_out(ctx, d_out, r, row_stride, patch_stride);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t extent = (poses.size() - 1) * patch_stride + (size_t)(r.h - 1) * row_stride + (size_t)r.w;
    const void* outs[1] = {d_out};
    rc = check_device_images(ctx, outs, 1, extent, "patch output");
    if (rc != FPM_OK) return rc;
    hipStream_t consumer = (hipStream_t)consumer_stream;
    // after what the consumer's stream already holds for the buffer, then the launch, then the consumer after the launch
    if (!ctx->in_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->in_ev, hipEventDisableTiming));
    if (!ctx->out_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->out_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ctx->in_ev, consumer));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->in_ev, 0));
    rc = enqueue_patches(ctx, r, poses, (uint8_t*)d_out, row_stride, patch_stride, nullptr);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipEventRecord(ctx->out_ev, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(consumer, ctx->out_ev, 0));
    return FPM_OK;
}

// --- patch comparison -----------------------------------------------------------------
int fpm_compare_derive(int64_t n, int64_t sum_i, int64_t sum_ii, int64_t sum_t, int64_t sum_tt, int64_t sum_it,
                       int32_t normalize, double* zncc, double* gain, double* offset, uint8_t lut[256]) {
    if (!zncc || !gain || !offset || n < 1 || n > kCompareMaxArea) return FPM_E_INVALID_ARG;
    // sums of n bytes and of their products, so that the three determinants are exact in 64 bits
    if (sum_i < 0 || sum_i > 255 * n || sum_t < 0 || sum_t > 255 * n || sum_ii < 0 || sum_ii > 65025 * n || sum_tt < 0 ||
        sum_tt > 65025 * n || sum_it < 0 || sum_it > 65025 * n)
        return FPM_E_INVALID_ARG;
    if (n * sum_ii < sum_i * sum_i || n * sum_tt < sum_t * sum_t) return FPM_E_INVALID_ARG;   // of no pixels (Cauchy-Schwarz)
    compare_derive(n, sum_i, sum_ii, sum_t, sum_tt, sum_it, normalize != 0, zncc, gain, offset, lut);
    return FPM_OK;
}

static int compare_args(fpm_ctx* ctx, int32_t threshold, int32_t flags) {
    if (threshold < 0 || threshold > 255) { ctx->err = "threshold must be 0 .. 255"; return FPM_E_INVALID_ARG; }
    if (flags & ~FPM_COMPARE_NORMALIZE) { ctx->err = "unknown comparison flags"; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

static int compare_entry(fpm_ctx* ctx, const HitQuery& q, const fpm_patch_rect* rect, int32_t threshold, int32_t flags,
                         fpm_compare_stats* out, uint8_t* diff, size_t row_stride, size_t patch_stride) {
    int rc = q.check(ctx);
    if (rc == FPM_OK) rc = compare_args(ctx, threshold, flags);
    if (rc != FPM_OK) return rc;
    fpm_patch_rect r;
    std::vector<PatchPose> poses;
    rc = hits_begin(ctx, q, compare_rect, rect, &r, poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    if (!out) { ctx->err = "null statistics buffer"; return FPM_E_INVALID_ARG; }
    if (diff && (rc = check_patch_out(ctx, diff, r, row_stride, patch_stride)) != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return compare_to_host(ctx, r, poses, threshold, flags, out, diff, row_stride, patch_stride);
}

int fpm_last_compare(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, int32_t threshold, int32_t flags,
                     fpm_compare_stats* out, int32_t cap, int32_t* n, uint8_t* diff, size_t row_stride,
                     size_t patch_stride) {
    return compare_entry(ctx, HitQuery::last(source, cap, n), rect, threshold, flags, out, diff, row_stride, patch_stride);
}

int fpm_compare_at(fpm_ctx* ctx, const fpm_patch_rect* rect, const int32_t* src_index, const float* lt,
                   const double* angles, int32_t n_poses, int32_t threshold, int32_t flags, fpm_compare_stats* out,
                   uint8_t* diff, size_t row_stride, size_t patch_stride) {
    return compare_entry(ctx, HitQuery::at(src_index, lt, angles, n_poses), rect, threshold, flags, out, diff, row_stride,
                         patch_stride);
}

// --- learning on the device -----------------------------------------------------------
int fpm_learn_derive(int64_t n, int64_t sum, int64_t sum_sq, double* mean, double* norm, double* inv_area,
                     int32_t* equal1) {
    if (!mean || !norm || !inv_area || !equal1 || n < 1 || n > ((int64_t)1 << 32)) return FPM_E_INVALID_ARG;
    if (sum < 0 || sum > 255 * n || sum_sq < 0 || sum_sq > 65025 * n) return FPM_E_INVALID_ARG;
    if ((unsigned __int128)n * (unsigned __int128)sum_sq < (unsigned __int128)sum * (unsigned __int128)sum)
        return FPM_E_INVALID_ARG;   // of no pixels (Cauchy-Schwarz)
    bool eq = false;
    learn_derive(n, sum, sum_sq, mean, norm, inv_area, &eq);
    *equal1 = eq ? 1 : 0;
    return FPM_OK;
}

// learnPattern (TemplateMatcher.cpp:45-95) on an image already in device memory
int fpm_learn_device(fpm_ctx* ctx, const void* d_image, int32_t w, int32_t h, size_t stride, size_t plane_stride,
                     int32_t format, void* producer_stream) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!d_image) { ctx->err = "empty template"; return FPM_E_INVALID_ARG; }
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    int rc = check_image_desc(ctx, 1, w, h, stride, plane_stride, format);
    if (rc == FPM_OK) rc = learn_size(ctx, w, h);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = check_device_images(ctx, &d_image, 1, image_extent(w, h, stride, plane_stride, format), "template");
    if (rc != FPM_OK) return rc;
    rc = learn_from_image(ctx, d_image, w, h, stride, plane_stride, format, (hipStream_t)producer_stream);
    return rc == FPM_OK ? rc : learn_fail(ctx, rc);
}

int fpm_learn_at(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, float lt_x, float lt_y, double angle) {
    if (!ctx) return FPM_E_INVALID_ARG;
    const RawPose pose{lt_x, lt_y, angle};
    return learn_pose_entry(ctx, rect, false, source, 0, &pose);
}

int fpm_learn_hit(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, int32_t index) {
    if (!ctx) return FPM_E_INVALID_ARG;
    return learn_pose_entry(ctx, rect, true, source, index, nullptr);
}

// --- variation model ------------------------------------------------------------------
int fpm_model_derive(int32_t n, int64_t sum, int64_t sum_sq, int32_t a, int32_t kq, int32_t* mean, int32_t* lo,
                     int32_t* hi) {
    if (!mean || !lo || !hi || n < 1 || n > kModelMaxSamples || a < 0 || a > 255 || kq < 0 || kq > 255) return FPM_E_INVALID_ARG;
    // sums of n bytes and of their squares: v <= v^2 <= 255 v and v^2 = v (mod 2) hold per sample, so for the sums
    if (sum < 0 || sum > 255 * (int64_t)n || sum_sq < sum || sum_sq > 255 * sum || ((sum_sq ^ sum) & 1)) return FPM_E_INVALID_ARG;
    if ((int64_t)n * sum_sq < sum * sum) return FPM_E_INVALID_ARG;   // of no samples (Cauchy-Schwarz)
    const ModelBand b = model_band((uint32_t)n, (uint32_t)sum, (uint32_t)sum_sq, (uint32_t)a, (uint32_t)kq);
    *mean = b.mean; *lo = b.lo; *hi = b.hi;
    return FPM_OK;
}

int fpm_model_clear(fpm_ctx* ctx) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (ctx->pending) { ctx->err = kInFlight; return FPM_E_INVALID_ARG; }
    ctx->model_n = 0;
    return FPM_OK;
}

int fpm_model_set_chunk(fpm_ctx* ctx, int32_t jobs) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (jobs < 0) { ctx->err = "chunk must be 0 (the engine's choice) or a number of jobs"; return FPM_E_INVALID_ARG; }
    ctx->model_chunk = jobs;
    return FPM_OK;
}

int fpm_model_info(const fpm_ctx* ctx, int32_t* n, fpm_patch_rect* rect) {
    if (!ctx || !n) return FPM_E_INVALID_ARG;
    *n = ctx->model_n;
    if (rect) *rect = ctx->model_n > 0 ? ctx->model_rect : fpm_patch_rect{0, 0, 0, 0};
    return FPM_OK;
}

static int model_train_entry(fpm_ctx* ctx, const HitQuery& q, const fpm_patch_rect* rect, int32_t flags) {
    int rc = q.check(ctx);
    if (rc != FPM_OK) return rc;
    if (flags & ~FPM_COMPARE_NORMALIZE) { ctx->err = "unknown training flags"; return FPM_E_INVALID_ARG; }
    fpm_patch_rect r;
    std::vector<PatchPose> poses;
    rc = hits_begin(ctx, q, compare_rect, rect, &r, poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return model_train(ctx, r, poses, flags);
}

// no capacity: every hit is taken, and *n_added is their count only once they are in the model
int fpm_model_train_last(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, int32_t flags, int32_t* n_added) {
    if (!ctx || !n_added) return FPM_E_INVALID_ARG;
    *n_added = 0;
    int32_t n = 0;
    const int rc = model_train_entry(ctx, HitQuery::last(source, INT32_MAX, &n), rect, flags);
    if (rc == FPM_OK) *n_added = n;
    return rc;
}

int fpm_model_train_at(fpm_ctx* ctx, const fpm_patch_rect* rect, const int32_t* src_index, const float* lt,
                       const double* angles, int32_t n_poses, int32_t flags) {
    return model_train_entry(ctx, HitQuery::at(src_index, lt, angles, n_poses), rect, flags);
}

int fpm_model_sums(fpm_ctx* ctx, uint32_t* sum, uint32_t* sum_sq) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (ctx->pending) { ctx->err = kInFlight; return FPM_E_INVALID_ARG; }
    fpm_patch_rect r;
    const int rc = model_need(ctx, &r);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)r.w * r.h, plane = px * sizeof(uint32_t);
    // training returns with the stream drained: the planes are complete
    if (sum) HIP_TRY(hipMemcpy(sum, ctx->d_model.p, plane, hipMemcpyDeviceToHost));
    if (sum_sq) HIP_TRY(hipMemcpy(sum_sq, ctx->d_model.as<uint32_t>() + px, plane, hipMemcpyDeviceToHost));
    return FPM_OK;
}

int fpm_model_images(fpm_ctx* ctx, int32_t a, int32_t kq, uint8_t* mean, uint8_t* lo, uint8_t* hi, size_t row_stride) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (ctx->pending) { ctx->err = kInFlight; return FPM_E_INVALID_ARG; }
    fpm_patch_rect r;
    int rc = model_need(ctx, &r);
    if (rc == FPM_OK) rc = model_args(ctx, a, kq);
    if (rc != FPM_OK) return rc;
    if (row_stride < (size_t)r.w) { ctx->err = "row_stride below the model's width"; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    rc = model_band_ensure(ctx, a, kq);
    if (rc != FPM_OK) return rc;
    const size_t pitch = (size_t)model_pitch(r.w), plane = pitch * r.h;
    uint8_t* outs[3] = {mean, lo, hi};
    for (int k = 0; k < 3; ++k)
        if (outs[k])
            HIP_TRY(hipMemcpy2DAsync(outs[k], row_stride, ctx->d_band.as<uint8_t>() + k * plane, pitch, r.w, r.h,
                                     hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return FPM_OK;
}

static int inspect_args(fpm_ctx* ctx, int32_t a, int32_t kq, int32_t flags) {
    if (flags & ~FPM_COMPARE_NORMALIZE) { ctx->err = "unknown inspection flags"; return FPM_E_INVALID_ARG; }
    return model_args(ctx, a, kq);
}

static int inspect_entry(fpm_ctx* ctx, const HitQuery& q, int32_t a, int32_t kq, int32_t flags, fpm_inspect_stats* out,
                         uint8_t* img, size_t row_stride, size_t patch_stride) {
    int rc = q.check(ctx);
    if (rc == FPM_OK) rc = inspect_args(ctx, a, kq, flags);
    if (rc != FPM_OK) return rc;
    fpm_patch_rect r;
    std::vector<PatchPose> poses;
    rc = hits_begin(ctx, q, model_rect, nullptr, &r, poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    if (!out) { ctx->err = "null statistics buffer"; return FPM_E_INVALID_ARG; }
    if (img && (rc = check_patch_out(ctx, img, r, row_stride, patch_stride)) != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return inspect_to_host(ctx, r, poses, a, kq, flags, out, img, row_stride, patch_stride);
}

int fpm_last_inspect(fpm_ctx* ctx, int32_t source, int32_t a, int32_t kq, int32_t flags, fpm_inspect_stats* out,
                     int32_t cap, int32_t* n, uint8_t* img, size_t row_stride, size_t patch_stride) {
    return inspect_entry(ctx, HitQuery::last(source, cap, n), a, kq, flags, out, img, row_stride, patch_stride);
}

int fpm_inspect_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                   int32_t a, int32_t kq, int32_t flags, fpm_inspect_stats* out, uint8_t* img, size_t row_stride,
                   size_t patch_stride) {
    return inspect_entry(ctx, HitQuery::at(src_index, lt, angles, n_poses), a, kq, flags, out, img, row_stride, patch_stride);
}

int fpm_model_learn(fpm_ctx* ctx) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (ctx->pending) { ctx->err = kInFlight; return FPM_E_INVALID_ARG; }
    fpm_patch_rect r;
    int rc = model_need(ctx, &r);
    if (rc == FPM_OK) rc = learn_size(ctx, r.w, r.h);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    // the mask is re-framed as the model is: its crop to the rectangle, which becomes the new template, so that it keeps
    // covering the same pixels.  The crop goes through a host temporary, since the plane's pitch follows the template.
    std::vector<uint8_t> crop;
    const bool had_mask = ctx->mask_set, was_on = ctx->mask_on;
    if (had_mask) {
        const int tw = ctx->tmpl[0].w;
        crop.resize((size_t)r.w * r.h);
        for (int y = 0; y < r.h; ++y)
            std::copy_n(ctx->mask_host.data() + (size_t)(r.y + y) * tw + r.x, r.w, crop.data() + (size_t)y * r.w);
        mask_drop(ctx);
    }
    rc = learn_from_model(ctx);
    if (rc != FPM_OK) return learn_fail(ctx, rc);
    ctx->model_rect = fpm_patch_rect{0, 0, r.w, r.h};   // the new template's frame: the region the model was trained on
    if (had_mask) {
        rc = mask_install(ctx, crop.data(), nullptr, (size_t)r.w);
        if (rc != FPM_OK) return rc;   // the template and the model stand; the mask is gone
        ctx->mask_on = was_on;
    }
    return FPM_OK;
}

// --- template masks -------------------------------------------------------------------
int fpm_mask_set(fpm_ctx* ctx, const uint8_t* mask, int32_t w, int32_t h, size_t stride) {
    if (!ctx) return FPM_E_INVALID_ARG;
    int rc = mask_state(ctx, false);
    if (rc == FPM_OK) rc = mask_dims(ctx, mask, w, h, stride);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return mask_install(ctx, mask, nullptr, stride);
}

int fpm_mask_set_device(fpm_ctx* ctx, const void* d_mask, int32_t w, int32_t h, size_t stride, void* producer_stream) {
    if (!ctx) return FPM_E_INVALID_ARG;
    int rc = mask_state(ctx, false);
    if (rc == FPM_OK) rc = mask_dims(ctx, d_mask, w, h, stride);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = check_device_images(ctx, &d_mask, 1, image_extent(w, h, stride, 0, FPM_FMT_GRAY8), "mask");
    if (rc != FPM_OK) return rc;
    if (!ctx->in_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->in_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ctx->in_ev, (hipStream_t)producer_stream));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->in_ev, 0));
    return mask_install(ctx, nullptr, (const uint8_t*)d_mask, stride);
}

int fpm_mask_clear(fpm_ctx* ctx) {
    if (!ctx) return FPM_E_INVALID_ARG;
    const int rc = mask_state(ctx, false);
    if (rc != FPM_OK) return rc;
    mask_drop(ctx);
    return FPM_OK;
}

int fpm_mask_enable(fpm_ctx* ctx, int32_t enable) {
    if (!ctx) return FPM_E_INVALID_ARG;
    const int rc = mask_state(ctx, true);
    if (rc != FPM_OK) return rc;
    ctx->mask_on = enable != 0;
    return FPM_OK;
}

int fpm_mask_info(const fpm_ctx* ctx, int32_t* width, int32_t* height, int64_t* count, int32_t* enabled) {
    if (!ctx) return FPM_E_INVALID_ARG;
    const bool has = ctx->learned && ctx->mask_set;
    if (width) *width = has ? ctx->tmpl[0].w : 0;
    if (height) *height = has ? ctx->tmpl[0].h : 0;
    if (count) *count = has ? ctx->mask_count : 0;
    if (enabled) *enabled = has && ctx->mask_on ? 1 : 0;
    return FPM_OK;
}

int fpm_mask_get(fpm_ctx* ctx, uint8_t* out, size_t stride) {
    if (!ctx) return FPM_E_INVALID_ARG;
    const int rc = mask_state(ctx, true);
    if (rc != FPM_OK) return rc;
    const int w = ctx->tmpl[0].w, h = ctx->tmpl[0].h;
    if (!out || stride < (size_t)w) { ctx->err = "null buffer or stride below the mask's width"; return FPM_E_INVALID_ARG; }
    for (int y = 0; y < h; ++y) std::copy_n(ctx->mask_host.data() + (size_t)y * w, w, out + (size_t)y * stride);
    return FPM_OK;
}

int fpm_mask_count(fpm_ctx* ctx, const fpm_patch_rect* rect, int64_t* n) {
    if (!ctx) return FPM_E_INVALID_ARG;
    int rc = mask_state(ctx, true);
    fpm_patch_rect r;
    if (rc == FPM_OK) rc = compare_rect(ctx, rect, &r);
    if (rc != FPM_OK) return rc;
    if (!n) { ctx->err = "null count"; return FPM_E_INVALID_ARG; }
    *n = mask_count_rect(ctx, r);
    return FPM_OK;
}

int fpm_model_profile(const fpm_ctx* ctx, int32_t which, double* ms, int64_t* launches, int64_t* bytes) {
    return kprof_out(ctx, kProfModelTrain, which, 2, ms, launches, bytes);
}

// --- defect blobs on the device -----------------------------------------------------------
static int blob_args(fpm_ctx* ctx, int64_t n, int32_t level, int32_t connectivity, int32_t min_area, int32_t cap_per_hit,
                     const fpm_blob_summary* summary, const fpm_blob* out) {
    if (const char* bad = blobs_bad_args(n, level, connectivity, min_area, cap_per_hit)) { ctx->err = bad; return FPM_E_INVALID_ARG; }
    if (!summary || !out) { ctx->err = "null blob summary or record buffer"; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

static int blobs_entry(fpm_ctx* ctx, const HitQuery& q, int32_t a, int32_t kq, int32_t flags, int32_t level,
                       int32_t connectivity, int32_t min_area, fpm_inspect_stats* stats, fpm_blob_summary* summary,
                       fpm_blob* out, int32_t cap_per_hit) {
    int rc = q.check(ctx);
    if (rc == FPM_OK) rc = inspect_args(ctx, a, kq, flags);
    if (rc != FPM_OK) return rc;
    fpm_patch_rect r;
    std::vector<PatchPose> poses;
    rc = hits_begin(ctx, q, model_rect, nullptr, &r, poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    rc = blob_args(ctx, (int64_t)poses.size(), level, connectivity, min_area, cap_per_hit, summary, out);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return blobs_of_poses(ctx, r, poses, a, kq, flags, level, connectivity, min_area, cap_per_hit, stats, summary, out);
}

int fpm_last_blobs(fpm_ctx* ctx, int32_t source, int32_t a, int32_t kq, int32_t flags, int32_t level,
                   int32_t connectivity, int32_t min_area, fpm_inspect_stats* stats, fpm_blob_summary* summary,
                   fpm_blob* out, int32_t cap_per_hit, int32_t cap, int32_t* n) {
    return blobs_entry(ctx, HitQuery::last(source, cap, n), a, kq, flags, level, connectivity, min_area, stats, summary, out,
                       cap_per_hit);
}

int fpm_blobs_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                 int32_t a, int32_t kq, int32_t flags, int32_t level, int32_t connectivity, int32_t min_area,
                 fpm_inspect_stats* stats, fpm_blob_summary* summary, fpm_blob* out, int32_t cap_per_hit) {
    return blobs_entry(ctx, HitQuery::at(src_index, lt, angles, n_poses), a, kq, flags, level, connectivity, min_area, stats,
                       summary, out, cap_per_hit);
}

int fpm_op_blobs(fpm_ctx* ctx, const uint8_t* images, int32_t n, int32_t w, int32_t h, size_t stride, int32_t level,
                 int32_t connectivity, int32_t min_area, fpm_blob_summary* summary, fpm_blob* out, int32_t cap_per_hit,
                 int32_t* labels) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (ctx->pending) { ctx->err = kInFlight; return FPM_E_INVALID_ARG; }
    if (!images || n < 1 || n > 65535 || w < 1 || h < 1 || (int64_t)w * h > ((int64_t)1 << 22) || stride < (size_t)w ||
        stride > (size_t)INT32_MAX) {
        ctx->err = "bad blob images";
        return FPM_E_INVALID_ARG;
    }
    int rc = blob_args(ctx, n, level, connectivity, min_area, cap_per_hit, summary, out);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    struct ProfOff {   // the launches below are not an inspection's: the profile counters stay as they were
        fpm_ctx* c; bool was;
        explicit ProfOff(fpm_ctx* x) : c(x), was(x->prof) { c->prof = false; }
        ~ProfOff() { c->prof = was; }
    } prof_off(ctx);
    const size_t pitch = round_up(stride, (size_t)64), rows = (size_t)n * h;
    BlobRun b;
    rc = blobs_reserve(ctx, n, w, h, min_area, cap_per_hit, labels != nullptr, &b);
    if (rc != FPM_OK) return rc;
    // all stride bytes of every row, as the caller has them (the kernels mask by u < w); of the last row of the last
    // image only the w bytes fpm_blobs_host's addressing guarantees.  One copy from the host: into place when the
    // stride is the pitch, else to a staging area behind the images and from there row by row on the device (a 2D copy
    // from pageable memory goes row by row over the bus)
    const size_t host_bytes = (rows - 1) * stride + (size_t)w;
    HIP_TRY(ctx->d_blobimg.ensure(pitch * rows + (pitch == stride ? 0 : round_up(host_bytes, (size_t)64))));
    uint8_t* d = ctx->d_blobimg.as<uint8_t>();
    if (pitch == stride) {
        HIP_TRY(hipMemcpyAsync(d, images, host_bytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
        uint8_t* stage = d + pitch * rows;
        HIP_TRY(hipMemcpyAsync(stage, images, host_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (rows > 1)
            HIP_TRY(hipMemcpy2DAsync(d, pitch, stage, stride, stride, rows - 1, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d + (rows - 1) * pitch, stage + (rows - 1) * stride, (size_t)w, hipMemcpyDeviceToDevice,
                               ctx->stream));
    }
    return blobs_run(ctx, b, d, pitch, pitch * (size_t)h, level, connectivity, min_area, cap_per_hit, summary, out, labels);
}

int fpm_blobs_set_round(fpm_ctx* ctx, int32_t images) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (images < 0) { ctx->err = "images per round must be >= 0"; return FPM_E_INVALID_ARG; }
    ctx->blobs_round = images;
    return FPM_OK;
}

int fpm_blobs_profile(const fpm_ctx* ctx, int32_t which, double* ms, int64_t* launches, int64_t* bytes) {
    return kprof_out(ctx, kProfBlobTile, which, 4, ms, launches, bytes);
}

// --- pose alignment --------------------------------------------------------------------
int fpm_align_solve(const fpm_align_sums* sums, double* du, double* dv, double* dphi) {
    if (!sums || !du || !dv || !dphi) return FPM_E_INVALID_ARG;
    return align_solve(*sums, du, dv, dphi) ? 1 : 0;
}

int fpm_align_update(int32_t src_w, int32_t src_h, const fpm_patch_rect* rect, float lt_x, float lt_y, double angle,
                     double du, double dv, double dphi, float* lt2_x, float* lt2_y, double* angle2) {
    if (!rect || !lt2_x || !lt2_y || !angle2 || src_w <= 0 || src_h <= 0 || rect->w < 1 || rect->h < 1) return FPM_E_INVALID_ARG;
    const RawPose q = align_update(src_w, src_h, *rect, RawPose{lt_x, lt_y, angle}, du, dv, dphi);
    *lt2_x = q.x; *lt2_y = q.y; *angle2 = q.angle;
    return FPM_OK;
}

static int align_args(fpm_ctx* ctx, int32_t iters, double max_step, int32_t flags, int32_t known) {
    if (iters < 1 || iters > 8) { ctx->err = "iters must be 1 .. 8"; return FPM_E_INVALID_ARG; }
    if (!(max_step > 0.0) || !(max_step <= 1024.0)) { ctx->err = "max_step must be above 0 and at most 1024 pixels"; return FPM_E_INVALID_ARG; }
    if (flags & ~known) { ctx->err = "unknown alignment flags"; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

// state, alignment rectangle and poses, then the output pointer under the entry's own text
static int align_begin_entry(fpm_ctx* ctx, const HitQuery& q, const fpm_patch_rect* rect, const void* out, const char* null_out,
                             fpm_patch_rect* r, std::vector<PatchPose>& poses) {
    // align_rect is compare_rect under narrower caps, so what passes it needs no second look by compare_rect: one rule
    // for all three entries
    const int rc = hits_begin(ctx, q, align_rect, rect, r, poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    if (!out) { ctx->err = null_out; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    return FPM_OK;
}

int fpm_align_sums_at(fpm_ctx* ctx, const fpm_patch_rect* rect, const int32_t* src_index, const float* lt,
                      const double* angles, int32_t n_poses, int32_t flags, fpm_align_sums* out) {
    const HitQuery q = HitQuery::at(src_index, lt, angles, n_poses);
    int rc = q.check(ctx);
    if (rc != FPM_OK) return rc;
    if (flags & ~FPM_COMPARE_NORMALIZE) { ctx->err = "unknown alignment flags"; return FPM_E_INVALID_ARG; }
    fpm_patch_rect r;
    std::vector<PatchPose> poses;
    rc = align_begin_entry(ctx, q, rect, out, "null sums buffer", &r, poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    return align_sums_to_host(ctx, r, poses, flags, out);
}

// known: the flags the entry takes.  FPM_ALIGN_ADOPT is fpm_align_last's alone (intended: only it has last poses to
// replace); `aligned` receives the returned poses when it is set.
static int align_entry(fpm_ctx* ctx, const HitQuery& q, const fpm_patch_rect* rect, int32_t iters, double max_step,
                       int32_t flags, int32_t known, fpm_align_result* out, std::vector<PatchPose>* aligned) {
    int rc = q.check(ctx);
    if (rc == FPM_OK) rc = align_args(ctx, iters, max_step, flags, known);
    if (rc != FPM_OK) return rc;
    fpm_patch_rect r;
    std::vector<PatchPose> poses;
    rc = align_begin_entry(ctx, q, rect, out, "null result buffer", &r, poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    return align_iterate(ctx, r, poses, iters, max_step, flags & FPM_COMPARE_NORMALIZE, out, aligned);
}

int fpm_align_at(fpm_ctx* ctx, const fpm_patch_rect* rect, const int32_t* src_index, const float* lt,
                 const double* angles, int32_t n_poses, int32_t iters, double max_step, int32_t flags,
                 fpm_align_result* out) {
    return align_entry(ctx, HitQuery::at(src_index, lt, angles, n_poses), rect, iters, max_step, flags, FPM_COMPARE_NORMALIZE,
                       out, nullptr);
}

int fpm_align_last(fpm_ctx* ctx, const fpm_patch_rect* rect, int32_t source, int32_t iters, double max_step,
                   int32_t flags, fpm_align_result* out, int32_t cap, int32_t* n) {
    std::vector<PatchPose> aligned;
    const int rc = align_entry(ctx, HitQuery::last(source, cap, n), rect, iters, max_step, flags,
                               FPM_COMPARE_NORMALIZE | FPM_ALIGN_ADOPT, out, &aligned);
    if (rc != FPM_OK || !(flags & FPM_ALIGN_ADOPT)) return rc;
    // the aligned poses become the last poses, in last_poses' order; the results and candidates stay what they were
    size_t i = 0;
    for (int s = 0; s < (int)ctx->poses.size() && s < ctx->S; ++s)
        if (source < 0 || s == source)
            for (RawPose& p : ctx->poses[s]) p = aligned[i++].pose;
    return FPM_OK;
}

int fpm_align_profile(const fpm_ctx* ctx, double* ms, int64_t* launches, int64_t* bytes) {
    return kprof_out(ctx, kProfAlign, 0, 0, ms, launches, bytes);
}

// --- edge calipers (fpm_caliper_pose, fpm_caliper_edges_host and fpm_caliper_derive: fpm_host.cpp) --
static int calipers_entry(fpm_ctx* ctx, const HitQuery& q, const fpm_caliper* cals, int32_t n_cals, int32_t cap_per_caliper,
                          fpm_caliper_summary* summary, fpm_edge* edges, int32_t* profiles, int32_t profile_stride) {
    int rc = q.check(ctx);
    if (rc == FPM_OK) rc = caliper_args(ctx, cals, n_cals, cap_per_caliper);
    // intended: a caliper reads level 0 alone, so the caller's poses need no template (caliper_state); the last
    // search's poses imply one (patch_state)
    if (rc == FPM_OK) rc = q.need_search() ? patch_state(ctx, true) : caliper_state(ctx);
    std::vector<PatchPose> poses;
    if (rc == FPM_OK) rc = q.resolve(ctx, "caliper buffers too small", poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    rc = caliper_outputs(ctx, poses.size(), cals, n_cals, cap_per_caliper, summary, edges, profiles, profile_stride);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return calipers_to_host(ctx, poses, cals, n_cals, cap_per_caliper, summary, edges, profiles, profile_stride);
}

int fpm_calipers_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                    const fpm_caliper* cals, int32_t n_cals, int32_t cap_per_caliper, fpm_caliper_summary* summary,
                    fpm_edge* edges, int32_t* profiles, int32_t profile_stride) {
    return calipers_entry(ctx, HitQuery::at(src_index, lt, angles, n_poses), cals, n_cals, cap_per_caliper, summary, edges,
                          profiles, profile_stride);
}

int fpm_last_calipers(fpm_ctx* ctx, int32_t source, const fpm_caliper* cals, int32_t n_cals, int32_t cap_per_caliper,
                      fpm_caliper_summary* summary, fpm_edge* edges, int32_t* profiles, int32_t profile_stride,
                      int32_t cap, int32_t* n) {
    return calipers_entry(ctx, HitQuery::last(source, cap, n), cals, n_cals, cap_per_caliper, summary, edges, profiles,
                          profile_stride);
}

int fpm_caliper_profile(const fpm_ctx* ctx, double* ms, int64_t* launches, int64_t* bytes) {
    return kprof_out(ctx, kProfCaliper, 0, 0, ms, launches, bytes);
}

// --- gray-value tools (fpm_hist_derive: fpm_host.cpp) ------------------------------------------
static int histogram_entry(fpm_ctx* ctx, const HitQuery& q, const fpm_patch_rect* rects, int32_t n_rects, uint32_t* hist) {
    int rc = q.check(ctx);
    if (rc != FPM_OK) return rc;
    std::vector<fpm_patch_rect> rs;
    std::vector<PatchPose> poses;
    rc = patch_state(ctx, q.need_search());
    if (rc == FPM_OK) rc = gray_rects(ctx, rects, n_rects, rs);
    if (rc == FPM_OK) rc = q.resolve(ctx, "histogram buffer too small", poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    if (!hist) { ctx->err = "null histogram buffer"; return FPM_E_INVALID_ARG; }
    if ((int64_t)poses.size() * n_rects > FPM_GRAY_MAX_JOBS) { ctx->err = "hits x rectangles above 65536"; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    return gray_to_host(ctx, rs, poses, hist);
}

int fpm_histogram_at(fpm_ctx* ctx, const fpm_patch_rect* rects, int32_t n_rects, const int32_t* src_index, const float* lt,
                     const double* angles, int32_t n_poses, uint32_t* hist) {
    return histogram_entry(ctx, HitQuery::at(src_index, lt, angles, n_poses), rects, n_rects, hist);
}

int fpm_last_histogram(fpm_ctx* ctx, const fpm_patch_rect* rects, int32_t n_rects, int32_t source, uint32_t* hist,
                       int32_t cap, int32_t* n) {
    return histogram_entry(ctx, HitQuery::last(source, cap, n), rects, n_rects, hist);
}

static int segment_args(fpm_ctx* ctx, int32_t threshold, int32_t polarity) {
    if (threshold < FPM_SEG_OTSU || threshold > 255) { ctx->err = "threshold must be 0 .. 255 or FPM_SEG_OTSU"; return FPM_E_INVALID_ARG; }
    if (polarity != 1 && polarity != -1) { ctx->err = "polarity must be +1 or -1"; return FPM_E_INVALID_ARG; }
    return FPM_OK;
}

static int segment_outputs(fpm_ctx* ctx, int64_t hits, const fpm_patch_rect& r, int32_t connectivity, int32_t min_area,
                           int32_t cap_per_hit, const fpm_segment_info* info, const fpm_blob_summary* summary,
                           const fpm_blob* out, const uint8_t* img, size_t row_stride, size_t patch_stride) {
    int rc = blob_args(ctx, hits, 0, connectivity, min_area, cap_per_hit, summary, out);
    if (rc != FPM_OK) return rc;
    if (!info) { ctx->err = "null segment info buffer"; return FPM_E_INVALID_ARG; }
    if (img) return check_patch_out(ctx, img, r, row_stride, patch_stride);
    return FPM_OK;
}

static int segment_entry(fpm_ctx* ctx, const HitQuery& q, const fpm_patch_rect* rect, int32_t threshold, int32_t polarity,
                         int32_t connectivity, int32_t min_area, fpm_segment_info* info, fpm_blob_summary* summary,
                         fpm_blob* out, int32_t cap_per_hit, uint8_t* img, size_t row_stride, size_t patch_stride) {
    int rc = q.check(ctx);
    if (rc == FPM_OK) rc = segment_args(ctx, threshold, polarity);
    if (rc != FPM_OK) return rc;
    fpm_patch_rect r;
    std::vector<PatchPose> poses;
    rc = hits_begin(ctx, q, compare_rect, rect, &r, poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    rc = segment_outputs(ctx, (int64_t)poses.size(), r, connectivity, min_area, cap_per_hit, info, summary, out, img,
                         row_stride, patch_stride);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return segment_of_poses(ctx, r, poses, threshold, polarity, connectivity, min_area, cap_per_hit, info, summary, out,
                            img, row_stride, patch_stride);
}

int fpm_last_segment(fpm_ctx* ctx, int32_t source, const fpm_patch_rect* rect, int32_t threshold, int32_t polarity,
                     int32_t connectivity, int32_t min_area, fpm_segment_info* info, fpm_blob_summary* summary,
                     fpm_blob* out, int32_t cap_per_hit, int32_t cap, int32_t* n, uint8_t* img, size_t row_stride,
                     size_t patch_stride) {
    return segment_entry(ctx, HitQuery::last(source, cap, n), rect, threshold, polarity, connectivity, min_area, info, summary,
                         out, cap_per_hit, img, row_stride, patch_stride);
}

int fpm_segment_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                   const fpm_patch_rect* rect, int32_t threshold, int32_t polarity, int32_t connectivity,
                   int32_t min_area, fpm_segment_info* info, fpm_blob_summary* summary, fpm_blob* out,
                   int32_t cap_per_hit, uint8_t* img, size_t row_stride, size_t patch_stride) {
    return segment_entry(ctx, HitQuery::at(src_index, lt, angles, n_poses), rect, threshold, polarity, connectivity, min_area,
                         info, summary, out, cap_per_hit, img, row_stride, patch_stride);
}

int fpm_gray_set_run(fpm_ctx* ctx, int32_t tiles) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (tiles < 0) { ctx->err = "tiles per workgroup must be >= 0"; return FPM_E_INVALID_ARG; }
    ctx->gray_run = tiles;
    return FPM_OK;
}

int fpm_gray_profile(const fpm_ctx* ctx, int32_t which, double* ms, int64_t* launches, int64_t* bytes) {
    return kprof_out(ctx, kProfGrayHist, which, 1, ms, launches, bytes);
}

// --- sub-pattern locators (fpm_locate_host and fpm_locate_derive: fpm_host.cpp) --------------------
static int locate_entry(fpm_ctx* ctx, const HitQuery& q, const fpm_feature* feats, int32_t n_feats, fpm_locate_result* results,
                        fpm_locate_raw* raw, int32_t* maps, int32_t map_stride) {
    int rc = q.check(ctx);
    if (rc != FPM_OK) return rc;
    int max_off = 0;
    std::vector<PatchPose> poses;
    rc = patch_state(ctx, q.need_search());
    if (rc == FPM_OK) rc = locate_args(ctx, feats, n_feats, maps, map_stride, &max_off);
    if (rc == FPM_OK) rc = q.resolve(ctx, "locate buffers too small", poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    if (!results) { ctx->err = "null result buffer"; return FPM_E_INVALID_ARG; }
    if ((int64_t)poses.size() * n_feats > FPM_LOCATE_MAX_JOBS) { ctx->err = "hits x features above 65536"; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    return locate_to_host(ctx, poses, feats, n_feats, max_off, results, raw, maps, map_stride);
}

int fpm_locate_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                  const fpm_feature* feats, int32_t n_feats, fpm_locate_result* results, fpm_locate_raw* raw, int32_t* maps,
                  int32_t map_stride) {
    return locate_entry(ctx, HitQuery::at(src_index, lt, angles, n_poses), feats, n_feats, results, raw, maps, map_stride);
}

int fpm_last_locate(fpm_ctx* ctx, int32_t source, const fpm_feature* feats, int32_t n_feats, fpm_locate_result* results,
                    fpm_locate_raw* raw, int32_t* maps, int32_t map_stride, int32_t cap, int32_t* n) {
    return locate_entry(ctx, HitQuery::last(source, cap, n), feats, n_feats, results, raw, maps, map_stride);
}

int fpm_locate_profile(const fpm_ctx* ctx, double* ms, int64_t* launches, int64_t* bytes) {
    return kprof_out(ctx, kProfLocate, 0, 0, ms, launches, bytes);
}

// --- edge probes (fpm_probe_matrix, fpm_probe_edges_host, fpm_probe_derive and the fits:
// fpm_host.cpp) ------------------------------------------------------------------------------------------------------
static int probes_entry(fpm_ctx* ctx, const HitQuery& q, const fpm_probe* probes, int32_t n_probes,
                        const fpm_probe_params* params, fpm_probe_summary* summary, fpm_probe_result* results,
                        int32_t* profiles, int32_t profile_stride) {
    int rc = q.check(ctx);
    if (rc == FPM_OK) rc = probe_args(ctx, probes, n_probes, params);
    // intended, as for the calipers: a probe reads level 0 alone, so the caller's poses need no template
    // (caliper_state); the last search's poses imply one (patch_state).  No rule ties a probe to the template's
    // rectangle -- it may be drawn past the part -- so step 4 is empty.
    if (rc == FPM_OK) rc = q.need_search() ? patch_state(ctx, true) : caliper_state(ctx);
    std::vector<PatchPose> poses;
    if (rc == FPM_OK) rc = q.resolve(ctx, "probe buffers too small", poses);
    if (rc != FPM_OK || poses.empty()) return rc;
    rc = probe_outputs(ctx, poses.size(), n_probes, *params, summary, results, profiles, profile_stride);
    if (rc != FPM_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return probes_to_host(ctx, poses, probes, n_probes, *params, summary, results, profiles, profile_stride);
}

int fpm_probes_at(fpm_ctx* ctx, const int32_t* src_index, const float* lt, const double* angles, int32_t n_poses,
                  const fpm_probe* probes, int32_t n_probes, const fpm_probe_params* params, fpm_probe_summary* summary,
                  fpm_probe_result* results, int32_t* profiles, int32_t profile_stride) {
    return probes_entry(ctx, HitQuery::at(src_index, lt, angles, n_poses), probes, n_probes, params, summary, results,
                        profiles, profile_stride);
}

int fpm_last_probes(fpm_ctx* ctx, int32_t source, const fpm_probe* probes, int32_t n_probes, const fpm_probe_params* params,
                    fpm_probe_summary* summary, fpm_probe_result* results, int32_t* profiles, int32_t profile_stride,
                    int32_t cap, int32_t* n) {
    return probes_entry(ctx, HitQuery::last(source, cap, n), probes, n_probes, params, summary, results, profiles,
                        profile_stride);
}

int fpm_probe_profile(const fpm_ctx* ctx, double* ms, int64_t* launches, int64_t* bytes) {
    return kprof_out(ctx, kProfProbe, 0, 0, ms, launches, bytes);
}

int fpm_template_operands(const fpm_ctx* ctx, int8_t* t8, size_t* t8_bytes, int32_t* tsum, size_t* tsum_count) {
    if (!ctx || !t8_bytes || !tsum_count) return FPM_E_INVALID_ARG;
    if (!ctx->learned) return FPM_E_NOT_LEARNED;
    size_t o8 = 0, os = 0;
    operand_sizes(ctx->tmpl, &o8, &os);
    *t8_bytes = o8;
    *tsum_count = os;
    if (!t8 && !tsum) return FPM_OK;
    // both arrays were complete when the learn returned; a search in flight only reads them
    if (hipSetDevice(ctx->device) != hipSuccess) return FPM_E_DEVICE;
    if (t8 && hipMemcpy(t8, ctx->d_tmpl8.p, o8, hipMemcpyDeviceToHost) != hipSuccess) return FPM_E_DEVICE;
    if (tsum && hipMemcpy(tsum, ctx->d_tsum.p, os * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return FPM_E_DEVICE;
    return FPM_OK;
}

// --- angle sharding of one search ---------------------------------------------------------
int fpm_set_angle_shard(fpm_ctx* ctx, int32_t shard, int32_t shards) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (shards < 1 || shard < 0 || shard >= shards) { ctx->err = "bad angle shard"; return FPM_E_INVALID_ARG; }
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    ctx->shard = shard;
    ctx->shards = shards;
    return FPM_OK;
}

int fpm_get_angle_shard(const fpm_ctx* ctx, int32_t* shard, int32_t* shards) {
    if (!ctx || !shard || !shards) return FPM_E_INVALID_ARG;
    *shard = ctx->shard;
    *shards = ctx->shards;
    return FPM_OK;
}

int fpm_last_candidates(const fpm_ctx* ctx, int32_t source, fpm_candidate* out, int32_t cap, int32_t* n) {
    if (!ctx || !n) return FPM_E_INVALID_ARG;
    *n = 0;
    if (source < 0 || source >= (int)ctx->cands.size()) return FPM_E_INVALID_ARG;
    const std::vector<fpm_candidate>& c = ctx->cands[source];
    *n = (int32_t)c.size();
    for (int i = 0; i < (int)c.size() && i < cap && out; ++i) out[i] = c[i];
    return (int)c.size() > cap ? FPM_E_CAPACITY : FPM_OK;
}

int fpm_merge_candidates(const fpm_params* p, int32_t tmpl_w, int32_t tmpl_h, const fpm_candidate* cand, int32_t n,
                         fpm_result* out, int32_t cap, int32_t* n_results) {
    if (!p || !n_results || tmpl_w <= 0 || tmpl_h <= 0 || n < 0 || (n > 0 && !cand)) return FPM_E_INVALID_ARG;
    *n_results = 0;
    if (n >= 2048) host_pool_warm(2000);   // a large tail: the pool's workers awake for its parallel regions
    std::vector<fpm_result> res;
    if (!merge_candidates(*p, tmpl_w, tmpl_h, cand, n, res, nullptr)) return FPM_E_INVALID_ARG;
    *n_results = (int32_t)res.size();
    for (int i = 0; i < (int)res.size() && i < cap && out; ++i) out[i] = res[i];
    return (int)res.size() > cap ? FPM_E_CAPACITY : FPM_OK;
}

int fpm_search_bytes(const fpm_ctx* ctx, int64_t* b_pyr, int64_t* b_top, int64_t* b_ref) {
    if (!ctx || !b_pyr || !b_top || !b_ref) return FPM_E_INVALID_ARG;
    *b_pyr = ctx->alg_bytes[0];
    *b_top = ctx->alg_bytes[1];
    *b_ref = ctx->alg_bytes[2];
    return FPM_OK;
}

int fpm_search_stats(const fpm_ctx* ctx, int64_t* stats, int32_t cap) {
    if (!ctx || !stats) return FPM_E_INVALID_ARG;
    int n = 0;
    for (int64_t v : ctx->stats)
        if (n < cap) stats[n++] = v;
    return n;
}

int fpm_op_overlap_filter(fpm_ctx* ctx, const float* corners, const double* scores, int32_t n, double max_overlap,
                          int32_t mode, int32_t* keep, int32_t* n_keep, int32_t* stats) {
    if (!ctx || !n_keep || n < 0 || (n > 0 && (!corners || !scores || !keep)) || (mode != 0 && mode != 1))
        return FPM_E_INVALID_ARG;
    *n_keep = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<HostMatch> v((size_t)n);
    for (int i = 0; i < n; ++i) {
        HostMatch& m = v[(size_t)i];
        m = HostMatch{};
        const float* c = corners + 6 * (size_t)i;
        m.rect = rrect_from3(f2(c[0], c[1]), f2(c[2], c[3]), f2(c[4], c[5]));
        m.score = scores[i];
        m.id = i;
    }
    int path = 0;
    OverlapStats st;
    if (mode == 1 && n > 0) {
        path = overlap_filter_device(ctx, v, max_overlap, 1, &st) ? 1 : 2;
        if (path == 2) filter_with_rotated_rect(v, max_overlap);
    } else {
        filter_with_rotated_rect(v, max_overlap);
    }
    for (size_t i = 0; i < v.size(); ++i) keep[i] = v[i].id;
    *n_keep = (int32_t)v.size();
    if (stats) { stats[0] = path; stats[1] = st.host_pairs; stats[2] = st.flags; stats[3] = st.entries; }
    return FPM_OK;
}

int fpm_template_info(const fpm_ctx* ctx, int32_t* levels, int32_t* border_color) {
    if (!ctx || !levels || !border_color) return FPM_E_INVALID_ARG;
    if (!ctx->learned) return FPM_E_NOT_LEARNED;
    *levels = (int32_t)ctx->tmpl.size();
    *border_color = ctx->border;
    return FPM_OK;
}

int fpm_template_level(const fpm_ctx* ctx, int32_t level, int32_t* w, int32_t* h, double* mean, double* norm,
                       double* inv_area, int32_t* result_equal1, uint8_t* pixels, size_t stride) {
    if (!ctx || !w || !h || !mean || !norm || !inv_area || !result_equal1) return FPM_E_INVALID_ARG;
    if (!ctx->learned) return FPM_E_NOT_LEARNED;
    if (level < 0 || level >= (int)ctx->tmpl.size()) return FPM_E_INVALID_ARG;
    const TmplLevel& t = ctx->tmpl[level];
    *w = t.w; *h = t.h; *mean = t.mean; *norm = t.norm; *inv_area = t.inv_area; *result_equal1 = t.equal1 ? 1 : 0;
    if (pixels && t.px.empty()) {
        // a level of a device-learned template, fetched on first use (the slab was complete when the learn returned)
        std::vector<uint8_t> px((size_t)t.w * t.h);
        if (hipSetDevice(ctx->device) != hipSuccess ||
            hipMemcpy2D(px.data(), t.w, ctx->d_tmpl.as<uint8_t>() + t.off, t.pitch, t.w, t.h, hipMemcpyDeviceToHost) != hipSuccess)
            return FPM_E_DEVICE;
        t.px = std::move(px);
    }
    if (pixels)
        for (int y = 0; y < t.h; ++y) std::memcpy(pixels + (size_t)y * stride, t.px.data() + (size_t)y * t.w, (size_t)t.w);
    return FPM_OK;
}

// ---- pixel operators ----------------------------------------------------------------------------------
int fpm_op_pyr_down(fpm_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, size_t ss, uint8_t* dst, size_t ds) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!src || !dst || w <= 0 || h <= 0 || ss < (size_t)w) { ctx->err = "bad image"; return FPM_E_INVALID_ARG; }
    const int dw = (w + 1) / 2, dh = (h + 1) / 2;
    if (ds < (size_t)dw) { ctx->err = "bad dst stride"; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    const int sp = round_up(w + 4, 64), dp = round_up(dw + 4, 64);
    HIP_TRY(ctx->d_op_a.ensure((size_t)sp * (h + 1)));
    HIP_TRY(ctx->d_op_b.ensure((size_t)dp * (dh + 1)));
    HIP_TRY(hipMemcpy2DAsync(ctx->d_op_a.p, sp, src, ss, w, h, hipMemcpyHostToDevice, ctx->stream));
    // 3-chunk segments: every image taller than 64 output rows goes through the carried-window path
    launch_pyr_down(ctx->d_op_a.as<uint8_t>(), w, h, sp, 0, ctx->d_op_b.as<uint8_t>(), dw, dh, dp, 0, 1, ctx->stream, 3);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(dst, ds, ctx->d_op_b.p, dp, dw, dh, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FPM_OK;
}

int fpm_op_bitwise_not(fpm_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, size_t ss, uint8_t* dst, size_t ds) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!src || !dst || w <= 0 || h <= 0 || ss < (size_t)w) { ctx->err = "bad image"; return FPM_E_INVALID_ARG; }
    if (ds < (size_t)w) { ctx->err = "bad dst stride"; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    const SrcLevel lv = level_layout(w, h);   // the search's level-0 layout
    HIP_TRY(ctx->d_op_a.ensure(lv.img_bytes));
    HIP_TRY(hipMemcpy2DAsync(ctx->d_op_a.p, lv.pitch, src, ss, w, h, hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, FPM_K_NOT, 2 * (int64_t)w * h);
        if (!launch_bitwise_not(ctx->d_op_a.as<uint8_t>(), w, h, lv.pitch, lv.img_bytes, 1, ctx->stream)) {
            ctx->err = "level layout: rows not 16-byte aligned";
            return FPM_E_INTERNAL;
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(dst, ds, ctx->d_op_a.p, lv.pitch, w, h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    return FPM_OK;
}

// k_stage_gray over one image, host in / host out.  The source goes to the device byte for byte at its own address
// modulo 16 and with its own strides, so the kernel form and the byte alignment are those of a device image laid out
// like it.  The destination rows travel to the device and back over min(dst_stride, pitch) bytes (w for the last row,
// which need not have more), so a byte the kernel wrote past w would show in the caller's buffer.
int fpm_op_to_gray(fpm_ctx* ctx, const void* src, int32_t w, int32_t h, size_t ss, size_t plane_stride, int32_t format,
                   int32_t invert, uint8_t* dst, size_t ds) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!src || !dst) { ctx->err = "bad image"; return FPM_E_INVALID_ARG; }
    const int rc = check_image_desc(ctx, 1, w, h, ss, plane_stride, format);
    if (rc != FPM_OK) return rc;
    if (ds < (size_t)w) { ctx->err = "bad dst stride"; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t extent = image_extent(w, h, ss, plane_stride, format);
    const size_t mis = (uintptr_t)src & 15;
    const SrcLevel lv = level_layout(w, h);   // the search's level-0 layout
    HIP_TRY(ctx->d_op_a.ensure(mis + extent + 16));
    HIP_TRY(ctx->d_op_b.ensure(lv.img_bytes));
    HIP_TRY(ctx->d_op_job.ensure(sizeof(void*)));
    const uint8_t* d_img = ctx->d_op_a.as<uint8_t>(mis);
    uint8_t* d_dst = ctx->d_op_b.as<uint8_t>();
    const size_t back = std::min(ds, (size_t)lv.pitch);
    HIP_TRY(hipMemcpyAsync(ctx->d_op_a.as<uint8_t>(mis), src, extent, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_op_job.p, &d_img, sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    if (h > 1) HIP_TRY(hipMemcpy2DAsync(d_dst, lv.pitch, dst, ds, back, h - 1, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_dst + (size_t)(h - 1) * lv.pitch, dst + (size_t)(h - 1) * ds, w, hipMemcpyHostToDevice, ctx->stream));
    const bool aligned = mis == 0 && (ss & 15) == 0 && (!fmt_planar(format) || (plane_stride & 15) == 0);
    if (!launch_stage_gray(ctx->d_op_job.as<const uint8_t*>(), 1, w, h, ss, plane_stride, format, aligned, d_dst, lv.pitch,
                           lv.img_bytes, invert != 0, ctx->stream)) {
        ctx->err = "level layout: rows not 16-byte aligned";
        return FPM_E_INTERNAL;
    }
    HIP_TRY(hipGetLastError());
    if (h > 1) HIP_TRY(hipMemcpy2DAsync(dst, ds, d_dst, lv.pitch, back, h - 1, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dst + (size_t)(h - 1) * ds, d_dst + (size_t)(h - 1) * lv.pitch, w, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FPM_OK;
}

int fpm_op_pyr_down2(fpm_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, size_t ss, uint8_t* dst1, size_t ds1,
                     uint8_t* dst2, size_t ds2, int32_t seg_chunks, int32_t chunk_rows) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!src || !dst1 || !dst2 || w <= 0 || h <= 0 || ss < (size_t)w || seg_chunks < 0 ||
        (chunk_rows != 0 && chunk_rows != 16 && chunk_rows != 32)) {
        ctx->err = "bad image";
        return FPM_E_INVALID_ARG;
    }
    const int bw = (w + 1) / 2, bh = (h + 1) / 2, cw = (bw + 1) / 2, ch = (bh + 1) / 2;
    if (ds1 < (size_t)bw || ds2 < (size_t)cw) { ctx->err = "bad dst stride"; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    // the search's level layout: pitch round_up(w + 4, 64), one spare row
    const int sp = round_up(w + 4, 64), bp = round_up(bw + 4, 64), cp = round_up(cw + 4, 64);
    const size_t boff = round_up((size_t)bp * (bh + 1), (size_t)256);
    HIP_TRY(ctx->d_op_a.ensure((size_t)sp * (h + 1)));
    HIP_TRY(ctx->d_op_b.ensure(boff + (size_t)cp * (ch + 1)));
    HIP_TRY(hipMemcpy2DAsync(ctx->d_op_a.p, sp, src, ss, w, h, hipMemcpyHostToDevice, ctx->stream));
    uint8_t* b = ctx->d_op_b.as<uint8_t>();
    launch_pyr_down2(ctx->d_op_a.as<uint8_t>(), w, h, sp, 0, b, bw, bh, bp, 0, b + boff, cw, ch, cp, 0, 1, ctx->stream,
                     seg_chunks, nullptr, 0, chunk_rows);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(dst1, ds1, b, bp, bw, bh, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(dst2, ds2, b + boff, cp, cw, ch, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FPM_OK;
}

int fpm_op_warp_affine(fpm_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, size_t ss, const double m[6],
                       uint8_t* dst, int32_t dw, int32_t dh, size_t ds, int32_t border) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!src || !dst || !m || w <= 0 || h <= 0 || dw <= 0 || dh <= 0 || ss < (size_t)w || ds < (size_t)dw) {
        ctx->err = "bad warp arguments";
        return FPM_E_INVALID_ARG;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const int sp = round_up(w + 4, 64), dp = round_up(dw + 4, 64);
    HIP_TRY(ctx->d_op_a.ensure((size_t)sp * (h + 1)));
    HIP_TRY(ctx->d_op_b.ensure((size_t)dp * (dh + 1)));
    HIP_TRY(ctx->d_op_job.ensure(sizeof(WarpJob)));
    WarpJob j{};
    j.src = ctx->d_op_a.as<uint8_t>(); j.sw = w; j.sh = h; j.sp = sp;
    j.dst = ctx->d_op_b.as<uint8_t>(); j.dw = dw; j.dh = dh; j.dp = dp;
    j.border = border;
    std::copy(m, m + 6, j.M);
    invert_affine(j.M);
    HIP_TRY(hipMemcpyAsync(ctx->d_op_job.p, &j, sizeof(j), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(ctx->d_op_a.p, sp, src, ss, w, h, hipMemcpyHostToDevice, ctx->stream));
    launch_warp(ctx->d_op_job.as<WarpJob>(), 1, dw * dh, ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(dst, ds, ctx->d_op_b.p, dp, dw, dh, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FPM_OK;
}

int fpm_op_ncc_map(fpm_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, size_t ss, int32_t layer, int32_t fold,
                   float* out) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!ctx->learned) { ctx->err = "template not learned"; return FPM_E_NOT_LEARNED; }
    if (!src || !out || w <= 0 || h <= 0 || ss < (size_t)w || layer < 0 || layer >= (int)ctx->tmpl.size()) {
        ctx->err = "bad ncc arguments";
        return FPM_E_INVALID_ARG;
    }
    const TmplLevel& t = ctx->tmpl[layer];
    if (w < t.w || h < t.h) { ctx->err = "image smaller than template level"; return FPM_E_SIZE; }
    HIP_TRY(hipSetDevice(ctx->device));
    const int ow = w - t.w + 1, oh = h - t.h + 1;
    const int sp = round_up(w + 4, 64);
    HIP_TRY(ctx->d_op_a.ensure((size_t)sp * (h + 1)));
    HIP_TRY(ctx->d_op_b.ensure(sizeof(float) * (size_t)ow * oh));
    HIP_TRY(ctx->d_op_job.ensure(sizeof(NccJob)));
    NccJob j{};
    j.img = ctx->d_op_a.as<uint8_t>(); j.iw = w; j.ih = h; j.ip = sp;
    j.tmpl = ctx->d_tmpl.as<uint8_t>() + t.off; j.tw = t.w; j.th = t.h; j.tp = t.pitch;
    j.out = ctx->d_op_b.as<float>(); j.ow = ow; j.oh = oh;
    j.fold = fold ? 1 : 0;
    j.equal1 = t.equal1 ? 1 : 0;
    j.mean = t.mean; j.norm = t.norm; j.inv_area = t.inv_area;
    HIP_TRY(hipMemcpyAsync(ctx->d_op_job.p, &j, sizeof(j), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(ctx->d_op_a.p, sp, src, ss, w, h, hipMemcpyHostToDevice, ctx->stream));
    if (ncc_tile_fits(t.w, t.h)) launch_ncc_tile(ctx->d_op_job.as<NccJob>(), 1, ow, oh, t.w, t.h, ctx->stream);
    else launch_ncc_map(ctx->d_op_job.as<NccJob>(), 1, ow * oh, t.w * t.h, ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->d_op_b.p, sizeof(float) * (size_t)ow * oh, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FPM_OK;
}

// One refinement layer on caller-supplied ROIs, by the search's own launches (enqueue_search's layer loop with
// step = 0: no candidate step, no prologue, no next-layer tables).
int fpm_op_refine(fpm_ctx* ctx, const uint8_t* const* levels, int32_t count, int32_t w, int32_t h, size_t stride,
                  int32_t layer, const float* lt, const double* angles, int32_t n, int32_t n3, int32_t fold,
                  int32_t round_rois, fpm_roi_record* rec, uint8_t* roi_pixels, int32_t* pixels_written) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (pixels_written) *pixels_written = 0;
    if (!ctx->learned) { ctx->err = "template not learned"; return FPM_E_NOT_LEARNED; }
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    constexpr int kMaxCoord = 8192;      // ROI coordinates stay inside the samplers' 16.16 fixed-point tables
    constexpr int64_t kMaxRois = 1 << 20;
    if (!levels || !lt || !angles || !rec || !pixels_written || count <= 0 || w <= 0 || h <= 0 || w > kMaxCoord ||
        h > kMaxCoord || stride < (size_t)w || n <= 0 || (int64_t)count * n * 3 > kMaxRois) {
        ctx->err = "bad refine arguments";
        return FPM_E_INVALID_ARG;
    }
    if (layer < 0 || layer >= (int)ctx->tmpl.size()) { ctx->err = "bad layer"; return FPM_E_INVALID_ARG; }
    if (n3 != 1 && n3 != 3) { ctx->err = "n3 must be 1 or 3"; return FPM_E_INVALID_ARG; }
    if (round_rois < 0 || round_rois % n3 != 0) {
        ctx->err = "round_rois must be a multiple of n3";
        return FPM_E_INVALID_ARG;
    }
    for (int i = 0; i < count; ++i)
        if (!levels[i]) { ctx->err = "null level image"; return FPM_E_INVALID_ARG; }
    const int C = count * n, total_rois = C * n3;
    for (int i = 0; i < 2 * C; ++i)
        if (!std::isfinite(lt[i]) || std::fabs(lt[i]) > (float)kMaxCoord) {
            ctx->err = "ptLT not finite or out of range";
            return FPM_E_INVALID_ARG;
        }
    for (int i = 0; i < total_rois; ++i)
        if (!std::isfinite(angles[i])) { ctx->err = "angle not finite"; return FPM_E_INVALID_ARG; }
    HIP_TRY(hipSetDevice(ctx->device));
    const TmplLevel& tl = ctx->tmpl[layer];
    hipStream_t st = ctx->stream;
    // the level images as a search's slab holds one level: the layout and the slack the samplers read into
    const SrcLevel lv = level_layout(w, h);
    HIP_TRY(ctx->d_op_a.ensure(lv.img_bytes * count + level_slab_slack(lv.pitch)));
    for (int s = 0; s < count; ++s)
        HIP_TRY(hipMemcpy2DAsync(ctx->d_op_a.as<uint8_t>() + lv.img_bytes * s, lv.pitch, levels[s], stride, w, h,
                                 hipMemcpyHostToDevice, st));
    // candidates: id = source * n + i, alive, its node = id; the kernels sample at state.lt * 2 (the search keeps ptLT at
    // the layer above's resolution), so the state holds ptLT / 2 -- exact for a float (a power-of-two scaling; the
    // values here are far from the subnormal range or zero), and the kernels see the caller's ptLT bit for bit
    std::vector<CandState> hs(C);
    std::vector<int32_t> hl(C + 1);
    std::vector<AngleNode> hn((size_t)total_rois);
    for (int i = 0; i < C; ++i) {
        hs[i].lt = f2(lt[2 * i] / 2, lt[2 * i + 1] / 2);
        hs[i].node = i; hs[i].alive = 1; hs[i].reached0 = 0; hs[i].pad = 0;
        hl[i] = i;
        for (int j = 0; j < n3; ++j) hn[(size_t)i * n3 + j] = make_node(angles[(size_t)i * n3 + j]);
    }
    hl[C] = C;   // the live count
    const size_t o_state = 0, o_live = round_up(sizeof(CandState) * C, (size_t)256),
                 o_nodes = o_live + round_up(sizeof(int32_t) * (C + 1), (size_t)256),
                 o_rec = o_nodes + round_up(sizeof(AngleNode) * total_rois, (size_t)256);
    HIP_TRY(ctx->d_op_b.ensure(o_rec + sizeof(RoiRecord) * (size_t)total_rois));
    HIP_TRY(hipMemcpyAsync(ctx->d_op_b.as<char>(o_state), hs.data(), sizeof(CandState) * C, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->d_op_b.as<char>(o_live), hl.data(), sizeof(int32_t) * (C + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->d_op_b.as<char>(o_nodes), hn.data(), sizeof(AngleNode) * total_rois, hipMemcpyHostToDevice,
                           st));
    HIP_TRY(hipMemsetAsync(ctx->d_op_b.as<char>(o_rec), 0, sizeof(RoiRecord) * (size_t)total_rois, st));
    const int slot_cap = round_rois > 0 ? std::min(round_rois, total_rois) : total_rois;
    const bool small = roi_small_fits(tl.w, tl.h);   // the search's form rule
    const RoiScratchDims rd = roi_scratch_dims(&tl, 1);
    if (!small)
        HIP_TRY(roi_scratch_ensure(rd, (size_t)slot_cap, ctx->d_rf_tab, ctx->d_rf_tdesc, ctx->d_rf_roi, ctx->d_rf_rowsum,
                                   ctx->d_rf_wtot, ctx->d_rf_wtotq, ctx->d_rf_wedge));
    RoiArgs ra{};
    ra.level = ctx->d_op_a.as<uint8_t>(); ra.level_stride = lv.img_bytes;
    ra.W = lv.w; ra.H = lv.h; ra.P = lv.pitch;
    ra.tmpl = ctx->d_tmpl.as<uint8_t>() + tl.off; ra.tw = tl.w; ra.th = tl.h; ra.tp = tl.pitch;
    ra.tmpl8 = ctx->d_tmpl8.as<int8_t>() + tl.off8; ra.tp8 = tl.p8; ra.nk = (tl.w + 63) / 64;
    ra.tsum = ctx->d_tsum.as<int32_t>() + tl.tsum_off;
    ra.n3 = n3;
    ra.fold = fold ? 1 : 0;
    ra.equal1 = tl.equal1 ? 1 : 0;
    ra.per_source = n;
    ra.mean = tl.mean; ra.norm = tl.norm; ra.inv_area = tl.inv_area;
    ra.live = ctx->d_op_b.as<int32_t>(o_live);
    ra.live_count = ra.live + C;
    ra.state = ctx->d_op_b.as<CandState>(o_state);
    ra.nodes = ctx->d_op_b.as<AngleNode>(o_nodes);
    ra.tab = ctx->d_rf_tab.as<int32_t>(); ra.tabw = roi_pitch_for(tl.w); ra.tabh = roi_tab_rows(tl.h);
    ra.tdesc = ctx->d_rf_tdesc.as<int4>(); ra.tdesc_stride = rd.tdesc_stride;
    ra.roi = ctx->d_rf_roi.as<uint8_t>(); ra.roi_pitch = roi_pitch_for(tl.w); ra.roi_stride = rd.roi_stride;
    ra.rowsum = ctx->d_rf_rowsum.as<uint32_t>();
    ra.wtot = ctx->d_rf_wtot.as<uint32_t>();
    ra.wtotq = ctx->d_rf_wtotq.as<uint64_t>();
    ra.wedge = ctx->d_rf_wedge.as<uint32_t>();
    ra.rec = ctx->d_op_b.as<RoiRecord>(o_rec);
    ra.step = 0;   // records only: no candidate step, no prev_rec prologue, no next-layer tables
    const bool want_px = roi_pixels && !small && !tl.equal1;
    const int RW = tl.w + 6, RH = tl.h + 6, txn = (RW + 31) / 32;
    std::vector<uint8_t> tiles;
    for (int base = 0; base < total_rois; base += slot_cap) {
        ra.slot_base = base;
        ra.slot_cap = std::min(slot_cap, total_rois - base);
        if (small) {
            ProfScope ps(ctx, FPM_K_ROI_SMALL, 0);
            launch_roi_small(ra, st);
            continue;
        }
        {
            ProfScope ps(ctx, FPM_K_ROI_TABLES, 0);
            launch_roi_tables(ra, st);
        }
        {
            ProfScope ps(ctx, FPM_K_ROI_WARP, 0);
            launch_roi_warp(ra, st);
        }
        {
            ProfScope ps(ctx, FPM_K_ROI_CORR, 0);
            launch_roi_corr(ra, st);
        }
        {
            ProfScope ps(ctx, FPM_K_ROI_EVAL, 0);
            launch_roi_eval(ra, st);
        }
        if (want_px) {   // this round's ROIs out of the tile-major scratch (32 x 32 tiles of 1 KB, bytes ^ 0x80)
            tiles.resize((size_t)ra.slot_cap * rd.roi_stride);
            HIP_TRY(hipMemcpyAsync(tiles.data(), ctx->d_rf_roi.p, tiles.size(), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (int k = 0; k < ra.slot_cap; ++k) {
                const uint8_t* t = tiles.data() + (size_t)k * rd.roi_stride;
                uint8_t* o = roi_pixels + (size_t)(base + k) * RW * RH;
                for (int y = 0; y < RH; ++y)
                    for (int x = 0; x < RW; ++x)
                        o[(size_t)y * RW + x] =
                            t[((size_t)((y >> 5) * txn + (x >> 5)) << 10) + (y & 31) * 32 + (x & 31)] ^ 0x80;
            }
        }
    }
    HIP_TRY(hipGetLastError());
    std::vector<RoiRecord> hr((size_t)total_rois);
    HIP_TRY(hipMemcpyAsync(hr.data(), ctx->d_op_b.as<char>(o_rec), sizeof(RoiRecord) * hr.size(), hipMemcpyDeviceToHost,
                           st));
    HIP_TRY(hipStreamSynchronize(st));
    prof_collect(ctx);
    for (int i = 0; i < total_rois; ++i) {
        fpm_roi_record& r = rec[i];
        r.score = hr[i].score; r.mx = hr[i].mx; r.my = hr[i].my; r.on_border = hr[i].on_border;
        std::copy(hr[i].vec, hr[i].vec + 9, r.vec);
    }
    *pixels_written = want_px ? 1 : 0;
    return FPM_OK;
}

// The top-layer peak pass on caller-supplied maps, by the search's own launchers: form 0 as enqueue_search's split branch
// (fused_lds == 0 && !use_mma), form 1 as its use_mma branch with the lists k_top_mma would have written built on the host.
int fpm_op_peaks(fpm_ctx* ctx, const float* const* maps, const int32_t* mw, const int32_t* mh, int32_t n_maps,
                 int32_t tw, int32_t th, int32_t cap, int32_t by_block, int32_t mfc, double thr, double overlap,
                 int32_t form, int32_t list_cap, uint32_t list_seed, fpm_peak* peaks, int32_t* counts,
                 int32_t* stats) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    if (!maps || !mw || !mh || !peaks || !counts || n_maps < 1 || n_maps > 65535 || tw < 1 || th < 1 || tw >= 65536 ||
        th >= 65536 || cap < 1 || (int64_t)n_maps * cap > FPM_PEAKS_MAX_SLOTS || (form != 0 && form != 1) ||
        list_cap < 0 || !std::isfinite(thr) || !(std::fabs(overlap) <= 16.0)) {
        ctx->err = "bad peaks arguments";
        return FPM_E_INVALID_ARG;
    }
    by_block = by_block ? 1 : 0;
    mfc = (mfc && by_block) ? 1 : 0;
    const int n = n_maps;
    NmsMaxima mx;
    std::vector<size_t> map_off(n), blk_off(n);
    size_t mo = 0, bo = 0;
    for (int i = 0; i < n; ++i) {
        if (!maps[i] || mw[i] < 1 || mh[i] < 1 || mw[i] >= 65536 || mh[i] >= 65536) {
            ctx->err = "bad map";
            return FPM_E_INVALID_ARG;
        }
        map_off[i] = mo;
        mo += round_up((size_t)mw[i] * mh[i], (size_t)64);
        if (mo > (size_t)FPM_PEAKS_MAX_PIXELS) { ctx->err = "maps too large"; return FPM_E_INVALID_ARG; }
        const int nb = nms_maxima_add(mx, mw[i], mh[i], tw, th, by_block, mfc);   // as build_plan
        blk_off[i] = bo;
        bo += round_up((size_t)nb, (size_t)64);
    }
    // form 1: what plan_top_mma admits to the list path (the greedy forms need thr > 0 and hold 256 peaks)
    if (form == 1 && (!(thr > 0.01) || !(overlap >= 0.0) || cap > 256 || mx.max_cells > 12 * 1024)) {
        ctx->err = "peaks: the list form needs thr > 0.01, overlap >= 0, cap <= 256 and at most 12288 cells per map";
        return FPM_E_INVALID_ARG;
    }
    const int def_cap = by_block ? kNmsCandCap : 512;   // plan_top_mma's tcand_cap
    const int lcap = form == 1 ? (list_cap > 0 ? std::min(list_cap, def_cap) : def_cap) : (by_block ? kNmsCandCap : 0);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // scratch: the maps in d_op_a; jobs, block maxima, peaks, counts, list counts, strip keys and lists in d_op_b
    const size_t o_jobs = 0, o_bmax = round_up(sizeof(NmsJob) * n, (size_t)256),
                 o_bloc = o_bmax + round_up(sizeof(float) * std::max<size_t>(bo, 1), (size_t)256),
                 o_peaks = o_bloc + round_up(sizeof(int32_t) * std::max<size_t>(bo, 1), (size_t)256),
                 o_counts = o_peaks + round_up(sizeof(Peak) * (size_t)n * cap, (size_t)256),
                 o_zero = o_counts + round_up(sizeof(int32_t) * n, (size_t)256),   // [n] list counts, [n][3] u64, [n][3]
                 o_skey = o_zero + round_up(sizeof(int32_t) * n, (size_t)8), o_sdone = o_skey + sizeof(uint64_t) * 3 * n,
                 o_cand = round_up(o_sdone + sizeof(int32_t) * 3 * n, (size_t)256),
                 o_cval = o_cand + round_up(sizeof(int32_t) * (size_t)lcap * n, (size_t)256),
                 o_end = o_cval + (form == 1 ? round_up(sizeof(float) * (size_t)lcap * n, (size_t)256) : 0);
    HIP_TRY(ctx->d_op_a.ensure(sizeof(float) * mo));
    HIP_TRY(ctx->d_op_b.ensure(o_end));
    std::vector<NmsJob> jobs(n);
    std::vector<int32_t> k_true(n, 0);
    for (int i = 0; i < n; ++i) {
        NmsJob& j = jobs[i];
        j.map = ctx->d_op_a.as<float>() + map_off[i];
        j.bmax = ctx->d_op_b.as<float>(o_bmax) + blk_off[i];
        j.bloc = ctx->d_op_b.as<int32_t>(o_bloc) + blk_off[i];
        j.mw = mw[i]; j.mh = mh[i];
        const size_t px = (size_t)mw[i] * mh[i];
        HIP_TRY(hipMemcpyAsync(j.map, maps[i], sizeof(float) * px, hipMemcpyHostToDevice, st));
        for (size_t k = 0; k < px; ++k) k_true[i] += (double)maps[i][k] >= thr ? 1 : 0;
    }
    HIP_TRY(hipMemcpyAsync(ctx->d_op_b.as<char>(o_jobs), jobs.data(), sizeof(NmsJob) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(ctx->d_op_b.as<char>(o_peaks), 0, sizeof(Peak) * (size_t)n * cap, st));
    HIP_TRY(hipMemsetAsync(ctx->d_op_b.as<char>(o_counts), 0xff, sizeof(int32_t) * n, st));   // -1: no kernel took the job
    HIP_TRY(hipMemsetAsync(ctx->d_op_b.as<char>(o_zero), 0, o_cand - o_zero, st));   // as k_warp / the pyramid launch zero them
    NmsArgs na{};
    na.jobs = ctx->d_op_b.as<NmsJob>(o_jobs);
    na.peaks = ctx->d_op_b.as<Peak>(o_peaks);
    na.counts = ctx->d_op_b.as<int32_t>(o_counts);
    na.tw = tw; na.th = th; na.cap = cap; na.by_block = by_block; na.mfc = mfc;
    na.thr = thr; na.overlap = overlap;
    int32_t* d_ccnt = ctx->d_op_b.as<int32_t>(o_zero);
    NmsLaunchInfo gi{}, ni{};
    std::vector<int32_t> hl;
    std::vector<float> hv;
    if (form == 0) {
        if (by_block) {
            na.cand = ctx->d_op_b.as<int32_t>(o_cand); na.cand_cnt = d_ccnt; na.cand_cap = kNmsCandCap;
            na.skey = ctx->d_op_b.as<uint64_t>(o_skey);
            na.sdone = ctx->d_op_b.as<int32_t>(o_sdone);
        }
        launch_nms(na, n, mx.max_blocks, mx.max_map_dim, mx.max_cells, st, mx.max_items, nullptr, mx.max_map_px, &ni);
    } else {
        // k_top_mma's lists: every pixel >= thr once, in no particular order (here: shuffled), the first lcap stored
        hl.assign((size_t)lcap * n, 0);
        hv.assign((size_t)lcap * n, 0.f);
        std::mt19937 rng(list_seed);
        std::vector<int32_t> idx;
        for (int i = 0; i < n; ++i) {
            idx.clear();
            const int32_t px = mw[i] * mh[i];
            for (int32_t k = 0; k < px; ++k)
                if ((double)maps[i][k] >= thr) idx.push_back(k);
            for (size_t k = idx.size(); k > 1; --k) std::swap(idx[k - 1], idx[rng() % k]);
            for (size_t k = 0; k < idx.size() && k < (size_t)lcap; ++k) {
                hl[(size_t)i * lcap + k] = idx[k];
                hv[(size_t)i * lcap + k] = maps[i][idx[k]];
            }
        }
        HIP_TRY(hipMemcpyAsync(ctx->d_op_b.as<char>(o_cand), hl.data(), sizeof(int32_t) * hl.size(), hipMemcpyHostToDevice,
                               st));
        HIP_TRY(hipMemcpyAsync(ctx->d_op_b.as<char>(o_cval), hv.data(), sizeof(float) * hv.size(), hipMemcpyHostToDevice,
                               st));
        HIP_TRY(hipMemcpyAsync(d_ccnt, k_true.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
        NmsArgs ga = na;
        ga.cand = ctx->d_op_b.as<int32_t>(o_cand); ga.cand_val = ctx->d_op_b.as<float>(o_cval);
        ga.cand_cnt = d_ccnt; ga.cand_cap = lcap;
        ga.reset_untaken = by_block;
        launch_top_greedy(ga, n, mx.max_cells, st, nullptr, &gi);
        NmsArgs fa = na;
        fa.cand = ga.cand; fa.cand_cnt = ga.cand_cnt; fa.cand_cap = lcap;
        if (by_block) {
            fa.skey = ctx->d_op_b.as<uint64_t>(o_skey);
            fa.sdone = ctx->d_op_b.as<int32_t>(o_sdone);
        }
        launch_nms(fa, n, mx.max_blocks, mx.max_map_dim, mx.max_cells, st, mx.max_items, nullptr, mx.max_map_px, &ni);
    }
    HIP_TRY(hipGetLastError());
    std::vector<Peak> hp((size_t)n * cap);
    std::vector<int32_t> hc(n), hk(n, 0);
    HIP_TRY(hipMemcpyAsync(hp.data(), ctx->d_op_b.as<char>(o_peaks), sizeof(Peak) * hp.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hc.data(), ctx->d_op_b.as<char>(o_counts), sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    if (form == 1 || by_block) HIP_TRY(hipMemcpyAsync(hk.data(), d_ccnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        counts[i] = hc[i];
        for (int k = 0; k < hc[i] && k < cap; ++k) {
            fpm_peak& p = peaks[(size_t)i * cap + k];
            const Peak& q = hp[(size_t)i * cap + k];
            p.x = q.x; p.y = q.y; p.score = q.score;
        }
    }
    if (stats) {
        stats[0] = (int32_t)(gi.kernels | ni.kernels);
        stats[1] = ni.lds_blocks; stats[2] = ni.cand_lds;
        stats[3] = form == 1 ? gi.greedy_cap : ni.greedy_cap;
        stats[4] = ni.blk_lds; stats[5] = lcap; stats[6] = mx.max_blocks; stats[7] = mx.max_cells;
        for (int i = 0; i < n; ++i) {
            int32_t* s = stats + FPM_PEAKS_STATS_CALL + FPM_PEAKS_STATS_JOB * i;
            s[0] = k_true[i]; s[1] = hk[i]; s[2] = hk[i] < 0 ? 1 : 0;
            s[3] = by_block ? -1 : nms_plain_form(ni.blk_lds, cap, (long)mw[i] * mh[i]);
        }
    }
    return FPM_OK;
}

// The top-layer scoring of the staged batch by the plan's own tables and launchers (enqueue_pyramid, then
// enqueue_top_split_maps or launch_top_mma on a copy of P.tma), and what it wrote: the maps, or k_top_mma's lists.
static_assert(kTopFormExact16 == FPM_TOP_FORM_EXACT16 && kTopFormExact14 == FPM_TOP_FORM_EXACT14 &&
                  kTopFormSmall == FPM_TOP_FORM_SMALL && kTopFormLarge == FPM_TOP_FORM_LARGE,
              "stats[5] of fpm_op_top_maps is top_mma_form's value");
int fpm_op_top_maps(fpm_ctx* ctx, int32_t form, double thr, int32_t* n_sources, int32_t* n_angles, int64_t* map_floats,
                    int32_t* list_cap, int32_t* geom, int32_t geom_cap, float* maps, int64_t maps_cap,
                    int32_t* list_count, int32_t* list_index, float* list_value, int64_t list_slots, int32_t* stats) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!ctx->learned) { ctx->err = "template not learned"; return FPM_E_NOT_LEARNED; }
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    if (ctx->S <= 0 || !ctx->staged || !ctx->src_valid) { ctx->err = "top maps: no staged sources"; return FPM_E_INVALID_ARG; }
    const bool sizing = !geom && !maps && !list_count && !list_index && !list_value;
    const bool want_maps = form == 0 || form == 1;
    if (form < 0 || form > 2 || !std::isfinite(thr) || (thr > 0 && !(thr > 0.01)) || geom_cap < 0 || maps_cap < 0 ||
        list_slots < 0 ||
        (!sizing && (!geom || (want_maps ? !maps : (!list_count || !list_index || !list_value))))) {
        ctx->err = "bad top maps arguments";
        return FPM_E_INVALID_ARG;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    struct ProfOff {   // the launches below are not the search's: the profile counters stay as they were
        fpm_ctx* c; bool was;
        explicit ProfOff(fpm_ctx* x) : c(x), was(x->prof) { c->prof = false; }
        ~ProfOff() { c->prof = was; }
    } prof_off(ctx);
    int rc = build_plan(ctx);
    if (rc != FPM_OK) return rc;
    Plan& P = ctx->plan;
    const int L = P.L, S = P.S, nang = P.nang, J = S * nang;
    std::vector<size_t> dense_off(nang);
    size_t dense = 0;
    for (int a = 0; a < nang; ++a) { dense_off[a] = dense; dense += (size_t)P.map_w[a] * P.map_h[a]; }
    const int lcap = P.top_mma ? P.tcand_cap : 0;
    if (n_sources) *n_sources = S;
    if (n_angles) *n_angles = nang;
    if (map_floats) *map_floats = (int64_t)dense;
    if (list_cap) *list_cap = lcap;
    TopMmaArgs ta = P.tma;
    if (stats) {
        std::fill(stats, stats + FPM_TOP_MAPS_STATS, 0);
        stats[0] = P.top_mma ? 1 : 0;
        stats[5] = -1;
        stats[7] = P.by_block ? 1 : 0;
        if (P.top_mma) {
            ta.mode = 1;
            stats[1] = lcap; stats[2] = ta.sw; stats[3] = ta.rt - ta.th; stats[4] = ta.nunits;
            stats[5] = top_mma_form(ta); stats[6] = top_mma_grid(ta);
        }
    }
    if (form != 0 && !P.top_mma) {
        ctx->err = "top maps: the plan does not take the matrix-core form";
        return FPM_E_SIZE;
    }
    if (sizing) return FPM_OK;
    if (geom_cap < nang || (want_maps && (uint64_t)maps_cap < (uint64_t)dense * S) ||
        (!want_maps && (uint64_t)list_slots < (uint64_t)lcap * J)) {
        ctx->err = "top maps: output capacity below the sizing call's";
        return FPM_E_CAPACITY;
    }
    for (int a = 0; a < nang; ++a) {
        geom[4 * a + 0] = P.top[a].bw; geom[4 * a + 1] = P.top[a].bh;
        geom[4 * a + 2] = P.map_w[a]; geom[4 * a + 3] = P.map_h[a];
    }
    if (J <= 0) return FPM_OK;
    hipStream_t st = ctx->stream;
    rc = apply_polarity(ctx);   // as start_staged, ahead of the pyramid
    if (rc != FPM_OK) return rc;
    enqueue_pyramid(ctx, form != 0);   // (the matrix-core form's list counts are among the counters it zeroes)
    if (want_maps)   // a pixel no kernel writes reads back as a NaN pattern
        HIP_TRY(hipMemsetAsync(P.d_map.p, 0xff, sizeof(float) * P.map_floats * S, st));
    if (form == 0) {
        enqueue_top_split_maps(ctx);
    } else {
        if (thr > 0) top_mma_thresholds(ta, thr, ctx->tmpl[L]);
        HIP_TRY(hipMemsetAsync(ta.cand_cnt, 0, sizeof(int32_t) * J, st));   // no job taken, no list entry yet
        if (form == 2) {
            HIP_TRY(hipMemsetAsync(ta.cand, 0xff, sizeof(int32_t) * (size_t)lcap * J, st));
            HIP_TRY(hipMemsetAsync(ta.cand_val, 0xff, sizeof(float) * (size_t)lcap * J, st));
        }
        ta.mode = form == 1 ? 1 : 0;
        launch_top_mma(ta, st);
    }
    HIP_TRY(hipGetLastError());
    if (want_maps) {
        std::vector<float> hm(P.map_floats * S);
        HIP_TRY(hipMemcpyAsync(hm.data(), P.d_map.p, sizeof(float) * hm.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int s = 0; s < S; ++s)
            for (int a = 0; a < nang; ++a)
                std::copy_n(hm.data() + P.map_floats * s + P.map_off[a], (size_t)P.map_w[a] * P.map_h[a],
                            maps + dense * s + dense_off[a]);
    } else {
        HIP_TRY(hipMemcpyAsync(list_count, ta.cand_cnt, sizeof(int32_t) * J, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(list_index, ta.cand, sizeof(int32_t) * (size_t)lcap * J, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(list_value, ta.cand_val, sizeof(float) * (size_t)lcap * J, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return FPM_OK;
}

// The fused top layer (k_top_fused) over the staged batch whatever the job count, by the plan's own job tables, job
// order and peak arguments (plan_nms_args): once as the product instantiation, once as the map-writing one.  Neither
// launch initialises candidates (ci = nullptr); the peaks and counts go to the operator's scratch, the maps to the
// plan's map scratch (NccJob::out), which a search of this form never reads.
int fpm_op_top_fused(fpm_ctx* ctx, int32_t* n_sources, int32_t* n_angles, int64_t* map_floats, int32_t* cap,
                     int32_t* geom, int32_t geom_cap, float* maps, int64_t maps_cap, fpm_peak* peaks, int32_t* counts,
                     fpm_peak* dump_peaks, int32_t* dump_counts, int64_t peak_slots, int32_t* stats) {
    if (!ctx) return FPM_E_INVALID_ARG;
    if (!ctx->learned) { ctx->err = "template not learned"; return FPM_E_NOT_LEARNED; }
    if (ctx->pending) { ctx->err = "a search is in flight (fpm_match_staged_finish first)"; return FPM_E_INVALID_ARG; }
    if (ctx->S <= 0 || !ctx->staged || !ctx->src_valid) { ctx->err = "top fused: no staged sources"; return FPM_E_INVALID_ARG; }
    const bool sizing = !geom && !maps && !peaks && !counts && !dump_peaks && !dump_counts;
    if (geom_cap < 0 || maps_cap < 0 || peak_slots < 0 ||
        (!sizing && (!geom || !maps || !peaks || !counts || !dump_peaks || !dump_counts))) {
        ctx->err = "bad top fused arguments";
        return FPM_E_INVALID_ARG;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    struct ProfOff {   // the launches below are not the search's: the profile counters stay as they were
        fpm_ctx* c; bool was;
        explicit ProfOff(fpm_ctx* x) : c(x), was(x->prof) { c->prof = false; }
        ~ProfOff() { c->prof = was; }
    } prof_off(ctx);
    int rc = build_plan(ctx);
    if (rc != FPM_OK) return rc;
    Plan& P = ctx->plan;
    const int S = P.S, nang = P.nang, J = S * nang;
    std::vector<size_t> dense_off(nang);
    size_t dense = 0;
    for (int a = 0; a < nang; ++a) { dense_off[a] = dense; dense += (size_t)P.map_w[a] * P.map_h[a]; }
    if (n_sources) *n_sources = S;
    if (n_angles) *n_angles = nang;
    if (map_floats) *map_floats = (int64_t)dense;
    if (cap) *cap = P.cap;
    size_t need = 0;
    const size_t lds = plan_top_fused_lds(ctx, &need);
    int copy_angles = 0;
    const TopFusedOpts opts = plan_top_fused_opts(ctx, &copy_angles);
    if (stats) {
        size_t chosen = 0;
        bool use_mma = false;
        plan_top_choice(ctx, &chosen, &use_mma);
        std::fill(stats, stats + FPM_TOP_FUSED_STATS, 0);
        stats[0] = (int32_t)need;
        stats[1] = (int32_t)top_fused_static_lds(false);
        stats[2] = (int32_t)top_fused_lds_limit();
        stats[3] = top_fused_grid(J);
        stats[4] = J;
        stats[5] = P.cap;
        stats[6] = chosen > 0 ? 1 : 0;
        stats[7] = (int32_t)top_fused_static_lds(true);
        stats[8] = copy_angles;
        stats[9] = opts.bound;
    }
    if (lds == 0 && J > 0) {
        ctx->err = "top fused: the plan cannot take the fused form (block mode, the template level or the LDS limit)";
        return FPM_E_SIZE;
    }
    if (sizing) return FPM_OK;
    const size_t slots = (size_t)J * P.cap;
    if (geom_cap < nang || (uint64_t)maps_cap < (uint64_t)dense * S || (uint64_t)peak_slots < (uint64_t)slots) {
        ctx->err = "top fused: output capacity below the sizing call's";
        return FPM_E_CAPACITY;
    }
    for (int a = 0; a < nang; ++a) {
        geom[4 * a + 0] = P.top[a].bw; geom[4 * a + 1] = P.top[a].bh;
        geom[4 * a + 2] = P.map_w[a]; geom[4 * a + 3] = P.map_h[a];
    }
    if (J <= 0) return FPM_OK;
    hipStream_t st = ctx->stream;
    // scratch: per launch [J][cap] peaks and [J] counts, uploaded from the caller's arrays so that a slot no kernel
    // writes comes back as the caller left it
    const size_t o_peaks[2] = {0, round_up(sizeof(Peak) * slots, (size_t)256)};
    const size_t o_counts[2] = {2 * o_peaks[1], 2 * o_peaks[1] + round_up(sizeof(int32_t) * J, (size_t)256)};
    HIP_TRY(ctx->d_op_b.ensure(o_counts[1] + sizeof(int32_t) * J));
    fpm_peak* hp_out[2] = {peaks, dump_peaks};
    int32_t* hc_out[2] = {counts, dump_counts};
    std::vector<Peak> hp[2];
    for (int v = 0; v < 2; ++v) {
        hp[v].resize(slots);
        for (size_t k = 0; k < slots; ++k) {
            Peak& q = hp[v][k];
            q.x = hp_out[v][k].x; q.y = hp_out[v][k].y; q.score = hp_out[v][k].score; q.pad = 0;
        }
        HIP_TRY(hipMemcpyAsync(ctx->d_op_b.as<char>(o_peaks[v]), hp[v].data(), sizeof(Peak) * slots, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->d_op_b.as<char>(o_counts[v]), hc_out[v], sizeof(int32_t) * J, hipMemcpyHostToDevice, st));
    }
    rc = apply_polarity(ctx);   // as start_staged, ahead of the pyramid
    if (rc != FPM_OK) return rc;
    // a pixel the map-writing launch leaves out reads back as a NaN pattern
    HIP_TRY(hipMemsetAsync(P.d_map.p, 0xff, sizeof(float) * P.map_floats * S, st));
    // as the search without the fused candidate init: the pyramid launches zero nothing, block 0 of the top kernel does
    enqueue_pyramid(ctx, false);
    for (int v = 0; v < 2; ++v) {
        NmsArgs na = plan_nms_args(ctx);
        na.peaks = ctx->d_op_b.as<Peak>(o_peaks[v]);
        na.counts = ctx->d_op_b.as<int32_t>(o_counts[v]);
        launch_top_fused(P.d_jobs.as<WarpJob>(P.off_warp), P.d_jobs.as<NccJob>(P.off_ncc), na, J, lds,
                         P.d_livecnt.as<int32_t>(), P.nzero, st, nullptr, P.d_jobs.as<int32_t>(P.off_order), v == 1,
                         opts);
        HIP_TRY(hipGetLastError());
    }
    std::vector<float> hm(P.map_floats * S);
    HIP_TRY(hipMemcpyAsync(hm.data(), P.d_map.p, sizeof(float) * hm.size(), hipMemcpyDeviceToHost, st));
    for (int v = 0; v < 2; ++v) {
        HIP_TRY(hipMemcpyAsync(hp[v].data(), ctx->d_op_b.as<char>(o_peaks[v]), sizeof(Peak) * slots, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(hc_out[v], ctx->d_op_b.as<char>(o_counts[v]), sizeof(int32_t) * J, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int s = 0; s < S; ++s)
        for (int a = 0; a < nang; ++a)
            std::copy_n(hm.data() + P.map_floats * s + P.map_off[a], (size_t)P.map_w[a] * P.map_h[a],
                        maps + dense * s + dense_off[a]);
    for (int v = 0; v < 2; ++v)
        for (size_t k = 0; k < slots; ++k) {
            fpm_peak& p = hp_out[v][k];
            const Peak& q = hp[v][k];
            p.x = q.x; p.y = q.y; p.score = q.score;
        }
    return FPM_OK;
}

// ---- profiling ----------------------------------------------------------------------------------------
int fpm_profile_enable(fpm_ctx* ctx, int32_t enable) {
    if (!ctx) return FPM_E_INVALID_ARG;
    ctx->prof = enable != 0;
    return FPM_OK;
}

int fpm_profile_reset(fpm_ctx* ctx) {
    if (!ctx) return FPM_E_INVALID_ARG;
    for (auto& k : ctx->kp) { k.ms = 0; k.launches = 0; k.bytes = 0; k.used = 0; }
    return FPM_OK;
}

int fpm_profile_last(const fpm_ctx* ctx, double* device_ms, double* host_ms, double* call_ms) {
    if (!ctx || !device_ms || !host_ms || !call_ms) return FPM_E_INVALID_ARG;
    *device_ms = ctx->last_device_ms;
    *host_ms = ctx->last_host_ms;
    *call_ms = ctx->last_call_ms;
    return FPM_OK;
}

int fpm_profile_get(const fpm_ctx* ctx, int32_t kernel, double* total_ms, int64_t* launches, int64_t* bytes) {
    if (!ctx || kernel < 0 || kernel >= FPM_K_COUNT || !total_ms || !launches || !bytes) return FPM_E_INVALID_ARG;
    *total_ms = ctx->kp[kernel].ms;
    *launches = ctx->kp[kernel].launches;
    *bytes = ctx->kp[kernel].bytes;
    return FPM_OK;
}

}  // extern "C"
