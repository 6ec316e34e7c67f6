// fpm_host.h — host-side stages of the search that are not data-parallel.
#pragma once
#include <functional>
#include <vector>

#include "../../include/fpm.h"
#include "fpm_geom.h"

namespace fpm {

// cv::RotatedRect (center, size, angle in degrees)
struct RRect {
    F2 c;
    float w, h, angle;
};

// s_MatchParameter subset carried through the host stages (DataStructures.h:58-94)
struct HostMatch {
    double ptx, pty;
    double score, angle;
    RRect rect;
    bool del;
    bool on_border;
    double vec[3][3];
    int32_t id;   // caller's index (fpm_op_overlap_filter)
};

RRect rrect_from3(F2 p1, F2 p2, F2 p3);                              // cv::RotatedRect(p1, p2, p3)
void rrect_corners(const RRect& r, F2 pt[4]);                        // cv::RotatedRect::points
bool rrect_pair_drops(const RRect& a, const RRect& b, double max_overlap);   // one pair of filterWithRotatedRect
int rrect_intersection(const RRect& a, const RRect& b, std::vector<F2>& pts);  // rotatedRectangleIntersection
void sort_pt_with_center(std::vector<F2>& pts);                      // TemplateMatcher.cpp:1093-1131
void sort_pt_with_center_keyed(std::vector<F2>& pts);                // the same with explicit acos keys (checks)
double contour_area(const std::vector<F2>& pts);                     // cv::contourArea
void filter_with_score(std::vector<HostMatch>& v, double score);     // TemplateMatcher.cpp:984-1000
void filter_with_rotated_rect(std::vector<HostMatch>& v, double max_overlap);  // :1133-1194
void subpix_estimation(const HostMatch* v, double* dx, double* dy, double* dangle,
                       double angle_step, int imax);                 // :1002-1072
bool score_big2small(const HostMatch& a, const HostMatch& b);        // compareScoreBig2Small (:14-17)
// runs fn(0 .. ntasks-1) on the host worker pool (FPM_HOST_THREADS, default min(hardware threads, 8)), caller included
void host_parallel(int ntasks, const std::function<void(int)>& fn);
int host_thread_count();   // threads host_parallel uses: FPM_HOST_THREADS, else the hardware concurrency capped at 8
// wake the pool's workers now and keep them spinning for `us` microseconds, so that a host tail expected after a device
// wait starts without the wake-up latency of sleeping threads
void host_pool_warm(int us);
// The tail of a blob entry (include/fpm.h, "defect blobs"), for one image: of the m candidate records in recs keep those
// with area >= min_area, sort them by seed, hand the first min(kept, cap) to out (out may be recs itself) with zeroed
// records behind them up to cap, and fill the summary.  missing = qualifying components that have no record in recs
// (0 for fpm_blobs_host, which passes every component; an entry with bounded record slots passes its overshoot); they
// count in n_blobs.  One function, so that every entry ends in the same filter, order, truncation and flags.
void blobs_tail(fpm_blob* recs, int64_t m, int64_t missing, int64_t fg_pixels, int32_t n_components, int32_t largest_area,
                int32_t min_area, int32_t cap, fpm_blob* out, fpm_blob_summary* summary);
// the argument rules the blob entries share; nullptr = fine, else what is wrong
const char* blobs_bad_args(int64_t n, int32_t level, int32_t connectivity, int32_t min_area, int32_t cap_per_hit);
// What one round of the device labelling leaves per image beside its records: the foreground
// pixels, all components, the qualifying ones (the true count, also beyond cap_dev) and the largest area.
struct BlobCounters {
    int32_t fg_pixels, n_components, n_qualifying, largest_area;
};
// Record slots per image of the device labelling: no w x h image has more components of at least min_area pixels than
// min(ceil(w h / 2), w h / min_area), so slots beyond that (or beyond cap_per_hit) would never be drawn.
int32_t blobs_cap_dev(int32_t w, int32_t h, int32_t min_area, int32_t cap_per_hit);
// One round's device output into the caller's memory, through blobs_tail: image i of the round has its first
// min(n_qualifying, cap_dev) records valid at recs + i * cap_dev (any order; sorted in place here) and goes to
// out + i * cap_per_hit and summary + i.  Pure host code: every write into caller memory of a device blob entry is here.
void blobs_gather(const BlobCounters* counters, fpm_blob* recs, int32_t images, int32_t cap_dev, int32_t min_area,
                  int32_t cap_per_hit, fpm_blob* out, fpm_blob_summary* summary);
// ---- edge calipers (include/fpm.h, "edge calipers"): the host half every caliper entry shares ----
// the range rules of one caliper; nullptr = fine, else what is wrong
const char* caliper_bad(const fpm_caliper& k);
// the sampling pose of caliper k on a hit at (lt, angle)
void caliper_pose(float lt_x, float lt_y, double angle, const fpm_caliper& k, float* ltk_x, float* ltk_y, double* angle_k);
// the step and edge rules on a profile of k.length entries: the first min(count, cap) raw records to out, zero-filled
// records behind them up to cap; returns the true count
int32_t caliper_edges(const int32_t* profile, const fpm_caliper& k, int32_t cap, fpm_edge_raw* out);
// one raw record of caliper k sampled at (ltk, angle_k) into *e; false (nothing written) for a record that is no edge
bool caliper_derive(const fpm_caliper& k, float ltk_x, float ltk_y, double angle_k, const fpm_edge_raw& r, fpm_edge* e);
// the returned record with the largest |d|, the earliest on ties; -1 for n = 0
int32_t caliper_strongest(const fpm_edge_raw* r, int32_t n);
// ---- edge probes (include/fpm.h, "edge probes"): the host half the probe entries share ----
// the range rules of a call's parameters and of one probe; nullptr = fine, else what is wrong
const char* probe_params_bad(const fpm_probe_params& p);
const char* probe_bad(const fpm_probe& k);
// what a probe contributes to the sampling matrix and the derivation: cos and sin of phi, the template point of
// sample (0, 0), hl and hw
struct ProbeGeom {
    double cp, sp, ox, oy, hl, hw;
};
ProbeGeom probe_geom(const fpm_probe& k, const fpm_probe_params& p);
// the step, edge and select rules on a profile of p.length entries into *out (flags = 0)
void probe_edges(const int32_t* profile, const fpm_probe_params& p, fpm_probe_raw* out);
// one raw record of a probe with geometry g on a hit at lt whose angle has the cos and sin (ca, sa) into *out; false
// (nothing written) for a record that is no edge.  The geometry is formed once per probe and the trig once per hit.
bool probe_derive(const ProbeGeom& g, const fpm_probe_params& p, float lt_x, float lt_y, double ca, double sa,
                  const fpm_probe_raw& r, fpm_probe_result* out);
// a hit's summary from its n results in ascending probe index
void probe_summarise(const fpm_probe_result* res, int32_t n, float lt_x, float lt_y, double angle, fpm_probe_summary* out);
// ---- gray-value tools (include/fpm.h, "gray-value tools") ----
// the statistics and Otsu's threshold of one histogram by the header's rule; false (nothing written) when its total
// exceeds 2^22
bool hist_derive(const uint32_t hist[256], fpm_hist_stats* out);
// ---- sub-pattern locators (include/fpm.h, "sub-pattern locators") ----
// the range rules of one feature that need no template (sizes, radii, reserved); nullptr = fine, else what is wrong
const char* feature_bad(const fpm_feature& f);
// fpm_compare_derive's zncc of the six sums, in its order
double locate_zncc(int64_t n, int64_t si, int64_t sii, int64_t st, int64_t stt, int64_t sit);
// sums, peak and raw record of one window against one template region (arguments checked by the caller); maps may be null
void locate_host(const uint8_t* window, size_t ws, const uint8_t* tmpl, size_t ts, int w, int h, int rx, int ry,
                 fpm_locate_raw* raw, int32_t* maps);
// one raw record into *out; false (nothing written) for a record no search of f can have produced
bool locate_derive(const fpm_feature& f, float lt_x, float lt_y, double angle, const fpm_locate_raw& r, fpm_locate_result* out);

}  // namespace fpm
