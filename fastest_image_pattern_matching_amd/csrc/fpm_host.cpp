// fpm_host.cpp — host stages of the search: final score filter, rotated-rectangle overlap suppression and the
// optional sub-pixel quadric fit.  These are O(n^2)/O(1) control code over a few hundred results, run once
// per search after the single device->host copy; they follow the reference line by line so that the surviving
// set and order are identical (TemplateMatcher.cpp:373-395, 984-1194) and the OpenCV geometry primitives
// they call (OpenCV 4.5.x semantics).  Compile with -ffp-contract=off.
#include "fpm_host.h"
#include "fpm_rrect.h"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <thread>

namespace fpm {
#ifdef FPM_HOST_STATS
long g_stats[40];
#endif

bool score_big2small(const HostMatch& a, const HostMatch& b) { return a.score > b.score; }

// worker threads for the overlap filter's independent components: FPM_HOST_THREADS if set (>= 1), else the
// hardware concurrency capped at 8
int host_thread_count() {
    static const int n = [] {
        if (const char* e = std::getenv("FPM_HOST_THREADS")) {
            const int v = std::atoi(e);
            if (v >= 1) return std::min(v, 64);
        }
        const int hw = (int)std::thread::hardware_concurrency();
        return std::max(1, std::min(hw, 8));
    }();
    return n;
}

// Persistent worker pool for the host tail's independent pieces (per-candidate geometry, per-cluster overlap
// tests).  Thread creation per search cost more than the work it spread; the workers spin for a short while after
// a region (the tail runs a few regions back to back) and then sleep on a condition variable.  One region at a time:
// a caller that finds the pool busy (another context finishing on another host thread) runs its tasks inline.
// Results never depend on which thread runs a task.
namespace {
// spin-wait hint: the x86 pause instruction where there is one, a scheduler yield elsewhere
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}

struct Pool {
    std::mutex m, region;
    std::condition_variable cv;
    std::atomic<uint64_t> gen{0};
    const std::function<void(int)>* fn = nullptr;   // guarded by m; null between regions
    int ntasks = 0;
    std::atomic<int> next{0}, done{0}, active{0};
    std::atomic<int64_t> spin_until{0};   // steady_clock ns: idle workers spin instead of sleeping until then

    static int64_t now_ns() {
        return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
            .count();
    }
    void worker() {
        uint64_t seen = 0;
        for (;;) {
            auto t0 = std::chrono::steady_clock::now();
            while (gen.load(std::memory_order_acquire) == seen) {
                if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(300) &&
                    now_ns() >= spin_until.load(std::memory_order_relaxed)) {
                    std::unique_lock<std::mutex> lk(m);
                    cv.wait(lk, [&] {
                        return gen.load(std::memory_order_acquire) != seen ||
                               now_ns() < spin_until.load(std::memory_order_relaxed);
                    });
                    t0 = std::chrono::steady_clock::now();
                } else {
                    cpu_relax();
                }
            }
            const std::function<void(int)>* f;
            int nt;
            {
                std::lock_guard<std::mutex> lk(m);
                seen = gen.load(std::memory_order_acquire);
                f = fn;
                nt = ntasks;
                if (f) active.fetch_add(1, std::memory_order_acq_rel);
            }
            if (!f) continue;
            for (int t = next.fetch_add(1); t < nt; t = next.fetch_add(1)) {
                (*f)(t);
                done.fetch_add(1, std::memory_order_acq_rel);
            }
            active.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
};

// Leaked on purpose: the detached workers block forever, nothing is torn down at exit -- so libfpm_hip.so must not be
// dlclose'd while the process lives (ctypes never unloads it; the drop-in links it)
Pool* pool_instance(int workers) {
    static Pool* p = [&] {
        Pool* q = new Pool;
        for (int i = 0; i < workers; ++i) std::thread([q] { q->worker(); }).detach();
        return q;
    }();
    return p;
}
}  // namespace

// FPM_HOST_WARM: 0 turns the warm-up off (processes sharing the host with other work), a positive value caps the
// spin in microseconds (default 10000); the warm-up only moves when the tail's workers start, never its results
static int host_warm_cap_us() {
    static const int cap = [] {
        const char* e = std::getenv("FPM_HOST_WARM");
        return e ? std::max(0, atoi(e)) : 10000;
    }();
    return cap;
}

void host_pool_warm(int us) {
    const int nthreads = host_thread_count();
    us = std::min(us, host_warm_cap_us());
    if (nthreads <= 1 || us <= 0) return;
    Pool* p = pool_instance(nthreads - 1);
    p->spin_until.store(Pool::now_ns() + (int64_t)us * 1000, std::memory_order_relaxed);
    std::lock_guard<std::mutex> lk(p->m);
    p->cv.notify_all();
}

void host_parallel(int ntasks, const std::function<void(int)>& fn) {
    const int nthreads = host_thread_count();
    if (ntasks <= 1 || nthreads <= 1) {
        for (int t = 0; t < ntasks; ++t) fn(t);
        return;
    }
    Pool* p = pool_instance(nthreads - 1);
    std::unique_lock<std::mutex> reg(p->region, std::try_to_lock);
    if (!reg.owns_lock()) {
        for (int t = 0; t < ntasks; ++t) fn(t);
        return;
    }
    {
        std::lock_guard<std::mutex> lk(p->m);
        p->fn = &fn;
        p->ntasks = ntasks;
        p->next.store(0);
        p->done.store(0);
        p->gen.fetch_add(1, std::memory_order_acq_rel);
    }
    p->cv.notify_all();
    static const bool trace = [] { const char* e = std::getenv("FPM_POOL_TRACE"); return e && *e == '1'; }();
    const auto r0 = std::chrono::steady_clock::now();
    int mine = 0;
    for (int t = p->next.fetch_add(1); t < ntasks; t = p->next.fetch_add(1)) {
        fn(t);
        ++mine;
        p->done.fetch_add(1, std::memory_order_acq_rel);
    }
    while (p->done.load(std::memory_order_acquire) < ntasks) cpu_relax();
    {
        std::lock_guard<std::mutex> lk(p->m);
        p->fn = nullptr;   // workers that wake from here on skip this region
    }
    while (p->active.load(std::memory_order_acquire) > 0) cpu_relax();
    if (trace)
        fprintf(stderr, "pool region: %d tasks, %d by the caller, %.1f us\n", ntasks, mine,
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - r0).count());
}

static inline double len2(float x, float y) { return std::sqrt((double)x * x + (double)y * y); }

RRect rrect_from3(F2 p1, F2 p2, F2 p3) {
    RRect r;
    r.c = f2(0.5f * (p1.x + p3.x), 0.5f * (p1.y + p3.y));
    const F2 e0 = f2(p1.x - p2.x, p1.y - p2.y);
    const F2 e1 = f2(p2.x - p3.x, p2.y - p3.y);
    // width = the edge whose slope lies in [-1, 1]; preference to e1 as in OpenCV
    const bool w_is_e1 = std::fabs(e1.y) < std::fabs(e1.x);
    const F2 we = w_is_e1 ? e1 : e0, he = w_is_e1 ? e0 : e1;
    r.angle = std::atan(we.y / we.x) * 180.0f / (float)kPi;
    r.w = (float)len2(we.x, we.y);
    r.h = (float)len2(he.x, he.y);
    return r;
}

void rrect_corners(const RRect& r, F2 pt[4]) {
    const double rad = r.angle * kPi / 180.;
    const float b = (float)std::cos(rad) * 0.5f;
    const float a = (float)std::sin(rad) * 0.5f;
    pt[0] = f2(r.c.x - a * r.h - b * r.w, r.c.y + b * r.h - a * r.w);
    pt[1] = f2(r.c.x + a * r.h - b * r.w, r.c.y - b * r.h - a * r.w);
    pt[2] = f2(2 * r.c.x - pt[0].x, 2 * r.c.y - pt[0].y);
    pt[3] = f2(2 * r.c.x - pt[1].x, 2 * r.c.y - pt[1].y);
}

// cv::rotatedRectangleIntersection on precomputed corners (fpm_rrect.h, shared with the device pair kernel)
static int rrect_isect(const RRect& ra, const RRect& rb, const F2* A, const F2* B, F2* pts, int* np) {
    return rrect_isect_pts(ra.w, ra.h, rb.w, rb.h, A, B, pts, np);
}

int rrect_intersection(const RRect& ra, const RRect& rb, std::vector<F2>& pts) {
    F2 A[4], B[4], p[24];
    rrect_corners(ra, A);
    rrect_corners(rb, B);
    int n = 0;
    const int kind = rrect_isect(ra, rb, A, B, p, &n);
    pts.assign(p, p + n);
    return kind;
}

// sortPtWithCenter (TemplateMatcher.cpp:1093-1131) with its own keys: acos(x) * R2D above the centre, 360 - that
// below, x = dot / |v|^2 (the squared norm is the reference's), 0 / 180 on the centre's row; std::sort by key.
static void sort_pts_keyed(F2* pts, int n) {
    F2 ctr = f2(0.f, 0.f);
    for (int i = 0; i < n; ++i) { ctr.x += pts[i].x; ctr.y += pts[i].y; }
    ctr.x = ctr.x / n;
    ctr.y = ctr.y / n;
    std::pair<F2, double> keyed[24];   // n <= 24 (rrect_isect)
    for (int i = 0; i < n; ++i) {
        const F2 d = f2(pts[i].x - ctr.x, pts[i].y - ctr.y);
        const float nn = d.x * d.x + d.y * d.y;
        double key;
        if (d.y < 0) key = std::acos(d.x / nn) * kR2D;
        else if (d.y > 0) key = 360 - std::acos(d.x / nn) * kR2D;
        else key = (d.x - ctr.x > 0) ? 0 : 180;
        keyed[i] = std::make_pair(pts[i], key);
    }
    std::sort(keyed, keyed + n,
              [](const std::pair<F2, double> l, const std::pair<F2, double> r) { return l.second < r.second; });
    for (int i = 0; i < n; ++i) pts[i] = keyed[i].first;
}

// The same permutation without a transcendental per point.  For n <= 16 libstdc++'s std::sort is one insertion
// sort (introsort stops at 16 elements), so the result depends only on the outcomes of `key_a < key_b`.  With every
// off-row |x| <= 1/2 the keys fall in disjoint bands -- row-left 0 < above (60..120) < row-right 180 < below
// (240..300) -- and within a band acos is strictly monotone with slope >= 1 in magnitude, so two x at least 2^-16
// apart have keys ordered as their x (acosf's error is a few ulp of at most 2^-22); only closer pairs, which may
// round to equal keys, compare acosf results exactly as the key does (both keys are monotone in the float acosf).
// Anything outside that envelope takes the keyed path.
static void sort_pts_center(F2* pts, int n) {
    if (n > 16) { sort_pts_keyed(pts, n); return; }
    F2 ctr = f2(0.f, 0.f);
    for (int i = 0; i < n; ++i) { ctr.x += pts[i].x; ctr.y += pts[i].y; }
    ctr.x = ctr.x / n;
    ctr.y = ctr.y / n;
    struct E { F2 p; float x; int band; };
    E e[16];
    for (int i = 0; i < n; ++i) {
        const F2 d = f2(pts[i].x - ctr.x, pts[i].y - ctr.y);
        e[i].p = pts[i];
        e[i].x = 0.f;
        if (d.y < 0 || d.y > 0) {
            const float nn = d.x * d.x + d.y * d.y;
            const float x = d.x / nn;
            if (!(std::fabs(x) <= 0.5f)) { sort_pts_keyed(pts, n); return; }
            e[i].x = x;
            e[i].band = d.y < 0 ? 1 : 3;
        } else {
            e[i].band = (d.x - ctr.x > 0) ? 0 : 2;
        }
    }
    auto less = [](const E& a, const E& b) {
        if (a.band != b.band) return a.band < b.band;
        if (a.band == 0 || a.band == 2) return false;
        if (std::fabs(a.x - b.x) >= 0x1p-16f) return a.band == 1 ? a.x > b.x : a.x < b.x;
        const float fa = std::acos(a.x), fb = std::acos(b.x);
        return a.band == 1 ? fa < fb : fa > fb;
    };
    for (int i = 1; i < n; ++i) {   // libstdc++ __insertion_sort
        const E v = e[i];
        int j = i;
        while (j > 0 && less(v, e[j - 1])) { e[j] = e[j - 1]; --j; }
        e[j] = v;
    }
    for (int i = 0; i < n; ++i) pts[i] = e[i].p;
}

void sort_pt_with_center(std::vector<F2>& pts) {
    if (!pts.empty()) sort_pts_center(pts.data(), (int)pts.size());
}

void sort_pt_with_center_keyed(std::vector<F2>& pts) {
    if (!pts.empty()) sort_pts_keyed(pts.data(), (int)pts.size());
}

static double contour_area_a(const F2* pts, int n) { return contour_area_pts(pts, n); }

double contour_area(const std::vector<F2>& pts) { return contour_area_a(pts.data(), (int)pts.size()); }

// filterWithRotatedRect's decision for one pair (pair_del below, without the score rule): does a's overlap with b
// exceed max_overlap (ratio to a's area)
bool rrect_pair_drops(const RRect& ra, const RRect& rb, double max_overlap) {
    F2 A[4], B[4], p[24];
    rrect_corners(ra, A);
    rrect_corners(rb, B);
    int np = 0;
    const int kind = rrect_isect(ra, rb, A, B, p, &np);
    if (kind == 0) return false;
    if (kind == 2) return true;
    if (np < 3) return false;
    sort_pts_center(p, np);
    return contour_area_a(p, np) / (ra.w * ra.h) > max_overlap;
}


void filter_with_score(std::vector<HostMatch>& v, double score) {
    // std::sort's permutation depends only on the comparison results, so sorting light (score, index) keys with
    // the same comparator reproduces the reference's order of equal scores; the heavy records move once
    struct K { double score; int i; };
    std::vector<K> k(v.size());
    for (size_t i = 0; i < v.size(); ++i) k[i] = {v[i].score, (int)i};
    std::sort(k.begin(), k.end(), [](const K& a, const K& b) { return a.score > b.score; });
    size_t n = 0;
    while (n < k.size() && !(k[n].score < score)) ++n;
    std::vector<HostMatch> out;
    out.reserve(n);
    for (size_t i = 0; i < n; ++i) out.push_back(v[k[i].i]);
    v.swap(out);
}

void filter_with_rotated_rect(std::vector<HostMatch>& v, double max_overlap) {
    if (v.empty()) return;
    const int n = (int)v.size();
    // FPM_TAIL_TIMES=1: phase clocks on stderr (profiling aid)
    static const bool tail_times = [] { const char* e = std::getenv("FPM_TAIL_TIMES"); return e && *e == '1'; }();
    using clk = std::chrono::steady_clock;
    const clk::time_point q0 = clk::now();
    clk::time_point q1 = q0, q2 = q0, q3 = q0;
    // corner bounding boxes: pairs whose boxes are > 1 px apart cannot have an edge crossing or a contained corner,
    // so rrect_intersection would return INTERSECT_NONE; skipping them keeps the reference's O(n^2) loop order
    // and deletions exactly while avoiding the exact test for far-apart detections
    std::vector<float> box((size_t)4 * n);
    std::vector<F2> corners((size_t)4 * n);
    auto geom = [&](int i0, int i1) {
        for (int i = i0; i < i1; ++i) {
            F2* c = &corners[(size_t)4 * i];
            rrect_corners(v[i].rect, c);
            float x0 = c[0].x, x1 = c[0].x, y0 = c[0].y, y1 = c[0].y;
            for (int k = 1; k < 4; ++k) {
                x0 = std::min(x0, c[k].x); x1 = std::max(x1, c[k].x);
                y0 = std::min(y0, c[k].y); y1 = std::max(y1, c[k].y);
            }
            box[4 * i] = x0 - 1.f; box[4 * i + 1] = y0 - 1.f; box[4 * i + 2] = x1 + 1.f; box[4 * i + 3] = y1 + 1.f;
        }
    };
    if (n <= 512) geom(0, n);
    else host_parallel((n + 511) / 512, [&](int t) { geom(t * 512, std::min(n, t * 512 + 512)); });
    q1 = clk::now();
    // the reference's inner-loop body for (i, j), boxes overlapping: the index it deletes, or -1
    auto pair_del = [&](int i, int j) {
        F2 pts[24];
        int np = 0;
        const int kind = rrect_isect(v[i].rect, v[j].rect, &corners[(size_t)4 * i], &corners[(size_t)4 * j], pts, &np);
#ifdef FPM_HOST_STATS
        g_stats[kind]++; g_stats[3 + np]++;
#endif
        if (kind == 0) return -1;
        bool drop = kind == 2;
        if (kind == 1) {
            if (np < 3) return -1;
            sort_pts_center(pts, np);
            const double ratio = contour_area_a(pts, np) / (v[i].rect.w * v[i].rect.h);
            drop = ratio > max_overlap;
        }
        return drop ? ((v[i].score >= v[j].score) ? j : i) : -1;
    };
    auto pair = [&](int i, int j) {
        const int d = pair_del(i, j);
        if (d >= 0) v[d].del = true;
    };
    auto overlap = [&](int i, int j) {
        const float* bi = &box[4 * i];
        const float* bj = &box[4 * j];
        return !(bj[0] > bi[2] || bj[2] < bi[0] || bj[1] > bi[3] || bj[3] < bi[1]);
    };
    if (n <= 64) {
        for (int i = 0; i + 1 < n; ++i) {
            if (v[i].del) continue;
            for (int j = i + 1; j < n; ++j)
                if (!v[j].del && overlap(i, j)) pair(i, j);
        }
    } else {
        // uniform grid over the boxes (cell = the largest box extent): for each i only the j > i whose boxes
        // overlap its box, in ascending order -- the same (i, j) sequence as the full loop minus no-op pairs
        float gx0 = box[0], gy0 = box[1], gx1 = box[2], gy1 = box[3], cs = 1.f;
        for (int i = 0; i < n; ++i) {
            gx0 = std::min(gx0, box[4 * i]); gy0 = std::min(gy0, box[4 * i + 1]);
            gx1 = std::max(gx1, box[4 * i + 2]); gy1 = std::max(gy1, box[4 * i + 3]);
            cs = std::max(cs, std::max(box[4 * i + 2] - box[4 * i], box[4 * i + 3] - box[4 * i + 1]));
        }
        const int gnx = std::min(1024, (int)((gx1 - gx0) / cs) + 1), gny = std::min(1024, (int)((gy1 - gy0) / cs) + 1);
        const float sx = gnx / std::max(gx1 - gx0, 1e-3f), sy = gny / std::max(gy1 - gy0, 1e-3f);
        auto cell = [&](float x, float s_, float o, int nmax) { return std::min(nmax - 1, std::max(0, (int)((x - o) * s_))); };
        // cell -> ascending box indices, as CSR (count, prefix sum, fill)
        const size_t ncell = (size_t)gnx * gny;
        std::vector<int> cell_off(ncell + 1, 0), cell_box;
        std::vector<int4> span(n);   // cx0, cy0, cx1, cy1 per box
        for (int i = 0; i < n; ++i) {
            span[i] = make_int4(cell(box[4 * i], sx, gx0, gnx), cell(box[4 * i + 1], sy, gy0, gny),
                                cell(box[4 * i + 2], sx, gx0, gnx), cell(box[4 * i + 3], sy, gy0, gny));
            for (int cy = span[i].y; cy <= span[i].w; ++cy)
                for (int cx = span[i].x; cx <= span[i].z; ++cx) cell_off[(size_t)cy * gnx + cx + 1]++;
        }
        for (size_t c = 0; c < ncell; ++c) cell_off[c + 1] += cell_off[c];
        cell_box.resize(cell_off[ncell]);
        {
            std::vector<int> fill(cell_off.begin(), cell_off.end() - 1);
            for (int i = 0; i < n; ++i)
                for (int cy = span[i].y; cy <= span[i].w; ++cy)
                    for (int cx = span[i].x; cx <= span[i].z; ++cx) cell_box[fill[(size_t)cy * gnx + cx]++] = i;
        }
        // v is sorted by descending score, so pair(i, j) with i < j only ever deletes j: i is decided by the pairs
        // (i', i), i' < i, with overlapping boxes.  Overlapping boxes share a grid cell, so the sets of boxes
        // connected through shared cells are closed under the overlap relation and independent of each other; they
        // are processed in parallel, each in the reference's ascending (i, j) order -- the same deletions exactly.
        std::vector<int> root(n);
        for (int i = 0; i < n; ++i) root[i] = i;
        auto find = [&](int x) { while (root[x] != x) { root[x] = root[root[x]]; x = root[x]; } return x; };
        for (size_t c = 0; c < ncell; ++c)
            for (int k = cell_off[c] + 1; k < cell_off[c + 1]; ++k) {
                const int a = find(cell_box[cell_off[c]]), b = find(cell_box[k]);
                if (a != b) root[std::max(a, b)] = std::min(a, b);
            }
        std::vector<int> comp_of(n, -1), comp_off, members, comp_size;
        int ncomp = 0;
        for (int i = 0; i < n; ++i) {
            const int r = find(i);
            if (comp_of[r] < 0) { comp_of[r] = ncomp++; comp_size.push_back(0); }
            comp_of[i] = comp_of[r];
            comp_size[comp_of[i]]++;
        }
        comp_off.assign(ncomp + 1, 0);
        for (int c = 0; c < ncomp; ++c) comp_off[c + 1] = comp_off[c] + comp_size[c];
        members.resize(n);
        {
            std::vector<int> fill(comp_off.begin(), comp_off.end() - 1);
            for (int i = 0; i < n; ++i) members[fill[comp_of[i]]++] = i;   // ascending within a component
        }
        // a box's position inside its component (members ascending): the components keep their deletion flags in
        // private arrays while they run and write them back at the end, so workers never share a written cache line
        std::vector<int> local(n);
        for (int c = 0; c < ncomp; ++c)
            for (int k = comp_off[c]; k < comp_off[c + 1]; ++k) local[members[k]] = k - comp_off[c];
        q2 = clk::now();
        auto run_comp = [&](int c, std::vector<int>& nb, std::vector<char>& del) {
            const int m0 = comp_off[c], m1 = comp_off[c + 1];
            del.assign(m1 - m0, 0);
            for (int k = m0; k < m1; ++k) {
                const int i = members[k];
                if (del[k - m0]) continue;
                nb.clear();
                for (int cy = span[i].y; cy <= span[i].w; ++cy)
                    for (int cx = span[i].x; cx <= span[i].z; ++cx) {
                        const size_t c = (size_t)cy * gnx + cx;
                        for (int k = cell_off[c]; k < cell_off[c + 1]; ++k)
                            if (cell_box[k] > i) nb.push_back(cell_box[k]);
                    }
                std::sort(nb.begin(), nb.end());
                nb.erase(std::unique(nb.begin(), nb.end()), nb.end());
                for (int j : nb)
                    if (!del[local[j]] && overlap(i, j)) {
                        const int d = pair_del(i, j);
                        if (d >= 0) del[local[d]] = 1;
                    }
            }
            for (int k = m0; k < m1; ++k)
                if (del[k - m0]) v[members[k]].del = true;
        };
        // workers only where there is exact-test work to spread (clusters of duplicate detections)
        if (ncomp < 8 || n - ncomp < 64) {
            std::vector<int> nb;
            std::vector<char> del;
            for (int c = 0; c < ncomp; ++c) run_comp(c, nb, del);
        } else {
            host_parallel(ncomp, [&](int c) {
                thread_local std::vector<int> nb;
                thread_local std::vector<char> del;
                run_comp(c, nb, del);
            });
        }
        q3 = clk::now();
        if (tail_times)
            fprintf(stderr, "overlap n=%d comps=%d geom %.3f grid+comps %.3f tests %.3f ms\n", n, ncomp,
                    std::chrono::duration<double, std::milli>(q1 - q0).count(),
                    std::chrono::duration<double, std::milli>(q2 - q1).count(),
                    std::chrono::duration<double, std::milli>(q3 - q2).count());
    }
    v.erase(std::remove_if(v.begin(), v.end(), [](const HostMatch& m) { return m.del; }), v.end());
}

// (A^T A)^-1 by LU with partial pivoting (cv::invert, DECOMP_LU -> hal::LU64f), n x n, row-major.
static bool invert_lu(std::vector<double> a, int n, std::vector<double>& inv) {
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) inv[(size_t)i * n + i] = 1.0;
    for (int i = 0; i < n; ++i) {
        int piv = i;
        for (int r = i + 1; r < n; ++r)
            if (std::fabs(a[(size_t)r * n + i]) > std::fabs(a[(size_t)piv * n + i])) piv = r;
        if (std::fabs(a[(size_t)piv * n + i]) < DBL_EPSILON * 100) return false;
        if (piv != i) {
            for (int c = i; c < n; ++c) std::swap(a[(size_t)i * n + c], a[(size_t)piv * n + c]);
            for (int c = 0; c < n; ++c) std::swap(inv[(size_t)i * n + c], inv[(size_t)piv * n + c]);
        }
        const double d = -1 / a[(size_t)i * n + i];
        for (int r = i + 1; r < n; ++r) {
            const double alpha = a[(size_t)r * n + i] * d;
            for (int c = i + 1; c < n; ++c) a[(size_t)r * n + c] += alpha * a[(size_t)i * n + c];
            for (int c = 0; c < n; ++c) inv[(size_t)r * n + c] += alpha * inv[(size_t)i * n + c];
        }
    }
    for (int i = n - 1; i >= 0; --i)
        for (int c = 0; c < n; ++c) {
            double s = inv[(size_t)i * n + c];
            for (int k = i + 1; k < n; ++k) s -= a[(size_t)i * n + k] * inv[(size_t)k * n + c];
            inv[(size_t)i * n + c] = s / a[(size_t)i * n + i];
        }
    return true;
}

void subpix_estimation(const HostMatch* v, double* dx, double* dy, double* dangle, double angle_step,
                       int imax) {
    double A[27][10], S[27];
    const double x0 = v[imax].ptx, y0 = v[imax].pty, t0 = v[imax].angle;
    int row = 0;
    for (int th = 0; th <= 2; ++th)
        for (int y = -1; y <= 1; ++y)
            for (int x = -1; x <= 1; ++x, ++row) {
                const double X = x0 + x, Y = y0 + y, T = (t0 + (th - 1) * angle_step) * kD2R;
                const double r[10] = {X * X, Y * Y, T * T, X * Y, X * T, Y * T, X, Y, T, 1.0};
                for (int k = 0; k < 10; ++k) A[row][k] = r[k];
                S[row] = v[imax + (th - 1)].vec[x + 1][y + 1];
            }
    std::vector<double> ata(100), inv;
    for (int i = 0; i < 10; ++i)
        for (int j = 0; j < 10; ++j) {
            double s = 0;
            for (int r = 0; r < 27; ++r) s += A[r][i] * A[r][j];
            ata[(size_t)i * 10 + j] = s;
        }
    if (!invert_lu(ata, 10, inv)) inv.assign(100, 0.0);
    double Z[10];
    std::vector<double> ia(10 * 27);
    for (int i = 0; i < 10; ++i)
        for (int r = 0; r < 27; ++r) {
            double s = 0;
            for (int k = 0; k < 10; ++k) s += inv[(size_t)i * 10 + k] * A[r][k];
            ia[(size_t)i * 27 + r] = s;
        }
    for (int i = 0; i < 10; ++i) {
        double s = 0;
        for (int r = 0; r < 27; ++r) s += ia[(size_t)i * 27 + r] * S[r];
        Z[i] = s;
    }
    const double K[3][3] = {{2 * Z[0], Z[3], Z[4]}, {Z[3], 2 * Z[1], Z[5]}, {Z[4], Z[5], 2 * Z[2]}};
    const double rhs[3] = {-Z[6], -Z[7], -Z[8]};
    // closed-form 3x3 inverse (cv::invert for n == 3)
    double det = K[0][0] * (K[1][1] * K[2][2] - K[1][2] * K[2][1]) - K[0][1] * (K[1][0] * K[2][2] - K[1][2] * K[2][0]) +
                 K[0][2] * (K[1][0] * K[2][1] - K[1][1] * K[2][0]);
    double t[9] = {0};
    if (det != 0.) {
        det = 1. / det;
        t[0] = (K[1][1] * K[2][2] - K[1][2] * K[2][1]) * det;
        t[1] = (K[0][2] * K[2][1] - K[0][1] * K[2][2]) * det;
        t[2] = (K[0][1] * K[1][2] - K[0][2] * K[1][1]) * det;
        t[3] = (K[1][2] * K[2][0] - K[1][0] * K[2][2]) * det;
        t[4] = (K[0][0] * K[2][2] - K[0][2] * K[2][0]) * det;
        t[5] = (K[0][2] * K[1][0] - K[0][0] * K[1][2]) * det;
        t[6] = (K[1][0] * K[2][1] - K[1][1] * K[2][0]) * det;
        t[7] = (K[0][1] * K[2][0] - K[0][0] * K[2][1]) * det;
        t[8] = (K[0][0] * K[1][1] - K[0][1] * K[1][0]) * det;
    }
    *dx = t[0] * rhs[0] + t[1] * rhs[1] + t[2] * rhs[2];
    *dy = t[3] * rhs[0] + t[4] * rhs[1] + t[5] * rhs[2];
    *dangle = (t[6] * rhs[0] + t[7] * rhs[1] + t[8] * rhs[2]) * kR2D;
}

// ---- defect blobs (include/fpm.h, "defect blobs") ----
const char* blobs_bad_args(int64_t n, int32_t level, int32_t connectivity, int32_t min_area, int32_t cap_per_hit) {
    if (level < 0 || level > 254) return "level must be 0 .. 254";
    if (connectivity != 4 && connectivity != 8) return "connectivity must be 4 or 8";
    if (min_area < 1) return "min_area must be at least 1";
    if (cap_per_hit < 1 || cap_per_hit > FPM_BLOBS_MAX_CAP) return "cap_per_hit must be 1 .. 65536";
    if (n * cap_per_hit > FPM_BLOBS_MAX_SLOTS) return "more than 2^22 record slots (n x cap_per_hit)";
    return nullptr;
}

void blobs_tail(fpm_blob* recs, int64_t m, int64_t missing, int64_t fg_pixels, int32_t n_components, int32_t largest_area,
                int32_t min_area, int32_t cap, fpm_blob* out, fpm_blob_summary* summary) {
    int64_t kept = 0;
    for (int64_t i = 0; i < m; ++i)
        if (recs[i].area >= min_area) recs[kept++] = recs[i];
    std::sort(recs, recs + kept, [](const fpm_blob& a, const fpm_blob& b) { return a.seed < b.seed; });
    const int64_t n_blobs = kept + missing, n_ret = std::min<int64_t>(kept, cap);
    if (out != recs) std::copy(recs, recs + n_ret, out);
    std::fill(out + n_ret, out + cap, fpm_blob{});
    summary->fg_pixels = fg_pixels;
    summary->n_components = n_components;
    summary->n_blobs = (int32_t)n_blobs;
    summary->n_returned = (int32_t)n_ret;
    summary->largest_area = largest_area;
    summary->flags = n_blobs > cap ? FPM_BLOBS_TRUNCATED : 0;
    summary->reserved = 0;
}

int32_t blobs_cap_dev(int32_t w, int32_t h, int32_t min_area, int32_t cap_per_hit) {
    const int64_t px = (int64_t)w * h;
    return (int32_t)std::min<int64_t>(cap_per_hit, std::max<int64_t>(1, std::min((px + 1) / 2, px / min_area)));
}

void blobs_gather(const BlobCounters* counters, fpm_blob* recs, int32_t images, int32_t cap_dev, int32_t min_area,
                  int32_t cap_per_hit, fpm_blob* out, fpm_blob_summary* summary) {
    for (int32_t i = 0; i < images; ++i) {
        const BlobCounters& c = counters[i];
        const int64_t valid = std::min<int64_t>(std::max(c.n_qualifying, 0), cap_dev);
        blobs_tail(recs + (size_t)i * cap_dev, valid, c.n_qualifying - valid, c.fg_pixels, c.n_components, c.largest_area,
                   min_area, cap_per_hit, out + (size_t)i * cap_per_hit, summary + i);
    }
}

// ---- edge calipers (include/fpm.h, "edge calipers").  The file is built with -ffp-contract=off: every product and sum
// below is rounded on its own, in the header's order.
const char* caliper_bad(const fpm_caliper& k) {
    if (!std::isfinite(k.cx) || !std::isfinite(k.cy) || !std::isfinite(k.phi)) return "caliper: cx, cy and phi must be finite";
    if (k.length < 2 || k.length > FPM_CALIPER_MAX_LENGTH) return "caliper: length must be 2 .. 1024";
    if (k.width < 1 || k.width > FPM_CALIPER_MAX_WIDTH) return "caliper: width must be 1 .. 256";
    if (k.half < 1 || k.half > FPM_CALIPER_MAX_HALF || 2 * k.half > k.length) return "caliper: half must be 1 .. 16 with 2 half <= length";
    if (k.contrast < 1 || k.contrast > 255) return "caliper: contrast must be 1 .. 255";
    if (k.polarity < -1 || k.polarity > 1) return "caliper: polarity must be +1, -1 or 0";
    if (k.reserved != 0) return "caliper: reserved must be 0";
    return nullptr;
}

namespace {
// the template point of sample (0, 0), the scan direction's cos and sin, and hw
struct CaliperFrame {
    double ox, oy, cp, sp, hw;
};
CaliperFrame caliper_frame(const fpm_caliper& k) {
    const double hl = (k.length - 1) / 2.0, hw = (k.width - 1) / 2.0;
    const double rp = k.phi * kD2R, cp = std::cos(rp), sp = std::sin(rp);
    return {k.cx - (hl * cp - hw * sp), k.cy - (hl * sp + hw * cp), cp, sp, hw};
}
}  // namespace

void caliper_pose(float lt_x, float lt_y, double angle, const fpm_caliper& k, float* ltk_x, float* ltk_y, double* angle_k) {
    const CaliperFrame f = caliper_frame(k);
    const double ra = angle * kD2R, c = std::cos(ra), s = std::sin(ra);
    *ltk_x = (float)((double)lt_x + (f.ox * c - f.oy * s));
    *ltk_y = (float)((double)lt_y + (f.ox * s + f.oy * c));
    *angle_k = angle + k.phi;
}

int32_t caliper_edges(const int32_t* profile, const fpm_caliper& k, int32_t cap, fpm_edge_raw* out) {
    const int L = k.length, s = k.half, thr = k.contrast * k.half * k.width;
    std::vector<int32_t> D((size_t)L + 1, 0);   // D[0 .. L], 0 outside s .. L - s
    for (int i = s; i <= L - s; ++i) {
        int32_t d = 0;
        for (int j = 0; j < s; ++j) d += profile[i + j] - profile[i - 1 - j];
        D[i] = d;
    }
    int32_t n = 0;
    for (int i = s; i <= L - s; ++i) {
        const int32_t d = D[i], dp = D[i - 1], dn = D[i + 1];
        const bool up = d >= thr && d > dp && d >= dn, down = -d >= thr && d < dp && d <= dn;
        if (!((k.polarity >= 0 && up) || (k.polarity <= 0 && down))) continue;
        if (n < cap) out[n] = fpm_edge_raw{i, dp, d, dn};
        ++n;
    }
    for (int32_t i = std::min(n, cap); i < cap; ++i) out[i] = fpm_edge_raw{0, 0, 0, 0};
    return n;
}

bool caliper_derive(const fpm_caliper& k, float ltk_x, float ltk_y, double angle_k, const fpm_edge_raw& r, fpm_edge* e) {
    if (r.d == 0 || r.index < k.half || r.index > k.length - k.half) return false;
    const int64_t g = r.d > 0 ? 1 : -1;
    const int64_t am = g * r.d_prev, a0 = g * r.d, ap = g * r.d_next;
    if (!(am < a0 && ap <= a0)) return false;   // the local-maximum rule: den < 0 and delta in (-0.5, 0.5] follow
    const int64_t den = (am - a0) + (ap - a0);
    const CaliperFrame f = caliper_frame(k);
    const double delta = 0.5 * (double)(am - ap) / (double)den;
    const double t = ((double)r.index - 0.5) + delta;
    const double rk = angle_k * kD2R, ck = std::cos(rk), sk = std::sin(rk);
    e->index = r.index; e->d_prev = r.d_prev; e->d = r.d; e->d_next = r.d_next;
    e->t = t;
    e->contrast = (double)a0 / (double)(k.half * k.width);
    e->tx = f.ox + (t * f.cp - f.hw * f.sp);
    e->ty = f.oy + (t * f.sp + f.hw * f.cp);
    e->sx = (double)ltk_x + (t * ck - f.hw * sk);
    e->sy = (double)ltk_y + (t * sk + f.hw * ck);
    return true;
}

int32_t caliper_strongest(const fpm_edge_raw* r, int32_t n) {
    int32_t best = -1;
    int64_t top = -1;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t a = r[i].d < 0 ? -(int64_t)r[i].d : (int64_t)r[i].d;
        if (a > top) { top = a; best = i; }
    }
    return best;
}

// ---- edge probes (include/fpm.h, "edge probes"): every product and sum below is rounded on its own, in the header's
// order.
const char* probe_params_bad(const fpm_probe_params& p) {
    if (p.length < FPM_PROBE_MIN_LENGTH || p.length > FPM_PROBE_MAX_LENGTH) return "probe: length must be 4 .. 64";
    if (p.width < 1 || p.width > FPM_PROBE_MAX_WIDTH) return "probe: width must be 1 .. 16";
    if (p.half < 1 || p.half > FPM_PROBE_MAX_HALF || 2 * p.half > p.length) return "probe: half must be 1 .. 8 with 2 half <= length";
    if (p.contrast < 1 || p.contrast > 255) return "probe: contrast must be 1 .. 255";
    if (p.polarity < -1 || p.polarity > 1) return "probe: polarity must be +1, -1 or 0";
    if (p.select < FPM_PROBE_NEAREST || p.select > FPM_PROBE_LAST) return "probe: unknown select rule";
    if (p.reserved[0] != 0 || p.reserved[1] != 0) return "probe: reserved must be 0";
    return nullptr;
}

const char* probe_bad(const fpm_probe& k) {
    if (!std::isfinite(k.x) || !std::isfinite(k.y) || !std::isfinite(k.phi)) return "probe: x, y and phi must be finite";
    return nullptr;
}

ProbeGeom probe_geom(const fpm_probe& k, const fpm_probe_params& p) {
    const double hl = (p.length - 1) / 2.0, hw = (p.width - 1) / 2.0;
    const double rp = k.phi * kD2R, cp = std::cos(rp), sp = std::sin(rp);
    return {cp, sp, k.x - (hl * cp - hw * sp), k.y - (hl * sp + hw * cp), hl, hw};
}

void probe_edges(const int32_t* profile, const fpm_probe_params& p, fpm_probe_raw* out) {
    const int L = p.length, s = p.half, thr = p.contrast * p.half * p.width;
    int32_t D[FPM_PROBE_MAX_LENGTH + 1] = {};   // D[0 .. L], 0 outside s .. L - s
    for (int i = s; i <= L - s; ++i)
        for (int j = 0; j < s; ++j) D[i] += profile[i + j] - profile[i - 1 - j];
    int32_t n = 0, best = 0;
    int64_t best_key = 0;
    for (int i = s; i <= L - s; ++i) {
        const int32_t d = D[i], dp = D[i - 1], dn = D[i + 1];
        const bool up = d >= thr && d > dp && d >= dn, down = -d >= thr && d < dp && d <= dn;
        if (!((p.polarity >= 0 && up) || (p.polarity <= 0 && down))) continue;
        ++n;
        // larger is better; a tie keeps the earlier index
        const int64_t key = p.select == FPM_PROBE_NEAREST ? 128 - std::abs(2 * i - L)
                          : p.select == FPM_PROBE_STRONGEST ? (int64_t)std::abs(d)
                          : p.select == FPM_PROBE_FIRST ? 128 - i : i;
        if (best == 0 || key > best_key) { best = i; best_key = key; }
    }
    *out = best ? fpm_probe_raw{best, n, D[best - 1], D[best], D[best + 1], 0} : fpm_probe_raw{0, 0, 0, 0, 0, 0};
}

bool probe_derive(const ProbeGeom& g, const fpm_probe_params& p, float lt_x, float lt_y, double ca, double sa,
                  const fpm_probe_raw& r, fpm_probe_result* out) {
    if (r.index == 0) {
        if (r.n_edges != 0 || r.d_prev != 0 || r.d != 0 || r.d_next != 0) return false;
        *out = fpm_probe_result{0, 0, 0, r.flags, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        return true;
    }
    if (r.d == 0 || r.index < p.half || r.index > p.length - p.half || r.n_edges < 1 || r.n_edges > p.length) return false;
    const int64_t sg = r.d > 0 ? 1 : -1;
    const int64_t am = sg * r.d_prev, a0 = sg * r.d, ap = sg * r.d_next;
    if (!(am < a0 && ap <= a0)) return false;   // the local-maximum rule: den < 0 and delta in (-0.5, 0.5] follow
    const int64_t den = (am - a0) + (ap - a0);
    const double delta = 0.5 * (double)(am - ap) / (double)den;
    const double t = ((double)r.index - 0.5) + delta;
    const double tx = g.ox + (t * g.cp - g.hw * g.sp), ty = g.oy + (t * g.sp + g.hw * g.cp);
    out->index = r.index; out->n_edges = r.n_edges; out->d = r.d; out->flags = r.flags;
    out->dev = t - g.hl;
    out->contrast = (double)a0 / (double)(p.half * p.width);
    out->tx = tx; out->ty = ty;
    out->sx = (double)lt_x + (tx * ca - ty * sa);
    out->sy = (double)lt_y + (tx * sa + ty * ca);
    return true;
}

void probe_summarise(const fpm_probe_result* res, int32_t n, float lt_x, float lt_y, double angle, fpm_probe_summary* out) {
    fpm_probe_summary s{};
    s.worst = -1;
    s.lt_x = lt_x; s.lt_y = lt_y; s.angle = angle;
    for (int32_t k = 0; k < n; ++k) {
        const fpm_probe_result& r = res[k];
        if (r.flags & FPM_PROBE_OUTSIDE) ++s.n_outside;
        if (r.index < 1) { ++s.n_missing; continue; }
        ++s.n_found;
        if (r.n_edges > 1) ++s.n_ambiguous;
        const double a = std::fabs(r.dev);
        if (s.worst < 0 || a > s.max_abs_dev) { s.worst = k; s.max_abs_dev = a; }
        s.sum_dev += r.dev;
        s.sum_dev_sq += r.dev * r.dev;
    }
    *out = s;
}

namespace {
// the fits' shared tail: rms and the largest |residual| over the points used
void fit_residual_stats(const std::vector<double>& res, double* rms, double* max_resid) {
    double ss = 0.0, mx = 0.0;
    for (double r : res) {
        ss += r * r;
        if (std::fabs(r) > mx) mx = std::fabs(r);
    }
    *rms = std::sqrt(ss / (double)res.size());
    *max_resid = mx;
}

bool fit_points_ok(const double* pts, int32_t n, int32_t least, double trim) {
    if (!pts || n < least || !std::isfinite(trim) || trim < 0.0) return false;
    for (int64_t i = 0; i < 2 * (int64_t)n; ++i)
        if (!std::isfinite(pts[i])) return false;
    return true;
}

// total least squares on the points idx of pts; res = the signed residuals in idx's order
fpm_line_fit line_fit_once(const double* pts, const std::vector<int32_t>& idx, std::vector<double>& res) {
    const double m = (double)idx.size();
    double sx = 0.0, sy = 0.0;
    for (int32_t i : idx) { sx += pts[2 * i]; sy += pts[2 * i + 1]; }
    const double mx = sx / m, my = sy / m;
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
    for (int32_t i : idx) {
        const double dx = pts[2 * i] - mx, dy = pts[2 * i + 1] - my;
        sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
    }
    const double theta = 0.5 * std::atan2(2.0 * sxy, sxx - syy), c = std::cos(theta), s = std::sin(theta);
    res.clear();
    for (int32_t i : idx) {
        const double dx = pts[2 * i] - mx, dy = pts[2 * i + 1] - my;
        res.push_back(dy * c - dx * s);
    }
    fpm_line_fit f{};
    f.angle = theta * kR2D;
    const double along = mx * c + my * s;
    f.px = mx - along * c;
    f.py = my - along * s;
    fit_residual_stats(res, &f.rms, &f.max_resid);
    f.n_used = (int32_t)idx.size();
    return f;
}

// Kasa's fit on centred coordinates, then at most 8 Gauss-Newton steps on the geometric residual
fpm_circle_fit circle_fit_once(const double* pts, const std::vector<int32_t>& idx, std::vector<double>& res) {
    const double m = (double)idx.size();
    fpm_circle_fit f{};
    f.n_used = (int32_t)idx.size();
    double sx = 0.0, sy = 0.0;
    for (int32_t i : idx) { sx += pts[2 * i]; sy += pts[2 * i + 1]; }
    const double mx = sx / m, my = sy / m;
    double suu = 0.0, suv = 0.0, svv = 0.0, suuu = 0.0, svvv = 0.0, suvv = 0.0, svuu = 0.0;
    for (int32_t i : idx) {
        const double u = pts[2 * i] - mx, v = pts[2 * i + 1] - my;
        const double uu = u * u, vv = v * v;
        suu += uu; suv += u * v; svv += vv;
        suuu += uu * u; svvv += vv * v; suvv += u * vv; svuu += v * uu;
    }
    res.assign(idx.size(), 0.0);
    const double det = suu * svv - suv * suv, tr = suu + svv;
    if (!(det > 1e-12 * (tr * tr))) {
        f.flags = FPM_FIT_COLLINEAR;
        return f;
    }
    const double bu = 0.5 * (suuu + suvv), bv = 0.5 * (svvv + svuu);
    double a = (bu * svv - bv * suv) / det, b = (bv * suu - bu * suv) / det;
    double r = std::sqrt((a * a + b * b) + tr / m);
    bool converged = false;
    for (int it = 0; it < 8 && !converged; ++it) {
        // the Jacobian's rows are (-ex, -ey, -1) and the residuals q = d - r: J^T J (da, db, dr) = -J^T q = (gx, gy, g1)
        double jxx = 0.0, jxy = 0.0, jx1 = 0.0, jyy = 0.0, jy1 = 0.0, gx = 0.0, gy = 0.0, g1 = 0.0;
        for (int32_t i : idx) {
            const double du = (pts[2 * i] - mx) - a, dv = (pts[2 * i + 1] - my) - b;
            const double d = std::sqrt(du * du + dv * dv);
            const double ex = d > 0.0 ? du / d : 0.0, ey = d > 0.0 ? dv / d : 0.0, q = d - r;
            jxx += ex * ex; jxy += ex * ey; jx1 += ex; jyy += ey * ey; jy1 += ey;
            gx += ex * q; gy += ey * q; g1 += q;
        }
        // [jxx jxy jx1; jxy jyy jy1; jx1 jy1 m] (da, db, dr) = (gx, gy, g1), by Cramer's rule
        const double c00 = jyy * m - jy1 * jy1, c01 = jxy * m - jy1 * jx1, c02 = jxy * jy1 - jyy * jx1;
        const double dd = (jxx * c00 - jxy * c01) + jx1 * c02;
        if (!(std::fabs(dd) > 0.0) || !std::isfinite(dd)) break;
        const double da = ((gx * c00 - jxy * (gy * m - jy1 * g1)) + jx1 * (gy * jy1 - jyy * g1)) / dd;
        const double db = ((jxx * (gy * m - jy1 * g1) - gx * c01) + jx1 * (jxy * g1 - gy * jx1)) / dd;
        const double dr = ((jxx * (jyy * g1 - gy * jy1) - jxy * (jxy * g1 - gy * jx1)) + gx * c02) / dd;
        a += da; b += db; r += dr;
        converged = std::fabs(da) <= 1e-10 && std::fabs(db) <= 1e-10 && std::fabs(dr) <= 1e-10;
    }
    if (!converged) f.flags |= FPM_FIT_NOT_CONVERGED;
    size_t k = 0;
    for (int32_t i : idx) {
        const double du = (pts[2 * i] - mx) - a, dv = (pts[2 * i + 1] - my) - b;
        res[k++] = std::sqrt(du * du + dv * dv) - r;
    }
    f.cx = mx + a; f.cy = my + b; f.r = r;
    fit_residual_stats(res, &f.rms, &f.max_resid);
    return f;
}

// fit, drop the points beyond trim, fit the rest once more
template <class Fit, class Once>
Fit fit_trimmed(const double* pts, int32_t n, double trim, int32_t least, Once once) {
    std::vector<int32_t> idx((size_t)n), kept;
    for (int32_t i = 0; i < n; ++i) idx[(size_t)i] = i;
    std::vector<double> res;
    Fit f = once(pts, idx, res);
    if (!(trim > 0.0)) return f;
    for (size_t k = 0; k < idx.size(); ++k)
        if (!(std::fabs(res[k]) > trim)) kept.push_back(idx[k]);
    if (kept.size() == idx.size()) return f;
    if ((int32_t)kept.size() < least) { f.flags |= FPM_FIT_TRIM_STARVED; return f; }
    return once(pts, kept, res);
}
}  // namespace

// ---- gray-value tools (include/fpm.h, "gray-value tools"): integers first, then f64 in the header's order; the file is
// built with -ffp-contract=off, so B's two products and its quotient are three roundings.
bool hist_derive(const uint32_t hist[256], fpm_hist_stats* out) {
    int64_t n = 0, sum = 0, sum_sq = 0;
    for (int b = 0; b < 256; ++b) n += (int64_t)hist[b];   // at most 256 * (2^32 - 1)
    if (n > ((int64_t)1 << 22)) return false;
    fpm_hist_stats s{};
    if (n == 0) {
        s.flags = FPM_HIST_EMPTY;
        *out = s;
        return true;
    }
    int32_t mn = -1, mx = -1;
    for (int b = 0; b < 256; ++b) {
        const int64_t h = (int64_t)hist[b];
        if (h == 0) continue;
        if (mn < 0) mn = b;
        mx = b;
        sum += h * b;
        sum_sq += h * b * b;
    }
    s.n = n; s.sum = sum; s.sum_sq = sum_sq;
    s.min = mn; s.max = mx;
    int64_t cum = 0;
    for (int v = 0; v < 256; ++v) {
        cum += (int64_t)hist[v];
        if (2 * cum >= n) { s.median = v; break; }
    }
    s.mean = (double)sum / (double)n;
    s.stddev = std::sqrt((double)(n * sum_sq - sum * sum)) / (double)n;
    if (mn == mx) {
        s.otsu = mn;
        s.flags = FPM_HIST_FLAT;
    } else {
        int64_t n0 = 0, s0 = 0;
        double best = -1.0;   // B >= 0 for every admissible t, and there is one: the first replaces this
        for (int t = 0; t < 255; ++t) {
            n0 += (int64_t)hist[t];
            s0 += (int64_t)hist[t] * t;
            if (n0 <= 0 || n0 >= n) continue;
            const int64_t N = n * s0 - n0 * sum;
            const double NN = (double)N * (double)N;
            const double dd = (double)n0 * (double)(n - n0);
            const double B = NN / dd;
            if (B > best) { best = B; s.otsu = t; }
        }
    }
    *out = s;
    return true;
}

// ---- sub-pattern locators (include/fpm.h, "sub-pattern locators"): integers first, then f64 in the header's order.
const char* feature_bad(const fpm_feature& f) {
    if (f.w < 1 || f.w > FPM_LOCATE_MAX_SIDE || f.h < 1 || f.h > FPM_LOCATE_MAX_SIDE) return "feature: w and h must be 1 .. 128";
    if (f.rx < 0 || f.rx > FPM_LOCATE_MAX_RADIUS || f.ry < 0 || f.ry > FPM_LOCATE_MAX_RADIUS) return "feature: rx and ry must be 0 .. 16";
    if (f.reserved[0] != 0 || f.reserved[1] != 0) return "feature: reserved must be 0";
    return nullptr;
}

double locate_zncc(int64_t n, int64_t si, int64_t sii, int64_t st, int64_t stt, int64_t sit) {
    const int64_t Di = n * sii - si * si, Dt = n * stt - st * st, N = n * sit - si * st;
    const double sdi = std::sqrt((double)Di), sdt = std::sqrt((double)Dt);
    return Di == 0 || Dt == 0 ? 0.0 : (double)N / (sdi * sdt);
}

void locate_host(const uint8_t* window, size_t ws, const uint8_t* tmpl, size_t ts, int w, int h, int rx, int ry,
                 fpm_locate_raw* raw, int32_t* maps) {
    const int nx = 2 * rx + 1, ny = 2 * ry + 1, noff = nx * ny;
    std::vector<int32_t> own;
    if (!maps) { own.resize((size_t)3 * noff); maps = own.data(); }
    int32_t *mi = maps, *mii = maps + noff, *mit = maps + 2 * noff;
    int64_t st = 0, stt = 0;
    for (int b = 0; b < h; ++b)
        for (int a = 0; a < w; ++a) {
            const int64_t t = tmpl[(size_t)b * ts + a];
            st += t; stt += t * t;
        }
    const int64_t n = (int64_t)w * h;
    int best = -1;
    double bz = 0.0;
    int bd = 0;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            int64_t si = 0, sii = 0, sit = 0;
            for (int b = 0; b < h; ++b) {
                const uint8_t* wr = window + (size_t)(b + j) * ws + i;
                const uint8_t* tr = tmpl + (size_t)b * ts;
                for (int a = 0; a < w; ++a) {
                    const int64_t v = wr[a];
                    si += v; sii += v * v; sit += v * tr[a];
                }
            }
            const int o = j * nx + i;
            mi[o] = (int32_t)si; mii[o] = (int32_t)sii; mit[o] = (int32_t)sit;
            const double z = locate_zncc(n, si, sii, st, stt, sit);
            const int dx = i - rx, dy = j - ry, d = dx * dx + dy * dy;
            // row-major order: among equal z and equal distance the earlier offset has the smaller dy, then dx
            if (best < 0 || z > bz || (z == bz && d < bd)) { best = o; bz = z; bd = d; }
        }
    fpm_locate_raw r{};
    const int pj = best / nx, pi = best - pj * nx;
    r.dx = pi - rx; r.dy = pj - ry;
    r.n = n; r.sum_t = st; r.sum_tt = stt;
    for (int j = -1; j <= 1; ++j)
        for (int i = -1; i <= 1; ++i) {
            const int qi = pi + i, qj = pj + j, e = (j + 1) * 3 + (i + 1);
            if (qi < 0 || qi >= nx || qj < 0 || qj >= ny) continue;
            r.s_i[e] = mi[qj * nx + qi]; r.s_ii[e] = mii[qj * nx + qi]; r.s_it[e] = mit[qj * nx + qi];
        }
    const int c = ry * nx + rx;
    r.c_i = mi[c]; r.c_ii = mii[c]; r.c_it = mit[c];
    *raw = r;
}

bool locate_derive(const fpm_feature& f, float lt_x, float lt_y, double angle, const fpm_locate_raw& r, fpm_locate_result* out) {
    if (r.n != (int64_t)f.w * f.h || r.dx < -f.rx || r.dx > f.rx || r.dy < -f.ry || r.dy > f.ry) return false;
    auto z = [&](int e) { return locate_zncc(r.n, r.s_i[e], r.s_ii[e], r.sum_t, r.sum_tt, r.s_it[e]); };
    fpm_locate_result o{};
    o.dx = r.dx; o.dy = r.dy;
    o.flags = r.flags & FPM_LOCATE_OUTSIDE;
    const double z0 = z(4);
    o.score = z0;
    o.score_nominal = locate_zncc(r.n, r.c_i, r.c_ii, r.sum_t, r.sum_tt, r.c_it);
    const int64_t Di = r.n * (int64_t)r.s_ii[4] - (int64_t)r.s_i[4] * r.s_i[4], Dt = r.n * r.sum_tt - r.sum_t * r.sum_t;
    if (Di == 0 || Dt == 0) o.flags |= FPM_LOCATE_FLAT;
    auto sub = [&](int em, int ep) {
        const double zm = z(em), zp = z(ep);
        const double den = (zm - z0) + (zp - z0);
        return den < 0.0 ? 0.5 * (zm - zp) / den : 0.0;
    };
    double ddx = 0.0, ddy = 0.0;
    if (r.dx == -f.rx || r.dx == f.rx) o.flags |= FPM_LOCATE_EDGE_X;
    else ddx = sub(3, 5);
    if (r.dy == -f.ry || r.dy == f.ry) o.flags |= FPM_LOCATE_EDGE_Y;
    else ddy = sub(1, 7);
    o.ox = (double)r.dx + ddx;
    o.oy = (double)r.dy + ddy;
    o.tx = ((double)f.x + (double)(f.w - 1) / 2.0) + o.ox;
    o.ty = ((double)f.y + (double)(f.h - 1) / 2.0) + o.oy;
    const double ra = angle * kD2R, c = std::cos(ra), s = std::sin(ra);
    o.sx = (double)lt_x + (o.tx * c - o.ty * s);
    o.sy = (double)lt_y + (o.tx * s + o.ty * c);
    *out = o;
    return true;
}

}  // namespace fpm

int fpm_locate_host(const uint8_t* window, size_t window_stride, const uint8_t* tmpl, size_t tmpl_stride, int32_t w,
                    int32_t h, int32_t rx, int32_t ry, fpm_locate_raw* raw, int32_t* maps) {
    const fpm_feature f{0, 0, w, h, rx, ry, {0, 0}};
    if (!window || !tmpl || !raw || fpm::feature_bad(f) || window_stride < (size_t)(w + 2 * rx) || tmpl_stride < (size_t)w)
        return FPM_E_INVALID_ARG;
    fpm::locate_host(window, window_stride, tmpl, tmpl_stride, w, h, rx, ry, raw, maps);
    return FPM_OK;
}

int fpm_locate_derive(const fpm_feature* feat, float lt_x, float lt_y, double angle, const fpm_locate_raw* raw,
                      fpm_locate_result* out) {
    if (!feat || !raw || !out || fpm::feature_bad(*feat) || !std::isfinite(lt_x) || !std::isfinite(lt_y) ||
        !std::isfinite(angle) || !fpm::locate_derive(*feat, lt_x, lt_y, angle, *raw, out))
        return FPM_E_INVALID_ARG;
    return FPM_OK;
}

int fpm_hist_derive(const uint32_t hist[256], fpm_hist_stats* out) {
    if (!hist || !out || !fpm::hist_derive(hist, out)) return FPM_E_INVALID_ARG;
    return FPM_OK;
}

int fpm_caliper_pose(float lt_x, float lt_y, double angle, const fpm_caliper* cal, float* ltk_x, float* ltk_y,
                     double* angle_k) {
    if (!cal || !ltk_x || !ltk_y || !angle_k || fpm::caliper_bad(*cal) || !std::isfinite(lt_x) || !std::isfinite(lt_y) ||
        !std::isfinite(angle))
        return FPM_E_INVALID_ARG;
    fpm::caliper_pose(lt_x, lt_y, angle, *cal, ltk_x, ltk_y, angle_k);
    return FPM_OK;
}

int fpm_caliper_edges_host(const int32_t* profile, const fpm_caliper* cal, int32_t cap_per_caliper, fpm_edge_raw* out,
                           int32_t* n_edges, int32_t* flags) {
    if (!profile || !cal || !out || !n_edges || !flags || fpm::caliper_bad(*cal) || cap_per_caliper < 1 ||
        cap_per_caliper > FPM_CALIPER_MAX_CAP)
        return FPM_E_INVALID_ARG;
    for (int32_t u = 0; u < cal->length; ++u)
        if (profile[u] < 0 || profile[u] > 255 * cal->width) return FPM_E_INVALID_ARG;   // of no width pixels
    *n_edges = fpm::caliper_edges(profile, *cal, cap_per_caliper, out);
    *flags = *n_edges > cap_per_caliper ? FPM_CALIPER_TRUNCATED : 0;
    return FPM_OK;
}

int fpm_caliper_derive(const fpm_caliper* cal, float ltk_x, float ltk_y, double angle_k, const fpm_edge_raw* raw,
                       int32_t n, fpm_edge* out) {
    if (!cal || n < 0 || (n > 0 && (!raw || !out)) || fpm::caliper_bad(*cal) || !std::isfinite(ltk_x) ||
        !std::isfinite(ltk_y) || !std::isfinite(angle_k))
        return FPM_E_INVALID_ARG;
    fpm_edge e;
    for (int32_t i = 0; i < n; ++i)   // every record is checked before the first is written
        if (!fpm::caliper_derive(*cal, ltk_x, ltk_y, angle_k, raw[i], &e)) return FPM_E_INVALID_ARG;
    for (int32_t i = 0; i < n; ++i) (void)fpm::caliper_derive(*cal, ltk_x, ltk_y, angle_k, raw[i], out + i);
    return FPM_OK;
}

int fpm_probe_matrix(int32_t src_w, int32_t src_h, float lt_x, float lt_y, double angle, const fpm_probe* probe,
                     const fpm_probe_params* params, double n[6]) {
    if (!probe || !params || !n || src_w <= 0 || src_h <= 0 || fpm::probe_params_bad(*params) || fpm::probe_bad(*probe) ||
        !std::isfinite(lt_x) || !std::isfinite(lt_y) || !std::isfinite(angle))
        return FPM_E_INVALID_ARG;
    const double rad = angle * fpm::kD2R;
    double M[6];
    fpm::patch_matrix(src_w, src_h, fpm::f2(lt_x, lt_y), std::cos(rad), std::sin(rad), 0, 0, M);
    fpm::invert_affine(M);
    const fpm::ProbeGeom g = fpm::probe_geom(*probe, *params);
    fpm::probe_compose(M, g.cp, g.sp, g.ox, g.oy, n);
    return FPM_OK;
}

int fpm_probe_edges_host(const int32_t* profile, const fpm_probe_params* params, fpm_probe_raw* out) {
    if (!profile || !params || !out || fpm::probe_params_bad(*params)) return FPM_E_INVALID_ARG;
    for (int32_t u = 0; u < params->length; ++u)
        if (profile[u] < 0 || profile[u] > 255 * params->width) return FPM_E_INVALID_ARG;   // of no width pixels
    fpm::probe_edges(profile, *params, out);
    return FPM_OK;
}

int fpm_probe_derive(const fpm_probe* probes, const fpm_probe_params* params, float lt_x, float lt_y, double angle,
                     const fpm_probe_raw* raw, int32_t n, fpm_probe_result* out) {
    if (!params || n < 0 || (n > 0 && (!probes || !raw || !out)) || fpm::probe_params_bad(*params) || !std::isfinite(lt_x) ||
        !std::isfinite(lt_y) || !std::isfinite(angle))
        return FPM_E_INVALID_ARG;
    const double rad = angle * fpm::kD2R, ca = std::cos(rad), sa = std::sin(rad);
    fpm_probe_result r;
    for (int32_t i = 0; i < n; ++i)   // every probe and record is checked before the first result is written
        if (fpm::probe_bad(probes[i]) ||
            !fpm::probe_derive(fpm::probe_geom(probes[i], *params), *params, lt_x, lt_y, ca, sa, raw[i], &r))
            return FPM_E_INVALID_ARG;
    for (int32_t i = 0; i < n; ++i)
        (void)fpm::probe_derive(fpm::probe_geom(probes[i], *params), *params, lt_x, lt_y, ca, sa, raw[i], out + i);
    return FPM_OK;
}

int fpm_fit_line(const double* pts, int32_t n, double trim, fpm_line_fit* out) {
    if (!out || !fpm::fit_points_ok(pts, n, 2, trim)) return FPM_E_INVALID_ARG;
    *out = fpm::fit_trimmed<fpm_line_fit>(pts, n, trim, 2, fpm::line_fit_once);
    return FPM_OK;
}

int fpm_fit_circle(const double* pts, int32_t n, double trim, fpm_circle_fit* out) {
    if (!out || !fpm::fit_points_ok(pts, n, 3, trim)) return FPM_E_INVALID_ARG;
    *out = fpm::fit_trimmed<fpm_circle_fit>(pts, n, trim, 3, fpm::circle_fit_once);
    return FPM_OK;
}

// Two-pass union-find over one image at a time: pass 1 links every foreground pixel to its left and upper neighbours
// (the smaller index becomes the parent, so a root is its component's seed), pass 2 resolves every pixel to its root,
// writes the label and adds the pixel to the root's record.
int fpm_blobs_host(const uint8_t* images, int32_t n, int32_t w, int32_t h, size_t stride, int32_t level,
                   int32_t connectivity, int32_t min_area, fpm_blob_summary* summary, fpm_blob* out,
                   int32_t cap_per_hit, int32_t* labels) {
    if (!images || !summary || !out || n < 1 || n > 65535 || w < 1 || h < 1 || (int64_t)w * h > ((int64_t)1 << 22) ||
        stride < (size_t)w || fpm::blobs_bad_args(n, level, connectivity, min_area, cap_per_hit))
        return FPM_E_INVALID_ARG;
    const int32_t npx = w * h;
    const bool c8 = connectivity == 8;
    std::vector<int32_t> parent((size_t)npx), slot((size_t)npx);
    std::vector<fpm_blob> recs;
    auto find = [&](int32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];   // path halving; parent[x] < x off a root
        return x;
    };
    auto unite = [&](int32_t a, int32_t b) {
        a = find(a); b = find(b);
        if (a < b) parent[b] = a;
        else if (b < a) parent[a] = b;
    };
    for (int32_t i = 0; i < n; ++i) {
        const uint8_t* img = images + (size_t)i * stride * h;
        auto fg = [&](int32_t u, int32_t v) { return (int)img[(size_t)v * stride + u] > level; };
        for (int32_t v = 0; v < h; ++v)
            for (int32_t u = 0; u < w; ++u) {
                const int32_t p = v * w + u;
                parent[p] = fg(u, v) ? p : -1;
                if (parent[p] < 0) continue;
                if (u > 0 && parent[p - 1] >= 0) unite(p, p - 1);
                if (v > 0) {
                    if (parent[p - w] >= 0) unite(p, p - w);
                    if (c8 && u > 0 && parent[p - w - 1] >= 0) unite(p, p - w - 1);
                    if (c8 && u < w - 1 && parent[p - w + 1] >= 0) unite(p, p - w + 1);
                }
            }
        recs.clear();
        int64_t fg_pixels = 0;
        int32_t largest = 0;
        for (int32_t v = 0; v < h; ++v)
            for (int32_t u = 0; u < w; ++u) {
                const int32_t p = v * w + u;
                int32_t* lab = labels ? labels + (size_t)i * npx + p : nullptr;
                if (parent[p] < 0) { if (lab) *lab = 0; continue; }
                const int32_t r = find(p);   // r <= p: a root is met first, in row-major order, as its own pixel
                parent[p] = r;
                if (r == p) {
                    slot[p] = (int32_t)recs.size();
                    recs.push_back(fpm_blob{i, p, 0, u, v, u, v, 0, 0, 0, 0});
                }
                fpm_blob& b = recs[(size_t)slot[r]];
                const int32_t e = img[(size_t)v * stride + u];
                b.area++;
                b.x0 = std::min(b.x0, u); b.y0 = std::min(b.y0, v);
                b.x1 = std::max(b.x1, u); b.y1 = std::max(b.y1, v);
                b.max_value = std::max(b.max_value, e);
                b.sum_value += e; b.sum_x += u; b.sum_y += v;
                fg_pixels++;
                if (lab) *lab = r + 1;
            }
        for (const fpm_blob& b : recs) largest = std::max(largest, b.area);
        fpm::blobs_tail(recs.data(), (int64_t)recs.size(), 0, fg_pixels, (int32_t)recs.size(), largest, min_area,
                        cap_per_hit, out + (size_t)i * cap_per_hit, summary + i);
    }
    return FPM_OK;
}
