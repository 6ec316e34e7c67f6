// Stand-alone sanitizer run of the host probe entries (fpm_probe_matrix, fpm_probe_edges_host, fpm_probe_derive,
// fpm_fit_line, fpm_fit_circle).  From the repository root:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       --offload-arch=gfx950 -x hip fastest_image_pattern_matching_amd/csrc/fpm_host.cpp scripts/probes_host_asan.cpp \
//       -fsanitize=address,undefined -pthread -o build/probes_host_asan && build/probes_host_asan
// It needs no device.  Profiles, probes, records, results and points live in heap buffers of exactly the sizes the entries
// are given, so a read or write past them ends the run.  The process's exit status is the check; the values themselves
// are checked by tests/test_probe_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../include/fpm.h"
int main() {
    const int lengths[] = {4, 5, 31, 32, 33, 63, 64}, widths[] = {1, 2, 15, 16}, halves[] = {1, 2, 8};
    unsigned seed = 1357;
    long found = 0, probes = 0, fits = 0;
    for (int L : lengths)
        for (int W : widths)
            for (int s : halves) {
                if (2 * s > L) continue;
                for (int sel = FPM_PROBE_NEAREST; sel <= FPM_PROBE_LAST; ++sel)
                    for (int kind = 0; kind < 3; ++kind) {
                        const fpm_probe_params prm{L, W, s, kind == 2 ? 255 : 1 + 11 * kind, kind - 1, sel, {0, 0}};
                        const int n = 1 + (L + W + s + sel + kind) % 9;
                        std::vector<fpm_probe> prb((size_t)n);
                        std::vector<fpm_probe_raw> raw((size_t)n);
                        for (int k = 0; k < n; ++k) {
                            prb[k] = fpm_probe{12.5 + L + k, -3.25 * k, 37.5 * k - 90.0};
                            std::vector<int32_t> prof((size_t)L);
                            for (int u = 0; u < L; ++u) {
                                seed = seed * 1664525u + 1013904223u;
                                prof[u] = kind == 0 ? (int32_t)((seed >> 8) % (255u * W + 1u))     // rough
                                        : kind == 1 ? ((u / 3) % 2) * 255 * W                       // saturated stripes
                                                    : (((u + k) / 8) % 2) * 255 * W;                // the extremes at s = 8
                            }
                            std::vector<fpm_probe_raw> one(1);
                            if (fpm_probe_edges_host(prof.data(), &prm, one.data()) != FPM_OK) return 1;
                            raw[k] = one[0];
                            std::vector<double> m(6);
                            if (fpm_probe_matrix(161, 97, 100.25f, 80.5f, 17.0 + k, &prb[k], &prm, m.data()) != FPM_OK) return 2;
                        }
                        std::vector<fpm_probe_result> res((size_t)n);
                        if (fpm_probe_derive(prb.data(), &prm, 100.25f, 80.5f, 17.0, raw.data(), n, res.data()) != FPM_OK) return 3;
                        std::vector<double> pts;
                        for (int k = 0; k < n; ++k) {
                            if (res[k].index == 0) continue;
                            if (!(std::fabs(res[k].dev) <= L)) return 4;
                            pts.push_back(res[k].sx);
                            pts.push_back(res[k].sy);
                            ++found;
                        }
                        probes += n;
                        const int np = (int)(pts.size() / 2);
                        std::vector<double> exact(pts);   // a heap buffer of exactly 2 np doubles
                        fpm_line_fit lf;
                        fpm_circle_fit cf;
                        for (double trim : {0.0, 0.75}) {
                            if (np >= 2 && fpm_fit_line(exact.data(), np, trim, &lf) != FPM_OK) return 5;
                            if (np >= 3 && fpm_fit_circle(exact.data(), np, trim, &cf) != FPM_OK) return 6;
                            fits += (np >= 2) + (np >= 3);
                        }
                        if (fpm_fit_line(exact.data(), 1, 0.0, &lf) != FPM_E_INVALID_ARG) return 7;
                        if (fpm_fit_circle(exact.data(), np < 2 ? np : 2, 0.0, &cf) != FPM_E_INVALID_ARG) return 8;
                    }
            }
    // a ring and a row of exact points, with one outlier each
    std::vector<double> ring, row;
    for (int k = 0; k < 64; ++k) {
        const double a = 6.283185307179586 * k / 64.0;
        ring.push_back(171.4 + 41.3 * std::cos(a) + (k == 9 ? 7.0 : 0.0));
        ring.push_back(118.7 + 41.3 * std::sin(a));
        row.push_back(3.0 + 1.5 * k);
        row.push_back(-2.0 + 0.25 * k + (k == 30 ? 9.0 : 0.0));
    }
    fpm_line_fit lf;
    fpm_circle_fit cf;
    if (fpm_fit_circle(ring.data(), 64, 1.0, &cf) != FPM_OK || cf.n_used != 63 || std::fabs(cf.r - 41.3) > 1e-9) return 9;
    if (fpm_fit_line(row.data(), 64, 1.0, &lf) != FPM_OK || lf.n_used != 63 || lf.max_resid > 1e-9) return 10;
    std::printf("probes host sanitizer run ok: %ld probes, %ld edges found, %ld fits\n", probes, found, fits);
    return 0;
}
