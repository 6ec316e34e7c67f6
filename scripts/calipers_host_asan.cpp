// Stand-alone sanitizer run of the host caliper entries (fpm_caliper_pose, fpm_caliper_edges_host, fpm_caliper_derive).
// From the repository root:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       --offload-arch=gfx950 -x hip fastest_image_pattern_matching_amd/csrc/fpm_host.cpp scripts/calipers_host_asan.cpp \
//       -fsanitize=address,undefined -pthread -o build/calipers_host_asan && build/calipers_host_asan
// It needs no device.  Profiles, records and edges live in heap buffers of exactly the sizes the entries are given, so
// a read or write past them ends the run.  The process's exit status is the check; the values themselves are checked
// by tests/test_caliper_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../include/fpm.h"
int main() {
    const int lengths[] = {2, 3, 4, 5, 63, 64, 65, 129, 1024}, widths[] = {1, 15, 16, 17, 33, 256}, halves[] = {1, 2, 16};
    unsigned seed = 2468;
    long total = 0, truncated = 0;
    for (int L : lengths)
        for (int W : widths)
            for (int s : halves) {
                if (2 * s > L) continue;
                for (int cap : {1, 8, 64})
                    for (int kind = 0; kind < 3; ++kind) {
                        fpm_caliper cal{12.5 + L, -3.25, 37.5 * kind - 90.0, L, W, s, kind == 2 ? 255 : 1 + 11 * kind, kind - 1, 0};
                        std::vector<int32_t> prof((size_t)L);
                        for (int u = 0; u < L; ++u) {
                            seed = seed * 1664525u + 1013904223u;
                            prof[u] = kind == 0 ? (int32_t)((seed >> 8) % (255u * W + 1u))     // rough
                                    : kind == 1 ? ((u / 3) % 2) * 255 * W                       // saturated stripes
                                                : ((u / 16) % 2) * 255 * W;                     // the extremes at s = 16
                        }
                        std::vector<fpm_edge_raw> raw((size_t)cap);
                        int32_t n = -1, flags = -1;
                        if (fpm_caliper_edges_host(prof.data(), &cal, cap, raw.data(), &n, &flags) != FPM_OK) return 1;
                        const int32_t nret = n < cap ? n : cap;
                        float x, y;
                        double a;
                        if (fpm_caliper_pose(100.25f, 80.5f, 17.0, &cal, &x, &y, &a) != FPM_OK) return 2;
                        std::vector<fpm_edge> e((size_t)nret);
                        if (fpm_caliper_derive(&cal, x, y, a, raw.data(), nret, e.data()) != FPM_OK) return 3;
                        for (int32_t i = 0; i < nret; ++i)
                            if (!(e[i].t > e[i].index - 1.0 && e[i].t <= e[i].index)) return 4;   // delta in (-0.5, 0.5]
                        total += n;
                        truncated += flags == FPM_CALIPER_TRUNCATED;
                    }
            }
    std::printf("calipers host sanitizer run ok: %ld edges, %ld truncated calipers\n", total, truncated);
    return 0;
}
