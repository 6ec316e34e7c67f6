// Stand-alone sanitizer run of the host gray-value entry (fpm_hist_derive).
// From the repository root:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       --offload-arch=gfx950 -x hip fastest_image_pattern_matching_amd/csrc/fpm_host.cpp scripts/gray_host_asan.cpp \
//       -fsanitize=address,undefined -pthread -o build/gray_host_asan && build/gray_host_asan
// It needs no device.  Every histogram lives in a heap buffer of exactly 256 words and every result in a heap buffer of
// exactly one record, so a read or write past either ends the run.  The process's exit status is the check; the values
// themselves are checked by tests/test_gray_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/fpm.h"

static int derive(const std::vector<uint32_t>& h, fpm_hist_stats* copy) {
    std::vector<fpm_hist_stats> out(1);
    std::memset(out.data(), 0x5a, sizeof(fpm_hist_stats));
    const int rc = fpm_hist_derive(h.data(), out.data());
    *copy = out[0];
    return rc;
}

int main() {
    unsigned seed = 1357;
    long flat = 0, empty = 0, total = 0;
    fpm_hist_stats s;
    for (int k = 0; k < 500; ++k) {   // random histograms: dense, sparse, few pixels
        std::vector<uint32_t> h(256, 0u);
        for (int b = 0; b < 256; ++b) {
            seed = seed * 1664525u + 1013904223u;
            const uint32_t v = (seed >> 8) % 2000u;
            h[b] = k % 3 == 0 ? v : (k % 3 == 1 ? (v < 200u ? v : 0u) : (v < 8u ? 1u : 0u));
        }
        if (derive(h, &s) != FPM_OK) return 1;
        if (s.n > 0 && !(s.min <= s.median && s.median <= s.max && s.min <= s.otsu && s.otsu <= s.max)) return 2;
        total += s.n;
        flat += (s.flags & FPM_HIST_FLAT) != 0;
        empty += (s.flags & FPM_HIST_EMPTY) != 0;
    }
    {   // empty
        std::vector<uint32_t> h(256, 0u);
        if (derive(h, &s) != FPM_OK || s.flags != FPM_HIST_EMPTY || s.n != 0 || s.otsu != 0) return 3;
    }
    for (int v : {0, 137, 255}) {   // flat, also at the largest count
        for (uint32_t n : {1u, 1000u, 1u << 22}) {
            std::vector<uint32_t> h(256, 0u);
            h[(size_t)v] = n;
            if (derive(h, &s) != FPM_OK || s.flags != FPM_HIST_FLAT || s.otsu != v || s.min != v || s.max != v) return 4;
        }
    }
    const int spikes[][2] = {{10, 200}, {0, 255}, {0, 1}, {254, 255}, {100, 101}};
    for (const auto& p : spikes) {   // two spikes: every t between them ties, the first wins
        std::vector<uint32_t> h(256, 0u);
        h[(size_t)p[0]] = 70;
        h[(size_t)p[1]] = 30;
        if (derive(h, &s) != FPM_OK || s.otsu != p[0] || s.flags != 0) return 5;
    }
    {   // symmetric: an exact tie between t and its mirror, the smaller wins
        std::vector<uint32_t> h(256, 0u);
        for (int b = 0; b < 128; ++b) {
            seed = seed * 1664525u + 1013904223u;
            h[(size_t)b] = h[(size_t)(255 - b)] = (seed >> 8) % 300u;
        }
        if (derive(h, &s) != FPM_OK || s.otsu > 127) return 6;
    }
    {   // the largest N: 2^21 pixels in each end bin
        std::vector<uint32_t> h(256, 0u);
        h[0] = h[255] = 1u << 21;
        if (derive(h, &s) != FPM_OK || s.otsu != 0 || s.mean != 127.5 || s.stddev != 127.5) return 7;
    }
    {   // argument errors: the output stays as it was
        std::vector<uint32_t> h(256, 0u);
        h[3] = (1u << 22) + 1u;
        if (derive(h, &s) != FPM_E_INVALID_ARG || s.n != 0x5a5a5a5a5a5a5a5aLL) return 8;
        for (auto& v : h) v = 0xffffffffu;
        if (derive(h, &s) != FPM_E_INVALID_ARG || s.flags != 0x5a5a5a5a) return 9;
        std::vector<fpm_hist_stats> out(1);
        if (fpm_hist_derive(nullptr, out.data()) != FPM_E_INVALID_ARG || fpm_hist_derive(h.data(), nullptr) != FPM_E_INVALID_ARG)
            return 10;
    }
    std::printf("gray host sanitizer run ok: %ld pixels, %ld flat and %ld empty histograms\n", total, flat, empty);
    return 0;
}
