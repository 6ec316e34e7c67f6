// Stand-alone sanitizer run of the host blob entry (fpm_blobs_host and its tail, blobs_tail).
// From the repository root:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       --offload-arch=gfx950 -x hip fastest_image_pattern_matching_amd/csrc/fpm_host.cpp scripts/blobs_host_asan.cpp \
//       -fsanitize=address,undefined -pthread -o build/blobs_host_asan && build/blobs_host_asan
// It needs no device.  The process's exit status is the check; the records themselves are checked by
// tests/test_blobs_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../include/fpm.h"
int main() {
    const int shapes[][2] = {{1, 1}, {5, 3}, {63, 15}, {64, 16}, {65, 17}, {130, 35}, {257, 50}};
    unsigned seed = 12345;
    long total = 0;
    for (const auto& s : shapes) {
        const int w = s[0], h = s[1], n = 6, stride = w + 3;
        std::vector<unsigned char> img((size_t)n * stride * h);
        for (int i = 0; i < n; ++i)
            for (int v = 0; v < h; ++v)
                for (int u = 0; u < stride; ++u) {
                    seed = seed * 1664525u + 1013904223u;
                    unsigned char p = 0;
                    if (i == 1) p = 255;
                    else if (i == 2) p = (u + v) % 2 ? 0 : 200;
                    else if (i == 3) p = (u % 2 == 0 || v == h - 1) ? 9 : 0;
                    else if (i >= 4) p = (unsigned char)(seed >> 24);
                    img[((size_t)i * h + v) * stride + u] = p;
                }
        for (int conn = 4; conn <= 8; conn += 4)
            for (int cap : {1, 64, 4096})
                for (int min_area : {1, 2, 9}) {
                    std::vector<fpm_blob_summary> sum(n);
                    std::vector<fpm_blob> out((size_t)n * cap);
                    std::vector<int32_t> lab((size_t)n * w * h);
                    const int rc = fpm_blobs_host(img.data(), n, w, h, stride, 100, conn, min_area, sum.data(), out.data(),
                                                  cap, cap == 64 ? nullptr : lab.data());
                    if (rc != FPM_OK) { std::printf("rc %d\n", rc); return 1; }
                    for (int i = 0; i < n; ++i) total += sum[i].n_blobs;
                }
    }
    std::printf("blobs_host sanitizer run ok: %ld blobs\n", total);
    return 0;
}
