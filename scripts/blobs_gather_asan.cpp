// Stand-alone sanitizer run of the device blob entries' host side: blobs_gather (and blobs_tail behind it), the only
// code of fpm_last_blobs / fpm_blobs_at / fpm_op_blobs that writes into caller memory.
// From the repository root (the ROCm include path is for the headers fpm_host.h pulls in; nothing of HIP is linked):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I/opt/rocm/include \
//       -D__HIP_PLATFORM_AMD__ fastest_image_pattern_matching_amd/csrc/fpm_host.cpp scripts/blobs_gather_asan.cpp \
//       -pthread -o build/blobs_gather_asan && build/blobs_gather_asan
// It needs no device.  "Device output" is made from fpm_blobs_host's full records (cap 65536): per image the counters
// and the records, shuffled and cut to cap_dev as a round of the kernels leaves them in the pinned buffer.  blobs_gather
// then writes into heap buffers of exactly n x cap_per_hit records and n summaries, and the result is held against
// fpm_blobs_host at the same cap: equal when the image is not truncated, else the contract's rule (cap records, each an
// exact record of the image, ascending and distinct by seed, the summary equal).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "../fastest_image_pattern_matching_amd/csrc/fpm_host.h"

static unsigned rnd_state = 2463534242u;
static unsigned rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 17; rnd_state ^= rnd_state << 5; return rnd_state; }

static bool same(const fpm_blob& a, const fpm_blob& b) { return std::memcmp(&a, &b, sizeof(fpm_blob)) == 0; }

int main() {
    const int shapes[][2] = {{1, 1}, {5, 3}, {63, 15}, {64, 16}, {65, 17}, {130, 35}, {257, 50}};
    const int kFull = 65536;
    long checked = 0, truncated = 0;
    for (const auto& s : shapes) {
        const int w = s[0], h = s[1], n = 6;
        std::vector<unsigned char> img((size_t)n * w * h);
        for (int i = 0; i < n; ++i)
            for (int v = 0; v < h; ++v)
                for (int u = 0; u < w; ++u) {
                    unsigned char p = 0;
                    if (i == 1) p = 255;
                    else if (i == 2) p = (u + v) % 2 ? 0 : 200;
                    else if (i == 3) p = (u % 2 == 0 || v == h - 1) ? 9 : 0;
                    else if (i >= 4) p = (unsigned char)(rnd() >> 24);
                    img[((size_t)i * h + v) * w + u] = p;
                }
        for (int conn = 4; conn <= 8; conn += 4)
            for (int cap : {1, 64, 4096})
                for (int min_area : {1, 2, 9}) {
                    // every qualifying record of every image
                    std::vector<fpm_blob_summary> fs(n);
                    std::vector<fpm_blob> fr((size_t)n * kFull);
                    if (fpm_blobs_host(img.data(), n, w, h, w, 100, conn, min_area, fs.data(), fr.data(), kFull, nullptr) != FPM_OK)
                        return 1;
                    // one round of device output: counters, and [image][cap_dev] records in slot order
                    const int cap_dev = fpm::blobs_cap_dev(w, h, min_area, cap);
                    std::unique_ptr<fpm::BlobCounters[]> cnt(new fpm::BlobCounters[n]);
                    std::unique_ptr<fpm_blob[]> dev(new fpm_blob[(size_t)n * cap_dev]);
                    std::memset(dev.get(), 0, sizeof(fpm_blob) * (size_t)n * cap_dev);
                    for (int i = 0; i < n; ++i) {
                        if (fs[i].flags) { std::printf("full run truncated\n"); return 1; }
                        fpm_blob* r = fr.data() + (size_t)i * kFull;
                        const int q = fs[i].n_blobs;
                        for (int k = q; k > 1; --k) std::swap(r[k - 1], r[rnd() % k]);
                        std::copy(r, r + std::min(q, cap_dev), dev.get() + (size_t)i * cap_dev);
                        cnt[i] = fpm::BlobCounters{(int32_t)fs[i].fg_pixels, fs[i].n_components, q, fs[i].largest_area};
                    }
                    // the caller's buffers, exactly as large as the entry's contract says
                    std::unique_ptr<fpm_blob[]> out(new fpm_blob[(size_t)n * cap]);
                    std::unique_ptr<fpm_blob_summary[]> sum(new fpm_blob_summary[n]);
                    fpm::blobs_gather(cnt.get(), dev.get(), n, cap_dev, min_area, cap, out.get(), sum.get());
                    // the host entry at the same cap
                    std::vector<fpm_blob_summary> hs(n);
                    std::vector<fpm_blob> hr((size_t)n * cap);
                    if (fpm_blobs_host(img.data(), n, w, h, w, 100, conn, min_area, hs.data(), hr.data(), cap, nullptr) != FPM_OK)
                        return 1;
                    // and every record again, in seed order, to look a truncated list's records up in
                    if (fpm_blobs_host(img.data(), n, w, h, w, 100, conn, min_area, fs.data(), fr.data(), kFull, nullptr) != FPM_OK)
                        return 1;
                    for (int i = 0; i < n; ++i) {
                        if (std::memcmp(&sum[i], &hs[i], sizeof(fpm_blob_summary)) != 0) { std::printf("summary differs\n"); return 1; }
                        const fpm_blob* g = out.get() + (size_t)i * cap;
                        const fpm_blob* e = hr.data() + (size_t)i * cap;
                        if (!(sum[i].flags & FPM_BLOBS_TRUNCATED)) {
                            for (int k = 0; k < cap; ++k)
                                if (!same(g[k], e[k])) { std::printf("records differ\n"); return 1; }
                        } else {
                            ++truncated;
                            if (sum[i].n_returned != cap) { std::printf("a truncated list holds cap records\n"); return 1; }
                            const fpm_blob* all = fr.data() + (size_t)i * kFull;
                            for (int k = 0; k < cap; ++k) {
                                if (k && g[k].seed <= g[k - 1].seed) { std::printf("seeds not ascending\n"); return 1; }
                                const fpm_blob* f = std::lower_bound(all, all + fs[i].n_blobs, g[k],
                                                                     [](const fpm_blob& a, const fpm_blob& b) { return a.seed < b.seed; });
                                if (f == all + fs[i].n_blobs || !same(*f, g[k])) { std::printf("not a record of the image\n"); return 1; }
                            }
                        }
                        ++checked;
                    }
                }
    }
    std::printf("blobs_gather sanitizer run ok: %ld images, %ld truncated\n", checked, truncated);
    return 0;
}
