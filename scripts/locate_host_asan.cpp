// Stand-alone sanitizer run of the host locator entries (fpm_locate_host, fpm_locate_derive).
// From the repository root:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       --offload-arch=gfx950 -x hip fastest_image_pattern_matching_amd/csrc/fpm_host.cpp scripts/locate_host_asan.cpp \
//       -fsanitize=address,undefined -pthread -o build/locate_host_asan && build/locate_host_asan
// It needs no device.  Every window and template region lives in a heap buffer of exactly its pixels, the maps in one of
// exactly 3 (2 rx + 1)(2 ry + 1) words and every record in a heap buffer of exactly one, so a read or write past any of
// them ends the run.  The process's exit status is the check; the values themselves are checked by
// tests/test_locate_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/fpm.h"

int main() {
    unsigned seed = 2468;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    const int shapes[][4] = {{1, 1, 0, 0}, {1, 1, 16, 16}, {128, 128, 0, 0}, {128, 128, 16, 16}, {128, 1, 3, 16}, {1, 128, 16, 3},
                             {9, 7, 3, 2}, {64, 33, 8, 8}, {65, 17, 1, 0}, {5, 63, 0, 1}};
    long peaks = 0, flat = 0, edges = 0;
    for (const auto& sh : shapes) {
        const int w = sh[0], h = sh[1], rx = sh[2], ry = sh[3], ww = w + 2 * rx, wh = h + 2 * ry;
        const int noff = (2 * rx + 1) * (2 * ry + 1);
        for (int kind = 0; kind < 4; ++kind) {   // random, planted, the largest values, flat
            std::vector<uint8_t> win((size_t)ww * wh), t((size_t)w * h);
            for (auto& v : win) v = kind == 2 ? 255 : (kind == 3 ? 9 : (uint8_t)next());
            for (auto& v : t) v = kind == 2 ? 255 : (uint8_t)next();
            const int px = (int)(next() % (unsigned)(2 * rx + 1)), py = (int)(next() % (unsigned)(2 * ry + 1));
            if (kind == 1)
                for (int b = 0; b < h; ++b) std::memcpy(&win[(size_t)(b + py) * ww + px], &t[(size_t)b * w], (size_t)w);
            std::vector<fpm_locate_raw> raw(1), raw2(1);
            std::vector<int32_t> maps((size_t)3 * noff);
            if (fpm_locate_host(win.data(), (size_t)ww, t.data(), (size_t)w, w, h, rx, ry, raw.data(), maps.data()) != FPM_OK) return 1;
            if (fpm_locate_host(win.data(), (size_t)ww, t.data(), (size_t)w, w, h, rx, ry, raw2.data(), nullptr) != FPM_OK) return 2;
            if (std::memcmp(raw.data(), raw2.data(), sizeof(fpm_locate_raw)) != 0) return 3;
            if (raw[0].n != (int64_t)w * h || raw[0].dx < -rx || raw[0].dx > rx || raw[0].dy < -ry || raw[0].dy > ry) return 4;
            if (raw[0].c_it != maps[(size_t)2 * noff + (size_t)ry * (2 * rx + 1) + rx]) return 5;
            std::vector<fpm_feature> f(1, fpm_feature{3, 5, w, h, rx, ry, {0, 0}});
            std::vector<fpm_locate_result> res(1);
            if (fpm_locate_derive(f.data(), 12.25f, -7.5f, 33.0, raw.data(), res.data()) != FPM_OK) return 6;
            if (!(res[0].score >= -1.0000001 && res[0].score <= 1.0000001) || !(res[0].ox >= raw[0].dx - 0.5 && res[0].ox <= raw[0].dx + 0.5))
                return 7;
            if (kind == 1 && !(res[0].flags & FPM_LOCATE_FLAT) && res[0].score < 0.999999) return 8;
            if (kind >= 2 && (res[0].flags & FPM_LOCATE_FLAT) == 0) return 9;
            if (kind >= 2 && (raw[0].dx != 0 || raw[0].dy != 0 || res[0].score != 0.0)) return 10;
            peaks += 1;
            flat += (res[0].flags & FPM_LOCATE_FLAT) != 0;
            edges += (res[0].flags & (FPM_LOCATE_EDGE_X | FPM_LOCATE_EDGE_Y)) != 0;
        }
    }
    {   // argument errors: the outputs stay as they were
        std::vector<uint8_t> win(144, 1), t(64, 2);
        std::vector<fpm_locate_raw> raw(1);
        std::memset(raw.data(), 0x5a, sizeof(fpm_locate_raw));
        const int bad[][4] = {{0, 8, 2, 2}, {8, 0, 2, 2}, {129, 8, 2, 2}, {8, 129, 2, 2}, {8, 8, -1, 2}, {8, 8, 2, -1}, {8, 8, 17, 2}, {8, 8, 2, 17}};
        for (const auto& b : bad)
            if (fpm_locate_host(win.data(), 200, t.data(), 200, b[0], b[1], b[2], b[3], raw.data(), nullptr) != FPM_E_INVALID_ARG) return 11;
        if (fpm_locate_host(win.data(), 11, t.data(), 8, 8, 8, 2, 2, raw.data(), nullptr) != FPM_E_INVALID_ARG ||
            fpm_locate_host(win.data(), 12, t.data(), 7, 8, 8, 2, 2, raw.data(), nullptr) != FPM_E_INVALID_ARG ||
            fpm_locate_host(nullptr, 12, t.data(), 8, 8, 8, 2, 2, raw.data(), nullptr) != FPM_E_INVALID_ARG ||
            fpm_locate_host(win.data(), 12, nullptr, 8, 8, 8, 2, 2, raw.data(), nullptr) != FPM_E_INVALID_ARG ||
            fpm_locate_host(win.data(), 12, t.data(), 8, 8, 8, 2, 2, nullptr, nullptr) != FPM_E_INVALID_ARG)
            return 12;
        if (raw[0].n != 0x5a5a5a5a5a5a5a5aLL || raw[0].c_it != 0x5a5a5a5a) return 13;
        if (fpm_locate_host(win.data(), 12, t.data(), 8, 8, 8, 2, 2, raw.data(), nullptr) != FPM_OK) return 14;
        std::vector<fpm_feature> f(1, fpm_feature{0, 0, 8, 8, 2, 2, {0, 0}});
        std::vector<fpm_locate_result> res(1);
        std::memset(res.data(), 0x5a, sizeof(fpm_locate_result));
        fpm_locate_raw r = raw[0];
        r.dx = 3;
        if (fpm_locate_derive(f.data(), 0.f, 0.f, 0.0, &r, res.data()) != FPM_E_INVALID_ARG) return 15;
        r = raw[0];
        r.n = 63;
        if (fpm_locate_derive(f.data(), 0.f, 0.f, 0.0, &r, res.data()) != FPM_E_INVALID_ARG) return 16;
        f[0].reserved[1] = 1;
        if (fpm_locate_derive(f.data(), 0.f, 0.f, 0.0, raw.data(), res.data()) != FPM_E_INVALID_ARG) return 17;
        if (fpm_locate_derive(nullptr, 0.f, 0.f, 0.0, raw.data(), res.data()) != FPM_E_INVALID_ARG ||
            fpm_locate_derive(f.data(), 0.f, 0.f, 0.0, nullptr, res.data()) != FPM_E_INVALID_ARG)
            return 18;
        if (res[0].flags != 0x5a5a5a5a) return 19;
    }
    std::printf("locate host sanitizer run ok: %ld peaks, %ld flat, %ld on the range's border\n", peaks, flat, edges);
    return 0;
}
