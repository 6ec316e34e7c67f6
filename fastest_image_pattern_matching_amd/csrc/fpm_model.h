// The variation model's per-pixel rule (include/fpm.h, "variation model") in exact integers, as
// one function for the device (k_model_prepare) and the host (fpm_model_derive): both run this code.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace fpm {

constexpr int kModelMaxSamples = 65535;   // n * 255^2 stays below 2^32: the planes are u32

// floor(sqrt(x)) of a 64-bit integer, exactly: the f64 root (x rounds on the way in above 2^53, the root rounds again)
// is at most a few units off, and the integer steps settle it.  x < 2^63, so (r + 1)^2 does not wrap.
__host__ __device__ inline uint64_t model_isqrt(uint64_t x) {
    uint64_t r = (uint64_t)sqrt((double)x);
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return r;
}

struct ModelBand {
    int32_t mean, lo, hi;   // lo = hi + 1: the empty interval
};

// n samples (1 .. 65535) with sum S and sum of squares Q at one pixel; a = absolute threshold 0 .. 255, kq = sigma
// multiple in sixteenths 0 .. 255.  V = n Q - S^2 <= 2^46 and kq^2 V < 2^62.
__host__ __device__ inline ModelBand model_band(uint32_t n, uint32_t S, uint32_t Q, uint32_t a, uint32_t kq) {
    const uint64_t n64 = n, s64 = S;
    const uint64_t V = n64 * (uint64_t)Q - s64 * s64;
    const uint64_t ks = model_isqrt(((uint64_t)(kq * kq) * V) >> 8), na = n64 * a;
    const uint64_t B = na > ks ? na : ks;
    ModelBand b;
    b.mean = (int32_t)((2 * s64 + n64) / (2 * n64));
    b.lo = s64 > B ? (int32_t)((s64 - B + n64 - 1) / n64) : 0;
    const uint64_t hi = (s64 + B) / n64;
    b.hi = hi > 255 ? 255 : (int32_t)hi;
    return b;
}

}  // namespace fpm
