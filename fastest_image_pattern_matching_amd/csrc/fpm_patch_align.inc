// The body of k_patch_align and k_patch_align_masked (fpm_kernels.hip includes it into both, after `constexpr bool MASK`
// and inside `template <bool LUT>`; `c` is the kernel's AlignArgs).  Text, not a function: the form without a mask comes
// out of the compiler as it did before there was a mask, register for register, which an inlined body did not.
    __shared__ __attribute__((aligned(16))) int32_t tab[kPatchTabWords];
    __shared__ __attribute__((aligned(16))) uint8_t FT[kPatchFtBytes];
    __shared__ __attribute__((aligned(16))) uint8_t lut[LUT ? 256 : 4];
    __shared__ unsigned long long part[4][kAlignFields];
    const PatchArgs& a = c.p;
    const int tid = threadIdx.x;
    if (LUT) {
        // the job index as patch_tile_stage derives it; the helper's first barrier orders these writes before any read
        const int job = xcd_remap(blockIdx.x, gridDim.x) / (a.tiles_x * a.tiles_y);
        if (tid < 64) ((uint32_t*)lut)[tid] = ((const uint32_t*)(c.luts + (size_t)job * 256))[tid];
    }
    const PatchTile T = patch_tile_stage(a, tab, FT, tid);
    const int r = tid >> 4, gx = (tid & 15) * 4;
    const int x = T.x0 + gx, y = T.y0 + r;
    const int left = a.pw - x;
    const int nu = y >= a.ph || left <= 0 ? 0 : (left < 4 ? left : 4);
    const uint32_t iw = patch_sample4(a, T, tab, FT, r, gx, nu);
    const int tx = c.rx + x, ty = c.ry + y;
    const bool row_used = nu > 0 && ty >= 1 && ty <= c.th - 2;   // rows ty - 1 and ty + 1 exist
    uint32_t cw = 0, lw = 0, rw = 0, uw = 0, dw = 0;   // the template at u, u - 1, u + 1, and in the rows above and below
    uint32_t mw = 0;                                    // MASK: 0xFF in the bytes of the pixels the mask keeps
    if (row_used) {
        const uint8_t* trow = c.tmpl + (size_t)ty * c.tp;
        const int c0 = tx & ~3, k = tx & 3;
        const uint32_t lo = *(const uint32_t*)(trow + c0);
        const uint32_t hi = c0 + 4 < c.tp ? *(const uint32_t*)(trow + c0 + 4) : 0u;
        const uint32_t pv = k == 0 && c0 >= 4 ? *(const uint32_t*)(trow + c0 - 4) : 0u;
        cw = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)k);
        lw = k == 0 ? __builtin_amdgcn_alignbyte(lo, pv, 3u) : __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(k - 1));
        rw = k == 3 ? hi : __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(k + 1));
        uw = tmpl_read4(trow - c.tp, tx, c.tp);
        dw = tmpl_read4(trow + c.tp, tx, c.tp);
        if (MASK) mw = tmpl_read4(c.mask + (size_t)ty * c.tp, tx, c.tp);
    }
    // the lane's local moments over its 4 pixels
    const int lv = r & 3;
    int n = 0, sxx = 0, sxy = 0, syy = 0, sxj = 0, syj = 0, sxr = 0, syr = 0, sjr = 0, srr = 0;
    uint32_t sjj = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const bool used = row_used && u < nu && tx + u >= 1 && tx + u <= c.tw - 2 && (!MASK || ((mw >> (8 * u)) & 1u));
        const int i = (iw >> (8 * u)) & 255;
        const int v = LUT ? (int)lut[i] : i;
        const int gxv = used ? (int)((rw >> (8 * u)) & 255) - (int)((lw >> (8 * u)) & 255) : 0;
        const int gyv = used ? (int)((dw >> (8 * u)) & 255) - (int)((uw >> (8 * u)) & 255) : 0;
        const int rv = used ? v - (int)((cw >> (8 * u)) & 255) : 0;   // unused: nothing (L[0] may not be 0)
        const int jl = (gx + u) * gyv - lv * gxv;
        n += used ? 1 : 0;
        sxx += gxv * gxv; sxy += gxv * gyv; syy += gyv * gyv;
        sxj += gxv * jl; syj += gyv * jl; sjj += (uint32_t)(jl * jl);
        sxr += gxv * rv; syr += gyv * rv; sjr += jl * rv; srr += rv * rv;
    }
    // wave totals in scalar registers (signed sums fold as their bit patterns: they fit 32 bits)
    const int64_t Sxx = wave_fold<false>((uint32_t)sxx), Syy = wave_fold<false>((uint32_t)syy);
    const int64_t Sxy = (int32_t)wave_fold<false>((uint32_t)sxy);
    const int64_t SxJ = (int32_t)wave_fold<false>((uint32_t)sxj), SyJ = (int32_t)wave_fold<false>((uint32_t)syj);
    const int64_t Sxr = (int32_t)wave_fold<false>((uint32_t)sxr), Syr = (int32_t)wave_fold<false>((uint32_t)syr);
    const int64_t SJr = (int32_t)wave_fold<false>((uint32_t)sjr);
    const int64_t Srr = wave_fold<false>((uint32_t)srr);
    const uint32_t jlo = wave_fold<false>(sjj & 0xffffu);                          // <= 64 * 65535
    const uint32_t jhn = wave_fold<false>((sjj >> 16) | ((uint32_t)n << 21));      // high halves < 2^21; n <= 256 above
    const int64_t SJJ = ((int64_t)(jhn & 0x1fffffu) << 16) + jlo;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t Xb = 2 * T.x0 - (a.pw - 1), Yb = 2 * (T.y0 + 4 * wave) - (a.ph - 1);
    int64_t f[kAlignFields];
    f[kAlnN] = jhn >> 21;
    f[kAlnHxx] = Sxx; f[kAlnHxy] = Sxy; f[kAlnHyy] = Syy;
    f[kAlnHxt] = Xb * Sxy - Yb * Sxx + 2 * SxJ;
    f[kAlnHyt] = Xb * Syy - Yb * Sxy + 2 * SyJ;
    f[kAlnHtt] = Xb * Xb * Syy - 2 * Xb * Yb * Sxy + Yb * Yb * Sxx + 4 * Xb * SyJ - 4 * Yb * SxJ + 4 * SJJ;
    f[kAlnGx] = Sxr; f[kAlnGy] = Syr;
    f[kAlnGt] = Xb * Syr - Yb * Sxr + 2 * SJr;
    f[kAlnSsd] = Srr;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kAlignFields; ++k) part[wave][k] = (unsigned long long)f[k];
    }
    __syncthreads();
    if (tid < kAlignFields) {
        const unsigned long long s = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (s) atomicAdd((unsigned long long*)&c.acc[T.job].f[tid], s);
    }
