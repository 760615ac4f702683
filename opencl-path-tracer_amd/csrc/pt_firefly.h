// Firefly clamp of the denoiser: a bounded copy of the current frame's demodulated colour, which k_temporal and k_denoise_prepare read in place of
// forming d themselves -- include/ptamd.h, "firefly clamp"; DESIGN.md section 9.  Nothing here is on the render path, and the accumulator is never
// written: the stage reads the accumulator and the albedo sums and writes a plane of its own.
#pragma once
#include "pt_denoise.h"

namespace ptd {

struct FireflyArgs {
    const float4* accum; // the two inputs of demodulatedMean
    const float4* albedoHits;
    float4* plane; // (d_out.rgb, s)
    uint32_t* counts; // [0] clamped, [1] nonfinite: zeroed on the stream before the launch
    uint32_t width, height;
    float spp, gspp;
    uint32_t rank; // 1 .. PT_FIREFLY_MAX_RANK
    float scale;
};

constexpr int kFireflyR = PT_FIREFLY_RADIUS;
constexpr int kFireflyLdsW = kAtrousTileW + 2 * kFireflyR, kFireflyLdsH = kAtrousTileH + 2 * kFireflyR; // 36 x 12

// exact, whatever the compiler is told about floating point: the exponent field is not all ones
__device__ inline bool finiteBits(float f) { return (asU(f) & 0x7F800000u) != 0x7F800000u; }

struct DemodulatedPixel {
    V3 d;
    float l; // L(d)
    bool finite; // the three components and L
};
__device__ __forceinline__ DemodulatedPixel demodulatedPixel(float4 s, float4 al, float spp, float gspp)
{
    DemodulatedPixel o;
    o.d = demodulatedMean(s, al, spp, gspp);
    o.l = luminance709(o.d.x, o.d.y, o.d.z);
    o.finite = finiteBits(o.d.x) && finiteBits(o.d.y) && finiteBits(o.d.z) && finiteBits(o.l);
    return o;
}

// 32 x 8 tiles of 256 threads, k_temporal_response's layout.  The tile and a 2-pixel halo of the LUMINANCE of d are staged as one float plane of 36 x 12
// in LDS (1 728 bytes), every element from its own two 16-byte loads; an entry outside the image or not finite is staged as -infinity, which no finite
// luminance is.  A thread stages its own pixel first and keeps that d in registers -- the centre is loaded and demodulated once --, then the first 176
// threads stage the halo: two rows of 36 above, two below, two columns of 8 on either side (432 elements per 256 pixels: 54 bytes read per pixel
// through the vector cache, 32 of them from memory).  The 24 taps are ds_read_b32 at [row][x + const]: a lane group of 32 reads 32 consecutive
// dwords, 32 different banks.
// The four largest neighbours are kept sorted in registers, t0 >= t1 >= t2 >= t3, all -infinity at first.  Inserting v is
//   t3 = med3(t2, t3, v),  t2 = med3(t1, t2, v),  t1 = med3(t0, t1, v),  t0 = max(t0, v)
// (the k-th largest of the old four and v is the median of its two old neighbours and v): four VALU operations per tap, no loop bound that diverges,
// no sort, no count -- fewer than `rank` neighbours counted exactly when t[rank - 1] is still -infinity, and the cap is +infinity then.
// 32 bytes read and 16 written per pixel.  The counters: one ballot and popcount per wave and counter, one integer atomicAdd by the wave's first lane
// where the count is not zero; no float atomics, plane and counts are bit-reproducible.
constexpr int kFireflyHaloRow = 2 * kFireflyR * kFireflyLdsW; // 144: the entries of the rows above and below the tile
constexpr int kFireflyHalo = kFireflyLdsW * kFireflyLdsH - kAtrousTileW * kAtrousTileH; // 176
static_assert(kFireflyHalo == kFireflyHaloRow + 2 * kFireflyR * kAtrousTileH && kFireflyHalo <= kAtrousTileW * kAtrousTileH, "the halo is staged in one pass");

__global__ void __launch_bounds__(256) k_firefly(FireflyArgs a)
{
    __shared__ float ldsL[kFireflyLdsH][kFireflyLdsW];
    const int W = (int)a.width, H = (int)a.height;
    const int tileX = blockIdx.x * kAtrousTileW, tileY = blockIdx.y * kAtrousTileH;
    const int x = tileX + (int)threadIdx.x, y = tileY + (int)threadIdx.y;
    const bool inside = x < W && y < H;
    const size_t p = (size_t)y * W + x; // (an address only where `inside`)
    const float never = -__builtin_inff();
    DemodulatedPixel dp;
    dp.d = mk(0.0f), dp.l = never, dp.finite = false;
    if (inside)
        dp = demodulatedPixel(a.accum[p], a.albedoHits[p], a.spp, a.gspp);
    ldsL[threadIdx.y + kFireflyR][threadIdx.x + kFireflyR] = inside && dp.finite ? dp.l : never;
    const int t = (int)(threadIdx.y * kAtrousTileW + threadIdx.x);
    if (t < kFireflyHalo) {
        int ly, lx;
        if (t < kFireflyHaloRow) { // rows 0, 1 and 10, 11, whole
            const int row = t / kFireflyLdsW;
            ly = row < kFireflyR ? row : row + kAtrousTileH, lx = t - row * kFireflyLdsW;
        } else { // columns 0, 1 and 34, 35 of the tile's eight rows
            const int u = t - kFireflyHaloRow, c = u & (2 * kFireflyR - 1);
            ly = kFireflyR + u / (2 * kFireflyR), lx = c < kFireflyR ? c : c + kAtrousTileW;
        }
        const int gx = tileX + lx - kFireflyR, gy = tileY + ly - kFireflyR;
        float l = never;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t q = (size_t)gy * W + gx;
            const DemodulatedPixel dq = demodulatedPixel(a.accum[q], a.albedoHits[q], a.spp, a.gspp);
            if (dq.finite)
                l = dq.l;
        }
        ldsL[ly][lx] = l;
    }
    __syncthreads();
    bool clamped = false, nonfinite = false;
    if (inside) {
        const int lx = (int)threadIdx.x, ly = (int)threadIdx.y; // the window's first entry
        float t0 = never, t1 = never, t2 = never, t3 = never;
#pragma unroll
        for (int j = 0; j <= 2 * kFireflyR; j++)
#pragma unroll
            for (int i = 0; i <= 2 * kFireflyR; i++) {
                if (i == kFireflyR && j == kFireflyR) // the centre is not its own neighbour
                    continue;
                const float v = ldsL[ly + j][lx + i];
                t3 = __builtin_amdgcn_fmed3f(t2, t3, v);
                t2 = __builtin_amdgcn_fmed3f(t1, t2, v);
                t1 = __builtin_amdgcn_fmed3f(t0, t1, v);
                t0 = fmaxf(t0, v);
            }
        const float r = a.rank == 1u ? t0 : (a.rank == 2u ? t1 : (a.rank == 3u ? t2 : t3));
        const float cap = r == never ? __builtin_inff() : a.scale * (r + 1e-3f);
        float4 out = make_float4(dp.d.x, dp.d.y, dp.d.z, 1.0f);
        if (!dp.finite) {
            out = make_float4(0.f, 0.f, 0.f, 0.f);
            nonfinite = true;
        } else if (dp.l > cap) {
            const float s = cap / dp.l;
            out = make_float4(dp.d.x * s, dp.d.y * s, dp.d.z * s, s);
            clamped = true;
        }
        a.plane[p] = out;
    }
    const unsigned long long nClamped = __ballot(clamped), nNonfinite = __ballot(nonfinite);
    if (((threadIdx.y * kAtrousTileW + threadIdx.x) & 63u) == 0u) {
        if (nClamped)
            atomicAdd(&a.counts[0], (uint32_t)__popcll(nClamped));
        if (nNonfinite)
            atomicAdd(&a.counts[1], (uint32_t)__popcll(nNonfinite));
    }
}

} // namespace ptd
