// Temporal history of the denoiser: the demodulated colour of earlier frames, reprojected into the current camera through the first hit and blended
// with the current frame -- include/ptamd.h, "temporal history"; DESIGN.md section 9.  Nothing here is on the render path: k_temporal reads the
// accumulator and the guide sums like k_denoise_prepare does, and the two history sets the context keeps for it.
#pragma once
#include "pt_firefly.h"

namespace ptd {

struct TemporalArgs {
    const float4* accum; // the current frame's three inputs, as k_denoise_prepare reads them
    const float4* albedoHits;
    const float4* normalDepth;
    const float4* histColour; // (d.rgb, N) of the newest set; nullptr: no history (first call, after a reset)
    const float4* histGuide; // (n.xyz, z) of that set
    float4* outColour; // the other set
    float4* outGuide;
    uint32_t width, height;
    float spp, gspp;
    float kNormal, invSigmaDepth, maxHistory;
    float invW, invH;
    V3 eye, screen, u, v; // current camera (a thin lens is taken as the pinhole through eyePoint)
    // the history's camera: its eye, and the three vectors that give lambda, alpha and beta of q = X - E' as plain dot products:
    //   s0.(q x v') = q.(v' x s0),   s0.(u' x q) = q.(s0 x u'),   each divided by det = s0.(u' x v') on the host
    V3 histEye, rowLambda, rowAlpha, rowBeta;
    // k_temporal<true> (instance motion): the two motion sums of the guide pass -- (sum of displacements.xyz, 0) and (sum of the normals then.xyz, 0)
    const float4* motion;
    const float4* prevNormal;
    // k_temporal<., true> (pt_set_temporal_variance): the luminance-variance plane of the newest set (read where histColour is) and of the other set
    const float* histVariance;
    float* outVariance;
    // k_temporal<., ., true> (pt_set_temporal_response): the fast history (d_f.rgb, N_f) of the newest set (read where histColour is) and of the other
    // set, the plane of luminance pairs (L(d_f), L(d_l)) k_temporal_response reads, and the fast history's cap
    const float4* histFast;
    float4* outFast;
    float2* outLuminance;
    float fastHistory;
    // k_temporal<., ., ., true> (pt_set_firefly_clamp): the clamped plane (d.rgb, s) k_firefly made of this frame; accum and albedoHits are not read
    const float4* firefly;
};

// The blend both histories go through: h = sum w d_h / Wsum, N = min(sum w N_h + 1, cap), d_out = h + (d - h) / N.  One function, so equal sums give
// equal bits (while a history is no longer than the fast cap the fast image IS the long one).
struct Blended {
    float hr, hg, hb; // h
    float r, g, b, n; // (d_out, N)
};
__device__ __forceinline__ Blended blendHistory(float sr, float sg, float sb, float sn, float sw, const V3& d, float cap)
{
    Blended o;
    o.hr = sr / sw, o.hg = sg / sw, o.hb = sb / sw;
    o.n = fminf(sn + 1.0f, cap);
    o.r = o.hr + (d.x - o.hr) / o.n, o.g = o.hg + (d.y - o.hg) / o.n, o.b = o.hb + (d.z - o.hb) / o.n;
    return o;
}

constexpr int kTemporalTileW = kAtrousTileW, kTemporalTileH = kAtrousTileH; // the filter's tile: a wave is two rows of 32 pixels

// One thread per pixel.  Three 16-byte reads of the current frame, up to eight gathered 16-byte reads of the history (the four bilinear taps of the
// reprojected position in both images: a tap outside the image loads nothing, one whose count is zero does not load its guide), two 16-byte writes.
// The taps of a wave lie in a compact patch of the history, which the vector cache and L2 serve; there is no fixed halo to stage.  No atomics: the
// output is bit-reproducible.
// MOTION (pt_set_instance_motion): two more 16-byte reads, issued with the first three -- 144 bytes per pixel instead of 112.  The first hit is taken to where
// it WAS before it goes into the history's camera, q = (E + z D + m / gspp) - E', and the taps' normal term compares the history's normal with the
// surface's normal THEN (the sum normalised as n is).  The set written out holds the current (n, z) all the same.  Zero motion sums and prevNormal ==
// normalDepth.xyz give the plain kernel's bits.
// VARIANCE (pt_set_temporal_variance): one more plane per set, v = the population variance of the luminances the pixel's history stands for.  Up to four
// more gathered 4-byte reads, issued with the colour taps (a tap outside the image loads nothing; one that does not count is not used), and one 4-byte
// write -- 120 bytes per pixel, 152 with MOTION.  Welford's update for a running mean of weight 1 / N:
//   v_out = (1 - alpha) (v_h + alpha (l - mu)^2),  alpha = 1 / N_out,  l = L(d),  mu = L(h),  v_h = sum w v_tap / Wsum;  0 where the pixel found no history
// -- sums and products of non-negative terms, nothing subtracted but l - mu.  The colour's arithmetic is untouched: outColour and outGuide have the bits
// of the VARIANCE-less kernel.
// RESPONSE (pt_set_temporal_response): one more float4 image per set, the fast history (d_f.rgb, N_f) -- the same taps, the same b exp(-(e_n + e_z)), a
// tap counting where ITS count is positive, capped at fast_history instead of max_history.  Four more gathered 16-byte reads, issued with the colour
// taps, one 16-byte write and one 8-byte write of (L(d_f), L(d_l)) for k_temporal_response -- 152 bytes per pixel against 112; the other modes add
// what they add above.  outColour is written UN-mixed, with the bits of the RESPONSE-less kernel: k_temporal_response mixes it in place.
// FIREFLY (pt_set_firefly_clamp): d is read from the clamped plane instead of being formed here -- one 16-byte read in place of two, 96 bytes per pixel
// against 112 --, and everything downstream (the blends, l of the variance, the luminance pairs) takes the clamped d because it takes d.  Where the
// plane holds d's own bits the outputs have the bits of the FIREFLY-less kernel, which is the kernel of before.
template <bool MOTION, bool VARIANCE = false, bool RESPONSE = false, bool FIREFLY = false>
__global__ void __launch_bounds__(256) k_temporal(TemporalArgs a)
{
    const int x = blockIdx.x * kTemporalTileW + threadIdx.x, y = blockIdx.y * kTemporalTileH + threadIdx.y;
    const int W = (int)a.width, H = (int)a.height;
    if (x >= W || y >= H)
        return;
    const size_t p = (size_t)y * W + x;
    float4 s, al;
    if constexpr (FIREFLY)
        s = a.firefly[p];
    else
        s = a.accum[p], al = a.albedoHits[p];
    const float4 g = a.normalDepth[p];
    float4 mv, pn;
    if constexpr (MOTION)
        mv = a.motion[p], pn = a.prevNormal[p];
    V3 d = xyz(s);
    if constexpr (!FIREFLY)
        d = demodulatedMean(s, al, a.spp, a.gspp);
    const float4 nz = guideOf(g, a.gspp);
    const float z = nz.w;
    a.outGuide[p] = nz;
    V3 nThen = xyz(nz); // what the history's normals are compared with
    if constexpr (MOTION)
        nThen = xyz(guideOf(pn, a.gspp));

    float outR = d.x, outG = d.y, outB = d.z, outN = 1.0f;
    float outV = 0.0f;
    float fastR = d.x, fastG = d.y, fastB = d.z, fastN = 1.0f;
    if (a.histColour) {
        // world point of the first hit through the pixel centre, then into the history's camera
        const float px = ((float)x + 0.5f) * a.invW, py = ((float)y + 0.5f) * a.invH;
        const V3 D = normalize(a.screen + a.u * px + a.v * py - a.eye);
        V3 X = a.eye + D * z;
        if constexpr (MOTION)
            X = X + mk(mv.x / a.gspp, mv.y / a.gspp, mv.z / a.gspp); // where the surface was: added before the history's eye is subtracted
        const V3 q = X - a.histEye;
        const float lambda = dot(q, a.rowLambda);
        if (lambda > 0.0f) {
            const float alpha = dot(q, a.rowAlpha), beta = dot(q, a.rowBeta);
            const float fx = fminf(fmaxf((float)W * (alpha / lambda) - 0.5f, -2.0f), (float)W + 1.0f);
            const float fy = fminf(fmaxf((float)H * (beta / lambda) - 0.5f, -2.0f), (float)H + 1.0f);
            const float zq = sqrtf(dot(q, q));
            const float flx = floorf(fx), fly = floorf(fy);
            const int x0 = (int)flx, y0 = (int)fly;
            const float ax = fx - flx, ay = fy - fly;
            // the (up to) four colour taps first, as independent loads in flight together; a tap outside the image reads nothing and counts for nothing
            float4 ch[4], fh[4];
            float vh[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
                ch[t] = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (VARIANCE)
                    vh[t] = 0.0f;
                if constexpr (RESPONSE)
                    fh[t] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (tx >= 0 && tx < W && ty >= 0 && ty < H) {
                    ch[t] = a.histColour[(size_t)ty * W + tx];
                    if constexpr (RESPONSE)
                        fh[t] = a.histFast[(size_t)ty * W + tx];
                    if constexpr (VARIANCE)
                        vh[t] = a.histVariance[(size_t)ty * W + tx];
                }
            }
            // ... then the guides of the taps that count (N_h > 0; RESPONSE: in either history)
            float sr = 0.f, sg = 0.f, sb = 0.f, sn = 0.f, sw = 0.f;
            float sv = 0.f;
            float fr = 0.f, fg = 0.f, fb = 0.f, fn = 0.f, fw = 0.f;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const bool counts = ch[t].w > 0.0f;
                bool countsFast = false;
                if constexpr (RESPONSE)
                    countsFast = fh[t].w > 0.0f;
                float w = 0.0f;
                if (counts || countsFast) {
                    const float4 gh = a.histGuide[(size_t)(y0 + (t >> 1)) * W + (x0 + (t & 1))];
                    const float b = ((t & 1) ? ax : 1.0f - ax) * ((t >> 1) ? ay : 1.0f - ay);
                    w = b * __expf(-guideTerms(nThen, zq, gh, a.kNormal, a.invSigmaDepth));
                }
                if constexpr (RESPONSE) { // (w is there for either history: each takes it where its own count is positive)
                    const float wf = countsFast ? w : 0.0f;
                    fr += wf * (countsFast ? fh[t].x : 0.0f), fg += wf * (countsFast ? fh[t].y : 0.0f), fb += wf * (countsFast ? fh[t].z : 0.0f);
                    fn += wf * (countsFast ? fh[t].w : 0.0f), fw += wf;
                    w = counts ? w : 0.0f;
                }
                sr += w * (counts ? ch[t].x : 0.0f), sg += w * (counts ? ch[t].y : 0.0f), sb += w * (counts ? ch[t].z : 0.0f);
                sn += w * (counts ? ch[t].w : 0.0f), sw += w;
                if constexpr (VARIANCE)
                    sv += w * (counts ? vh[t] : 0.0f);
            }
            if (sw >= 1e-12f) {
                const Blended o = blendHistory(sr, sg, sb, sn, sw, d, a.maxHistory);
                outN = o.n, outR = o.r, outG = o.g, outB = o.b;
                if constexpr (VARIANCE) {
                    const float alpha = 1.0f / outN, delta = luminance709(d.x, d.y, d.z) - luminance709(o.hr, o.hg, o.hb);
                    outV = (1.0f - alpha) * (sv / sw + alpha * delta * delta);
                }
            }
            if constexpr (RESPONSE)
                if (fw >= 1e-12f) {
                    const Blended o = blendHistory(fr, fg, fb, fn, fw, d, a.fastHistory);
                    fastN = o.n, fastR = o.r, fastG = o.g, fastB = o.b;
                }
        }
    }
    a.outColour[p] = make_float4(outR, outG, outB, outN);
    if constexpr (VARIANCE)
        a.outVariance[p] = outV;
    if constexpr (RESPONSE) {
        a.outFast[p] = make_float4(fastR, fastG, fastB, fastN);
        a.outLuminance[p] = make_float2(luminance709(fastR, fastG, fastB), luminance709(outR, outG, outB));
    }
}

// The second half of the temporal response (include/ptamd.h, "temporal response"): per pixel the means of both luminances and the fast one's
// population variance over the 7 x 7 window clipped to the image, the mix factor
//   t = |mu_f - mu_l| / (sigma_response sigma_f / sqrt(n_p) + relative_floor (max(mu_f, mu_l) + 1e-3)),   s = clamp(t - 1, 0, 1)
// and (d, N) += s ((d_f, N_f) - (d, N)), stored in place only where s > 0 -- safe, because neighbours read the luminance plane, never colour_count.
struct ResponseArgs {
    const float2* luminance; // (L(d_f), L(d_l)), as k_temporal<., ., true> wrote it
    float4* colour; // the newest set's colour_count: read, and written where s > 0
    const float4* fast;
    float* mix; // s
    uint32_t width, height;
    float sigmaResponse, relativeFloor;
};

constexpr int kResponseR = PT_RESPONSE_RADIUS, kResponseTaps = 2 * kResponseR + 1;
constexpr int kResponseLdsW = kTemporalTileW + 2 * kResponseR, kResponseLdsH = kTemporalTileH + 2 * kResponseR; // 38 x 14

// 32 x 8 tiles of 256 threads.  The tile and a 3-pixel halo of the luminance plane are staged as two float planes of 38 x 14 in LDS (4 256 bytes); a
// lane group of 32 reads [row][x + const], 32 consecutive dwords: conflict-free, as the variance filter's staged V.  Out-of-image entries are staged
// as zeros and carry weight 0.  The weights are not a third plane: the 0 / 1 plane of the window is the outer product of a row and a column vector,
// held in 14 registers -- pass two costs a subtract, a multiply by the column's weight and a multiply-add per tap, what a third plane would cost
// without its 49 LDS reads; clipped loop bounds would have kept the loops from unrolling (a compare and a branch per tap on divergent bounds).
// Pass one needs no weights: zeros add nothing to the two sums, and n_p is the product of the two clipped extents.  Two passes, the second over
// (l_f - mu_f)^2: never E[x^2] - E[x]^2.  8 bytes read and 4 written per pixel; where s > 0, 32 more read and 16 written -- 60 at most, 12 where the
// image is steady.  Held to 64 VGPRs (8 waves per SIMD): the second pass reads the fast plane from LDS again rather than keep 49 values in registers --
// a block stages, waits and computes in turn, and it is the other blocks of the CU that fill those waits.  No atomics: bit-reproducible.
__global__ void __launch_bounds__(256, 8) k_temporal_response(ResponseArgs a)
{
    __shared__ float ldsFast[kResponseLdsH][kResponseLdsW], ldsLong[kResponseLdsH][kResponseLdsW];
    const int W = (int)a.width, H = (int)a.height;
    const int tileX = blockIdx.x * kTemporalTileW, tileY = blockIdx.y * kTemporalTileH;
    const int x = tileX + (int)threadIdx.x, y = tileY + (int)threadIdx.y;
    const bool inside = x < W && y < H;
    for (int i = (int)(threadIdx.y * kTemporalTileW + threadIdx.x); i < kResponseLdsW * kResponseLdsH; i += kTemporalTileW * kTemporalTileH) {
        const int ly = i / kResponseLdsW, lx = i - ly * kResponseLdsW;
        const int gx = tileX + lx - kResponseR, gy = tileY + ly - kResponseR;
        float2 l = make_float2(0.f, 0.f);
        if (gx >= 0 && gx < W && gy >= 0 && gy < H)
            l = a.luminance[(size_t)gy * W + gx];
        ldsFast[ly][lx] = l.x, ldsLong[ly][lx] = l.y;
    }
    __syncthreads();
    if (!inside)
        return;
    const int lx = (int)threadIdx.x, ly = (int)threadIdx.y; // the window's first entry
    float sumF = 0.f, sumL = 0.f;
#pragma unroll
    for (int j = 0; j < kResponseTaps; j++)
#pragma unroll
        for (int i = 0; i < kResponseTaps; i++)
            sumF += ldsFast[ly + j][lx + i], sumL += ldsLong[ly + j][lx + i];
    float wx[kResponseTaps], wy[kResponseTaps];
    float nx = 0.f, ny = 0.f;
#pragma unroll
    for (int i = 0; i < kResponseTaps; i++) {
        wx[i] = (x + i - kResponseR >= 0 && x + i - kResponseR < W) ? 1.0f : 0.0f;
        wy[i] = (y + i - kResponseR >= 0 && y + i - kResponseR < H) ? 1.0f : 0.0f;
        nx += wx[i], ny += wy[i];
    }
    const float np = nx * ny; // (at least 1: the pixel itself)
    const float muF = sumF / np, muL = sumL / np;
    asm volatile("" ::: "memory"); // (no instruction: the second pass reads LDS again, the first pass's 49 values do not stay in registers)
    float varF = 0.f;
#pragma unroll
    for (int j = 0; j < kResponseTaps; j++) {
        float row = 0.f;
#pragma unroll
        for (int i = 0; i < kResponseTaps; i++) {
            const float delta = ldsFast[ly + j][lx + i] - muF;
            row += (delta * wx[i]) * delta;
        }
        varF += wy[j] * row;
    }
    varF /= np;
    const float t = fabsf(muF - muL) / (a.sigmaResponse * sqrtf(varF) / sqrtf(np) + a.relativeFloor * (fmaxf(muF, muL) + 1e-3f));
    const float s = fminf(fmaxf(t - 1.0f, 0.0f), 1.0f);
    const size_t p = (size_t)y * W + x;
    a.mix[p] = s;
    if (s > 0.0f) { // the pixel's own two records are read only where they are mixed: a steady image moves 12 bytes per pixel, not 44
        const float4 c = a.colour[p], f = a.fast[p];
        a.colour[p] = make_float4(c.x + s * (f.x - c.x), c.y + s * (f.y - c.y), c.z + s * (f.z - c.z), c.w + s * (f.w - c.w));
    }
}

// pt_denoise over the history (PT_DENOISE_INPUT_TEMPORAL, _VARIANCE) with iterations == 0: the newest d re-modulated with the current albedo
__global__ void __launch_bounds__(256) k_temporal_resolve(const float4* __restrict__ histColour, const float4* __restrict__ albedoHits,
    float4* __restrict__ out, uint32_t n, float gspp, uint32_t tonemapped, float relativeAperture, float shutterTime, float ISO)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float4 h = histColour[i];
    out[i] = remodulated(h.x, h.y, h.z, albedoHits[i], gspp, tonemapped != 0u, relativeAperture, shutterTime, ISO);
}

} // namespace ptd
