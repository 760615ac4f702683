// Temporal history of the denoiser: the demodulated colour of earlier frames, reprojected into the current camera through the first hit and blended
// with the current frame -- include/ptamd.h, "temporal history"; DESIGN.md section 9.  Nothing here is on the render path: k_temporal reads the
// accumulator and the guide sums like k_denoise_prepare does, and the two history sets the context keeps for it.
#pragma once
#include "pt_denoise.h"

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
};

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
template <bool MOTION, bool VARIANCE = false>
__global__ void __launch_bounds__(256) k_temporal(TemporalArgs a)
{
    const int x = blockIdx.x * kTemporalTileW + threadIdx.x, y = blockIdx.y * kTemporalTileH + threadIdx.y;
    const int W = (int)a.width, H = (int)a.height;
    if (x >= W || y >= H)
        return;
    const size_t p = (size_t)y * W + x;
    const float4 s = a.accum[p], al = a.albedoHits[p], g = a.normalDepth[p];
    float4 mv, pn;
    if constexpr (MOTION)
        mv = a.motion[p], pn = a.prevNormal[p];
    const V3 d = demodulatedMean(s, al, a.spp, a.gspp);
    const float4 nz = guideOf(g, a.gspp);
    const float z = nz.w;
    a.outGuide[p] = nz;
    V3 nThen = xyz(nz); // what the history's normals are compared with
    if constexpr (MOTION)
        nThen = xyz(guideOf(pn, a.gspp));

    float outR = d.x, outG = d.y, outB = d.z, outN = 1.0f;
    float outV = 0.0f;
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
            float4 ch[4];
            float vh[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
                ch[t] = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (VARIANCE)
                    vh[t] = 0.0f;
                if (tx >= 0 && tx < W && ty >= 0 && ty < H) {
                    ch[t] = a.histColour[(size_t)ty * W + tx];
                    if constexpr (VARIANCE)
                        vh[t] = a.histVariance[(size_t)ty * W + tx];
                }
            }
            // ... then the guides of the taps that count (N_h > 0)
            float sr = 0.f, sg = 0.f, sb = 0.f, sn = 0.f, sw = 0.f;
            float sv = 0.f;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const bool counts = ch[t].w > 0.0f;
                float w = 0.0f;
                if (counts) {
                    const float4 gh = a.histGuide[(size_t)(y0 + (t >> 1)) * W + (x0 + (t & 1))];
                    const float b = ((t & 1) ? ax : 1.0f - ax) * ((t >> 1) ? ay : 1.0f - ay);
                    w = b * __expf(-guideTerms(nThen, zq, gh, a.kNormal, a.invSigmaDepth));
                }
                sr += w * (counts ? ch[t].x : 0.0f), sg += w * (counts ? ch[t].y : 0.0f), sb += w * (counts ? ch[t].z : 0.0f);
                sn += w * (counts ? ch[t].w : 0.0f), sw += w;
                if constexpr (VARIANCE)
                    sv += w * (counts ? vh[t] : 0.0f);
            }
            if (sw >= 1e-12f) {
                const float hr = sr / sw, hg = sg / sw, hb = sb / sw;
                outN = fminf(sn + 1.0f, a.maxHistory);
                outR = hr + (d.x - hr) / outN, outG = hg + (d.y - hg) / outN, outB = hb + (d.z - hb) / outN;
                if constexpr (VARIANCE) {
                    const float alpha = 1.0f / outN, delta = luminance709(d.x, d.y, d.z) - luminance709(hr, hg, hb);
                    outV = (1.0f - alpha) * (sv / sw + alpha * delta * delta);
                }
            }
        }
    }
    a.outColour[p] = make_float4(outR, outG, outB, outN);
    if constexpr (VARIANCE)
        a.outVariance[p] = outV;
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
