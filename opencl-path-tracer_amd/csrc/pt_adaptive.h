// Adaptive sampling: the bookkeeping between two rounds of a converging render -- include/ptamd.h, "adaptive sampling"; DESIGN.md section 10.  Nothing
// here is on the render path: a round's samples are two plain pt_render runs into the half accumulators A and B; the kernels below count them, judge
// every 8 x 8 block by the difference of its two halves and write the accumulator the rest of the library reads.
#pragma once
#include "pt_firefly.h"

namespace ptd {

// The integer counters of one evaluation, zeroed on the stream before the launch.  Every wave adds to them, and 32 400 waves (1080p) adding to five words
// of one cache line take 1.2 ms -- the atomics of one line are served one after the other, whatever the kernel's 60 bytes per pixel take.  So there are
// kAdaptiveStripes copies, each on a 128-byte line of its own; block b adds to copy b % kAdaptiveStripes, the host combines them after the read-back.
constexpr uint32_t kAdaptiveStripes = 64;
struct alignas(128) AdaptiveCounters {
    uint32_t active; // blocks whose next flag is set
    uint32_t nonfinite; // pixels whose e was not finite
    uint32_t maxErrorBits; // the bits of the largest E_b: E_b >= 0, so unsigned order is float order
    uint32_t maxNotCount; // ~(the smallest block count): a maximum, so that zero is its neutral element too
    unsigned long long total; // the sum of counts over the image
};

struct AdaptiveArgs {
    const float4* A; // the two half accumulators: sums, like the accumulator
    const float4* B;
    uint32_t* counts; // per pixel
    float* error; // per pixel: e
    float* blockError; // per block: E_b
    uint32_t* flags; // per block: read as the set that was just rendered, written as the next round's
    AdaptiveCounters* counters; // kAdaptiveStripes of them
    float4* accum; // the published accumulator
    uint32_t width, height, blocksX, blocks;
    uint32_t add; // 2h: what the round gave every pixel of a flagged block (0: evaluate the state as it stands)
    uint32_t spp; // S' = S + add: the largest count, pt_samples_per_pixel after the round
    uint32_t minSamples, maxSamples;
    float threshold;
};

// (A + B) * (S' / n): each pixel's mean times the global sample count, so that whoever divides by pt_samples_per_pixel gets the mean.  n == S' selects
// the scale 1 instead of computing it -- x / x is 1 only under a correctly rounded division, which this library's build does not use -- and leaves the
// bits of A + B; n == 0 is written 0.
__device__ __forceinline__ float4 adaptivePublished(float4 a, float4 b, uint32_t n, uint32_t spp)
{
    if (n == 0u)
        return make_float4(0.f, 0.f, 0.f, 0.f);
    const float s = n == spp ? 1.0f : (float)spp / (float)n;
    return make_float4((a.x + b.x) * s, (a.y + b.y) * s, (a.z + b.z) * s, 0.f);
}

// One wave64 per 8 x 8 block, four blocks per workgroup of 256; lane l is pixel (8 bx + l % 8, 8 by + l / 8).  The eight lanes of a row read one
// 128-byte line of A and one of B: no LDS.  A lane outside the image (blocks on the right and bottom edges) loads nothing and adds +0 to the sums.
// The count of a block is constant over its pixels (pt_render_adaptive keeps it so, pt_write_adaptive checks it), so the wave takes it from lane 0,
// whose pixel is always inside.  E_b is the butterfly sum (__shfl_xor over 32, 16, ... 1: every lane ends with the same bits) divided by the number
// of pixels inside.  One integer atomic per wave and counter, by lane 0; no float atomics, every plane and counter is bit-reproducible.
// 32 B read + 4 B read and written (counts) + 4 B (e) + 16 B (accumulator) per pixel: 60 B.
__global__ void __launch_bounds__(256) k_adaptive_eval(AdaptiveArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6); // wave-uniform
    if (b >= a.blocks)
        return;
    const uint32_t bx = b % a.blocksX, by = b / a.blocksX;
    const uint32_t x = bx * 8u + (lane & 7u), y = by * 8u + (lane >> 3);
    const bool inside = x < a.width && y < a.height;
    const size_t p = (size_t)y * a.width + x; // (an address only where `inside`)
    const bool wasActive = a.add != 0u && a.flags[b] != 0u;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
    uint32_t n = 0;
    if (inside) {
        A = a.A[p], B = a.B[p];
        n = a.counts[p] + (wasActive ? a.add : 0u);
        if (wasActive)
            a.counts[p] = n;
    }
    float e = 0.0f;
    bool bad = false;
    if (inside && n > 0u) {
        const float fn = (float)n, hn = fn * 0.5f; // (n is even: exactly n / 2)
        const float mr = (A.x + B.x) / fn, mg = (A.y + B.y) / fn, mb = (A.z + B.z) / fn;
        const float num = fabsf(A.x / hn - B.x / hn) + fabsf(A.y / hn - B.y / hn) + fabsf(A.z / hn - B.z / hn);
        const float den = 2.0f * sqrtf(fmaxf(mr + mg + mb, 0.0f) + 1e-3f);
        e = num / den;
        bad = !finiteBits(e);
        if (bad) // more samples never cure it: it must not keep its block alive for ever
            e = 0.0f;
    }
    if (inside) {
        a.error[p] = e;
        a.accum[p] = adaptivePublished(A, B, n, a.spp);
    }
    float sum = e;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        sum += __shfl_xor(sum, m, 64);
    const unsigned long long nBad = __ballot(bad);
    const uint32_t countB = (uint32_t)__shfl((int)n, 0, 64);
    if (lane == 0u) {
        const uint32_t nB = min(8u, a.width - bx * 8u) * min(8u, a.height - by * 8u);
        const float Eb = sum / (float)nB;
        const bool active = countB < a.minSamples || (countB < a.maxSamples && !(Eb < a.threshold));
        a.blockError[b] = Eb;
        a.flags[b] = active ? 1u : 0u;
        AdaptiveCounters* k = a.counters + (b % kAdaptiveStripes);
        if (active)
            atomicAdd(&k->active, 1u);
        if (nBad)
            atomicAdd(&k->nonfinite, (uint32_t)__popcll(nBad));
        atomicMax(&k->maxErrorBits, asU(Eb));
        atomicMax(&k->maxNotCount, ~countB);
        atomicAdd(&k->total, (unsigned long long)countB * nB);
    }
}

} // namespace ptd
