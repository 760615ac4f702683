// Device vector helpers and the two PRNGs of the path.
#pragma once
#include "pt_hostdev.h" // (V3 and its operators)
#include <cfloat>

namespace ptd {

__device__ inline float saturate(float a) { return fminf(fmaxf(a, 0.0f), 1.0f); }
__device__ inline float asF(uint32_t u) { return __uint_as_float(u); }
__device__ inline uint32_t asU(float f) { return __float_as_uint(f); }

// ---- division, square root and normalize of the shading kernel without the compiler's range scaling --------------------------
// The device pass is built with -fno-hip-fp32-correctly-rounded-divide-sqrt (ptamd/build.py), and what the compiler makes of the plain
// operators under it is v_rcp_f32 / v_sqrt_f32 wrapped in a rescaling: `a / b` = ldexp(frexp_mant(a) * rcp(frexp_mant(b)), frexp_exp(a) -
// frexp_exp(b)), 8 vector instructions; sqrtf(x) = x < 2^-96 ? ldexp(sqrt(ldexp(x, 32)), -16) : sqrt(x), 6.  frexp and ldexp move powers
// of two, which is exact, and the two hardware instructions see the same mantissa either way; the wrapping only serves operands they flush
// (denormals) and reciprocals that would be denormal.  The helpers below are the bare instructions.
// CONTRACT: fastDiv(a, b), fastSqrt(x), fastDiv(V3, s) and fastNormalize(v) return the bits of `a / b`, sqrtf(x), `v / s` and normalize(v)
// as this build compiles them whenever every operand and every result is a normal float, +-0, +-inf or NaN.  They differ only for a denormal
// denominator or one with |b| > 2^126 (its reciprocal is denormal: flushed to zero), a denormal x under the root (taken as zero), and a
// denormal quotient (flushed).  k_shade's denominators are cosines, lengths of scene-scale vectors, material parameters and constants, and
// where one of them reaches zero the plain operator divides by zero just the same.  v_rsq_f32 is NOT used for normalize: it rounds
// differently from rcp(sqrt(x)) and would change bits.  The product is kept out of fused multiply-adds (contract off): the rescaled form it
// replaces ends in an ldexp, which no neighbouring addition could ever be fused with.
// PT_SHADE_RANGE_SAFE = 1: the helpers are the plain operators and sqrtf -- the code before they existed, for A / B and equality checks
// (tests/test_gpu_fastmath.py, k_math_probe).  fastRcp is the bare instruction in either build (the traversal kernels use it).
#ifndef PT_SHADE_RANGE_SAFE
#define PT_SHADE_RANGE_SAFE 0
#endif
__device__ inline float fastRcp(float x) { return __builtin_amdgcn_rcpf(x); } // v_rcp_f32, 1 ulp
#if PT_SHADE_RANGE_SAFE
__device__ inline float fastDiv(float a, float b) { return a / b; }
__device__ inline float fastSqrt(float x) { return sqrtf(x); }
__device__ inline V3 fastDiv(V3 a, float s) { return a / s; }
__device__ inline V3 fastNormalize(V3 a) { return normalize(a); }
__device__ inline V3 fastNormalize(V3 a, float) { return normalize(a); }
#else
__device__ inline float fastDiv(float a, float b)
{
#pragma clang fp contract(off)
    return a * fastRcp(b);
}
__device__ inline float fastSqrt(float x) // v_sqrt_f32, 1 ulp
{
    float r = __builtin_amdgcn_sqrtf(x);
    asm("" : "+v"(r)); // opaque to the optimiser, which would merge a reciprocal taken of this root into one v_rsq_f32 (see above); no instruction
    return r;
}
__device__ inline V3 fastDiv(V3 a, float s) // one reciprocal, three products
{
#pragma clang fp contract(off)
    const float r = fastRcp(s);
    return { a.x * r, a.y * r, a.z * r };
}
__device__ inline V3 fastNormalize(V3 a, float len2) // len2 = dot(a, a), which the caller already has: one root, one reciprocal, three products
{
    const float r = fastRcp(fastSqrt(len2));
    {
#pragma clang fp contract(off)
        return { a.x * r, a.y * r, a.z * r };
    }
}
__device__ inline V3 fastNormalize(V3 a) { return fastNormalize(a, dot(a, a)); } // (the dot contracted as normalize's is: pt_hostdev.h)
#endif

// ---- production PRNG: counter-based, stateless (replaces clRNG; DESIGN.md "PRNG") ------------
// The stream of a path is named by 64 bits -- k0 = mix32(pixel ^ mix32(seed ^ phi)), k1 = mix32(sample ^ c), both
// bijections, so distinct (pixel, sample) pairs never share a stream (a 32-bit key would: a batch holds ~2^32 pairs) --
// and walks a Weyl sequence with its own odd step gamma = mix32(k0 ^ k1 ^ c') | 1, so two streams do not overlap in
// shifted windows either.  Draw number ctr = depth * 16 + dim + 1 (depth 0 = camera ray, 1 + b = shade at bounce b;
// dim = index of the draw inside that stage, draw order of SURVEY Appendix C):
//   x = k0 + gamma * ctr;  x ^= x >> 16;  x *= 0x21f0aaad;  x ^= k1;  x ^= x >> 15;  x *= 0x735a2d97;  x ^= x >> 15
//   u = (x >> 8) * 2^-24 in [0,1)      ('lowbias32' finaliser with the second key word injected between its rounds).
// A stage owns the 16 slots dim = 0..15; a 17th draw would be the next depth's first.  tests/test_prng_cpu.py holds that budget (the most draws any stage
// makes, over every integrator, light choice and camera, counted by the oracle) and tests/test_gpu_prng.py states the overlap as a fact.
// Zero bytes of state traffic; independent of queue slot, compaction order and GPU count.
__host__ __device__ inline uint32_t mix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x21f0aaadu;
    x ^= x >> 15;
    x *= 0x735a2d97u;
    x ^= x >> 15;
    return x;
}
struct CounterKey {
    uint32_t k0, k1, gamma;
};
__host__ __device__ inline CounterKey counterKey(uint32_t pixel, uint32_t sample, uint32_t seed)
{
    CounterKey k;
    k.k0 = mix32(pixel ^ mix32(seed ^ 0x9E3779B9u));
    k.k1 = mix32(sample ^ 0x85EBCA6Bu);
    k.gamma = mix32(k.k0 ^ k.k1 ^ 0xC2B2AE35u) | 1u;
    return k;
}
__host__ __device__ inline uint32_t counterHash(uint32_t weyl, uint32_t k1)
{
    uint32_t x = weyl;
    x ^= x >> 16;
    x *= 0x21f0aaadu;
    x ^= k1;
    x ^= x >> 15;
    x *= 0x735a2d97u;
    x ^= x >> 15;
    return x;
}

// ---- parity PRNG: clRNG LFSR113 (third_party/clRNG/include/clRNG/private/lfsr113.c.h:61-93) ----
struct Rng {
    uint32_t g0, g1, g2, g3; // LFSR113 state (parity mode)
    uint32_t weyl, gamma, k1; // counter mode: weyl = k0 + gamma * (depth*16 + dim + 1) of the NEXT draw
    bool lfsr;

    __device__ inline float u01()
    {
        if (lfsr) {
            uint32_t b;
            b = ((g0 << 6) ^ g0) >> 13;
            g0 = ((g0 & 4294967294u) << 18) ^ b;
            b = ((g1 << 2) ^ g1) >> 27;
            g1 = ((g1 & 4294967288u) << 2) ^ b;
            b = ((g2 << 13) ^ g2) >> 21;
            g2 = ((g2 & 4294967280u) << 7) ^ b;
            b = ((g3 << 3) ^ g3) >> 12;
            g3 = ((g3 & 4294967168u) << 13) ^ b;
            uint32_t z = g0 ^ g1 ^ g2 ^ g3;
            return (float)((double)z * 2.3283063e-10); // double constant, as clRNG (can round to 1.0f)
        }
        const uint32_t h = counterHash(weyl, k1);
        weyl += gamma;
        return (float)(h >> 8) * (1.0f / 16777216.0f);
    }
    // clrngLfsr113RandomInteger(i, j) = i + (int)((j-i+1) * U01)
    __device__ inline int randomInteger(int i, int j)
    {
        int r = i + (int)((float)(j - i + 1) * u01());
        if (!lfsr && r > j)
            r = j;
        return r;
    }
};

__device__ inline Rng rngCounter(uint32_t pixel, uint32_t sample, uint32_t seed, uint32_t depth)
{
    Rng r;
    r.g0 = r.g1 = r.g2 = r.g3 = 0;
    const CounterKey k = counterKey(pixel, sample, seed);
    r.weyl = k.k0 + k.gamma * (depth * 16u + 1u);
    r.gamma = k.gamma;
    r.k1 = k.k1;
    r.lfsr = false;
    return r;
}
__device__ inline Rng rngLfsrLoad(const uint4* streams, uint32_t slot)
{
    uint4 s = streams[slot];
    Rng r;
    r.g0 = s.x, r.g1 = s.y, r.g2 = s.z, r.g3 = s.w;
    r.weyl = r.gamma = r.k1 = 0;
    r.lfsr = true;
    return r;
}
__device__ inline void rngLfsrStore(uint4* streams, uint32_t slot, const Rng& r) { streams[slot] = make_uint4(r.g0, r.g1, r.g2, r.g3); }

} // namespace ptd
