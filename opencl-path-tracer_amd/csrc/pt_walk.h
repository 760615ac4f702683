// What every traversal kernel spells the same (k_trace, k_trace_team, k_trace_packet, k_trace_multi): the launch arguments, the diagnostics
// macros and the STEPS of the walk -- a ray's zero-component fix-up, the slab test of a 4-wide quantised node, the sort of its children, a
// triangle record's fetch, Moeller-Trumbore and its accept test, a ray taken into an instance, the two ways a ray ends.  Each is a plain
// function of values, written once: "the same hits, to the bit" is what the tests of the packet, bundle and team kernels assert against
// k_trace, and a step that exists twice has to be kept bit-compatible by hand.  The loops, stacks and votes are the kernels' own.
#pragma once
#include "pt_shade.h"
#include <type_traits>

namespace ptd {

typedef float f2 __attribute__((ext_vector_type(2)));

// guided self-scheduling of the queue claims (k_trace, k_trace_packet): a claim takes at most (entries left) / (waves x this), so that towards the end of
// the queue no wave is left with a long span while the others have run dry.  Unguided / 1 / 2 / 4: 8.47 / 8.52 / 8.50 / 8.43 Grays/s
constexpr uint32_t kGuidedSpans = 1;

struct TraceArgs {
    SceneDev sc;
    // closest-hit: rays from (rayO, rayD), results to (hit, inst)
    // any-hit: rays from (shO, shD, shC); unoccluded contributions are added to accum
    const float4* rayO;
    const float4* rayD;
    const float4* rayC;
    float4* hit;
    int32_t* inst;
    AccumView accum;
    uint32_t* occluded; // optional (test hook): 1/0 per shadow ray
    // queue words of this launch, all in the sample's control block (one pointer + the pass index instead of three
    // pointers: the any-hit kernel sits at the scalar-register limit of 7 waves per SIMD):
    //   entries in the queue  ctl->extCount[pass] / shadowCount[pass]; fetch cursor (zero at launch)  ctl->extCursor[pass] /
    //   shadowCursor[pass]; any-hit launches add their unoccluded rays (= accumulator updates) to ctl->depositsShadow
    Control* ctl;
    uint32_t pass;
    // packet kernel, first pass of a batch: the camera rays are generated from the entry index instead of read from the queue
    uint32_t fused;
    uint32_t noOrigins; // fused bundles of a pinhole camera: only the direction (with the pixel in .w) is queued for k_shade, which knows the eye and derives the rest from the entry index
    const uint32_t* pixelList;
    FrameParams fp;
    uint32_t* spill; // kSpillStack * totalThreads dwords
    uint32_t totalThreads;
    uint32_t parityShadow; // any-hit: entries carry a FINISHED flag in rayC.w (reference semantics)
    // k_trace<., true>: the table of folded instance transforms, entry 1 + k = (1/s, w) of instance k (the identity for instances that take the general
    // route), entry 0 = the identity; instFoldCount 0: nothing is folded (more instances than the table holds, parity mode, PT_FLAG_PARKED_INSTANCES)
    // k_trace<., 2> (the general route): the ENTRY records, two float4 per instance -- (1 / s, w) and (root reference, simple flag, s, -); instFoldCount != 0: some
    // entered instance is NOT a translation + uniform scale (its 3 x 4 rows are wanted)
    const float4* instFold;
    uint32_t instFoldCount;
};

#ifdef PT_TRACE_STATS
// diagnostic build only (tools/mkvariants.sh stats "-DPT_TRACE_STATS"): where do the lanes of a wave go?  The production build compiles every macro to nothing.
// k_trace: [0] iterations, [1] sum of active lanes, [2..4] iterations per kind, [5..7] lanes served per kind, [8] hand-outs, [9] rays, [10..17] wave cycles per phase
__device__ unsigned long long g_traceStats[64]; // [0..17] closest-hit launches, [24..41] any-hit launches, [48..63] packet and bundle kernels
constexpr int kTraceStats = 18;
#define PT_STAT_BEGIN unsigned long long statAcc[kTraceStats] = {}
#define PT_STAT(i, v) statAcc[i] += (unsigned long long)(v)
#define PT_TIC(t) const unsigned long long t = __builtin_readcyclecounter()
#define PT_TOC(i, t) statAcc[i] += __builtin_readcyclecounter() - t
#define PT_STAT_END(base)                                   \
    if (lane == 0)                                          \
        for (int i = 0; i < kTraceStats; i++)               \
            atomicAdd(&g_traceStats[i + (base)], statAcc[i])
#else
#define PT_STAT_BEGIN
#define PT_STAT(i, v)
#define PT_TIC(t)
#define PT_TOC(i, t)
#define PT_STAT_END(base)
#endif

// v_fma_f32 that stays a plain v_fma_f32 (the vectoriser would pack two of them into one v_pk_fma_f32: a half-rate instruction that competes with the
// conversions, compares and selects around it, while a plain FP32 multiply-add next to one of those issues at about half its price -- measured,
// profiles/round5/r5r_valu_issue_pairs.md: v_cmp / v_cndmask / v_min3 / v_cvt_f32_ubyte + v_fma_f32 pairs take 2.55 units against 2.0 for the half-rate one alone)
__device__ inline float fmaPlain(float a, float b, float c)
{
    float r;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// 3 * x as one shift-add (the compiler turns "x * 48" and "(x + 2 x) << 4" alike into v_mul_lo_u32: a quarter-rate instruction)
__device__ inline uint32_t times3(uint32_t x)
{
    uint32_t r;
    asm("v_lshl_add_u32 %0, %1, 1, %1" : "=v"(r) : "v"(x));
    return r;
}
// the distances to a child's entry and exit planes of one axis: q * a + b for both.  (Rounds 2-4 built them as 12 v_pk_fma_f32 instead of 24 v_fma_f32:
// 11 040 -> 11 270 Mrays/s without the packed form, see fmaPlain)
__device__ inline f2 planePair(const f2 q, const float a, const float b) { return { fmaPlain(q.x, a, b), fmaPlain(q.y, a, b) }; }
// Reciprocal direction for the slab test, clamped to +-1e18: a zero (or FLT_MIN, scene.cl:123-137)
// component then yields plane distances of +-1e18 * (b - o) -- far beyond any scene, with the correct
// sign -- instead of the inf - inf = NaN the one-FMA form would produce from an infinite reciprocal.
__device__ inline float rcpSlab(float x) { return fminf(fmaxf(fastRcp(x), -1e18f), 1e18f); }

// The reference nudges exactly-zero components of the ray it takes into an instance (NO_PARALLEL_RAYS, scene.cl:123-137).  Instances copied to
// world space are never "entered", so every kernel applies the same nudge to the world-space ray it starts with: identical for the identity and
// axis-aligned transforms, and the top-level box tests do not notice 1e-38.
template <typename Vec> // V3, or a queue entry's float4 (.w -- length / pixel / state -- stays)
__device__ inline void nudgeZero(Vec& o, Vec& d)
{
    if (d.x == 0.0f) d.x = FLT_MIN;
    if (d.y == 0.0f) d.y = FLT_MIN;
    if (d.z == 0.0f) d.z = FLT_MIN;
    if (o.x == 0.0f) o.x = -FLT_MIN;
    if (o.y == 0.0f) o.y = -FLT_MIN;
    if (o.z == 0.0f) o.z = -FLT_MIN;
}

// ---- inner step: the four quantised child boxes of a WideNode (pt_device.h) against one ray ----------------------------------------------
// box plane = origin + scale * q  =>  t = q * (scale / d) + (origin - o) / d : one FMA per plane.  (origin - o) / d comes from the live registers:
// keeping -o/d around as well would cost three VGPRs, and 72 is what 7 waves per SIMD allow.  Entry / exit planes are chosen by the sign of the
// ray direction (whole dwords: 4 children at once) instead of min/max per plane pair; an empty slot is an inverted box (q 255..0) and can never
// satisfy exit >= entry -- and if round-off ever made it, its reference is a degenerate triangle.
// A, B, C: the node's first three 16-byte words (origin + x scale | x and y planes | z planes + y and z scales); the packet kernels bring A and the
// scales of C through scalar loads and the plane dwords through vector loads, the per-ray kernels all three as vector loads: values either way.
struct SlabSetup {
    float ax, ay, az, bx, by, bz; // t = q * a + b per axis
    uint32_t qnx, qfx, qny, qfy, qnz, qfz; // entry (near) and exit (far) plane bytes of the four children
};
// (two halves, so that the signs are taken AFTER the coefficients where they come from invDir: the order the kernels were written in, and the per-ray
// kernels' instruction streams depend on it)
__device__ inline void slabCoefficients(SlabSetup& s, const uint4 A, const uint4 C, const V3 o, const V3 invDir)
{
    s.ax = asF(A.w) * invDir.x, s.ay = asF(C.z) * invDir.y, s.az = asF(C.w) * invDir.z;
    s.bx = (asF(A.x) - o.x) * invDir.x, s.by = (asF(A.y) - o.y) * invDir.y, s.bz = (asF(A.z) - o.z) * invDir.z;
}
__device__ inline void slabPlanes(SlabSetup& s, const uint4 B, const uint4 C, const bool nx, const bool ny, const bool nz)
{
    s.qnx = nx ? B.y : B.x, s.qfx = nx ? B.x : B.y;
    s.qny = ny ? B.w : B.z, s.qfy = ny ? B.z : B.w;
    s.qnz = nz ? C.y : C.x, s.qfz = nz ? C.x : C.y;
}
// nx, ny, nz: invDir's signs, for the packet kernels, which keep them per packet (wave-uniform on the beam walk's packets) ...
__device__ inline SlabSetup slabSetup(const uint4 A, const uint4 B, const uint4 C, const V3 o, const V3 invDir, const bool nx, const bool ny, const bool nz)
{
    SlabSetup s;
    slabCoefficients(s, A, C, o, invDir);
    slabPlanes(s, B, C, nx, ny, nz);
    return s;
}
// ... and taken from invDir here, for the per-ray and team kernels
__device__ inline SlabSetup slabSetup(const uint4 A, const uint4 B, const uint4 C, const V3 o, const V3 invDir)
{
    SlabSetup s;
    slabCoefficients(s, A, C, o, invDir);
    slabPlanes(s, B, C, invDir.x < 0.f, invDir.y < 0.f, invDir.z < 0.f);
    return s;
}
// (entry, exit) distance of child k.  The accept test of bvh.cl:72,114 on the (slightly larger) quantised box is the caller's: the per-ray and team
// kernels test exit >= entry && exit >= 0 && entry < limit, the packet kernels a folded form with ballots.  Called per child inside the callers' unrolled
// loops: all four children into arrays ahead of the accept tests costs k_trace 3 to 6 instructions and another schedule.
__device__ inline f2 childSlab(const SlabSetup& s, const int k)
{
    const f2 qx = { (float)((s.qnx >> (8 * k)) & 0xFFu), (float)((s.qfx >> (8 * k)) & 0xFFu) };
    const f2 qy = { (float)((s.qny >> (8 * k)) & 0xFFu), (float)((s.qfy >> (8 * k)) & 0xFFu) };
    const f2 qz = { (float)((s.qnz >> (8 * k)) & 0xFFu), (float)((s.qfz >> (8 * k)) & 0xFFu) };
    const f2 tx = planePair(qx, s.ax, s.bx), ty = planePair(qy, s.ay, s.by), tz = planePair(qz, s.az, s.bz);
    return { fmaxf(fmaxf(tx.x, ty.x), tz.x), fminf(fminf(tx.y, ty.y), tz.y) };
}

// the four (entry distance, reference) pairs of a node, invisible children at +inf: compare-exchange of two of them
__device__ inline void sortSwap(float& ki, float& kj, uint32_t& ri, uint32_t& rj)
{
    const bool sw = kj < ki;
    const float tk = sw ? kj : ki;
    kj = sw ? ki : kj;
    ki = tk;
    const uint32_t tr = sw ? rj : ri;
    rj = sw ? ri : rj;
    ri = tr;
}
// any occluder will do: only move the nearest visible child to the front (three comparators; the pushed children stay nearly ordered, which is worth
// more than picking the nearest with two minima -- 72.6 against 70.5-70.9 ms of shadow traversal per batch -- and the full sort buys nothing: 72.4)
__device__ inline void sort4NearestToFront(float (&key)[4], uint32_t (&ref)[4])
{
    sortSwap(key[0], key[1], ref[0], ref[1]), sortSwap(key[2], key[3], ref[2], ref[3]), sortSwap(key[0], key[2], ref[0], ref[2]);
}
// nearest first: the full 5-comparator network.  (Closest hit with three / four comparators -- the nearest first, the others as they come / and the
// farthest last -- was measured: 12 064 / 12 003 against 12 012-12 038 Mrays/s, the saved selects go into extra node visits.)
__device__ inline void sort4Nearest(float (&key)[4], uint32_t (&ref)[4])
{
    sort4NearestToFront(key, ref);
    sortSwap(key[1], key[3], ref[1], ref[3]), sortSwap(key[1], key[2], ref[1], ref[2]);
}

// ---- leaf step ------------------------------------------------------------------------------------------------------------------
// a triangle record's first 36 bytes (TriIsect a, b, c.x) -> vertex and edges
__device__ inline void triEdges(const float4 ta, const float4 tb, const float tcx, V3* v0, V3* e1, V3* e2)
{
    *v0 = mk(ta.x, ta.y, ta.z), *e1 = mk(ta.w, tb.x, tb.y), *e2 = mk(tb.z, tb.w, tcx);
}
// ... fetched per lane: base (scalar registers) + 32-bit byte offset, one shift instead of two 64-bit vector operations per step (nodes and triangle
// records < 4 GB: refused at upload otherwise, ptamd.hip).  The packet kernels fetch theirs through scalar loads and call triEdges.
__device__ inline void fetchTri(const SceneDev& sc, const uint32_t index, V3* v0, V3* e1, V3* e2)
{
    static_assert(sizeof(TriIsect) == 48, "48 = 3 << 4: a shift-add and a shift instead of a quarter-rate 32-bit multiply");
    const TriIsect* tp = (const TriIsect*)((const char*)sc.tris + (size_t)(uint32_t)(times3(index) << 4));
    const float4 ta = tp->a, tb = tp->b;
    const float tcx = tp->c.x;
    triEdges(ta, tb, tcx, v0, e1, e2);
}

// Moeller-Trumbore (shapes.cl:20-72), operation by operation.  Rounds 1-4 wrote the test as cross / dot expressions and left the choice of fused
// multiply-adds to the compiler: every kernel then had to happen on the same choice ("the same hits as k_trace, to the bit" is what the tests of the
// packet, bundle and team kernels assert), and a build option that changes the choice in one of them (round 5: -fno-slp-vectorize) moves
// barycentrics in their fifth digit (cancellation in T x e1).  So the sequence those builds emitted is spelled out once, for every kernel:
//   cross(a, b).x = fma(a.y, b.z, -(a.z * b.y))              dot(a, b) = fma(a.z, b.z, fma(a.x, b.x, a.y * b.y))
//   det           = e1.z * P.z + fma(e1.x, P.x, e1.y * P.y)  (the last product rounded on its own)
// The bundle kernel computes the origin half once per triangle and the ray half per ray; the others call triangleTest.
__device__ inline V3 crossExact(const V3 a, const V3 b)
{
#pragma clang fp contract(off)
    return mk(__builtin_fmaf(a.y, b.z, -(a.z * b.y)), __builtin_fmaf(a.z, b.x, -(a.x * b.z)), __builtin_fmaf(a.x, b.y, -(a.y * b.x)));
}
__device__ inline float dotExact(const V3 a, const V3 b)
{
#pragma clang fp contract(off)
    return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.x, b.x, a.y * b.y));
}
// the half that only knows the origin
__device__ inline void triOriginHalf(const V3 o, const V3 v0, const V3 e1, const V3 e2, V3* T, V3* Q, float* e2Q)
{
#pragma clang fp contract(off)
    *T = mk(o.x - v0.x, o.y - v0.y, o.z - v0.z);
    *Q = crossExact(*T, e1);
    *e2Q = dotExact(e2, *Q);
}
// the half per ray: det (PT_TRI_HIT rejects |det| < FLT_MIN), u, v, t
__device__ inline void triRayHalf(const V3 d, const V3 e1, const V3 e2, const V3 T, const V3 Q, const float e2Q, float* det, float* u, float* v, float* t)
{
#pragma clang fp contract(off)
    const V3 P = crossExact(d, e2);
    const float pz = e1.z * P.z;
    *det = pz + __builtin_fmaf(e1.x, P.x, e1.y * P.y);
    const float inv = fastRcp(*det);
    *u = dotExact(T, P) * inv;
    *v = dotExact(d, Q) * inv;
    *t = e2Q * inv;
}
__device__ inline void triangleTest(const V3 o, const V3 d, const V3 v0, const V3 e1, const V3 e2, float* det, float* u, float* v, float* t)
{
    V3 T, Q;
    float e2Q;
    triOriginHalf(o, v0, e1, e2, &T, &Q, &e2Q);
    triRayHalf(d, e1, e2, T, Q, e2Q, det, u, v, t);
}
// the reference's two-sided accept tests (shapes.cl:20-72) and the `t < closestT` of its leaf loop (scene.cl:168-195).  A macro, not a function: the
// optimiser flattens a function's && chain before it is inlined, and every traversal kernel then comes out with another schedule (k_trace<true, .> trade
// two compares for their negations, the closest-hit kernels move by 1 to 30 instructions); spelled in place the chain is what rounds 1-6 compiled
#define PT_TRI_HIT(det, u, v, t, tLimit) (!((det) > -FLT_MIN && (det) < FLT_MIN) && !((u) < 0.f || (u) > 1.f) && !((v) < 0.f || (u) + (v) > 1.f) && (t) > 0.f && (t) < (tLimit))

// A ray taken into an instance's space (scene.cl:116-139): rows r0..r2 of the inverse transform; the direction is NOT
// renormalised, so t is shared between the two spaces; exactly-zero components are nudged (NO_PARALLEL_RAYS, scene.cl:123-137).
// One spelling (explicit FMAs) for every kernel that enters instances, so that they produce the same bits.
__device__ inline void rayIntoInstance(const float4 r0, const float4 r1, const float4 r2, const V3 o, const V3 d, V3* to, V3* td)
{
    *to = mk(fmaf(r0.x, o.x, fmaf(r0.y, o.y, fmaf(r0.z, o.z, r0.w))), fmaf(r1.x, o.x, fmaf(r1.y, o.y, fmaf(r1.z, o.z, r1.w))),
        fmaf(r2.x, o.x, fmaf(r2.y, o.y, fmaf(r2.z, o.z, r2.w))));
    *td = mk(fmaf(r0.x, d.x, fmaf(r0.y, d.y, r0.z * d.z)), fmaf(r1.x, d.x, fmaf(r1.y, d.y, r1.z * d.z)), fmaf(r2.x, d.x, fmaf(r2.y, d.y, r2.z * d.z)));
    nudgeZero(*to, *td);
}

// ---- the end of a ray (scene.cl:257) ----------------------------------------------------------------------------------------------
// an unoccluded shadow ray (its queue entry's contribution, its pixel in pixelWord): the deposit of intersectShadows (kernel.cl:132-135); one live
// path per accumulator entry: plain read-modify-write
__device__ inline void depositUnoccluded(const TraceArgs& a, const float4 contrib, const uint32_t pixelWord)
{
    float4* ap = a.accum.at(asU(contrib.w) >> 16, pixelWord);
    float4 px = *ap;
    px.x += contrib.x, px.y += contrib.y, px.z += contrib.z;
    *ap = px;
}
// the closest hit of queue entry idx (prim < 0: none).  A hit on a world-space copy of an instance (no instance was entered: inst < 0) goes back to
// (original triangle, instance), which the copy's record carries
__device__ inline void writeClosestHit(const TraceArgs& a, const SceneDev& sc, const uint32_t idx, const float t, const float u, const float v, int prim, int inst)
{
    if (prim >= 0 && inst < 0) {
        const float4 tc = sc.tris[prim].c;
        prim = (int)asU(tc.y);
        inst = (int)asU(tc.z);
    }
    a.hit[idx] = make_float4(prim >= 0 ? t : INFINITY, u, v, asF((uint32_t)prim));
    a.inst[idx] = inst;
}

} // namespace ptd
