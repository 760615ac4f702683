// First-hit guide buffers and the edge-avoiding a-trous wavelet denoiser (Dammertz et al. 2010) -- include/ptamd.h, "guides and denoiser"; DESIGN.md
// section 9.  Nothing here is on the render path: the guides come from a pass of their own (camera rays into a scratch queue, the per-ray closest-hit
// kernel over it, k_guides), the filter reads the accumulator and the guide sums and writes an image of its own.
#pragma once
#include "pt_shade.h"

namespace ptd {

constexpr float kGuideSkyDepth = 1e6f; // PT_GUIDE_SKY_DEPTH
constexpr float kAlbedoFloor = 1e-3f; // demodulation divides by max(albedo, this)

// ---- guide pass ---------------------------------------------------------------------------------
// Camera rays of guide sample fp.sample for the first n owned pixels, one entry per pixel in the order of the pixel list -- the ray pt_render traces
// for that sample index (primaryRay: same keying of the counter PRNG, pinhole and thin lens).  Thread 0 arms the scratch control block's pass 0.
__global__ void __launch_bounds__(256) k_guide_gen(FrameParams fp, float4* __restrict__ qO, float4* __restrict__ qD, const uint32_t* __restrict__ pixelList,
    uint32_t n, Control* __restrict__ ctl)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0u) {
        ctl->extCount[0] = n;
        ctl->extCursor[0] = 0u;
    }
    if (k >= n)
        return;
    const uint32_t pixel = pixelList ? pixelList[k] : k;
    V3 o, d;
    primaryRay(fp, pixel, 0u, &o, &d);
    qO[k] = make_float4(o.x, o.y, o.z, asF(pixel));
    qD[k] = make_float4(d.x, d.y, d.z, asF(packState(0u, 0u, 0u)));
}

// One thread owns one pixel: it adds the deposits of this sample's first hit to the pixel's two sums (plain read-modify-write: the launches of
// consecutive samples are ordered on the stream, so a pixel's samples are summed in sample order and the sums are bit-reproducible).
//   albedoHits  += (albedo.rgb, 1)   DIFFUSE: diffuseColour, or the texture fetch shadeHit makes (alpha-0 texel: 1,1,1); PBR: baseColour;
//                                    REFRACTIVE / BASIC_REFRACTIVE / EMISSIVE: (1,1,1).  A miss: (1,1,1, 0).
//   normalDepth += (N.xyz, t)        N: interpolated shading normal, to world space with the instance's normal transform, normalised, turned to face
//                                    the ray.  A miss: (-D, PT_GUIDE_SKY_DEPTH).
// A thin lens traces un-normalised directions (camera.cl:71-75): its deposits use D / |D| and t * |D|, so that normal and distance mean the same
// for both cameras.
// MODE 1 (pt_set_instance_motion; include/ptamd.h, "instance motion"): two more sums, from the MotionRecord of the hit instance --
//   motion     += (A X + t, 0)       X = O + t D, the world hit point with the queue's own origin and un-normalised direction: where that point was in the
//                                    scene state the history was made under, minus where it is.  A miss: 0.
//   prevNormal += (n_then, 0)        N's expression on the previous invTransform's rows, flipped iff N was.  A miss: -D.
// An instance whose previous transform has the current one's bits deposits exact zeros and the bits of N.  k_guides<0> is the kernel of before.
// MODE 2 (pt_set_vertex_motion; include/ptamd.h, "vertex motion"): the mesh was refitted since the state the history was made under.  `then` holds that
// state's shading records (a snapshot: never the inactive dynamic set, which the next upload may be overwriting), `rowsThen` three rows per instance --
// the linear part L of the world transform the instance had then.  With x(record) = v0 + e1 u + e2 v (guidePoint, the same operations for both records),
//   motion     += (A X + t + L (x(then) - x(now)), 0)        W_then x_then - X = (P X - X) + L_then (x_then - x_now), exactly
//   prevNormal += (n_then, 0)                                the snapshot's interpolated normal through the previous rows
// A triangle whose snapshot has the current record's bits has x(then) - x(now) == 0 and deposits what mode 1 deposits, bit for bit.  The current line,
// the snapshot's six quarters, the instance, the motion record and the three rows are 27 independent 16-byte loads, issued before the first use.
struct GuideMotionArgs {
    const MotionRecord* records; // indexed like sc.instances
    float4* motion;
    float4* prevNormal;
    const TriFat* then; // MODE 2: the previous state's shading records, indexed like sc.triFat
    const float4* rowsThen; // MODE 2: three per instance
};

// the hit point in object space from a shading record's v0 / edge1 / edge2 quarters (TriFat::e1e, e2v, v0c): spelled with fmaf so that the current record
// and the snapshot go through the same instructions whatever the compiler would have contracted
__device__ inline V3 guidePoint(const float4 e1e, const float4 e2v, const float4 v0c, float u, float v)
{
    return mk(fmaf(e1e.w, v, fmaf(e1e.x, u, e2v.z)), fmaf(e2v.x, v, fmaf(e1e.y, u, e2v.w)), fmaf(e2v.y, v, fmaf(e1e.z, u, v0c.x)));
}

// The terminal deposit of a guide ray, stated once for k_guides and k_guide_chain: the normal and the albedo of a hit as the comment of k_guides has them.
// guideShadingNormal: the interpolated shading normal, object space (the motion modes take it through the previous transform as well);
// guideNormal: that normal to world space, normalised, turned to face the ray of direction D (`flip`: it was turned).  All three hand VALUES back: with
// the albedo passed by reference k_guides<1> and <2> came out with another schedule (EXPERIMENTS.md, "Guide chain").
__device__ __forceinline__ V3 guideShadingNormal(const float4 f0, const float4 f1, const float4 f2, float u, float v)
{
    const V3 n0 = xyz(f0), n1 = xyz(f1), n2 = xyz(f2);
    return normalize(n0 + (n1 - n0) * u + (n2 - n0) * v); // object space (shadeHit)
}
struct GuideNormal {
    V3 N;
    bool flip;
};
__device__ __forceinline__ GuideNormal guideNormal(const Instance& in, V3 shadingNormal, V3 D)
{
    GuideNormal r;
    r.N = normalize(normalTransform(in, shadingNormal));
    r.flip = dot(r.N, D) > 0.0f;
    if (r.flip)
        r.N = r.N * -1.0f;
    return r;
}
// guideAlbedo: `albedo` comes in as (1,1,1), what REFRACTIVE / BASIC_REFRACTIVE / EMISSIVE keep
__device__ __forceinline__ V3 guideAlbedo(const SceneDev& sc, const MatView& mat, const float4 f0, const float4 f1, const float4 f2, const float4 f3, float u, float v,
    V3 albedo)
{
    if (mat.type == MAT_PBR) {
        albedo = mat.colour;
    } else if (mat.type == MAT_DIFFUSE) {
        albedo = mat.colour;
        if (mat.texId != -1) {
            albedo = diffuseColourTextured(sc, mat, f0, f1, f2, f3, u, v);
            if (albedo.x == -1.0f) // alpha-0 texel
                albedo = mk(1.0f);
        }
    }
    return albedo;
}

template <int MODE> // 0: no motion; 1: instance motion; 2: instance and vertex motion
__global__ void __launch_bounds__(256) k_guides(SceneDev sc, const float4* __restrict__ qO, const float4* __restrict__ qD, const float4* __restrict__ hit,
    const int32_t* __restrict__ hitInst, uint32_t n, uint32_t thinLens, float4* __restrict__ albedoHits, float4* __restrict__ normalDepth, GuideMotionArgs mo)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const float4 ro = qO[k];
    const uint32_t pixel = asU(ro.w);
    const float4 rd = qD[k], h = hit[k];
    V3 D = xyz(rd);
    float scale = 1.0f;
    if (thinLens) {
        scale = sqrtf(dot(D, D));
        D = D / scale;
    }
    const int32_t prim = (int32_t)asU(h.w);
    V3 albedo = mk(1.0f), N = D * -1.0f;
    V3 moved = mk(0.0f), nThen = N;
    float t = kGuideSkyDepth, hits = 0.0f;
    if (prim >= 0) {
        const TriFat* fp = &sc.triFat[prim];
        const float4 f0 = fp->n0u, f1 = fp->n1u, f2 = fp->n2u, f3 = fp->vvvm, f6 = fp->v0c, f7 = fp->mat;
        const float u = h.y, v = h.z;
        const Instance in = sc.instances[hitInst[k]];
        MotionRecord rec;
        if constexpr (MODE >= 1) // six more 16-byte loads, in flight with the triangle's and the instance's
            rec = mo.records[hitInst[k]];
        float4 f4, f5, t0, t1, t2, t4, t5, t6, l0, l1, l2;
        if constexpr (MODE == 2) {
            const TriFat* tp = &mo.then[prim];
            const float4* lp = &mo.rowsThen[3 * hitInst[k]];
            f4 = fp->e1e, f5 = fp->e2v;
            t0 = tp->n0u, t1 = tp->n1u, t2 = tp->n2u, t4 = tp->e1e, t5 = tp->e2v, t6 = tp->v0c;
            l0 = lp[0], l1 = lp[1], l2 = lp[2];
        }
        const V3 shadingNormal = guideShadingNormal(f0, f1, f2, u, v);
        const GuideNormal facing = guideNormal(in, shadingNormal, D);
        N = facing.N;
        const bool flip = facing.flip;
        if constexpr (MODE >= 1) {
            Instance then = in;
            then.r0 = rec.p0, then.r1 = rec.p1, then.r2 = rec.p2;
            V3 shadingNormalThen = shadingNormal;
            if constexpr (MODE == 2) {
                const V3 m0 = xyz(t0), m1 = xyz(t1), m2 = xyz(t2);
                shadingNormalThen = normalize(m0 + (m1 - m0) * u + (m2 - m0) * v);
            }
            nThen = normalize(normalTransform(then, shadingNormalThen));
            if (flip)
                nThen = nThen * -1.0f;
            const V3 X = xyz(ro) + xyz(rd) * h.x;
            moved = mk(dot(xyz(rec.a0), X) + rec.a0.w, dot(xyz(rec.a1), X) + rec.a1.w, dot(xyz(rec.a2), X) + rec.a2.w);
            if constexpr (MODE == 2) {
                const V3 delta = guidePoint(t4, t5, t6, u, v) - guidePoint(f4, f5, f6, u, v); // object space; 0 exactly where the bits agree
                moved = moved + mk(fmaf(l0.z, delta.z, fmaf(l0.y, delta.y, l0.x * delta.x)), fmaf(l1.z, delta.z, fmaf(l1.y, delta.y, l1.x * delta.x)),
                                    fmaf(l2.z, delta.z, fmaf(l2.y, delta.y, l2.x * delta.x)));
            }
        }
        const MatView mat = loadMaterial(f6, f7);
        albedo = guideAlbedo(sc, mat, f0, f1, f2, f3, u, v, albedo);
        t = h.x * scale;
        hits = 1.0f;
    }
    float4 a = albedoHits[pixel], g = normalDepth[pixel], m, pn;
    if constexpr (MODE >= 1)
        m = mo.motion[pixel], pn = mo.prevNormal[pixel];
    a.x += albedo.x, a.y += albedo.y, a.z += albedo.z, a.w += hits;
    g.x += N.x, g.y += N.y, g.z += N.z, g.w += t;
    albedoHits[pixel] = a;
    normalDepth[pixel] = g;
    if constexpr (MODE >= 1) {
        m.x += moved.x, m.y += moved.y, m.z += moved.z;
        pn.x += nThen.x, pn.y += nThen.y, pn.z += nThen.z;
        mo.motion[pixel] = m;
        mo.prevNormal[pixel] = pn;
    }
}

// The snapshot k_guides<2> reads, for a state whose tree was REBUILT since the previous one (pt_set_rebuilt_motion; include/ptamd.h, "rebuilt motion"): the
// triangles are numbered anew, so "then" is gathered through the caller's map --
//   out[i] = map[i] == PT_NO_PREVIOUS_TRIANGLE ? now[i] : then[map[i]]
// a copy of 128-byte records, bits untouched.  Eight lanes move one record, a float4 each: a wave64 moves eight whole 128-byte lines per load and per
// store, no line is split, the stores are consecutive.  The compare against nThen is the only guard there is: an index that is not below it (the marker
// is the largest) never becomes an address, whatever the host validated; it gives the current record.
__global__ void __launch_bounds__(256) k_gather_then(const TriFat* __restrict__ then, uint32_t nThen, const TriFat* __restrict__ now,
    const uint32_t* __restrict__ map, TriFat* __restrict__ out, uint32_t nNow)
{
    const uint32_t i = blockIdx.x * 32u + (threadIdx.x >> 3), piece = threadIdx.x & 7u;
    if (i >= nNow)
        return;
    const uint32_t j = map[i];
    const float4* src = j < nThen ? (const float4*)(then + j) : (const float4*)(now + i);
    ((float4*)(out + i))[piece] = src[piece];
}

// ---- guide chain (include/ptamd.h, "guide chain") ------------------------------------------------
// With pt_set_guide_chain(K > 0) a guide ray follows refraction to the first surface that is not glass.  Per sample the guide pass launches k_guide_gen and
// then, for stage j = 0 .. K, the per-ray closest-hit kernel over stage j's queue (pass j of the guide pass's control block) and k_guide_chain(j):
// one thread per entry of stage j.  An entry whose hit is REFRACTIVE / BASIC_REFRACTIVE, whose interface transmits and whose stage is below K goes on:
//   N     the normal guideNormal gives (what a terminal hit would deposit)         ior   refractiveIndexBasic / refractiveIndexRough (MatView p0 / p1)
//   n1n2  1 / ior where shadeHit's real normal faces the ray (its own compare per material: > kEPS for BASIC_REFRACTIVE, > 0 for REFRACTIVE), else ior
//   cos1 = -N.D,   Kt = 1 - n1n2^2 (1 - cos1^2),   transmitted iff Kt > kEPS,   T = normalize(n1n2 D + N (n1n2 cos1 - sqrt(Kt)))
//   next entry: origin X + T kEPS (X = O + t D of the queue's own origin and direction, as k_shade forms it), direction T, dist + t
// (rough glass is followed along its mean direction; absorption and Fresnel are ignored: the guides describe surfaces).  Every other entry is TERMINAL
// -- a hit that is not glass, a miss, total internal reflection, stage K on glass -- and deposits what k_guides<0> deposits, through the same two
// functions, with the distance dist + t (a miss: PT_GUIDE_SKY_DEPTH as it is, and -D of this segment).  Stage 0 with dist = 0 adds the bits k_guides<0> adds.
// A pixel has exactly one live entry per sample and one terminal deposit, and the launches of a sample are ordered on the stream: a plain
// read-modify-write, sums in sample order whatever order the compaction leaves the later stages in.
// Compaction as k_shade's: ranks from a wave64 ballot, the waves' counts through LDS, ONE atomicAdd per workgroup on the next stage's count (none where
// nothing goes on).  The two queues ping-pong (stage j reads queue j & 1); the counts and cursors of stages 1 .. K are zeroed by the host's memset nodes
// before stage 0.  The entry, its hit, the instance index, the eight quarters of the triangle's record and the instance are issued before the first use.
struct GuideChainArgs {
    SceneDev sc;
    const float4* qO; // stage j: origin.xyz, bits(pixel)
    const float4* qD; // direction.xyz, bits(state)
    const float* qDist; // distance travelled before this segment (not read at stage 0)
    const float4* hit;
    const int32_t* hitInst;
    float4* outO; // stage j + 1
    float4* outD;
    float* outDist;
    Control* ctl;
    uint32_t stage, last; // last: stage == K, glass is terminal
    uint32_t capacity; // entries a queue holds
    uint32_t thinLens; // stage 0 of a thin-lens camera: the direction is not normalised
    float4* albedoHits;
    float4* normalDepth;
    int4* terminals; // test hook (pt_debug_guide_chain_terminals), else null: per pixel (prim, top-level leaf, stage, 1: total internal reflection) of the terminal
    const float4* qTint; // REFLECT only: the tint of stage j's entries (not read at stage 0) ...
    float4* outTint; // ... and of stage j + 1's
};

// REFLECT (include/ptamd.h, "guide reflections"; pt_set_guide_reflections with K > 0 over a scene that holds glass or a MIRROR): an entry also goes on
//   * from a MIRROR -- MAT_PBR, metallic, smoothness > kMaxSmoothness: what k_shade treats as a specular bounce (dospecular) -- with its tint times the
//     base colour (one multiply per component, in stage order; Fresnel is ignored, rough metal is followed along the mirror direction), and
//   * from glass whose interface does not transmit (total internal reflection), tint unchanged,
// along R = normalize(D + N (2 cos1)) if and only if G.R > kEPS, G the real normal turned to the ray's side (a bent shading normal that would send the
// reflection through the surface is where k_shade ends such a path: the surface is terminal).  The next entry starts at X + R kEPS with dist + t, as a
// transmitted one.  The terminal's albedo is tint (.) what it deposits otherwise (a miss: the tint itself), multiplied onto the VALUE guideAlbedo hands
// back; an entry that met neither a MIRROR nor a total internal reflection has tint exactly 1 and deposits the bits of k_guide_chain<false>.  The tint
// travels in one more float4 plane per queue, issued with the entry's other loads; the number of reflections followed so far travels in the `plane`
// field of the state word (the trace kernels read the flags and nothing else of it) and is what the terminal record's fourth word holds.
// k_guide_chain<false> is the kernel of before, instruction for instruction.
template <bool REFLECT>
__global__ void __launch_bounds__(256) k_guide_chain(GuideChainArgs a)
{
    __shared__ uint32_t sCount[4], sBase;
    const uint32_t count = min(a.ctl->extCount[a.stage], a.capacity);
    if (blockIdx.x * 256u >= count) // the whole workgroup: the grid covers the queue's capacity, the count is a device word
        return;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool live = k < count;
    bool goOn = false;
    V3 nextO = mk(0.0f), nextD = mk(0.0f);
    float nextDist = 0.0f;
    uint32_t pixel = 0u;
    V3 tint = mk(1.0f); // (REFLECT)
    uint32_t nextCount = 0u;
    if (live) {
        const float4 ro = a.qO[k], rd = a.qD[k], h = a.hit[k];
        const int32_t hinst = a.hitInst[k];
        const float before = a.stage ? a.qDist[k] : 0.0f;
        if constexpr (REFLECT) {
            if (a.stage)
                tint = xyz(a.qTint[k]);
        }
        pixel = asU(ro.w);
        V3 D = xyz(rd);
        float scale = 1.0f;
        if (a.thinLens) {
            scale = sqrtf(dot(D, D));
            D = D / scale;
        }
        const int32_t prim = (int32_t)asU(h.w);
        V3 albedo = mk(1.0f), N = D * -1.0f;
        float t = kGuideSkyDepth, hits = 0.0f;
        int32_t leaf = -1, reflected = 0;
        if constexpr (REFLECT)
            reflected = (int32_t)(asU(rd.w) >> 16); // reflections followed so far
        if (prim >= 0) {
            const TriFat* fp = &a.sc.triFat[prim];
            const float4 f0 = fp->n0u, f1 = fp->n1u, f2 = fp->n2u, f3 = fp->vvvm, f4 = fp->e1e, f5 = fp->e2v, f6 = fp->v0c, f7 = fp->mat;
            const float u = h.y, v = h.z;
            const Instance in = a.sc.instances[hinst];
            N = guideNormal(in, guideShadingNormal(f0, f1, f2, u, v), D).N;
            const MatView mat = loadMaterial(f6, f7);
            t = h.x * scale;
            leaf = (int32_t)in.topNode;
            const bool basic = mat.type == MAT_BASIC_REFRACTIVE;
            if constexpr (REFLECT) {
                const bool glass = basic || mat.type == MAT_REFRACTIVE;
                const bool mirror = mat.type == MAT_PBR && mat.metallic && mat.p0 > kMaxSmoothness;
                if ((glass || mirror) && !a.last) {
                    const V3 edge1 = xyz(f4), edge2 = mk(f4.w, f5.x, f5.y);
                    const V3 realNormal = fastNormalize(normalTransform(in, cross(edge1, edge2)));
                    const float facing = dot(realNormal, D * -1.0f);
                    const float cos1 = -dot(N, D);
                    bool reflect = mirror;
                    if (glass) {
                        const float ior = basic ? mat.p0 : mat.p1;
                        const float n1n2 = (basic ? facing > kEPS : facing > 0.0f) ? 1.0f / ior : ior;
                        const float Kt = 1.0f - (n1n2 * n1n2) * (1.0f - cos1 * cos1);
                        if (Kt > kEPS) {
                            goOn = true;
                            nextD = normalize(n1n2 * D + N * (n1n2 * cos1 - sqrtf(Kt)));
                            nextCount = (uint32_t)reflected;
                        } else {
                            reflect = true;
                        }
                    }
                    if (reflect) {
                        const V3 R = normalize(D + N * (2.0f * cos1));
                        const float side = dot(realNormal, R);
                        if ((facing > 0.0f ? side : -side) > kEPS) { // G.R, G the real normal on the ray's side
                            goOn = true;
                            nextD = R;
                            nextCount = (uint32_t)reflected + 1u;
                            if (mirror)
                                tint = mk(tint.x * mat.colour.x, tint.y * mat.colour.y, tint.z * mat.colour.z);
                        }
                    }
                    if (goOn) {
                        nextO = xyz(ro) + xyz(rd) * h.x + nextD * kEPS;
                        nextDist = before + t;
                    }
                }
            } else if ((basic || mat.type == MAT_REFRACTIVE) && !a.last) {
                const V3 edge1 = xyz(f4), edge2 = mk(f4.w, f5.x, f5.y);
                const V3 realNormal = fastNormalize(normalTransform(in, cross(edge1, edge2))); // as shadeHit forms it: mirrored instances take the path's side
                const float facing = dot(realNormal, D * -1.0f);
                const float ior = basic ? mat.p0 : mat.p1;
                const float n1n2 = (basic ? facing > kEPS : facing > 0.0f) ? 1.0f / ior : ior;
                const float cos1 = -dot(N, D);
                const float Kt = 1.0f - (n1n2 * n1n2) * (1.0f - cos1 * cos1);
                if (Kt > kEPS) {
                    goOn = true;
                    nextD = normalize(n1n2 * D + N * (n1n2 * cos1 - sqrtf(Kt)));
                    nextO = xyz(ro) + xyz(rd) * h.x + nextD * kEPS;
                    nextDist = before + t;
                } else {
                    reflected = 1;
                }
            }
            if (!goOn) {
                albedo = guideAlbedo(a.sc, mat, f0, f1, f2, f3, u, v, albedo);
                t = before + t;
                hits = 1.0f;
            }
        }
        if (!goOn) {
            if constexpr (REFLECT)
                albedo = mk(tint.x * albedo.x, tint.y * albedo.y, tint.z * albedo.z);
            float4 al = a.albedoHits[pixel], g = a.normalDepth[pixel];
            al.x += albedo.x, al.y += albedo.y, al.z += albedo.z, al.w += hits;
            g.x += N.x, g.y += N.y, g.z += N.z, g.w += t;
            a.albedoHits[pixel] = al;
            a.normalDepth[pixel] = g;
            if (a.terminals)
                a.terminals[pixel] = make_int4(prim, leaf, (int32_t)a.stage, reflected);
        }
    }
    const unsigned long long going = __ballot(goOn);
    if (lane == 0)
        sCount[wave] = (uint32_t)__popcll(going);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < 4u; w++) {
            const uint32_t n = sCount[w];
            sCount[w] = sum;
            sum += n;
        }
        sBase = sum ? atomicAdd(&a.ctl->extCount[a.stage + 1u], sum) : 0u;
    }
    __syncthreads();
    if (goOn) {
        const uint32_t slot = sBase + sCount[wave] + (uint32_t)__popcll(going & ((1ull << lane) - 1ull));
        if (slot < a.capacity) { // (always: stage j + 1 holds at most the entries of stage j)
            a.outO[slot] = make_float4(nextO.x, nextO.y, nextO.z, asF(pixel));
            a.outD[slot] = make_float4(nextD.x, nextD.y, nextD.z, asF(packState(0u, a.stage + 1u, REFLECT ? nextCount : 0u)));
            a.outDist[slot] = nextDist;
            if constexpr (REFLECT)
                a.outTint[slot] = make_float4(tint.x, tint.y, tint.z, 0.0f);
        }
    }
}

// ---- filter -------------------------------------------------------------------------------------
constexpr uint32_t kInputAccum = 0, kInputTemporal = 1, kInputTemporalVariance = 2; // PT_DENOISE_INPUT_*

__device__ inline float luminance709(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
__device__ inline float albedoOf(float sum, float gspp) { return fmaxf(sum / gspp, kAlbedoFloor); }

// d = c / max(a, 1e-3):   c = accum.rgb / spp, a = albedo sum / gspp
__device__ inline V3 demodulatedMean(float4 s, float4 al, float spp, float gspp)
{
    return mk(s.x / spp / albedoOf(al.x, gspp), s.y / spp / albedoOf(al.y, gspp), s.z / spp / albedoOf(al.z, gspp));
}

// (n, z):   n = normal sum normalised (zero stays zero), z = distance sum / gspp
__device__ inline float4 guideOf(float4 g, float gspp)
{
    const float len = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
    const float inv = len > 0.0f ? 1.0f / len : 0.0f;
    return make_float4(g.x * inv, g.y * inv, g.z * inv, g.w / gspp);
}

// e_n + e_z of a tap whose guide is gq, seen from a surface of normal n at distance z (include/ptamd.h has the terms)
__device__ inline float guideTerms(V3 n, float z, float4 gq, float kNormal, float invSigmaDepth)
{
    const float en = kNormal * fmaxf(0.0f, 1.0f - (n.x * gq.x + n.y * gq.y + n.z * gq.z));
    const float ez = fabsf(z - gq.w) * invSigmaDepth / (fminf(z, gq.w) + 1e-6f);
    return en + ez;
}

// the output pixel of a demodulated colour: times the current albedo, linear or through pt_resolve's tone curve
__device__ inline float4 remodulated(float r, float g, float b, float4 al, float gspp, bool tonemapped, float relativeAperture, float shutterTime, float ISO)
{
    r *= albedoOf(al.x, gspp), g *= albedoOf(al.y, gspp), b *= albedoOf(al.z, gspp);
    if (tonemapped) {
        const float exposure = resolveExposure(relativeAperture, shutterTime, ISO);
        r = resolveChannel(r * exposure), g = resolveChannel(g * exposure), b = resolveChannel(b * exposure);
    }
    return make_float4(r, g, b, 1.0f);
}

// d0 and the guide normalisation in one pass over the inputs, so that a tap of the filter costs two 16-byte loads:
//   colour = (d0, its fourth component)    guide = guideOf(normal_depth)
//   PT_DENOISE_INPUT_ACCUM              d0 = demodulatedMean(accum, albedo sums),   the luminance of d0
//   PT_DENOISE_INPUT_TEMPORAL           d0 = the newest history's d,                the luminance of d0
//   PT_DENOISE_INPUT_TEMPORAL_VARIANCE  the same d0,                                V_0 = v / max(N, 1): the variance of the history's MEAN
// FIREFLY (pt_set_firefly_clamp, PT_DENOISE_INPUT_ACCUM alone): `source` is the clamped plane (d.rgb, s) k_firefly made of the accumulator, d0 is its
// rgb and the albedo sums are not read.  The FIREFLY-less instantiations are the kernels of before.
template <uint32_t INPUT, bool FIREFLY = false>
__global__ void __launch_bounds__(256) k_denoise_prepare(const float4* __restrict__ source, const float* __restrict__ histVariance,
    const float4* __restrict__ albedoHits, const float4* __restrict__ normalDepth, float4* __restrict__ colour, float4* __restrict__ guide, uint32_t n,
    float spp, float gspp)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float4 s = source[i], g = normalDepth[i];
    V3 d = xyz(s);
    if constexpr (INPUT == kInputAccum && !FIREFLY)
        d = demodulatedMean(s, albedoHits[i], spp, gspp);
    float fourth;
    if constexpr (INPUT == kInputTemporalVariance)
        fourth = histVariance[i] / fmaxf(s.w, 1.0f);
    else
        fourth = luminance709(d.x, d.y, d.z);
    colour[i] = make_float4(d.x, d.y, d.z, fourth);
    guide[i] = guideOf(g, gspp);
}

// iterations == 0, linear output: the mean radiance as it is
__global__ void __launch_bounds__(256) k_denoise_mean(const float4* __restrict__ accum, float4* __restrict__ out, uint32_t n, float spp)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float4 s = accum[i];
    out[i] = make_float4(s.x / spp, s.y / spp, s.z / spp, 1.0f);
}

enum : uint32_t { ATROUS_MORE = 0, ATROUS_LAST_HDR = 1, ATROUS_LAST_TONEMAPPED = 2 };
struct AtrousArgs {
    const float4* colour; // (d_i.rgb, luminance); VARIANCE: (d_i.rgb, V_i), the variance of d_i's luminance
    const float4* guide; // n.xyz, z
    float4* out; // d_{i+1} in the same form, or the final image
    const float4* albedoHits; // last iteration: re-modulation
    uint32_t width, height;
    int32_t step; // 2^i
    float kNormal, invSigmaDepth, invSigmaLum; // invSigmaLum = 1 / (sigma_lum * 2^-i)
    uint32_t mode; // ATROUS_*
    float gspp;
    float relativeAperture, shutterTime, ISO; // ATROUS_LAST_TONEMAPPED
    // VARIANCE (pt_set_temporal_variance; include/ptamd.h, "temporal variance")
    const float4* history; // (d.rgb, N) of the newest history set: s(p) comes from its count
    float sigmaVariance, relativeFloor;
    float invFullHistory; // 1 / (full_history - 1)
};

constexpr int kAtrousTileW = 32, kAtrousTileH = 8; // 256 threads; a wave is two rows of 32 pixels
constexpr int kAtrousMaxHalo = 4; // 2 * step for the steps staged in LDS (1 and 2)
constexpr int kAtrousLdsW = kAtrousTileW + 2 * kAtrousMaxHalo, kAtrousLdsH = kAtrousTileH + 2 * kAtrousMaxHalo;

// One iteration: d_{i+1}(p) = sum_q k(q - p) w_i(p, q) d_i(q) / sum_q k w_i over the 5 x 5 taps q = p + step * (dx, dy) inside the image, k the outer
// product of (1/16, 1/4, 3/8, 1/4, 1/16), w_i = exp(-(e_n + e_z + e_l)) -- one exp per tap (include/ptamd.h has the three terms).
// STEP_IN_LDS (steps 1 and 2): the tile and its halo of 2 * step pixels are staged in LDS, both images as float4.  Every tap is two 16-byte LDS reads
// (ds_read_b128) at [row][x + const]: the 16 lanes such a read serves together (MI355X_MICROARCH.md, LDS: {0-3, 12-15, 20-27} and its three
// translates) lie in ONE row of 32 consecutive float4, i.e. on 16 different 16-byte slots of the 256-byte bank row whatever the pitch -- no conflicts,
// no padding.  Steps >= 4 would need a halo larger than the tile: their taps are global loads (strided gathers over two images of 15-33 MB, served
// by L2 / the memory-side cache).
// VARIANCE: the filter over the temporal history.  The luminance term moves from the relative one to a variance one as the pixel's history grows,
// s(p) = clamp((N(p) - 1) / (full_history - 1), 0, 1):
//   e_l = s e_var + (1 - s) e_plain,   e_var = |L_p - L_q| / (sigma_variance g(p) + relative_floor (max(L_p, L_q) + 1e-3)),   e_plain = the plain e_l
//   g(p)^2 = the 3 x 3 binomial mean of V_i over the neighbours at distance 1 inside the image, whatever the step
//   d_{i+1}(p) = sum w d_i(q) / sum w,   V_{i+1}(p) = sum w^2 V_i(q) / (sum w)^2
// A tap stays two 16-byte loads: the luminance is recomputed per tap (three FMAs), the fourth component carries V.  STEP_IN_LDS: V is staged a second
// time as a plane of floats, from which the 3 x 3 comes (the halo is at least 2) -- nine ds_read_b32 at [row][x + const], 32 consecutive dwords per lane
// group and so on 32 different banks; the same reads out of the float4 image would be 16 bytes apart, four lanes to a bank (MI355X_MICROARCH.md, LDS).
// Steps >= 4: nine adjacent 4-byte global reads beside the 50 16-byte ones.  That plane is the guided instantiation's alone: 23 040 B of LDS against the
// plain one's 20 480, which is exactly 8 workgroups in a CU's 160 KB.
template <bool STEP_IN_LDS, bool VARIANCE = false>
__global__ void __launch_bounds__(256) k_atrous(AtrousArgs a)
{
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x = blockIdx.x * kAtrousTileW + tx, y = blockIdx.y * kAtrousTileH + ty;
    const int W = (int)a.width, H = (int)a.height;
    __shared__ float4 ldsC[STEP_IN_LDS ? kAtrousLdsH * kAtrousLdsW : 1];
    __shared__ float4 ldsG[STEP_IN_LDS ? kAtrousLdsH * kAtrousLdsW : 1];
    __shared__ float ldsV[STEP_IN_LDS && VARIANCE ? kAtrousLdsH * kAtrousLdsW : 1];
    const int halo = 2 * a.step, pitch = kAtrousTileW + 2 * halo; // (the launch keeps halo <= kAtrousMaxHalo for STEP_IN_LDS)
    if constexpr (STEP_IN_LDS) {
        const int rows = kAtrousTileH + 2 * halo, x0 = (int)blockIdx.x * kAtrousTileW - halo, y0 = (int)blockIdx.y * kAtrousTileH - halo;
        for (int e = ty * kAtrousTileW + tx; e < rows * pitch; e += kAtrousTileW * kAtrousTileH) {
            const int ly = e / pitch, lx = e - ly * pitch;
            const int gx = x0 + lx, gy = y0 + ly;
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f), g = c; // outside the image: never read (the loops skip those)
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                c = a.colour[(size_t)gy * W + gx];
                g = a.guide[(size_t)gy * W + gx];
            }
            ldsC[e] = c;
            ldsG[e] = g;
            if constexpr (VARIANCE)
                ldsV[e] = c.w;
        }
        __syncthreads();
    }
    if (x >= W || y >= H)
        return;
    const size_t p = (size_t)y * W + x;
    float count;
    if constexpr (VARIANCE)
        count = a.history[p].w;
    float4 cp, gp;
    if constexpr (STEP_IN_LDS) {
        cp = ldsC[(ty + halo) * pitch + tx + halo];
        gp = ldsG[(ty + halo) * pitch + tx + halo];
    } else {
        cp = a.colour[p];
        gp = a.guide[p];
    }
    float lp = cp.w, sigmaG, s;
    if constexpr (VARIANCE) {
        const float bin[3] = { 0.25f, 0.5f, 0.25f };
        float nv = 0.f, nk = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= H)
                continue;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx;
                if (qx < 0 || qx >= W)
                    continue;
                float vq;
                if constexpr (STEP_IN_LDS)
                    vq = ldsV[(ty + halo + dy) * pitch + tx + halo + dx];
                else
                    vq = a.colour[(size_t)qy * W + qx].w;
                const float k = bin[dy + 1] * bin[dx + 1];
                nv += k * vq, nk += k;
            }
        }
        // (the centre counts with 1/4: nk >= 1/4)
        sigmaG = a.sigmaVariance * sqrtf(nv / nk);
        s = fminf(fmaxf((count - 1.0f) * a.invFullHistory, 0.0f), 1.0f);
        lp = luminance709(cp.x, cp.y, cp.z);
    }
    const float kern[5] = { 1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f };
    float sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= H)
            continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= W)
                continue;
            float4 cq, gq;
            if constexpr (STEP_IN_LDS) {
                const int e = (ty + halo + dy * a.step) * pitch + tx + halo + dx * a.step;
                cq = ldsC[e];
                gq = ldsG[e];
            } else {
                cq = a.colour[(size_t)qy * W + qx];
                gq = a.guide[(size_t)qy * W + qx];
            }
            float lq = cq.w;
            if constexpr (VARIANCE)
                lq = luminance709(cq.x, cq.y, cq.z);
            const float eg = guideTerms(xyz(gp), gp.w, gq, a.kNormal, a.invSigmaDepth); // (stated before e_l: the instruction schedule follows this order)
            const float diff = fabsf(lp - lq), top = fmaxf(lp, lq) + 1e-3f;
            float el = diff * a.invSigmaLum / top;
            if constexpr (VARIANCE)
                el = s * (diff / (sigmaG + a.relativeFloor * top)) + (1.0f - s) * el;
            const float w = kern[dy + 2] * kern[dx + 2] * __expf(-(eg + el));
            sr += w * cq.x, sg += w * cq.y, sb += w * cq.z, sw += w;
            if constexpr (VARIANCE)
                sv += w * w * cq.w;
        }
    }
    // (the centre tap has w = k(0): sw >= 9/64)
    const float r = sr / sw, g = sg / sw, b = sb / sw;
    if (a.mode == ATROUS_MORE) {
        a.out[p] = make_float4(r, g, b, VARIANCE ? sv / (sw * sw) : luminance709(r, g, b));
        return;
    }
    a.out[p] = remodulated(r, g, b, a.albedoHits[p], a.gspp, a.mode == ATROUS_LAST_TONEMAPPED, a.relativeAperture, a.shutterTime, a.ISO);
}

} // namespace ptd
