// Persistent-wave two-level BVH traversal for gfx950 (closest-hit and any-hit).
//
// What it computes is the reference's traceRay (assets/cl/scene.cl:61-271): closest (or any) hit of a
// ray with the instanced scene -- instance transform without renormalisation (so t is shared between
// world and object space), the zero-component fix-up, two-sided Moeller-Trumbore with the reference's
// accept tests, `t < closestT` updates in leaf order, any-hit early out.  The ORDER in which
// subtrees are visited is ours (nearer child box first at both levels; the reference orders the top
// level by box-centre distance, scene.cl:141-157): the closest hit does not depend on it, only which
// of two hits at exactly the same t is reported.
//
// How it runs is CDNA4-specific (measurements behind every choice: DESIGN.md section 6):
//  * persistent waves at 7 waves/SIMD (72 VGPRs, 5 KB LDS per wave): the grid is sized to the machine; a wave
//    claims queue entries in spans of up to 512 with ONE atomicAdd (a device-scope word sustains only ~88
//    atomics/us) and copies the 64 entries it will hand out next into LDS ASYNCHRONOUSLY (two global_load_lds_dwordx4:
//    no staging registers, the kernel stays at 72 VGPRs): a hand-out -- consecutive entries for consecutive idle lanes
//    (ballot rank) -- reads LDS instead of stalling on HBM, so it can run as soon as 8 lanes are idle;
//  * ONE traversal stack in LDS, laid out [entry][thread of the block] (a wave's push/pop touches 64 consecutive dwords:
//    conflict-free ds_read/ds_write_b32; the stack position is kept as the byte offset into it), 12 entries; top level and bottom level share it, separated by a
//    sentinel entry that restores the world-space ray (re-read from the queue: instances are rarely entered, see
//    below); deeper entries spill to a lane-interleaved region in global memory;
//  * 4-wide nodes with 8-bit quantised child boxes (WideNode, 64 B = four 16-byte loads for four children) at
//    both levels, so one code path -- and one slot in the vote below -- serves both; entry/exit plane bytes are
//    picked per ray-direction sign as whole dwords, planes are one FMA each
//    (q * (2^e / d) + (origin - o) / d, reciprocal clamped so axis-parallel rays stay NaN-free), the four
//    (distance, reference) pairs go through a 5-comparator network, pushes are branch-free and the stack top is
//    prefetched before the node fetch;
//  * each loop iteration executes the step kind most lanes are waiting for (ballot majority vote: inner step or
//    leaf; one compare on the lane's current reference per vote -- a lane without a ray holds kRefIdle there) instead of serialising both for a fraction of the lanes; the rare kinds -- enter / leave an instance,
//    write the result -- park the lane until the hot loop breaks and are served in batches outside it.  (Most
//    scenes never enter an instance: ptamd.hip copies instances to world space at upload while a byte budget
//    lasts, which removed two parked steps per instance visit.)  Measured in round 3 and not kept: an any-hit lane on the
//    losing side of the vote working on the TOP OF ITS STACK instead when that is of the winning kind (a shadow ray may visit
//    in any order) -- in inner steps / in leaf steps / in both: 43.5 / 41.2 / 42.7 ms of any-hit traversal per batch against
//    40.4: the near-first descent finds occluders sooner than fuller steps save.
#pragma once
#include "pt_walk.h"

namespace ptd {

#ifndef PT_REFILL_IDLE
#define PT_REFILL_IDLE 8 // hand out new rays once this many lanes are idle; with (PT_PARKED_BREAK, _ANY) = (32, 48): 4 / 8 / 12 / 16 -> 8 810 / 8 865 /
#endif                   // 8 867 / 8 803 Mrays/s; (16, 24, 40) with the rays read from the queue at the hand-out, round 1's setting: 8 727
#ifndef PT_TRACE_MIN_WAVES
#define PT_TRACE_MIN_WAVES 7
#endif
#ifndef PT_PARKED_BREAK
#define PT_PARKED_BREAK 32 // (this, PT_PARKED_BREAK_ANY) at 8 idle lanes: (16, 24) / (24, 40) / (32, 48) / (40, 56) / (48, 60) -> 8 702 / 8 823 / 8 883 /
#endif                     // 8 860 / 8 733 Mrays/s: every pass over the parked lanes costs the whole wave
#ifndef PT_VOTE_INNER
#define PT_VOTE_INNER 2 // an inner step runs when 2 * (lanes wanting one) >= 3 * (lanes wanting a leaf): leaf steps are the
#define PT_VOTE_LEAF 3 // long ones (sequential triangle fetches), so they are not left waiting for a majority
#endif
#ifndef PT_LDS_STACK
#define PT_LDS_STACK 12 // 16 and 10 measure the same on the benchmark scene; deeper entries spill to global memory
#endif
constexpr int kLdsStack = PT_LDS_STACK; // stack entries kept in LDS per lane
#ifndef PT_LDS_STACK_TL
#define PT_LDS_STACK_TL PT_LDS_STACK // ... in the instantiations that enter instances
#endif
constexpr int kLdsStackTL = PT_LDS_STACK_TL;
constexpr int kTraversalStackMax = (kLdsStackTL < kLdsStack ? kLdsStackTL : kLdsStack) + 100; // what every instantiation can hold (LDS + spill, kSpillStack below)
constexpr uint32_t kInstFoldTable = 96; // entries of the per-workgroup table of folded instance transforms (entry 0: the identity): scenes of up to 95 instances.  (20 B
                                        // each beside 20.5 KB of stacks and staged rays: 7 workgroups per CU must stay within 160 KB -- at 128 entries the any-hit
                                        // instantiation's 23 056 B round up past a seventh of it and the kernel runs at 6 waves per SIMD: 89.1 -> 94.6 ms per batch)
constexpr int kSpillStack = 100; // further entries in global memory
constexpr int kTraceBlock = 256;
#ifndef PT_PARKED_BREAK_ANY
#define PT_PARKED_BREAK_ANY 48
#endif
constexpr int kParkedBreakAny = PT_PARKED_BREAK_ANY; // same, any-hit traversal (only unoccluded rays park: they have a deposit to make)
constexpr int kParkedBreak = PT_PARKED_BREAK; // leave the hot loop once this many lanes are parked on a special step or idle
// the instantiations that enter instances park far more often (every instance entry and exit): they are served earlier.
// Benchmark scene, every instance entered, (closest, any hit) = (12, 16) / (16, 24) / (16, 32) / (24, 40) / (32, 48):
// 8 191 / 8 234 / 8 233 / 8 221 / 8 032 Mrays/s (with the one-pass special section; 7 663 / 7 682 / 7 563 for the last three before it)
#ifndef PT_PARKED_BREAK_TL
#define PT_PARKED_BREAK_TL 16
#define PT_PARKED_BREAK_ANY_TL 24
#endif
constexpr int kRefillIdleLanes = PT_REFILL_IDLE; // hand out new rays once this many lanes are idle
#ifndef PT_REFILL_IDLE_TL
#define PT_REFILL_IDLE_TL 8 // the same in the instantiations that enter instances
#endif

// TWO_LEVEL: the tree holds instance references (instances that were not copied to world space at upload); scenes that are one
// world-space tree run the instantiation without the instance code.  Entering and leaving an instance are PARKED steps (served in
// batches outside the hot loop, see the kernel).  Measured alternatives (round 3, benchmark scene with every instance entered, ms per
// 256-sample batch of closest-hit bounce rays / shadow rays; parked: 30.4 / 53.1): both inside the hot loop at no extra iteration --
// the ray transformed at the head of the inner step on the instance's root, the world-space ray re-read from the queue at the pop
// of the sentinel -- 81 / 61 (nearly every iteration has SOME lane entering or leaving, so every iteration pays for both, and the
// kernel spills at 72 VGPRs); only the leave inside, the world-space ray of every lane parked in LDS in place of the staged
// packet: 36.1 / 54.4 at 7 waves per SIMD, 32.9 / 56.1 at 6.
#ifndef PT_TRACE_MIN_WAVES_TL
#define PT_TRACE_MIN_WAVES_TL 7
#endif
// LEVELS 2 (round 6): ANY instance transform, any number of instances, nothing parked but the end of a ray (scene.cl:116-139 in full).
//  * Entering an instance is a LEAF-KIND step: the top-level leaf of an instance is its instance reference, a lane that stands on one votes with the lanes
//    that stand on triangle leaves, and in the leaf iteration it fetches the 3 x 4 inverse transform (48 bytes: the size of a triangle record) instead of
//    triangles, takes its ray into the instance's space (rayIntoInstance: the arithmetic of the parked route, bit for bit) and continues at the mesh's
//    root.  Per visit that is one triangle test's worth of instructions shared by the lanes that enter in the same iteration -- no waiting for a quorum
//    of parked lanes, no pass outside the hot loop.
//  * Leaving an instance is NOTHING: the lane keeps the WORLD-space ray in its registers for the whole traversal; the instance-space ray (origin,
//    1 / direction, direction: nine floats) lives in a per-lane LDS slot written at the entry.  Every step reads its ray through an ADDRESS select --
//    object-space references (known from the reference's index alone, as in the folded route) read the lane's slot, world-space references a shared
//    all-zero entry -- and one multiply-add per component, ray = world * m + slot with m = 0 / 1: no vector select per component, no sentinel on
//    the stack, no re-read of the queue, no second pass.  An LDS read costs the vector ALU nothing (the kernel is vector-issue bound).
//  * LDS per wave: the slots (9 x 65 floats) take the place of the staged ray packet, which this instantiation does without (the hand-out reads
//    the queue itself: round 1's way, ~1.5 % slower on the flat scene): 12 stack entries + slots = 5.4 KB, 7 waves per SIMD.
#ifndef PT_TRACE_MIN_WAVES_GEN
#define PT_TRACE_MIN_WAVES_GEN 7
#endif
#ifndef PT_LDS_STACK_GEN
#define PT_LDS_STACK_GEN PT_LDS_STACK
#endif
constexpr int kObjPlanes = 9; // origin xyz, 1 / direction xyz, direction xyz
template <bool ANY_HIT, int LEVELS>
__global__ void __launch_bounds__(kTraceBlock, LEVELS == 2 ? PT_TRACE_MIN_WAVES_GEN : (LEVELS == 1 ? PT_TRACE_MIN_WAVES_TL : PT_TRACE_MIN_WAVES)) k_trace(TraceArgs a)
{
    // (Measured in round 6 and not kept: LEVELS 1 with the table of folded transforms read from GLOBAL memory past 95 entries -- 32 bytes per entry, two more
    // vector loads per object-space step, no entry step, the staged packet kept: 8 431 against 8 361 Mrays/s for LEVELS 2 on 208 translated + uniformly
    // scaled instances: one mechanism instead of two.)
    constexpr bool TWO_LEVEL = LEVELS == 1, GENERAL = LEVELS == 2;
    constexpr bool STAGED = !GENERAL; // the next 64 queue entries of the wave copied into LDS ahead of the hand-out
    constexpr int kLdsStack = GENERAL ? PT_LDS_STACK_GEN : (TWO_LEVEL ? kLdsStackTL : ptd::kLdsStack); // (shadows the namespace constant inside this kernel)
    __shared__ uint32_t ldsStack[kLdsStack][kTraceBlock]; // [entry][thread]: a lane's entries lie kSpStep bytes apart whichever wave it is in (see spB)
    __shared__ float4 ldsRays[STAGED ? kTraceBlock / 64 : 1][2][STAGED ? 64 : 1]; // the claimed packet: origins, directions (entry e of the packet at [.][e])
    __shared__ float ldsObj[GENERAL ? kTraceBlock / 64 : 1][GENERAL ? kObjPlanes : 1][GENERAL ? 65 : 1]; // [.][plane][lane]; [.][plane][64] = 0: what world-space steps read
    // TWO_LEVEL, round 5: instances whose transform is a translation + uniform scale are traversed WITHOUT parking and without an entry step.
    // The lane keeps the WORLD-space ray in its registers; while it walks object-space nodes / triangles -- known from the reference alone:
    // node indices below the first top-level node or in the run of per-instance root copies, triangle indices of the caller's numbering --
    // the ray is taken into the instance's space on the fly,
    //   o' = o * (1/s) + w,   1/d' = (1/d) * s,   d' = d * (1/s)        (t is shared between the spaces, scene.cl:118-121)
    // with (1/s, w) read from a per-workgroup LDS table indexed by the lane's current instance (entry 0 = the identity, read by world-space
    // steps and, through their own identity entries, by lanes inside a general instance, whose registers hold the instance-space ray): no
    // branch, no parked step.  The top-level leaf of such an instance refers to the instance's own copy of its mesh's root node (object space;
    // the copies form the last run of the node array, copy k = instance k): reaching it sets the lane's instance.  (ptamd.hip, convertDynamic.)
    __shared__ float4 ldsInstFold[TWO_LEVEL ? kInstFoldTable : 1];
    __shared__ float ldsInstScale[TWO_LEVEL ? kInstFoldTable : 1]; // s of the same entries (1 / x is a quarter-rate instruction; an LDS read is none of the vector ALU's)
    // unoccluded shadow rays of each wave so far (any-hit): kept in LDS, not in a register -- the kernel sits at the 72
    // VGPRs / ~96 SGPRs that 7 waves per SIMD allow -- and added to the device counter once, when the wave retires
    __shared__ uint32_t ldsDeposits[kTraceBlock / 64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t gtid = blockIdx.x * kTraceBlock + threadIdx.x;
#define spill (a.spill + gtid) /* entry e at spill[e * totalThreads]; recomputed where used (rare) to save two registers */
    // Ray finished: closestT != maxT decides hit/miss (scene.cl:257); a shadow ray only gets here unoccluded (an occluded one retires in its leaf step).
    // ONE definition for the two special-step schemes below -- as a macro, with the closest hit written in place (writeClosestHit's arithmetic, pt_walk.h, on the
    // lane's own registers): as a lambda like push / pop it costs k_trace<false, 0> 12 bytes of scratch, as a function, or with the record passed on by value, the
    // three closest-hit instantiations come out with another schedule
#define finishRay()                                                                                                  \
    {                                                                                                                \
        if (ANY_HIT) {                                                                                               \
            if (a.occluded)                                                                                          \
                a.occluded[rayIdx] = 0u;                                                                             \
            depositUnoccluded(a, a.rayC[rayIdx], asU(a.rayD[rayIdx].w));                                             \
        } else {                                                                                                     \
            if (hprim >= 0 && hinst < 0) { /* hit on a world-space copy of an instance: back to (original triangle, instance) */ \
                const float4 tc = sc.tris[hprim].c;                                                                  \
                hprim = (int)asU(tc.y);                                                                              \
                hinst = (int)asU(tc.z);                                                                              \
            }                                                                                                        \
            a.hit[rayIdx] = make_float4(hprim >= 0 ? tClosest : INFINITY, hu, hv, asF((uint32_t)hprim));             \
            a.inst[rayIdx] = hinst;                                                                                  \
        }                                                                                                            \
        cur = kRefIdle;                                                                                              \
    }
    const uint32_t total = a.totalThreads;
    const uint32_t count = ANY_HIT ? a.ctl->shadowCount[a.pass] : a.ctl->extCount[a.pass];
    const SceneDev& sc = a.sc;
    if (ANY_HIT && lane == 0)
        ldsDeposits[wave] = 0u;
    if constexpr (TWO_LEVEL) {
        if (threadIdx.x < kInstFoldTable) {
            const float4 e = threadIdx.x < a.instFoldCount ? a.instFold[threadIdx.x] : make_float4(1.f, 0.f, 0.f, 0.f);
            ldsInstFold[threadIdx.x] = e;
            ldsInstScale[threadIdx.x] = e.x == 1.f ? 1.f : 1.0f / e.x;
        }
        __syncthreads();
    }
    const bool fold = TWO_LEVEL && a.instFoldCount != 0u; // wave-uniform
    if constexpr (GENERAL) {
        if (lane < (uint32_t)kObjPlanes)
            ldsObj[wave][lane][64] = 0.f; // (read by this wave alone, LDS operations of a wave complete in order: no barrier)
    }

    auto push = [&](int slot, uint32_t v) {
        if (slot < kLdsStack)
            ldsStack[slot][threadIdx.x] = v;
        else
            spill[(size_t)(slot - kLdsStack) * total] = v;
    };
    // always a plain ds_read_b32; the (rare) spilled entry overrides it.  Selecting between the two
    // addresses instead makes hipcc emit ONE flat_load on the critical pop -> node-fetch path.
    auto pop = [&](int slot) -> uint32_t {
        uint32_t v = ldsStack[min(slot, kLdsStack - 1)][threadIdx.x];
        if (slot >= kLdsStack)
            v = ((const volatile uint32_t*)spill)[(size_t)(slot - kLdsStack) * total]; // volatile: keeps the two loads apart
        return v;
    };

    PT_STAT_BEGIN;
    PT_TIC(tKernel);
    // A lane without a ray holds kRefIdle in `cur`: there is no separate "active" flag.  Every vote below is a ballot of ONE compare on `cur` (the
    // compiler turns that into the compare alone; a ballot of `flag && compare` it lowers as the and, a select to 0 / 1 and a compare with 0 -- two
    // more vector instructions per vote of a vector-issue-bound loop), and the counts that have no compare of their own are differences of the ones that have.
    static_assert(kTraceBlock % 64 == 0, "the votes count 64 lanes per wave");
    auto lanesOf = [](unsigned long long mask) -> int { // lanes in a ballot's mask: a 32-bit scalar
        int n = __popcll(mask);
        asm("" : "+s"(n)); // (comparing the 64-bit population count with a constant otherwise goes to the VECTOR unit as a 64-bit compare)
        return n;
    };
    auto votes = [&](bool p) -> int { return lanesOf(__ballot(p)); };
    bool exhausted = false; // wave-uniform: queue has no more rays
    uint32_t rayIdx = 0;
    // ray of the space being traversed (world or instance): origin, direction, 1/direction, -origin/direction
    V3 co = mk(0.f), cd = mk(0.f), cid = mk(0.f);
    float tClosest = 0.f, hu = 0.f, hv = 0.f;
    int hprim = -1, hinst = -1, curInst = -1;
    uint32_t cur = kRefIdle;
    // The stack position, in the form the LDS address needs: the byte offset of the lane's next free entry in ldsStack, entries * kSpStep + thread * 4.
    // A push stores at spB and adds kSpStep, the prefetch of the top reads at spB - kSpStep, and "empty" / "three more fit" / "spilled" are compares
    // of spB with constants: no `entry << 8 | lane` rebuilt per access, no register for the lane's base.  The cold paths (spill, the parked steps)
    // take the entry count out of it.
    constexpr uint32_t kSpStep = kTraceBlock * 4u;
    uint32_t spB = threadIdx.x * 4u;
    auto spEntries = [&]() -> int { return (int)(spB / kSpStep); };
    auto ldsAt = [&](uint32_t ofs) -> uint32_t& { return *(uint32_t*)((char*)&ldsStack[0][0] + ofs); };
    // value of pop() given the prefetched LDS entry `top` (does not move the stack position)
    auto popTop = [&](uint32_t top) -> uint32_t {
        uint32_t v = spB >= kSpStep ? top : kRefFinish;
        if (spB >= (uint32_t)(kLdsStack + 1) * kSpStep)
            v = ((const volatile uint32_t*)spill)[(size_t)(spEntries() - 1 - kLdsStack) * total];
        return v;
    };
    auto setRay = [&](V3 o, V3 d) {
        co = o;
        cd = d;
        cid = mk(rcpSlab(d.x), rcpSlab(d.y), rcpSlab(d.z));
    };

    // ---- per-wave ray packets (see header comment) ---------------------------------------------
    uint32_t poolBase = 0, poolNext = 0, poolEnd = 0; // wave-uniform
    // Claiming queue entries: the first packet of every wave is static (wave w takes entries [64w, 64w+64)),
    // later ones come from ONE shared cursor in spans of up to 512 entries -- a single device-scope word
    // sustains only ~88 atomics/us (MI355X_MICROARCH.md, row `dequeue`), which at 64 rays per atomic would
    // cap the kernel near 5.6 Grays/s and costs ~46 us per launch for the 4096 initial requests alone.
    const uint32_t totalWaves = total >> 6, gwave = gtid >> 6;
    const uint32_t spanSize = 64u * min(8u, max(1u, count / (totalWaves * 64u * 8u)));
    // (Shrinking the static packets of small launches -- the passes of a 1-spp 1280 x 720 frame hold 0.1-0.9 M rays for 0.46 M lanes --
    // so that every wave gets a share of >= 8 rays was measured in round 3: 1.34 instead of 1.37 ms per frame alone, 1.18 instead of
    // 1.03 ms together with the overlapped passes of ptamd.hip: more resident waves slow every wave's iteration down.)
    uint32_t spanNext = gwave * 64u, spanEnd = spanNext + 64u; // wave-uniform: claimed, not yet loaded
    auto requestPacket = [&]() {
        if (spanNext >= spanEnd) {
            uint32_t base = 0xFFFFFFC0u; // "nothing left"
            // guided self-scheduling (kGuidedSpans): towards the end of the queue claim less (`spanEnd`, this wave's previous claim, lags the
            // cursor: an upper bound of what is left)
            const uint32_t left = count > spanEnd ? count - spanEnd : 0u;
            const uint32_t claim = min(spanSize, max(64u, (left / (totalWaves * kGuidedSpans)) & ~63u));
            // (small launches -- the passes of a 1-spp frame -- are covered by the static packets: no dynamic part, and no wave asks the
            // cursor just to learn that: 7 168 such atomics were ~80 us of a 100-250 us launch)
            if (gwave * 64u < count && (count + 63u) / 64u > totalWaves) {
                if (lane == 0)
                    base = atomicAdd(ANY_HIT ? &a.ctl->shadowCursor[a.pass] : &a.ctl->extCursor[a.pass], claim);
                base = totalWaves * 64u + (uint32_t)__builtin_amdgcn_readfirstlane((int)base); // (lane 0's: every lane of the wave is here)
            }
            spanNext = base;
            spanEnd = base + claim;
        }
        const uint32_t base = spanNext;
        spanNext += 64u;
        poolBase = base;
        poolNext = 0;
        poolEnd = base < count ? min(64u, count - base) : 0u;
        if (STAGED && poolEnd) { // wave-uniform.  Lane l copies entry l (clamped: the tail of the last packet is never handed out)
            const uint32_t e = base + min(lane, poolEnd - 1u);
            // every lane has read its ray of the previous packet (the reads were waited for before the rays were used)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.rayO + e), (__attribute__((address_space(3))) void*)&ldsRays[wave][0][0], 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.rayD + e), (__attribute__((address_space(3))) void*)&ldsRays[wave][1][0], 16, 0, 0);
        }
    };
    requestPacket();

    while (true) {
        // ---- hand rays to idle lanes ----------------------------------------------------------
        PT_TIC(tHand);
        if (!exhausted) {
            const unsigned long long idle = __ballot(cur == kRefIdle);
            const int nIdle = lanesOf(idle);
            if (nIdle >= (TWO_LEVEL ? PT_REFILL_IDLE_TL : kRefillIdleLanes)) {
                const uint32_t avail = poolEnd - poolNext;
                if (avail == 0u) {
                    exhausted = true; // the request issued after the last hand-out came back empty
                } else {
                    PT_TIC(tShfl);
                    const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
                    const int e = (int)min(poolNext + rank, 63u);
                    float4 ro, rd;
                    // the packet is only claimed; the lanes that take a ray read it straight from the queue
                    // (consecutive entries for consecutive idle lanes) -- no packet registers, no shuffles
                    ro = rd = make_float4(0, 0, 0, 0);
                    if constexpr (STAGED) {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the packet's copy into LDS has landed
                        if (cur == kRefIdle && rank < avail) {
                            ro = ldsRays[wave][0][e];
                            rd = ldsRays[wave][1][e];
                        }
                    } else if (cur == kRefIdle && rank < avail) {
                        ro = a.rayO[poolBase + (uint32_t)e];
                        rd = a.rayD[poolBase + (uint32_t)e];
                    }
                    PT_TOC(16, tShfl);
                    PT_TIC(tAssign);
                    if (cur == kRefIdle && rank < avail) {
                        const uint32_t idx = poolBase + (uint32_t)e;
                        float tMax = ANY_HIT ? ro.w : INFINITY;
                        asm volatile("" : "+v"(tMax)); // own register: hipcc 7.2 otherwise lets the flag load below alias ro.w and drops the tClosest assignment
                        uint32_t state = asU(rd.w); // closest-hit: parity mode keeps finished rays in the queue
                        if (ANY_HIT) // contribution and pixel stay in the queue until the ray turns out unoccluded
                            state = a.parityShadow ? asU(a.rayC[idx].w) : 0u;
                        const bool live = (state & FLAG_FINISHED) == 0u;
                        if (!ANY_HIT && !live) {
                            a.hit[idx] = make_float4(INFINITY, 0.f, 0.f, asF(0xFFFFFFFFu));
                            a.inst[idx] = -1;
                        }
                        if (live) {
                            rayIdx = idx;
                            nudgeZero(ro, rd);
                            setRay(xyz(ro), xyz(rd));
                            tClosest = tMax;
                            hprim = -1;
                            hinst = -1;
                            curInst = -1;
                            hu = hv = 0.f;
                            cur = sc.rootRef; // (the lane has a ray from here on)
                            spB = threadIdx.x * 4u;
                        }
                    }
                    PT_TOC(17, tAssign);
                    PT_STAT(8, 1);
                    PT_STAT(9, min((uint32_t)nIdle, avail));
                    poolNext += min((uint32_t)nIdle, avail);
                    if (poolNext == poolEnd) {
                        PT_TIC(tReq);
                        requestPacket();
                        PT_TOC(15, tReq);
                    }
                }
            }
        }
        PT_TOC(14, tHand);
        PT_TIC(tSpec);
        if constexpr (TWO_LEVEL) {
            // ---- parked lanes of a tree with instances: ONE pass serves them all -------------------------------------------
            // A parked lane has popped its leave-instance sentinel, stands before an instance, or is done.  What it needs follows from
            // what comes NEXT: after the sentinel the next stack entry -- an instance (world-space ray from the queue, then the
            // transform: exit and entry in one step), a top-level node or leaf (the world-space ray), nothing (the result).  Round 2
            // looped here, one kind of step per round: an exit followed by an entry was two rounds.
            const bool wantSpecial = cur >= kRefFirstSpecial && cur != kRefIdle;
            const unsigned long long m = __ballot(cur >= kRefFirstSpecial) & ~__ballot(cur == kRefIdle); // (one compare per ballot, see `votes`)
            if (m != 0ull) {
                PT_STAT(4, 1);
                PT_STAT(7, __popcll(m));
                const bool leaving = wantSpecial && cur == kRefLeaveInstance;
                if (leaving) {
                    curInst = -1;
                    if (spB >= kSpStep) {
                        spB -= kSpStep;
                        cur = pop(spEntries());
                    } else {
                        cur = kRefFinish;
                    }
                }
                const bool finishing = cur == kRefFinish; // (such a lane was parked: it stood on this reference or has just popped its way to it)
                if (ANY_HIT) { // a shadow ray only gets here unoccluded (an occluded one retires in its leaf step)
                    const uint32_t nFin = (uint32_t)__popcll(__ballot(finishing));
                    if (lane == 0)
                        ldsDeposits[wave] += nFin;
                }
                if (finishing) {
                    finishRay()
                } else if (wantSpecial) {
                    V3 wo = co, wd = cd; // the world-space ray: still in the registers, unless the lane comes out of an instance
                    if (leaving) { // ... then from the queue again, with the hand-out's fix-up (instances are rarely entered: ptamd.hip copies them to world space)
                        const float4 qo = a.rayO[rayIdx], qd = a.rayD[rayIdx];
                        wo = xyz(qo), wd = xyz(qd);
                        nudgeZero(wo, wd);
                    }
                    if (refCount(cur) == kRefSpecial) {
                        // -------- enter instance refIndex(cur) (scene.cl:116-139); instances are only ever entered from world space
                        const uint32_t what = refIndex(cur);
                        const Instance in = sc.instances[what];
                        curInst = (int)what; // instance index; pt_intersect reports the top-level leaf
                        if (fold && in.folded) {
                            // a folded instance reached through its instance reference (the start states of the shared descent come from the top level
                            // that holds those): the lane keeps the world-space ray, the steps below take it into the instance's space on the fly
                            setRay(wo, wd);
                        } else {
                            V3 to, td;
                            rayIntoInstance(in.r0, in.r1, in.r2, wo, wd, &to, &td);
                            setRay(to, td);
                            push(spEntries(), kRefLeaveInstance);
                            spB += kSpStep;
                        }
                        cur = in.rootRef;
                    } else {
                        setRay(wo, wd); // back in world space, at a top-level node or leaf
                    }
                }
            }
        } else {
            // ---- resolve special references: in these instantiations the end of a traversal alone (one world-space tree has no instance
            // references, GENERAL enters them in its leaf steps) -------------------
            // They are kept OUT of the hot loop below: lanes that reach one park until the loop breaks, then all
            // of them are served here at once.  The hot loop thus only ever changes (cur, spB, closest hit) and
            // the ray-space registers stay loop-invariant in it.
            // The one special reference a lane of these instantiations can stand on is kRefFinish (the tree holds no other; kRefIdle is no ray), and
            // finishing leaves the lane idle: one vote, one pass.
            const bool finishing = cur == kRefFinish; // (GENERAL: an instance reference is a leaf-kind step of the hot loop)
            const unsigned long long m = __ballot(finishing);
            if (m != 0ull) {
                PT_STAT(4, 1);
                PT_STAT(7, __popcll(m));
                if (ANY_HIT) { // a shadow ray only gets here unoccluded (an occluded one retires in its leaf step)
                    const uint32_t nFin = (uint32_t)__popcll(m);
                    if (lane == 0)
                        ldsDeposits[wave] += nFin;
                }
                if (finishing)
                    finishRay()
            }
        }
        PT_TOC(13, tSpec);
        if (__ballot(cur != kRefIdle) == 0ull) {
            if (exhausted)
                break;
            continue;
        }

        // ---- hot loop: inner steps and leaves, until enough lanes are parked (special) or idle -------
        while (true) {
            // the entry a pop would return, fetched before the node / triangle loads so that its LDS latency
            // hides under theirs (whichever step runs this iteration pops at most once, and only when it has
            // pushed nothing)
            // (two instructions: a minimum and a saturating subtraction.  An empty stack reads the block's first dword, a spilled one entry
            // kLdsStack - 1 of the block's last thread: inside the array, and popTop does not use the value in either case.)
            const uint32_t topOf = min(spB, (uint32_t)kLdsStack * kSpStep + (kSpStep - 4u));
            const uint32_t stackTop = ldsAt(topOf >= kSpStep ? topOf - kSpStep : 0u);
            // Three votes, one compare each: inner nodes lie below the leaves, the parked kinds and kRefIdle above them.  (GENERAL: an instance reference
            // is a leaf-kind step; what parks is kRefFinish alone, which with kRefIdle tops the range -- instance indices end below kSpecialIdle.)
            const bool wantInner = cur < (1u << kRefIndexBits);
            const bool parkedOrIdle = cur >= (GENERAL ? kRefIdle : kRefFirstSpecial);
            const bool wantLeaf = !wantInner && !parkedOrIdle;
            const int nInner = votes(wantInner), nParkedOrIdle = votes(parkedOrIdle), nIdle = votes(cur == kRefIdle);
            const int nLeaf = 64 - nInner - nParkedOrIdle;
            PT_STAT(0, 1);
            PT_STAT(1, nInner + nLeaf);
            // leave when nothing is left to do here, when enough lanes are parked on a special step, or when
            // enough lanes are idle for a hand-out (and the queue still has rays)
            const int nSpecial = nParkedOrIdle - nIdle;
            const int nWork = nInner + nLeaf;
            constexpr int parkedBreak = TWO_LEVEL ? (ANY_HIT ? PT_PARKED_BREAK_ANY_TL : PT_PARKED_BREAK_TL) : (ANY_HIT ? kParkedBreakAny : kParkedBreak);
            if (nWork == 0 || nSpecial >= parkedBreak || (!exhausted && 64 - nWork - nSpecial >= (TWO_LEVEL ? PT_REFILL_IDLE_TL : kRefillIdleLanes)))
                break;
            const bool innerTurn = nInner * PT_VOTE_INNER >= nLeaf * PT_VOTE_LEAF;
            if (innerTurn) {
                PT_STAT(2, 1);
                PT_STAT(5, nInner);
                PT_TIC(tInner);
                if (wantInner) {
                    // -------- inner step at either level: one 64-byte fetch, FOUR quantised child boxes ----------
                    // TWO_LEVEL: the lane's instance and its table entry, ahead of the node fetch (the LDS read hides under it)
                    float4 foldIs = make_float4(1.f, 0.f, 0.f, 0.f);
                    float foldScale = 1.f;
                    if constexpr (TWO_LEVEL) {
                        const uint32_t ni = refIndex(cur), rk = ni - sc.instRootBase;
                        if (rk < sc.numInstRoots) // an instance's copy of its mesh root: from here on (until the walk is back at world-space references) the lane is inside instance rk
                            curInst = (int)rk;
                        const bool object = ni - sc.firstWorldNode >= sc.instRootBase - sc.firstWorldNode; // (unsigned: below the first world-space node, or behind the last)
                        const uint32_t slot = fold && object ? (uint32_t)curInst + 1u : 0u;
                        foldIs = ldsInstFold[slot];
                        foldScale = ldsInstScale[slot];
                    }
                    float genM = 1.f;
                    V3 genO = mk(0.f), genI = mk(0.f);
                    if constexpr (GENERAL) { // the LDS reads ahead of the node fetch: their latency hides under it
                        const bool object = refIndex(cur) < sc.firstWorldNode; // a node of a mesh tree (the top level and the world-space copies come behind them)
                        const uint32_t slot = object ? lane : 64u;
                        genM = object ? 0.f : 1.f;
                        genO = mk(ldsObj[wave][0][slot], ldsObj[wave][1][slot], ldsObj[wave][2][slot]);
                        genI = mk(ldsObj[wave][3][slot], ldsObj[wave][4][slot], ldsObj[wave][5][slot]);
                    }
                    // base (scalar registers) + 32-bit byte offset: one shift instead of two 64-bit vector operations per step (nodes < 4 GB: refused at upload otherwise)
                    const uint4* wp = (const uint4*)((const char*)sc.wide + (size_t)(uint32_t)(refIndex(cur) << 6));
                    const uint4 A = wp[0], B = wp[1];
                    const uint4 C = wp[2];
                    const uint4 D = wp[3];
                    // the ray in the node's space (TWO_LEVEL: object-space nodes are seen through the lane's instance, see the top)
                    V3 no = co, nid = cid;
                    if constexpr (TWO_LEVEL) {
                        no = mk(fmaf(co.x, foldIs.x, foldIs.y), fmaf(co.y, foldIs.x, foldIs.z), fmaf(co.z, foldIs.x, foldIs.w));
                        nid = mk(cid.x * foldScale, cid.y * foldScale, cid.z * foldScale);
                    }
                    if constexpr (GENERAL) { // world * m + slot: the lane's instance-space ray at object-space nodes (m = 0), the world-space ray elsewhere (slot = 0)
                        no = mk(fmaf(co.x, genM, genO.x), fmaf(co.y, genM, genO.y), fmaf(co.z, genM, genO.z));
                        nid = mk(fmaf(cid.x, genM, genI.x), fmaf(cid.y, genM, genI.y), fmaf(cid.z, genM, genI.z));
                    }
                    const SlabSetup slab = slabSetup(A, B, C, no, nid);
                    float key[4];
                    uint32_t ref[4] = { D.x, D.y, D.z, D.w };
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const f2 tt = childSlab(slab, k);
                        // accept test of bvh.cl:72,114 on the (slightly larger) quantised box
                        const bool vis = tt.y >= tt.x && tt.y >= 0.f && tt.x < tClosest;
                        key[k] = vis ? tt.x : INFINITY;
                    }
                    auto visible = [&](int k) { return key[k] < INFINITY ? 1 : 0; };
                    if (ANY_HIT)
                        sort4NearestToFront(key, ref);
                    else
                        sort4Nearest(key, ref);
                    // farthest first onto the stack, continue with the nearest
                    if (spB < (uint32_t)(kLdsStack - 2) * kSpStep) { // three more entries fit the LDS part
                        // common case, branch-free: every candidate is stored, the stack position only moves past the
                        // ones that are kept (a rejected one is overwritten by the next store)
                        ldsAt(spB) = ref[3];
                        spB += visible(3) ? kSpStep : 0u;
                        ldsAt(spB) = ref[2];
                        spB += visible(2) ? kSpStep : 0u;
                        ldsAt(spB) = ref[1];
                        spB += visible(1) ? kSpStep : 0u;
                    } else {
                        if (visible(3)) {
                            push(spEntries(), ref[3]);
                            spB += kSpStep;
                        }
                        if (visible(2)) {
                            push(spEntries(), ref[2]);
                            spB += kSpStep;
                        }
                        if (visible(1)) {
                            push(spEntries(), ref[1]);
                            spB += kSpStep;
                        }
                    }
                    // no visible child => nothing was pushed => the prefetched stack top is still the top
                    const uint32_t next = popTop(stackTop);
                    if (visible(0))
                        cur = ref[0];
                    else
                        cur = next, spB = spB >= kSpStep ? spB - kSpStep : spB;
                }
                PT_TOC(11, tInner);
            } else {
                PT_STAT(3, 1);
                PT_STAT(6, nLeaf);
                PT_TIC(tLeaf);
                const uint32_t kindBits = refCount(cur);
                if (GENERAL && wantLeaf && kindBits == kRefSpecial) {
                    // -------- enter instance refIndex(cur) (scene.cl:116-139): a leaf-kind step.  The lane's registers keep the world-space ray; the
                    // instance-space ray goes into the lane's LDS slot, where the steps on the instance's nodes and triangles read it
                    // Two records per instance.  The ENTRY record (32 bytes, a.instFold[2 what]: (1 / s, w), then root reference, "simple" flag, s) serves the common
                    // transform -- a translation + uniform scale -- with the folded route's arithmetic: three FMAs, six products, no reciprocal, no zero-component
                    // fix-ups (the world ray has had its own).  A crowd of such instances runs this block in four leaf iterations of five (208 instances: +19 %
                    // vector instructions per ray against the copied scene with the full transform in it, profiles/round6/r6d_*); the full 3 x 4 transform
                    // (rayIntoInstance on the 64-byte Instance record: the parked route's arithmetic, bit for bit) runs only where a lane needs it.
                    const uint32_t what = refIndex(cur);
                    const float4* ep = (const float4*)((const char*)a.instFold + (size_t)(what << 5));
                    const float4 ef = ep[0], et = ep[1];
                    // (a scene that holds instances of the other kind -- a.instFoldCount, wave-uniform -- fetches their rows in the same round trip: fetched only once
                    // the flag has arrived they cost the general scene a second, dependent one -- 0.999 against 1.008 of the copied scene; both forms behind
                    // branches of their own, the entry record's first half fetched inside: 0.879 against 0.899 on the uniform crowd)
                    const bool rows = a.instFoldCount != 0u;
                    const Instance* ip = (const Instance*)((const char*)sc.instances + (size_t)(what << 6));
                    static_assert(sizeof(Instance) == 64, "an instance record is addressed by index << 6");
                    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
                    if (rows)
                        r0 = ip->r0, r1 = ip->r1, r2 = ip->r2;
                    const uint32_t root = asU(et.x);
                    const bool simple = asU(et.y) != 0u;
                    V3 to = mk(fmaf(co.x, ef.x, ef.y), fmaf(co.y, ef.x, ef.z), fmaf(co.z, ef.x, ef.w));
                    V3 td = mk(cd.x * ef.x, cd.y * ef.x, cd.z * ef.x);
                    V3 tid = mk(cid.x * et.z, cid.y * et.z, cid.z * et.z);
                    if (rows && __ballot(!simple) != 0ull) { // (wave-uniform)
                        if (!simple) {
                            rayIntoInstance(r0, r1, r2, co, cd, &to, &td);
                            tid = mk(rcpSlab(td.x), rcpSlab(td.y), rcpSlab(td.z));
                        }
                    }
                    ldsObj[wave][0][lane] = to.x, ldsObj[wave][1][lane] = to.y, ldsObj[wave][2][lane] = to.z;
                    ldsObj[wave][3][lane] = tid.x, ldsObj[wave][4][lane] = tid.y, ldsObj[wave][5][lane] = tid.z;
                    ldsObj[wave][6][lane] = td.x, ldsObj[wave][7][lane] = td.y, ldsObj[wave][8][lane] = td.z;
                    curInst = (int)what;
                    cur = root; // nothing pushed: what lies below on the stack are world-space references, which read the world-space ray
                } else if (wantLeaf) {
                    // -------- leaf (scene.cl:168-195) with Moeller-Trumbore (shapes.cl:20-72) -----------------
                    const uint32_t first = refIndex(cur), n = kindBits;
                    V3 lo_ = co, ld_ = cd; // the ray in the triangles' space
                    bool inObject = false;
                    if constexpr (GENERAL) {
                        inObject = first < sc.numTriangles + 1u; // the caller's (object-space) triangles; world-space copies come behind them
                        const uint32_t slot = inObject ? lane : 64u;
                        const float m = inObject ? 0.f : 1.f;
                        lo_ = mk(fmaf(co.x, m, ldsObj[wave][0][slot]), fmaf(co.y, m, ldsObj[wave][1][slot]), fmaf(co.z, m, ldsObj[wave][2][slot]));
                        ld_ = mk(fmaf(cd.x, m, ldsObj[wave][6][slot]), fmaf(cd.y, m, ldsObj[wave][7][slot]), fmaf(cd.z, m, ldsObj[wave][8][slot]));
                    }
                    if constexpr (TWO_LEVEL) {
                        inObject = first < sc.numTriangles + 1u; // the caller's (object-space) triangles; world-space copies come behind them
                        const float4 is = ldsInstFold[fold && inObject ? (uint32_t)curInst + 1u : 0u];
                        lo_ = mk(fmaf(co.x, is.x, is.y), fmaf(co.y, is.x, is.z), fmaf(co.z, is.x, is.w)); // rayIntoInstance's arithmetic for such a matrix, bit for bit
                        ld_ = mk(cd.x * is.x, cd.y * is.x, cd.z * is.x);
                    }
                    bool done = false;
                    for (uint32_t k = 0; k < n; k++) {
                        V3 v0, e1, e2;
                        fetchTri(sc, first + k, &v0, &e1, &e2);
                        float det, u, v, t;
                        triangleTest(lo_, ld_, v0, e1, e2, &det, &u, &v, &t);
                        const bool hit = PT_TRI_HIT(det, u, v, t, tClosest);
                        if (hit) {
                            if (ANY_HIT) {
                                done = true;
                                break;
                            }
                            tClosest = t;
                            hu = u;
                            hv = v;
                            hprim = (int)(first + k);
                            hinst = (TWO_LEVEL || GENERAL) ? (inObject ? curInst : -1) : curInst;
                        }
                    }
                    if (ANY_HIT && done) { // occluded: nothing to deposit
                        if (a.occluded)
                            a.occluded[rayIdx] = 1u;
                        cur = kRefIdle;
                    } else {
                        cur = popTop(stackTop);
                        spB = spB >= kSpStep ? spB - kSpStep : spB;
                    }
                }
                PT_TOC(12, tLeaf);
            }
        }
    }
    if (ANY_HIT && lane == 0 && ldsDeposits[wave])
        atomicAdd(&a.ctl->depositsShadow, ldsDeposits[wave]);
    PT_TOC(10, tKernel);
    PT_STAT_END(ANY_HIT ? 24 : 0);
}

#undef spill
#undef finishRay

} // namespace ptd
