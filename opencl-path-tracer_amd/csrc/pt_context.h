// The context of the C-ABI (include/ptamd.h): device buffers, the two static scenes and the two dynamic sets a context holds, error reporting.
// Included by ptamd.hip alone (one translation unit: the kernels -- pt_shade.h, then pt_walk.h, the steps every traversal kernel shares, under pt_trace.h / pt_packet.h /
// pt_packet_multi.h / pt_team.h --, pt_context.h, pt_schedule.h, then the C-ABI shell; the conversion is pt_convert.cpp).
#pragma once

namespace {

thread_local std::string g_createError;

// What the runtime allocates is owned by one of the four types below: freed by the destructor, moved but never copied, and counted -- device allocations,
// pinned allocations, events, owned streams alive in this process (pt_debug_live_resources).  None of them may have static storage duration: nothing is
// freed after the HIP runtime has shut down.
std::atomic<uint32_t> g_live[4];

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {} // (no copies: the compiler refuses them from here on)
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count)
    {
        release();
        n = count;
        if (count == 0)
            return hipSuccess;
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess)
            g_live[0]++;
        return e;
    }
    void release()
    {
        if (p) {
            (void)hipFree(p);
            g_live[0]--;
        }
        p = nullptr;
        n = 0;
    }
    // The whole buffer on stream `s`: zeroed; allocated and zeroed if it is not there yet; to and from the host.  copyTo / copyFrom issue the
    // asynchronous copy alone, for buffers that travel together behind one synchronisation; read / write are one copy and the synchronisation.  A null
    // `host` is skipped on the way out (the entry points that allow one say so).
    hipError_t zero(hipStream_t s) { return hipMemsetAsync(p, 0, n * sizeof(T), s); }
    hipError_t ensureZeroed(size_t count, hipStream_t s)
    {
        if (p)
            return hipSuccess;
        const hipError_t e = alloc(count);
        return e == hipSuccess ? zero(s) : e;
    }
    hipError_t copyTo(void* host, hipStream_t s) const { return host ? hipMemcpyAsync(host, p, n * sizeof(T), hipMemcpyDeviceToHost, s) : hipSuccess; }
    hipError_t copyFrom(const void* host, hipStream_t s) { return hipMemcpyAsync(p, host, n * sizeof(T), hipMemcpyHostToDevice, s); }
    hipError_t read(void* host, hipStream_t s) const
    {
        const hipError_t e = copyTo(host, s);
        return e == hipSuccess ? hipStreamSynchronize(s) : e;
    }
    hipError_t write(const void* host, hipStream_t s)
    {
        const hipError_t e = copyFrom(host, s);
        return e == hipSuccess ? hipStreamSynchronize(s) : e;
    }
};

// `count` records of pinned host memory
template <typename T>
struct Pinned {
    T* p = nullptr;
    Pinned() = default;
    Pinned(Pinned&&) = delete;
    ~Pinned() { release(); }
    hipError_t alloc(size_t count)
    {
        release();
        const hipError_t e = hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess)
            g_live[1]++;
        else
            p = nullptr;
        return e;
    }
    void release()
    {
        if (p) {
            (void)hipHostFree(p);
            g_live[1]--;
        }
        p = nullptr;
    }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {} // (pt_ctx::profEvents grows)
    ~Event()
    {
        if (e) {
            (void)hipEventDestroy(e);
            g_live[2]--;
        }
    }
    hipError_t create(bool timing = false) // (if there is none yet)
    {
        if (e)
            return hipSuccess;
        const hipError_t rc = timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (rc == hipSuccess)
            g_live[2]++;
        else
            e = nullptr;
        return rc;
    }
    operator hipEvent_t() const { return e; }
};

// a stream the context created (`owned`), or the caller's (pt_set_stream), which is never destroyed
struct Stream {
    hipStream_t s = nullptr;
    bool owned = false;
    Stream() = default;
    Stream(Stream&&) = delete;
    ~Stream() { adopt(nullptr); }
    hipError_t create()
    {
        adopt(nullptr);
        const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e == hipSuccess)
            g_live[3]++, owned = true;
        else
            s = nullptr;
        return e;
    }
    void adopt(hipStream_t callers)
    {
        if (owned && s) {
            (void)hipStreamDestroy(s);
            g_live[3]--;
        }
        s = callers;
        owned = false;
    }
    operator hipStream_t() const { return s; }
};

// Pinned staging memory that asynchronous copies read from (grow-only, like the device buffers), the event recorded behind the copies out of it, and whether
// such copies may still be in flight.  Each caller states its own capacity when it grows the memory.
struct Staging {
    Pinned<unsigned char> mem;
    size_t bytes = 0;
    Event read;
    bool busy = false;
    hipError_t wait() // until the last copies out of the memory are done (normally long done)
    {
        if (busy) {
            const hipError_t e = hipEventSynchronize(read);
            if (e != hipSuccess)
                return e;
            busy = false;
        }
        return hipSuccess;
    }
    hipError_t reserve(size_t need, size_t capacity) // (new memory has no copies in flight)
    {
        if (bytes >= need)
            return hipSuccess;
        bytes = 0;
        const hipError_t e = mem.alloc(capacity);
        if (e == hipSuccess)
            bytes = capacity, busy = false;
        return e;
    }
    hipError_t recordRead(hipStream_t s)
    {
        const hipError_t e = hipEventRecord(read, s);
        if (e == hipSuccess)
            busy = true;
        return e;
    }
};

// Two width * height float4 planes that are made, cleared, read and written together: allocated (zeroed, on the context's stream) at first use.
struct PlanePair {
    DevBuf<float4> plane[2];
    float4* operator[](int k) const { return plane[k].p; }
    int ensure(pt_ctx* c);
    int zero(pt_ctx* c);
    int read(pt_ctx* c, float* out0, float* out1); // (either may be null)
    int write(pt_ctx* c, const float* in0, const float* in1);
};

// a queue's three planes of `count` entries each (stops at the first error)
inline hipError_t allocPlanes(DevBuf<float4>& a, DevBuf<float4>& b, DevBuf<float4>& c, size_t count)
{
    hipError_t e = a.alloc(count);
    if (e == hipSuccess && (e = b.alloc(count)) == hipSuccess)
        e = c.alloc(count);
    return e;
}
struct RayQueueBuf {
    DevBuf<float4> o, d, thr;
    RayQueue view() const { return { o.p, d.p, thr.p }; }
    hipError_t alloc(size_t count) { return allocPlanes(o, d, thr, count); }
    void release() { o.release(), d.release(), thr.release(); }
};
struct ShadowQueueBuf {
    DevBuf<float4> o, d, c;
    ShadowQueue view() const { return { o.p, d.p, c.p }; }
    hipError_t alloc(size_t count) { return allocPlanes(o, d, c, count); }
    void release() { o.release(), d.release(), c.release(); }
};

} // namespace

// Everything pt_upload_static derives from the caller's static arrays -- the host half (ptconv::StaticHost, pt_convert.h: what the conversion makes) and the
// device's master copies.  A context holds TWO (like the dynamic sets, like the reference's double-buffered cl::Buffers): renders and refits work on the
// current one while pt_upload_static_async converts a rebuilt scene into the other; pt_frame_tick adopts it together with the dynamic state built on it.
struct StaticScene {
    ptconv::StaticHost host;
    // one master copy of the converted arrays on the device, from which a dynamic set refreshes its own copy (device to device) when its version is stale
    DevBuf<WideNode> dWide;
    DevBuf<WideBoxes> dBoxes;
    DevBuf<uint32_t> dLeafOfs, dRefTri;
    DevBuf<TriIsect> dTris;
    DevBuf<TriFat> dFat;
    uint64_t onDeviceTopology = 0; // the host.topology the master copy was made from (a conversion that runs again makes a new one)
    // refit (pt_update_geometry): the caller's vertices on the device (the triangles' intersection and shading records are re-made
    // from them by k_refit_tris), pinned staging for them and for the re-quantised nodes, guarded by an event of its own
    DevBuf<pt_vertex> dVerts;
    DevBuf<pt_sub_bvh_node> dNodes; // the caller's nodes as last handed in
    DevBuf<uint32_t> dKidBoxNode;
    DevBuf<float> dExtra;
    // refit on the device alone (pt_refit_vertices): who a packed node reports to and how many arrivals complete it (k_refit_tree, pt_bake.h)
    DevBuf<uint32_t> dParent, dNeed, dArrived;
    uint64_t refitTablesFor = 0; // topology the tables were made for (0: none)
    bool refitTablesOk = false; // false: a node has two parents (roots that share a subtree): the caller refits on the host (pt_update_geometry)
    bool latestInStage = false; // the caller's latest vertices and nodes live in `stage` (vertices first), not in host.rawVerts / host.hostSubNodes
    Staging stage;
    DevBuf<TriShade> triShade;
    DevBuf<Material> materials;
    bool have = false; // holds a converted scene
};

struct pt_ctx {
    pt_config cfg {};
    std::string error;
    int device = 0;
    int numCUs = 0;
    // The streams come first: members are destroyed in reverse order, so everything below is freed before a stream is destroyed.  ~pt_ctx waits for all four.
    Stream stream; // renders (the context's own, or the caller's: pt_set_stream)
    Stream copyStream;
    // small launches (a 1-spp interactive frame): the shadow rays of bounce b are traced on `sideStream` while the main stream traces
    // the extension rays of bounce b + 1 (independent: both only need shade b; shade b + 1 waits for both)
    Stream sideStream;
    Stream sideStream2; // one sample in flight: the shadow passes of a frame alternate between two side streams (each bounce has its own shadow queue AND
                        // accumulator plane: nothing orders them but their own shade launch)
    Event evStart, evStop;
    std::vector<Event> profEvents;
    bool profile = false;

    ~pt_ctx()
    {
        (void)hipSetDevice(device);
        for (hipStream_t s : { stream.s, copyStream.s, sideStream.s, sideStream2.s }) // (the copy stream: a never-adopted upload may still be copying into the sets)
            if (s)
                (void)hipStreamSynchronize(s);
    }

    // The dynamic part of the scene -- what pt_upload_dynamic(_async) produces: 4-wide nodes of both levels, intersection
    // triangles (object space + world-space copies of instances), instances, lights -- exists TWICE, like the reference's
    // double-buffered cl::Buffers (m_topBvhBuffers[2], m_emissiveTrianglesBuffers[2], ... src/raytracer.h:93-106): renders
    // enqueued so far keep reading set `active` while the next state is converted on the host and copied into the other set on
    // the copy stream; pt_frame_tick makes the render stream wait for that copy and flips (RayTracer::frameTick,
    // src/raytracer.cpp:183-189; the barrier of :593).
    struct DynamicSet {
        DevBuf<WideNode> wide;
        DevBuf<TriIsect> tris;
        DevBuf<TriFat> fat; // shading records: they hold v0 / edges / normals, which a refitted mesh changes with the trees
        DevBuf<Instance> instances;
        DevBuf<Light> lights;
        DevBuf<BakeJob> jobs; // world-space copies to make (pt_bake.h)
        uint64_t staticVersion = 0; // version of the static arrays this set holds (0: none)
        int staticIndex = 0; // which of the context's two static scenes this state was built on
        uint32_t numTris = 0, firstWorldNode = 0; // of that scene, as the kernels need them (SceneDev)
        Staging stage; // what the asynchronous copies of an upload read from (its event: recorded on the copy stream)
        uint32_t numLights = 0, rootRef = 0;
        uint32_t foldedInstances = 0, instRootBase = 0, numInstRoots = 0;
        DevBuf<float4> instFold; // the table of folded instance transforms (pt_trace.h)
        DevBuf<uint32_t> instRootSrc;
        uint32_t instFoldCount = 0;
        uint32_t rootRefFolded = 0; // the same top level for the per-ray kernels: entry nodes in place of the instances that are a translation + uniform scale (pt_trace.h)
        bool packetOk = false;
        uint32_t stackNeed = 0; // worst-case traversal stack of this state (pt_stats.stack_need)
        bool hasInstances = false; // the tree holds instance references (instances that were not copied to world space)
        bool generalRoute = false; // ... and the per-ray kernels enter them as leaf-kind steps (pt_trace.h, LEVELS 2): some transform is not a translation + uniform scale, or there are more than the fold table holds
        uint32_t enteredInstances = 0; // instances that are entered at traversal (not copied to world space)
        std::vector<uint32_t> instanceTopNode; // instance index -> top-level leaf node index
        std::vector<Instance> hostInstances; // the instance table as uploaded (pt_set_instance_motion reads the current invTransform rows from it)
        uint32_t numTopNodes = 0; // top-level nodes of this state as the caller counts them
        Event uploaded; // recorded on the copy stream after the set's last upload
        Event lastUse; // recorded on the render stream when the set stopped being the active one
        bool used = false;
    } dyn[2];
    StaticScene stat[2];
    StaticScene* st = &stat[0]; // the static scene the entry points work on: the current one, except while pt_upload_static_async converts the other
    int statCur = 0; // static scene of the active dynamic set
    int statPending = -1; // converted by pt_upload_static_async, waiting for a dynamic state and pt_frame_tick
    uint64_t staticVersions = 0; // versions of the static arrays are drawn from one counter (a dynamic set compares the one it holds with the scene's)
    int active = 0; // set the render kernels read
    int pending = -1; // set with an upload in flight / finished that pt_frame_tick will switch to
    Event evShaded[kMaxPasses], evShadowed[kMaxPasses]; // (the side streams' shadow passes, at the top of the struct)
    // With ONE sample in flight the shadow rays deposit into an accumulator of their own (merged into the accumulator proper at the end of pt_render) from a shadow
    // queue per bounce: the shadow passes then depend on nothing but their own shade launch and run back to back on the side stream
    DevBuf<float4> accumShadow;
    ShadowQueueBuf shadowQ[kMaxPasses];
    bool mergePending = false;
    DevBuf<uint8_t> texMaterial, texSky; // float4 or BGRA8 texels (Texture::format)
    SceneDev scene {};
    bool haveStatic = false, haveDynamic = false, haveCamera = false;

    // frame state
    CameraDev camera {};
    DevBuf<uint32_t> pixelList;
    std::vector<uint32_t> hostPixelList; // what pixelList holds (pt_set_tiles with the same list again is a no-op)
    DevBuf<uint32_t> pixelOrdinal; // global pixel -> position in pixelList (only when the context owns part of the frame)
    DevBuf<float4> resolveTmp; // pt_resolve's output staging (allocated at first use)
    uint32_t numOwned = 0;
    uint32_t capacity = 0;
    // Queues smaller than a batch (pt_config.ext_queue_fraction / shadow_queue_fraction, round 6): entries the second extension queue (and, for batches of a
    // pinhole's bundles, the origin / throughput planes of the first) and the shadow queue hold; == capacity without fractions.  A batch is sized so that what its
    // passes emit fits, from the largest ratios seen in this epoch (camera, scene state, textures, tiling): extension rays of the FIRST pass (every later pass emits
    // at most what it was handed), shadow rays of ANY pass (a later pass can emit more of them than the first: glass in front of diffuse walls).
    uint32_t capExt = 0, capShadow = 0;
    bool q0Small = false; // the first queue's origin / throughput planes hold capExt entries (camera rays queued as directions only)
    bool ratiosKnown = false;
    double ratioExt = 0, ratioShadow = 0; // (extension rays emitted by pass 0, shadow rays emitted by the pass that emitted most) / (entries of the batch), the largest of this epoch
    double ratioShadowFirst = 0; // (shadow rays emitted by pass 0) / (entries of the batch), the largest of this epoch: pt_stats.first_pass_shadow_ratio
    Pinned<uint32_t> overflowPinned; // one word, set by k_clamp_counts when a batch emitted more than a queue holds after all: sticky, reported by pt_synchronize and the image reads
    uint32_t batchSamples = 0, probeBatches = 0;
    uint32_t epoch = 0, passCountsEpoch = 0; // camera / scene state / tiling the ratios belong to; ... the report in flight was launched in
    bool identityPixels = true;
    DevBuf<float4> accumOwn, accumPlanes;
    uint32_t packetBlocks[2] = { 0, 0 };
    uint32_t multiBlocks[2][2] = {}; // persistent grid of k_trace_multi [pinhole | a thin lens's converging bundles][without | with instance references in the tree]
    // live entries per pass of the most recent batch whose counters have come back (a HINT for the next batch's k_shade launches:
    // copied to pinned memory by the stream at the end of every batch, never waited for)
    Pinned<uint32_t> passCountsPinned; // as many words as passCountsHint
    Event passCountsCopied;
    uint32_t passCountsHint[2 * (kMaxPasses + 1)] = {}; // extension rays per pass, then shadow rays per pass
    uint32_t passCountsEntries = 0; // entries of the batch the hint comes from (0: no hint yet)
    uint32_t passCountsPending = 0; // entries of the batch whose copy is in flight
    uint32_t shadeHeadShift = 0; // diagnostics (PTAMD_SHADE_HEAD_SHIFT): shrinks the head of the split k_shade launches so that tests reach the tile-walking kernel
    uint32_t packetUse = 0; // bit 0: primary rays, bit 1: their shadow rays, bit 2: the pt_intersect test hook
    uint64_t packetLaunches = 0, genLaunches = 0, bundleLaunches = 0;
    float4* accum = nullptr;
    uint32_t planes = 1; // samples in flight (fixed schedule)
    uint32_t spp = 0;

    // queues
    RayQueueBuf rays[2], stagedRays;
    ShadowQueueBuf shadow, stagedShadow;
    DevBuf<float4> hitH;
    DevBuf<int32_t> hitInst;
    DevBuf<uint32_t> activeFlag;
    DevBuf<uint4> streams;
    DevBuf<Control> control;
    DevBuf<Totals> totals;
    DevBuf<uint32_t> spill;
    size_t spillHalf = 0;
    uint32_t traceBlocks[3] = { 0, 0, 0 }; // persistent grids: [0] one world-space tree, [1] trees with instance references (folded / parked), [2] the general route (pt_trace.h, LEVELS 2)
    uint32_t teamBlocks = 0; // grid of k_trace_team (pt_team.h: four lanes per ray, for launches that do not fill the machine)
    float teamRounds = 1.5f; // (1 / 1.5 / 1.7 / 2 / 3 measured on four scenes, tools/r5_frames_env.sh) ... used where the previous batch's pass held at most this many rays per team
    uint32_t teamUse = 7; // bit 0: the camera rays of 1-spp frames, bit 2: their shadow rays, bit 1: later passes by the previous batch's counters (PTAMD_TEAM_USE: diagnostics)
    uint32_t batchEntries = 0; // entries of the batch being enqueued (renderSampleFixed)
    uint64_t teamLaunches = 0;
    uint32_t foldPlanes = 0; // extra accumulator planes written since the last fold (folded at the end of pt_render)
    bool queuesReady = false;

    // first-hit guide buffers and the denoiser (pt_denoise.h): two width * height float4 sums over `guideSpp` guide samples, the scratch queue of the guide
    // pass (one sample of the owned pixels; allocated at first use, whatever the render queues look like), the filter's two ping-pong images and its
    // normalised guide image
    PlanePair guides; // [0] (albedo.rgb, hits), [1] (normal.xyz, depth)
    uint32_t guideSpp = 0;
    DevBuf<float4> guideRayO, guideRayD, guideHit;
    DevBuf<int32_t> guideHitInst;
    DevBuf<Control> guideCtl;
    // guide chain (pt_set_guide_chain; pt_denoise.h, k_guide_chain): the second scratch queue the stages ping-pong with, and the distance travelled so
    // far as a float plane per queue -- allocated at the first guide call with the chain on over a scene that holds glass
    uint32_t guideChain = 0; // max_transmissions; 0 = off
    DevBuf<float4> guideChainO, guideChainD;
    DevBuf<float> guideChainDist[2];
    DevBuf<int4> guideChainTerminals; // pt_debug_guide_chain_terminals (test hook): width * height records, allocated while enabled
    // guide reflections (pt_set_guide_reflections; k_guide_chain<true>): the tint of a chain's entries, a float4 plane per queue -- allocated at the first
    // guide call that runs the reflecting kernel
    bool guideReflections = false;
    DevBuf<float4> guideChainTint[2];
    DevBuf<float4> denoiseColour[2], denoiseGuide;
    Event evDenoise[2];

    // temporal history (pt_temporal.h): two sets for ping-pong of two width * height float4 images each -- (d.rgb, N) and (n.xyz, z) --, allocated at
    // the first temporal call; the camera set `temporalNewest` was made under.  pt_clear and pt_set_camera leave all of it alone.
    PlanePair temporal[2]; // of each set: [0] (d.rgb, N), [1] (n.xyz, z)
    int temporalNewest = 0;
    uint32_t temporalFrames = 0; // pt_temporal_accumulate calls (or 1 after pt_write_temporal) since the last reset: 0 = no history
    CameraDev temporalCamera {};
    uint32_t sampleBase = 0; // pt_set_sample_base: added to the sample index pt_render and pt_render_guides key the counter PRNG with

    // temporal variance (include/ptamd.h): one more plane per history set, width * height floats -- the variance of the luminances the pixel's history
    // stands for --, allocated (zeroed) at the first temporal call with the mode on.  The mode changes only while there is no history.
    struct Variance {
        DevBuf<float> plane[2];
        bool set = false;
        float sigma = 0, relativeFloor = 0, fullHistory = 0; // pt_variance_params, defaults resolved
    } variance;

    // temporal response (include/ptamd.h): one more float4 image per history set, the fast history (d_f.rgb, N_f), and two scratch planes -- the
    // luminance pairs k_temporal<., ., true> leaves for k_temporal_response, and the mix factor s of the last accumulate --, allocated (zeroed) at the
    // first temporal call with the mode on.  The mode changes only while there is no history.
    struct Response {
        DevBuf<float4> fast[2];
        DevBuf<float2> luminance;
        DevBuf<float> mix;
        bool set = false;
        float fastHistory = 0, sigma = 0, relativeFloor = 0; // pt_response_params, defaults resolved
    } response;

    // firefly clamp (include/ptamd.h; pt_firefly.h): the clamped plane (d.rgb, s), width * height float4, and its two counters (clamped, nonfinite) --
    // allocated at the first evaluation with the mode on, made afresh by every call that consumes the plane.  The mode may change at any time.
    struct Firefly {
        DevBuf<float4> plane;
        DevBuf<uint32_t> counts;
        bool set = false;
        bool evaluated = false; // the plane and the counters hold an evaluation
        uint32_t rank = 0;
        float scale = 0; // pt_firefly_params, defaults resolved
    } firefly;

    // adaptive sampling (include/ptamd.h; pt_adaptive.h): the two half accumulators, the per-pixel counts and errors, one error and one flag per 8 x 8
    // block, the counters of an evaluation and the pinned area the flags and counters are read back into (flags first) -- `buf`, made whole at the first
    // pt_render_adaptive / pt_write_adaptive, freed when the mode is turned off and by pt_destroy.  The mode changes only while there are no samples.
    struct Adaptive {
        struct Buffers {
            DevBuf<float4> half[2];
            DevBuf<uint32_t> counts, flags;
            DevBuf<float> error, blockError;
            DevBuf<ptd::AdaptiveCounters> counters;
            Pinned<uint32_t> back; // `blocks` flags, then the AdaptiveCounters
        };
        std::unique_ptr<Buffers> buf;
        bool set = false;
        pt_adaptive_params prm {}; // defaults resolved
        pt_adaptive_stats stats {}; // of the last evaluation
        Event events[2]; // around an evaluation's launches
        double timing[4] = {}; // pt_debug_adaptive_timing: device ms in evaluations, their number, host ms changing the pixel list, list changes
    } adaptive;

    // instance motion (include/ptamd.h): one record per instance of the ACTIVE dynamic state (indexed like its instance table, which is how the guide
    // pass meets a hit), and the two guide sums made from them -- (displacement.xyz, 0) and (normal then.xyz, 0), width * height float4 each, allocated at
    // the first pt_set_instance_motion / pt_write_motion_guides.  pt_frame_tick forgets the motion; pt_clear zeroes the sums and keeps it.
    struct InstanceMotion {
        DevBuf<MotionRecord> records;
        std::vector<MotionRecord> host;
        bool set = false;
        uint32_t moving = 0;
    } motion;
    PlanePair motionGuides; // [0] (displacement.xyz, 0), [1] (normal then.xyz, 0)

    // vertex motion (include/ptamd.h): a snapshot of the shading records the previous dynamic state held (numTris of them, taken on the render stream by
    // pt_set_vertex_motion: the guide pass never reads the inactive set, which the next upload may be overwriting), and three float4 rows per instance of
    // the active state -- the linear part of the world transform the instance had then.  Grow-only; pt_frame_tick forgets the motion.  While it is set
    // without an instance motion, motion.records holds identity records (A = t = 0, the current rows).
    struct VertexMotion {
        DevBuf<TriFat> fatThen;
        DevBuf<float4> rows;
        std::vector<float4> rowsHost;
        bool set = false; // forgetting the motion clears this alone: `deformed` and rebuiltMotion.set are written whenever it is set and read only while it is
        bool deformed = false; // the previous state held another version of the static arrays: k_guides<2> runs
    } vertexMotion;

    // rebuilt motion (include/ptamd.h): the second way to fill fatThen, for a state whose tree was rebuilt -- the caller's map (active triangle -> triangle
    // of the previous state) on the device, where k_gather_then reads it, and the pinned copy the asynchronous upload reads from (its event: created at the
    // first call, recorded on the render stream).  Grow-only.  Set: the vertex motion above (set, deformed) came from pt_set_rebuilt_motion.
    struct RebuiltMotion {
        DevBuf<uint32_t> map;
        Staging stage;
        bool set = false;
        uint32_t followed = 0;
    } rebuiltMotion;

    double msLastRender = 0, msIntersect = 0, msShade = 0, msShadow = 0, msGen = 0, msPacket = 0;
};

namespace {

int fail(pt_ctx* ctx, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->error = buf;
    else
        g_createError = buf;
    return code;
}

#define HIPCHK(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t _e = (call);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(ctx, PT_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// The bodies below build std::vectors and call std::function; nothing may escape across the C ABI, so every entry
// point that can allocate runs inside this guard and reports a failure like any other (the host library's capi.cpp
// does the same).
template <typename F>
int guarded(pt_ctx* c, const char* what, F&& body)
{
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(c, PT_ERR_UNSUPPORTED, "%s: out of host memory", what);
    } catch (const std::exception& e) {
        return fail(c, PT_ERR_INVALID, "%s: %s", what, e.what());
    } catch (...) {
        return fail(c, PT_ERR_INVALID, "%s: unknown exception", what);
    }
}

inline AccumView accumView(const pt_ctx* c) { return { c->accum, c->accumPlanes.p, c->pixelOrdinal.p, c->planes - 1u }; }
inline uint32_t maxBounces(const pt_ctx* c) { return c->cfg.max_bounces ? c->cfg.max_bounces : 4u; }
inline bool parityMode(const pt_ctx* c) { return c->cfg.rng_mode == PT_RNG_LFSR113_PARITY; }
// anything but the integrator the reference compiles in (neeIsShading, uniform light choice) runs the general shading kernel
inline bool generalShading(const pt_ctx* c) { return (c->cfg.flags & (PT_FLAG_INTEGRATOR_MIS | PT_FLAG_COMPARE_SHADING | PT_FLAG_SOLID_ANGLE_LIGHTS)) != 0u; }

void refreshSceneView(pt_ctx* c)
{
    SceneDev& s = c->scene; // (s.nodes stays null: no kernel walks pair nodes)
    const pt_ctx::DynamicSet& d = c->dyn[c->active];
    s.wide = d.wide.p;
    s.tris = d.tris.p;
    s.triFat = d.fat.p;
    s.materials = c->st->materials.p;
    s.instances = d.instances.p;
    s.lights = d.lights.p;
    s.numLights = d.numLights;
    s.rootRef = d.rootRef;
    s.firstWorldNode = d.firstWorldNode; // (of the static scene the active dynamic set was built on)
    s.instRootBase = d.numInstRoots ? d.instRootBase : 0x7FFFFFFFu; // (nothing folded: no node lies behind the world-space ones)
    s.numInstRoots = d.numInstRoots;
    s.materialTex.texels = c->texMaterial.p;
    s.sky.texels = c->texSky.p;
    s.numTriangles = c->haveDynamic ? d.numTris : c->st->host.numTris;
}

template <typename T>
int uploadVec(pt_ctx* c, DevBuf<T>& buf, const std::vector<T>& host)
{
    // grow-only: a rebuilt scene of about the old size reuses the old buffers (hipFree waits for the whole device -- a frame loop that rebuilds a
    // tree per frame, pt_upload_static_async, must not)
    if (!buf.p || buf.n < std::max<size_t>(host.size(), 1))
        HIPCHK(c, buf.alloc(std::max<size_t>(host.size() + host.size() / 8, 1)));
    if (!host.empty())
        HIPCHK(c, hipMemcpy(buf.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return PT_OK;
}

int PlanePair::zero(pt_ctx* c)
{
    for (DevBuf<float4>& b : plane)
        HIPCHK(c, b.zero(c->stream));
    return PT_OK;
}

int PlanePair::ensure(pt_ctx* c)
{
    for (DevBuf<float4>& b : plane)
        HIPCHK(c, b.ensureZeroed((size_t)c->cfg.width * c->cfg.height, c->stream));
    return PT_OK;
}

int PlanePair::read(pt_ctx* c, float* out0, float* out1)
{
    if (const int rc = ensure(c))
        return rc;
    HIPCHK(c, plane[0].copyTo(out0, c->stream));
    HIPCHK(c, plane[1].read(out1, c->stream));
    return PT_OK;
}

int PlanePair::write(pt_ctx* c, const float* in0, const float* in1)
{
    if (const int rc = ensure(c))
        return rc;
    HIPCHK(c, plane[0].copyFrom(in0, c->stream));
    HIPCHK(c, plane[1].write(in1, c->stream));
    return PT_OK;
}

} // namespace
