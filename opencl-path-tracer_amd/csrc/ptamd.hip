// C-ABI implementation (include/ptamd.h) of the gfx950 ray-queue render path: context, scene
// conversion into the HBM layouts of pt_device.h, the launch schedule that replaces the reference's
// RayTracer::traceRays (src/raytracer.cpp:289-430), and the kernel-granular test hooks.
#include "../../include/ptamd.h"
#include "pt_shade.h"
#include "pt_trace.h"
#include "pt_packet.h"
#include "pt_packet_multi.h"
#include "pt_bake.h"
#include "pt_team.h"
#include "pt_denoise.h"
#include "pt_temporal.h"
#include "pt_adaptive.h"
#ifndef PT_PACK_WIDE
#define PT_PACK_WIDE 1
#endif
#include <algorithm>
#include <atomic>
#include <dlfcn.h>
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h> // only for the two enumerators pt_reduce_accum passes (the library itself is bound at run time, below)
#define PT_HAVE_RCCL_HEADER 1
#endif
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

using namespace ptd;

#include "pt_convert.h"
#include "pt_context.h"
#include "pt_schedule.h"

namespace {

// The conversion's options for one upload call: pt_config, the diagnostic variables of tools/README.md and EXPERIMENTS.md, the kernels' limits
// (pt_convert.cpp reads no environment).  `async`: pt_upload_static_async, whose records the device makes unless PTAMD_HOST_RECORDS is set.
static ptconv::ConvertOptions convertOptions(const pt_config& cfg, bool async = false)
{
    ptconv::ConvertOptions o;
    o.flags = cfg.flags;
    o.parity = cfg.rng_mode == PT_RNG_LFSR113_PARITY;
    if (const char* e = getenv("PTAMD_LEAF_FORMATION")) {
        unsigned cap = o.costs.cap;
        if (sscanf(e, "%u,%lf,%lf,%lf,%lf", &cap, &o.costs.inner, &o.costs.leaf0, &o.costs.tri, &o.costs.alpha) >= 1)
            o.costs.cap = std::min(cap, kMaxLeafTris);
    }
    if (const char* e = getenv("PTAMD_MAX_LEAF"))
        o.maxLeaf = std::max(1u, std::min((uint32_t)atoi(e), kMaxLeafTris));
    if (const char* e = getenv("PTAMD_BAKE_BUDGET_GB")) // diagnostics (bench.py, two_level_general: the copied scene as the yardstick of the entered one)
        o.bakeBudgetBytes = (uint64_t)std::max(0.0, atof(e) * (double)(1ull << 30));
    o.noFoldedInstances = getenv("PTAMD_NO_FOLDED_INSTANCES") != nullptr;
    if (const char* e = getenv("PTAMD_GENERAL_ROUTE"))
        o.generalRoute = atoi(e) != 0 ? 1 : 0;
    const char* seq = getenv("PTAMD_BUILD_THREADS"); // (1: everything on the calling thread, as the host library's builders read it)
    o.sequential = seq && atoi(seq) == 1;
    o.hostRecords = !async || getenv("PTAMD_HOST_RECORDS"); // (PTAMD_HOST_RECORDS=1: the records of a rebuilt scene on the host too -- A / B)
    o.timing = getenv("PTAMD_UPLOAD_TIMING") != nullptr;
    o.collapseReport = getenv("PTAMD_COLLAPSE_REPORT") != nullptr;
    o.stackMax = (uint32_t)kTraversalStackMax, o.packetStack = kPacketStack, o.foldTable = kInstFoldTable;
    return o;
}

// the caller's latest arrays where the conversion cannot find them in the host vectors: in the staging memory after a refit on the device (pt_update_geometry)
static ptconv::Latest latestOf(const StaticScene& s)
{
    if (!s.latestInStage)
        return {};
    return { (const pt_vertex*)s.stage.mem.p, (const pt_sub_bvh_node*)(s.stage.mem.p + (size_t)s.host.numVerts * sizeof(pt_vertex)) };
}

// the host's mirrors brought up to the caller's latest arrays (the host vectors take them over from the staging memory)
static void refreshHost(StaticScene& s)
{
    ptconv::refreshHostGeometry(s.host, latestOf(s));
    s.latestInStage = false;
}

// What a refit re-makes from the caller's arrays on the device, enqueued on the copy stream: with `nodes`, every packed node re-quantised from the caller's nodes
// (k_refit_nodes; pt_refit_vertices has k_refit_tree recompute the boxes instead), then the triangles' intersection and shading records (k_refit_tris).
static void launchRefit(pt_ctx* c, bool nodes)
{
    static_assert(sizeof(VertexIn) == sizeof(pt_vertex) && sizeof(SubNodeIn) == sizeof(pt_sub_bvh_node), "the refit kernels read the caller's records as they are");
    StaticScene& g = *c->st;
    if (nodes && !g.host.wide.empty()) {
        RefitNodeArgs rn {};
        rn.nodes = (const SubNodeIn*)g.dNodes.p, rn.kidBoxNode = g.dKidBoxNode.p, rn.extra = g.dExtra.p, rn.wide = g.dWide.p, rn.boxes = g.dBoxes.p;
        rn.emptyRef = g.host.emptyRef, rn.n = (uint32_t)g.host.wide.size();
        hipLaunchKernelGGL(k_refit_nodes, dim3((rn.n + 127u) / 128u), dim3(128), 0, c->copyStream, rn);
    }
    RefitArgs ra {};
    ra.verts = (const VertexIn*)g.dVerts.p, ra.tri = g.triShade.p, ra.mats = g.materials.p, ra.tris = g.dTris.p, ra.fat = g.dFat.p, ra.n = g.host.numTris;
    hipLaunchKernelGGL(k_refit_tris, dim3((ra.n + 255u) / 256u), dim3(256), 0, c->copyStream, ra);
}

// the static arrays' master copy in device memory (the two dynamic sets take theirs from it, device to device)
static int uploadStaticGeom(pt_ctx* c, const ptconv::ConvertOptions& o)
{
    StaticScene& g = *c->st;
    if (g.onDeviceTopology == g.host.topology)
        return PT_OK;
    ptconv::StageTimer tm("uploadStaticGeom", o.timing);
    // the copy stream may still be reading the old master (a set being refreshed from it)
    HIPCHK(c, hipStreamSynchronize(c->copyStream));
    tm.lap("syncCopyStream");
    if (g.host.hostGeomStale) { // refitted before the master copy ever reached the device
        refreshHost(g);
        ptconv::buildFat(g.host);
    }
    int rc;
    if (g.host.deviceMakesRecords) {
        // the topology and the caller's arrays as they are; the records on the device (what pt_update_geometry does after a refit: the same kernels from the same
        // boxes with the same routines -- a context that adopts this scene holds the bytes a fresh one makes on the host, tests/test_gpu_dynamic.py)
        const std::vector<float> extra = ptconv::extraBoxes(g.host); // (boxes of the pair nodes that cut a leaf of more than two triangles)
        const size_t nT = c->st->host.numTris;
        if ((rc = uploadVec(c, g.dWide, g.host.wide)) || (rc = uploadVec(c, g.dLeafOfs, g.host.leafOfs)) || (rc = uploadVec(c, g.dRefTri, g.host.refTri))
            || (rc = uploadVec(c, g.dVerts, c->st->host.rawVerts)) || (rc = uploadVec(c, c->st->triShade, c->st->host.hostTriShade))
            || (rc = uploadVec(c, g.dNodes, c->st->host.hostSubNodes)) || (rc = uploadVec(c, g.dKidBoxNode, g.host.kidBoxNode)) || (rc = uploadVec(c, g.dExtra, extra)))
            return rc;
        if (g.dBoxes.n < std::max<size_t>(g.host.wide.size(), 1))
            HIPCHK(c, g.dBoxes.alloc(g.host.wide.size() + g.host.wide.size() / 8 + 1));
        if (g.dTris.n < nT + 1)
            HIPCHK(c, g.dTris.alloc(nT + nT / 8 + 1));
        if (g.dFat.n < std::max<size_t>(nT, 1))
            HIPCHK(c, g.dFat.alloc(nT + nT / 8 + 1));
        tm.lap("uploads");
        HIPCHK(c, hipMemsetAsync(g.dTris.p + nT, 0, sizeof(TriIsect), c->copyStream)); // what an unused child slot refers to
        launchRefit(c, true);
        HIPCHK(c, hipGetLastError());
        tm.lap("kernels");
        g.onDeviceTopology = g.host.topology;
        return PT_OK;
    }
    std::vector<TriIsect> tris = c->st->host.hostTris;
    tris.push_back(TriIsect { make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0) }); // what an unused child slot refers to
    if ((rc = uploadVec(c, g.dWide, g.host.wide)) || (rc = uploadVec(c, g.dBoxes, g.host.boxes)) || (rc = uploadVec(c, g.dLeafOfs, g.host.leafOfs))
        || (rc = uploadVec(c, g.dRefTri, g.host.refTri)) || (rc = uploadVec(c, g.dTris, tris)) || (rc = uploadVec(c, g.dFat, g.host.fat))
        || (rc = uploadVec(c, g.dVerts, c->st->host.rawVerts)) || (rc = uploadVec(c, c->st->triShade, c->st->host.hostTriShade))
        || (rc = uploadVec(c, g.dNodes, c->st->host.hostSubNodes)) || (rc = uploadVec(c, g.dKidBoxNode, g.host.kidBoxNode)))
        return rc;
    tm.lap("uploads");
    g.onDeviceTopology = g.host.topology;
    return PT_OK;
}

// `async`: into c->st without touching the render stream or the dynamic state (pt_upload_static_async: c->st is the scene that is not current)
static int uploadStaticImpl(pt_ctx* c, const pt_vertex* verts, uint32_t nV, const pt_triangle* tris, uint32_t nT, const pt_material* mats,
    uint32_t nM, const pt_sub_bvh_node* nodes, uint32_t nN, bool async = false)
{
    if (!c)
        return PT_ERR_INVALID;
    const ptconv::ConvertOptions o = convertOptions(c->cfg, async);
    ptconv::StageTimer tm("uploadStatic", o.timing);
    std::string why;
    if (const int rc = ptconv::convertStatic(c->st->host, o, c->staticVersions, verts, nV, tris, nT, mats, nM, nodes, nN, tm, why))
        return fail(c, rc, "%s", why.c_str());
    c->st->latestInStage = false;
    c->st->have = true;
    HIPCHK(c, hipSetDevice(c->device));
    if (!async) {
        HIPCHK(c, hipStreamSynchronize(c->stream)); // renders in flight read these buffers
        c->haveStatic = true;
        c->haveDynamic = false; // top-level leaves reference sub-BVH roots: must be re-uploaded
        c->pending = -1;
        c->statPending = -1; // (a rebuilt scene that was waiting for its frame tick is dropped with the dynamic state)
    }
    // (pt_upload_static_async: the materials go last.  A blocking copy issued while a frame of the current scene holds every compute unit with its persistent
    // waves waited for most of that frame -- 0.43 ms of a 1080p frame, tools/rebuild_timing.py --1080p -- and the conversion above is host work the frame can hide)
    std::vector<Material> hMats(nM);
    static_assert(sizeof(Material) == sizeof(pt_material), "material record is copied verbatim");
    std::memcpy(hMats.data(), mats, (size_t)nM * sizeof(pt_material));
    if (const int rc = uploadVec(c, c->st->materials, hMats))
        return rc;
    tm.lap("materials");
    if (!async)
        refreshSceneView(c);
    return PT_OK;
}

// Who a packed node reports to in a bottom-up pass, and how many arrivals complete it (k_refit_tree).  Made once per topology.
static int ensureRefitTables(pt_ctx* c)
{
    StaticScene& g = *c->st;
    if (g.refitTablesFor == g.host.topology)
        return PT_OK;
    const size_t n = g.host.wide.size();
    std::vector<uint32_t> parent(n, 0xFFFFFFFFu), need(n, 1u);
    bool ok = true;
    for (size_t q = 0; q < n; q++)
        for (int k = 0; k < 4; k++) {
            const uint32_t r = g.host.wide[q].child[k];
            if (r == g.host.emptyRef || refCount(r) != 0u)
                continue;
            const uint32_t ch = refIndex(r);
            if (ch >= n || ch == q || parent[ch] != 0xFFFFFFFFu) { // (two parents: roots that share a subtree -- the bottom-up pass would complete the child once and leave one parent waiting)
                ok = false;
                continue;
            }
            parent[ch] = ((uint32_t)q << 2) | (uint32_t)k;
            need[q]++;
        }
    g.refitTablesOk = ok;
    g.refitTablesFor = g.host.topology;
    if (!ok)
        return PT_OK;
    HIPCHK(c, hipStreamSynchronize(c->copyStream)); // (an earlier refit may still be walking the old tables)
    int rc;
    if ((rc = uploadVec(c, g.dParent, parent)) || (rc = uploadVec(c, g.dNeed, need)))
        return rc;
    if (!g.dArrived.p || g.dArrived.n < std::max<size_t>(n, 1))
        HIPCHK(c, g.dArrived.alloc(std::max<size_t>(n + n / 8, 1)));
    HIPCHK(c, hipMemset(g.dArrived.p, 0, g.dArrived.n * sizeof(uint32_t)));
    return PT_OK;
}

template <typename T>
int growTo(pt_ctx* c, DevBuf<T>& buf, size_t count)
{
    if (buf.n >= std::max<size_t>(count, 1))
        return PT_OK;
    HIPCHK(c, buf.alloc(std::max<size_t>(count + count / 8, 1))); // some headroom: the number of world-space copies varies from state to state
    return PT_OK;
}

// the grid of a kernel whose workgroup is one tileW x tileH tile of the frame
dim3 tileGrid(uint32_t W, uint32_t H, uint32_t tileW, uint32_t tileH) { return dim3((W + tileW - 1) / tileW, (H + tileH - 1) / tileH); }

// pt_render_guides: the n hits of the guide pass's scratch queue into the guide sums; MOTION as k_guides knows it (pt_denoise.h)
template <int MOTION>
void launchGuides(pt_ctx* c, uint32_t n, const GuideMotionArgs& motion)
{
    hipLaunchKernelGGL(k_guides<MOTION>, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, c->scene, c->guideRayO.p, c->guideRayD.p, c->guideHit.p, c->guideHitInst.p,
        n, c->camera.thinLens, c->guides[0], c->guides[1], motion);
}

} // namespace


// =================================================================================================
extern "C" {

const char* pt_version(void) { return "ptamd 0.1 (gfx950)"; }

#ifdef PT_TRACE_STATS
// diagnostic builds only: read and clear the traversal-loop counters
int pt_debug_trace_stats(unsigned long long* out, unsigned int n) // n <= 64 counters (pt_walk.h, g_traceStats)
{
    n = std::min(n, 64u);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_traceStats), sizeof(unsigned long long) * n) != hipSuccess)
        return -1;
    unsigned long long zero[64] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_traceStats), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif

// Diagnostic (bench.py): GB/s (read + written) of a float4 grid-stride device copy of `bytes` bytes, the best of `repeat` timed runs after a warm-up.
int pt_debug_copy_bandwidth(pt_ctx* c, size_t bytes, uint32_t repeat, float* gbps_out)
{
    return guarded(c, "pt_debug_copy_bandwidth", [&]() -> int {
    if (!c || !gbps_out || bytes < (1u << 20))
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = bytes / sizeof(float4);
    DevBuf<float4> src, dst;
    HIPCHK(c, src.alloc(n));
    HIPCHK(c, dst.alloc(n));
    HIPCHK(c, hipMemsetAsync(src.p, 0x3c, n * sizeof(float4), c->stream));
    Event e0, e1;
    HIPCHK(c, e0.create(true));
    HIPCHK(c, e1.create(true));
    const uint32_t blocks = (uint32_t)c->numCUs * 4u; // 1 024 workgroups of 256 on an MI355X (pt_bake.h: the best of the shapes tried)
    float best = 0.f;
    for (uint32_t r = 0; r <= std::max(repeat, 1u); r++) { // (run 0: warm-up)
        (void)hipEventRecord(e0, c->stream);
        hipLaunchKernelGGL(k_copy_probe, dim3(blocks), dim3(256), 0, c->stream, src.p, dst.p, n);
        (void)hipEventRecord(e1, c->stream);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (r > 0 && ms > 0.f)
            best = std::max(best, (float)(2.0 * (double)n * sizeof(float4) / (ms * 1e-3) / 1e9));
    }
    *gbps_out = best;
    return PT_OK;
    });
}

// Test hook (tests/test_gpu_fastmath.py): k_math_probe over n pairs; `out` receives ten planes of n floats (pt_shade.h).
int pt_debug_math_probe(pt_ctx* c, const float* a, const float* b, uint32_t n, float* out)
{
    return guarded(c, "pt_debug_math_probe", [&]() -> int {
    if (!c || !a || !b || !out || n == 0)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> dA, dB, dOut;
    HIPCHK(c, dA.alloc(n));
    HIPCHK(c, dB.alloc(n));
    HIPCHK(c, dOut.alloc((size_t)n * 10));
    HIPCHK(c, hipMemcpy(dA.p, a, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dB.p, b, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_math_probe, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, dA.p, dB.p, n, dOut.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, dOut.p, (size_t)n * 10 * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
    });
}

// Test hook (tests/test_gpu_prng.py): k_rng_probe over n entries of eight words; `out` receives twenty words per entry (pt_shade.h).
int pt_debug_rng_probe(pt_ctx* c, const uint32_t* in, uint32_t n, uint32_t* out)
{
    return guarded(c, "pt_debug_rng_probe", [&]() -> int {
    if (!c || !in || !out || n == 0 || n > (1u << 24))
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<uint32_t> dIn, dOut;
    HIPCHK(c, dIn.alloc((size_t)n * 8));
    HIPCHK(c, dOut.alloc((size_t)n * 20));
    HIPCHK(c, hipMemcpy(dIn.p, in, (size_t)n * 8 * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_rng_probe, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, dIn.p, n, dOut.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, dOut.p, (size_t)n * 20 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return PT_OK;
    });
}

// Test hook, no device needed (tests/test_gpu_lifetime.py): what the owning types of pt_context.h hold alive in this process, all contexts and hooks together --
// device allocations, pinned allocations, events, streams the library created.
int pt_debug_live_resources(uint32_t out[4])
{
    if (!out)
        return PT_ERR_INVALID;
    for (int k = 0; k < 4; k++)
        out[k] = g_live[k].load();
    return PT_OK;
}

const char* pt_last_error(const pt_ctx* ctx) { return ctx ? ctx->error.c_str() : g_createError.c_str(); }

// Test hook, no device needed: the host side of quantiseWideNode (pt_hostdev.h) -- up to four child boxes (lo / hi: 4 x 3 floats; empty[k] != 0:
// unused slot) into the 64-byte node the traversal kernels read.  tests/test_abi_and_layout.py checks the planes it makes against the
// expression the kernels evaluate (origin + 2^exp * q): every child box must lie inside its quantised box.
int pt_debug_quantise_node(const float* lo12, const float* hi12, const uint32_t* refs4, const uint8_t* empty4, uint32_t emptyRef, void* out64)
{
    if (!lo12 || !hi12 || !refs4 || !empty4 || !out64)
        return PT_ERR_INVALID;
    float lo[4][3], hi[4][3];
    bool empty[4];
    for (int k = 0; k < 4; k++) {
        empty[k] = empty4[k] != 0;
        for (int a = 0; a < 3; a++)
            lo[k][a] = lo12[k * 3 + a], hi[k][a] = hi12[k * 3 + a];
    }
    WideNode w;
    quantiseWideNode(lo, hi, refs4, empty, emptyRef, &w);
    std::memcpy(out64, &w, sizeof(w));
    return PT_OK;
}

// Test hook, no device needed: what pt_upload_static (the records made on the host) and, given a top level, pt_upload_dynamic make of these arrays, as one line
// -- FNV-1a hashes of every array of the static part | of every array of the dynamic state, and the figures of its instance route (tests/test_convert.py).
int pt_debug_convert(const pt_config* cfg, const pt_vertex* verts, uint32_t nV, const pt_triangle* tris, uint32_t nT, const pt_material* mats, uint32_t nM,
    const pt_sub_bvh_node* nodes, uint32_t nN, const pt_emissive_triangle* lights, uint32_t nL, const pt_top_bvh_node* topNodes, uint32_t nTop, uint32_t topRoot,
    char* line, size_t lineBytes)
{
    return guarded(nullptr, "pt_debug_convert", [&]() -> int {
        if (!cfg || !line)
            return fail(nullptr, PT_ERR_INVALID, "pt_debug_convert: null argument");
        const ptconv::ConvertOptions o = convertOptions(*cfg);
        ptconv::StaticHost s;
        ptconv::DynamicHost d;
        uint64_t versions = 0;
        std::string why;
        ptconv::StageTimer tm("convert", o.timing);
        int rc = ptconv::convertStatic(s, o, versions, verts, nV, tris, nT, mats, nM, nodes, nN, tm, why);
        if (rc == PT_OK && nTop)
            rc = ptconv::convertDynamic(s, o, versions, {}, lights, nL, topNodes, nTop, topRoot, d, why);
        if (rc)
            return fail(nullptr, rc, "%s", why.c_str());
        auto fnv = [](const void* p, size_t n) {
            uint64_t h = 1469598103934665603ull;
            for (size_t i = 0; i < n; i++)
                h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
            return (unsigned long long)h;
        };
        char buf[1024];
        int n = snprintf(buf, sizeof buf, "wide %zu %016llx boxes %016llx leafOfs %016llx refTri %zu %016llx kidSrc %016llx kidBoxNode %016llx stackNeed %016llx fat %016llx pairs %zu %016llx",
            s.wide.size(), fnv(s.wide.data(), s.wide.size() * sizeof(WideNode)), fnv(s.boxes.data(), s.boxes.size() * sizeof(s.boxes[0])),
            fnv(s.leafOfs.data(), s.leafOfs.size() * 4), s.refTri.size(), fnv(s.refTri.data(), s.refTri.size() * 4), fnv(s.kidSrc.data(), s.kidSrc.size() * 4),
            fnv(s.kidBoxNode.data(), s.kidBoxNode.size() * 4), fnv(s.stackNeed.data(), s.stackNeed.size() * 4), fnv(s.fat.data(), s.fat.size() * sizeof(s.fat[0])),
            s.hostBottomNodes.size(), fnv(s.hostBottomNodes.data(), s.hostBottomNodes.size() * sizeof(PairNode)));
        if (nTop)
            n += snprintf(buf + n, sizeof buf - n, " | topWide %zu %016llx instances %zu %016llx lights %zu %016llx jobs %zu %016llx instanceTopNode %016llx instRoots %zu %016llx "
                "instRootSrc %016llx instFold %zu %016llx hasInstances %d enteredInstances %u enteredGeneral %u foldedInstances %u generalRoute %d bakedNodes %u bakedTris %u "
                "stackNeed %u rootRef %08x rootRefFolded %08x",
                d.topWide.size(), fnv(d.topWide.data(), d.topWide.size() * sizeof(WideNode)), d.instances.size(), fnv(d.instances.data(), d.instances.size() * sizeof(Instance)),
                d.lights.size(), fnv(d.lights.data(), d.lights.size() * sizeof(Light)), d.jobs.size(), fnv(d.jobs.data(), d.jobs.size() * sizeof(BakeJob)),
                fnv(d.instanceTopNode.data(), d.instanceTopNode.size() * 4), d.instRoots.size(), fnv(d.instRoots.data(), d.instRoots.size() * sizeof(WideNode)),
                fnv(d.instRootSrc.data(), d.instRootSrc.size() * 4), d.instFold.size(), fnv(d.instFold.data(), d.instFold.size() * sizeof(float4)), (int)d.hasInstances,
                d.enteredInstances, d.enteredGeneral, d.foldedInstances, (int)d.generalRoute, d.bakedNodes, d.bakedTris, d.stackNeed, d.rootRef, d.rootRefFolded);
        if ((size_t)n >= lineBytes)
            return fail(nullptr, PT_ERR_INVALID, "pt_debug_convert: the line takes %d bytes", n + 1);
        std::memcpy(line, buf, (size_t)n + 1);
        return PT_OK;
    });
}

int pt_create(const pt_config* cfg, pt_ctx** out)
{
    return guarded(nullptr, "pt_create", [&]() -> int {
    if (!cfg || !out)
        return fail(nullptr, PT_ERR_INVALID, "pt_create: null argument");
    if (cfg->width == 0 || cfg->height == 0 || (uint64_t)cfg->width * cfg->height > 0x7FFFFFFFull)
        return fail(nullptr, PT_ERR_INVALID, "pt_create: bad image size %ux%u", cfg->width, cfg->height);
    if (cfg->max_bounces > (uint32_t)kMaxPasses - 1)
        return fail(nullptr, PT_ERR_INVALID, "pt_create: max_bounces > %d", kMaxPasses - 1);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail(nullptr, PT_ERR_HIP, "pt_create: no HIP device (%s) -- this library has no CPU fallback", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= count)
        return fail(nullptr, PT_ERR_INVALID, "pt_create: device %d out of range (%d devices)", cfg->device, count);
    pt_ctx* c = new pt_ctx();
    c->cfg = *cfg;
    c->packetUse = (cfg->flags & PT_FLAG_NO_PACKETS) ? 0u : kPacketUseDefault;
    if (cfg->flags & PT_FLAG_PACKET_INTERSECT)
        c->packetUse |= 4u;
    if (const char* hs = getenv("PTAMD_SHADE_HEAD_SHIFT"))
        c->shadeHeadShift = (uint32_t)std::max(0, atoi(hs));
    if (const char* pk = getenv("PTAMD_PACKET")) // diagnostics: which launches may use k_trace_packet (bit 0 primary, 1 shadow, 2 pt_intersect)
        if (!(cfg->flags & PT_FLAG_NO_PACKETS))
            c->packetUse = (uint32_t)atoi(pk) | (c->packetUse & 4u);
    c->device = cfg->device;
    auto bail = [&](hipError_t err, const char* what) {
        int rc = fail(nullptr, PT_ERR_HIP, "pt_create: %s: %s", what, hipGetErrorString(err));
        delete c;
        return rc;
    };
    if ((e = hipSetDevice(c->device)) != hipSuccess)
        return bail(e, "hipSetDevice");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, c->device)) != hipSuccess)
        return bail(e, "hipGetDeviceProperties");
    c->numCUs = prop.multiProcessorCount;
    if ((e = c->stream.create()) != hipSuccess)
        return bail(e, "hipStreamCreate");
    if ((e = c->copyStream.create()) != hipSuccess)
        return bail(e, "hipStreamCreate (copy stream)");
    if ((e = c->evStart.create(true)) != hipSuccess || (e = c->evStop.create(true)) != hipSuccess || (e = c->evDenoise[0].create(true)) != hipSuccess
        || (e = c->evDenoise[1].create(true)) != hipSuccess) // (the filter's two with the context: a pt_denoise that refuses leaves nothing behind)
        return bail(e, "hipEventCreate");
    if ((e = c->sideStream.create()) != hipSuccess || (e = c->sideStream2.create()) != hipSuccess)
        return bail(e, "hipStreamCreate (side stream)");
    for (int k = 0; k < kMaxPasses; k++)
        if ((e = c->evShaded[k].create()) != hipSuccess || (e = c->evShadowed[k].create()) != hipSuccess)
            return bail(e, "hipEventCreate");
    for (auto& d : c->dyn)
        if ((e = d.uploaded.create()) != hipSuccess || (e = d.lastUse.create()) != hipSuccess || (e = d.stage.read.create()) != hipSuccess)
            return bail(e, "hipEventCreate");
    for (StaticScene& s : c->stat)
        if ((e = s.stage.read.create()) != hipSuccess)
            return bail(e, "hipEventCreate");
    if ((e = c->passCountsPinned.alloc(sizeof(c->passCountsHint) / sizeof(uint32_t))) != hipSuccess || (e = c->passCountsCopied.create()) != hipSuccess)
        return bail(e, "pinned counters");
    std::memset(c->passCountsPinned.p, 0, sizeof(c->passCountsHint));
    if ((e = c->overflowPinned.alloc(1)) != hipSuccess)
        return bail(e, "pinned overflow word");
    *c->overflowPinned.p = 0u;
    if ((e = c->totals.alloc(1)) != hipSuccess || (e = hipMemsetAsync(c->totals.p, 0, sizeof(Totals), c->stream)) != hipSuccess)
        return bail(e, "alloc totals");
    if ((e = c->accumOwn.alloc((size_t)cfg->width * cfg->height)) != hipSuccess
        || (e = hipMemsetAsync(c->accumOwn.p, 0, (size_t)cfg->width * cfg->height * sizeof(float4), c->stream)) != hipSuccess)
        return bail(e, "alloc accumulator");
    c->accum = c->accumOwn.p;
    c->numOwned = cfg->width * cfg->height;
    c->identityPixels = true;
    *out = c;
    int rc = pt_set_tiles(c, nullptr, 0);
    if (rc) {
        g_createError = c->error;
        pt_destroy(c);
        *out = nullptr;
        return rc;
    }
    return PT_OK;
    });
}

// (~pt_ctx, pt_context.h: waits for the context's streams, then every member frees what it owns; null: nothing)
void pt_destroy(pt_ctx* c) { delete c; }

int pt_set_stream(pt_ctx* c, void* hip_stream)
{
    if (!c)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hip_stream)
        c->stream.adopt((hipStream_t)hip_stream); // (the caller's: never destroyed here)
    else
        HIPCHK(c, c->stream.create());
    return PT_OK;
}

// A REBUILT scene per frame as a frame-loop citizen (the other branch of MeshSequence::buildBvh, reference src/model/mesh_sequence.cpp:89-96, whose
// result transferDynamicData uploads every tick, src/raytracer.cpp:510-568): the same arrays as pt_upload_static, converted into the context's
// SECOND static scene and copied to the device without touching the render stream -- the frames enqueued so far, and any enqueued before the flip,
// keep rendering the old trees.  Follow with pt_upload_dynamic_async (lights and top level OF THE NEW SCENE: its leaves name the new sub-BVH roots)
// and pt_frame_tick, which adopts both.  pt_update_geometry / pt_refit_vertices keep addressing the current scene until then.
int pt_upload_static_async(pt_ctx* c, const pt_vertex* verts, uint32_t nV, const pt_triangle* tris, uint32_t nT, const pt_material* mats,
    uint32_t nM, const pt_sub_bvh_node* nodes, uint32_t nN)
{
    return guarded(c, "pt_upload_static_async", [&]() -> int {
        if (!c)
            return PT_ERR_INVALID;
        if (!c->haveStatic || !c->haveDynamic) // nothing is rendering yet: the plain upload does
            return uploadStaticImpl(c, verts, nV, tris, nT, mats, nM, nodes, nN);
        HIPCHK(c, hipSetDevice(c->device));
        // the other scene's master copies may still be read by copies the copy stream has queued (a dynamic set refreshing itself from them,
        // world-space copy kernels): that stream only -- the render stream is never waited for
        HIPCHK(c, hipStreamSynchronize(c->copyStream));
        const int target = 1 - c->statCur;
        if (c->pending >= 0 && c->dyn[c->pending].staticIndex == target)
            c->pending = -1; // a dynamic state built on the scene that is about to be replaced: never adopted
        c->statPending = -1;
        StaticScene* const cur = c->st;
        c->st = &c->stat[target];
        int rc = uploadStaticImpl(c, verts, nV, tris, nT, mats, nM, nodes, nN, true);
        if (rc == PT_OK)
            rc = uploadStaticGeom(c, convertOptions(c->cfg));
        if (rc != PT_OK)
            c->st->have = false;
        c->st = cur;
        if (rc == PT_OK)
            c->statPending = target;
        return rc;
    });
}

int pt_upload_static(pt_ctx* c, const pt_vertex* verts, uint32_t nV, const pt_triangle* tris, uint32_t nT, const pt_material* mats,
    uint32_t nM, const pt_sub_bvh_node* nodes, uint32_t nN)
{
    return guarded(c, "pt_upload_static", [&]() -> int { return uploadStaticImpl(c, verts, nV, tris, nT, mats, nM, nodes, nN); });
}

// New vertex data and refitted boxes for an UNCHANGED topology (what refitBVH, src/bvh/refit_bvh.cpp:6-34, leaves of a deforming
// mesh; the reference rewrites the dynamic tail of its vertex and sub-BVH buffers every tick, src/raytracer.cpp:510-568).  The
// arrays are the caller's whole vertex and sub-BVH arrays again; triangles, materials and node links must be the ones uploaded.
// Takes effect with the next pt_upload_dynamic(_async) + pt_frame_tick; renders in flight are not disturbed.
//
// A refit cannot change what the conversion of pt_upload_static decided -- which descendants of a binary node became the children of
// its 4-wide node (the collapse's split choices), the breadth-first packing, the leaves' triangle references, the stack bound -- so all
// of that is kept (ptconv::StaticHost::kidSrc / kidBoxNode / kidEmpty / leafOfs / refTri / stackNeed) and only what moves is re-made, ON THE
// DEVICE: the caller's vertex and node arrays travel as they are through pinned staging on the copy stream (an event of its own guards
// the staging memory: no stream is synchronised), k_refit_nodes gathers every packed node's child boxes from the caller's nodes and
// re-quantises it (quantiseWideNode: the host's routine), k_refit_tris re-makes the triangles' intersection and shading records.  The
// host's half is the topology check and two copies into pinned memory; its own mirrors of the converted arrays go stale and are
// refreshed from the staging memory only if the whole conversion ever runs again.  (Round 3 re-ran the whole conversion here --
// collapse, packing, 128 bytes of shading record per triangle on one host thread -- and re-uploaded everything behind a
// synchronisation of the copy stream.)
int pt_update_geometry(pt_ctx* c, const pt_vertex* verts, uint32_t nV, const pt_sub_bvh_node* nodes, uint32_t nN)
{
    return guarded(c, "pt_update_geometry", [&]() -> int {
        if (!c)
            return PT_ERR_INVALID;
        if (!c->haveStatic)
            return fail(c, PT_ERR_STATE, "pt_update_geometry: call pt_upload_static first");
        if (c->statPending >= 0) // (the caller's offsets and counts are those of the rebuilt scene already; the scene that still renders is the old one)
            return fail(c, PT_ERR_STATE, "pt_update_geometry: a rebuilt scene (pt_upload_static_async) is waiting for pt_frame_tick: refit after the tick");
        if (!verts || !nodes || nV != c->st->host.numVerts || nN != c->st->host.numRefNodes)
            return fail(c, PT_ERR_INVALID, "pt_update_geometry: the vertex and node counts must be the uploaded ones (%u, %u)", c->st->host.numVerts, c->st->host.numRefNodes);
        for (uint32_t i = 0; i < nN; i++)
            if (nodes[i].leftChildOrFirstTriangle != c->st->host.hostSubNodes[i].leftChildOrFirstTriangle || nodes[i].triangleCount != c->st->host.hostSubNodes[i].triangleCount)
                return fail(c, PT_ERR_INVALID, "pt_update_geometry: node %u changed its links: a refit keeps the topology (use pt_upload_static for a rebuilt tree)", i);
        HIPCHK(c, hipSetDevice(c->device));
        StaticScene& g = *c->st;
        if (g.onDeviceTopology != g.host.topology) {
            // nothing of the old geometry is on the device yet: everything on the host, the first upload takes it from the host arrays
            refreshHost(g); // (an earlier device-side refit may have left the host mirrors behind)
            ptconv::refitPairBoxes(g.host, verts, nodes, false);
            ptconv::refitWideOnHost(g.host);
            c->st->host.rawVerts.assign(verts, verts + nV);
            c->st->host.hostSubNodes.assign(nodes, nodes + nN);
            g.latestInStage = false;
            c->st->host.hostGeomStale = true; // hostTris / hostVerts / sg.host.fat follow at the upload
            g.host.version = ++c->staticVersions;
            return PT_OK;
        }
        // ---- the device's master copy: the caller's vertices and nodes AS THEY ARE through pinned staging on the copy stream; the packed nodes
        // re-quantised (k_refit_nodes) and the triangle records re-made (k_refit_tris) there.  The staging memory doubles as the host's copy of the
        // caller's latest arrays (refreshHostGeometry reads it if the whole conversion ever runs again).
        ptconv::refitPairBoxes(g.host, verts, nodes, true); // the boxes of the pair nodes that split an oversized leaf (rare): recomputed here
        const std::vector<float> extra = ptconv::extraBoxes(g.host);
        const size_t bytesV = (size_t)nV * sizeof(pt_vertex), bytesN = (size_t)nN * sizeof(pt_sub_bvh_node), bytesE = extra.size() * sizeof(float);
        const size_t total = bytesV + bytesN + bytesE;
        HIPCHK(c, g.stage.wait()); // the previous refit's copies out of the staging memory
        if (g.stage.bytes < total && g.latestInStage)
            refreshHost(g); // (the staging memory holds the host's only copy of the latest arrays: take it over before it goes)
        HIPCHK(c, g.stage.reserve(total, total + total / 8));
        unsigned char* st = g.stage.mem.p;
        std::memcpy(st, verts, bytesV);
        std::memcpy(st + bytesV, nodes, bytesN);
        g.latestInStage = true;
        c->st->host.hostGeomStale = true;
        g.host.version = ++c->staticVersions;
        HIPCHK(c, hipMemcpyAsync(g.dVerts.p, st, bytesV, hipMemcpyHostToDevice, c->copyStream));
        HIPCHK(c, hipMemcpyAsync(g.dNodes.p, st + bytesV, bytesN, hipMemcpyHostToDevice, c->copyStream));
        if (bytesE) {
            std::memcpy(st + bytesV + bytesN, extra.data(), bytesE);
            if (g.dExtra.n < extra.size())
                HIPCHK(c, g.dExtra.alloc(extra.size()));
            HIPCHK(c, hipMemcpyAsync(g.dExtra.p, st + bytesV + bytesN, bytesE, hipMemcpyHostToDevice, c->copyStream));
        }
        HIPCHK(c, g.stage.recordRead(c->copyStream));
        launchRefit(c, true);
        HIPCHK(c, hipGetLastError());
        return PT_OK;
    });
}

// A deformed frame of the same topology, refitted ON THE DEVICE: the caller hands over the vertices of the mesh that moved -- `nV` records that
// replace [firstVertex, firstVertex + nV) of the vertex array pt_upload_static took -- and nothing else.  The device re-makes the triangles'
// intersection and shading records (k_refit_tris) and recomputes every box of its packed trees bottom-up from the triangles (k_refit_tree:
// what refitBVH does on the host in the reference, src/bvh/refit_bvh.cpp:6-34, and what pt_update_geometry expects the caller to have done),
// on the copy stream, nothing synchronised.  Takes effect with the next pt_upload_dynamic(_async) + pt_frame_tick, like pt_update_geometry.
// The host's share of a tick is one copy of the moved vertices into pinned memory.
int pt_refit_vertices(pt_ctx* c, uint32_t firstVertex, const pt_vertex* verts, uint32_t nV)
{
    return guarded(c, "pt_refit_vertices", [&]() -> int {
        if (!c)
            return PT_ERR_INVALID;
        if (!c->haveStatic)
            return fail(c, PT_ERR_STATE, "pt_refit_vertices: call pt_upload_static first");
        if (c->statPending >= 0) // (a refit between a rebuild and its tick addressed the OLD scene with the NEW scene's offsets)
            return fail(c, PT_ERR_STATE, "pt_refit_vertices: a rebuilt scene (pt_upload_static_async) is waiting for pt_frame_tick: refit after the tick");
        if (!verts || nV == 0 || (uint64_t)firstVertex + nV > c->st->host.numVerts)
            return fail(c, PT_ERR_INVALID, "pt_refit_vertices: [%u, %u + %u) is not a range of the %u uploaded vertices", firstVertex, firstVertex, nV, c->st->host.numVerts);
        HIPCHK(c, hipSetDevice(c->device));
        StaticScene& g = *c->st;
        int rc;
        if ((rc = uploadStaticGeom(c, convertOptions(c->cfg))) || (rc = ensureRefitTables(c))) // (the master copy reaches the device with the first dynamic upload at the latest)
            return rc;
        if (!g.refitTablesOk)
            return fail(c, PT_ERR_UNSUPPORTED, "pt_refit_vertices: two roots of the sub-BVH array share a subtree: refit on the host and use pt_update_geometry");
        // the host's copy of the caller's arrays: rawVerts takes the new vertices; the node boxes go stale (nobody refits them here) and are
        // recomputed from the vertices only if the whole conversion ever runs again (refreshHostGeometry)
        HIPCHK(c, g.stage.wait()); // the previous refit's copies out of the staging memory, which is read and then rewritten below
        if (g.latestInStage) { // an earlier pt_update_geometry left the latest arrays in the staging memory: take them over first
            const ptconv::Latest l = latestOf(g);
            g.host.rawVerts.assign(l.verts, l.verts + g.host.numVerts);
            g.host.hostSubNodes.assign(l.nodes, l.nodes + g.host.numRefNodes);
            g.latestInStage = false;
        }
        std::memcpy(c->st->host.rawVerts.data() + firstVertex, verts, (size_t)nV * sizeof(pt_vertex));
        c->st->host.hostNodeBoxesStale = true;
        c->st->host.hostGeomStale = true;
        const size_t bytesV = (size_t)nV * sizeof(pt_vertex);
        HIPCHK(c, g.stage.reserve(bytesV, bytesV + bytesV / 8));
        std::memcpy(g.stage.mem.p, verts, bytesV);
        g.host.version = ++c->staticVersions;
        HIPCHK(c, hipMemcpyAsync(g.dVerts.p + firstVertex, g.stage.mem.p, bytesV, hipMemcpyHostToDevice, c->copyStream));
        HIPCHK(c, g.stage.recordRead(c->copyStream));
        if (!g.host.wide.empty()) {
            RefitTreeArgs rt {};
            rt.verts = (const VertexIn*)g.dVerts.p, rt.tri = c->st->triShade.p, rt.wide = g.dWide.p, rt.boxes = g.dBoxes.p;
            rt.parent = g.dParent.p, rt.need = g.dNeed.p, rt.arrived = g.dArrived.p, rt.emptyRef = g.host.emptyRef, rt.n = (uint32_t)g.host.wide.size();
            hipLaunchKernelGGL(k_refit_tree, dim3((rt.n + 127u) / 128u), dim3(128), 0, c->copyStream, rt);
        }
        launchRefit(c, false);
        HIPCHK(c, hipGetLastError());
        return PT_OK;
    });
}

} // extern "C"


extern "C" {

// Convert the next dynamic state on the host -- the top level, the instance table, the lights: the trees below are static -- and
// start putting it into the INACTIVE set on the copy stream (a few KB of copies and, where instances are copied to world space, two
// kernels); returns without waiting for the device.  Renders already enqueued (and any enqueued before the next pt_frame_tick)
// keep using the active set.
int pt_upload_dynamic_async(pt_ctx* c, const pt_emissive_triangle* lights, uint32_t nL, const pt_top_bvh_node* topNodes, uint32_t nTop, uint32_t topRoot)
{
    return guarded(c, "pt_upload_dynamic_async", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    if (!c->haveStatic)
        return fail(c, PT_ERR_STATE, "pt_upload_dynamic: call pt_upload_static first");
    HIPCHK(c, hipSetDevice(c->device));
    // a rebuilt scene is waiting (pt_upload_static_async): this state is built on IT -- its top-level leaves name the new sub-BVH roots
    struct UseScene {
        pt_ctx* c;
        StaticScene* saved;
        ~UseScene() { c->st = saved; }
    } useScene { c, c->st };
    if (c->statPending >= 0)
        c->st = &c->stat[c->statPending];
    const ptconv::ConvertOptions o = convertOptions(c->cfg);
    ptconv::StageTimer tm("uploadDynamicAsync", o.timing);
    ptconv::DynamicHost h;
    std::string why;
    int rc = ptconv::convertDynamic(c->st->host, o, c->staticVersions, latestOf(*c->st), lights, nL, topNodes, nTop, topRoot, h, why);
    if (!c->st->host.hostGeomStale) // (a conversion of the static part ran again and took the latest arrays over)
        c->st->latestInStage = false;
    tm.lap("convertDynamic");
    if (rc)
        return fail(c, rc, "%s", why.c_str());
    if ((rc = uploadStaticGeom(c, o)))
        return rc;
    tm.lap("uploadStaticGeom");
    StaticScene& sg = *c->st;
    const int target = c->haveDynamic ? 1 - c->active : c->active; // nothing active yet: fill the active set itself
    pt_ctx::DynamicSet& d = c->dyn[target];
    // the copies may not start before the renders that still read this set are done (it was the active set until the last tick),
    // nor before an earlier, never-adopted upload into it has finished (same stream: ordered)
    if (d.used)
        HIPCHK(c, hipStreamWaitEvent(c->copyStream, d.lastUse, 0));
    const size_t staticNodes = sg.host.wide.size(), staticTris = (size_t)c->st->host.numTris + 1;
    // (+ 1: the SMALL traversal instantiations fetch 96 bytes from wherever a lane stands -- 32 beyond a node, 48 beyond a one-triangle leaf)
    const size_t needWide = staticNodes + h.topSlots + h.bakedNodes + h.instRoots.size() + 1, needTris = staticTris + h.bakedTris + 1;
    // the traversal kernels address nodes and triangle records by base + 32-bit byte offset (fetchTri, pt_walk.h; the node fetches of pt_trace.h and pt_team.h)
    uint64_t offsetLimit = 0xFFFFFFFFull;
    if (const char* e = getenv("PTAMD_OFFSET_LIMIT")) // (tests: the refusal below without a 4 GB scene)
        offsetLimit = std::min<uint64_t>(offsetLimit, strtoull(e, nullptr, 10));
    if (needWide * sizeof(WideNode) > offsetLimit || needTris * sizeof(TriIsect) > offsetLimit)
        return fail(c, PT_ERR_UNSUPPORTED, "scene of %zu packed nodes and %zu triangle records (world-space copies included): more than 4 GB of either; enter the instances instead (PT_FLAG_NO_BAKED_INSTANCES)",
            needWide, needTris);
    const size_t bytes[7] = { h.topWide.size() * sizeof(WideNode), h.instances.size() * sizeof(Instance), h.lights.size() * sizeof(Light),
        h.jobs.size() * sizeof(BakeJob), h.instRoots.size() * sizeof(WideNode), h.instFold.size() * sizeof(float4), h.instRootSrc.size() * sizeof(uint32_t) };
    const size_t total = bytes[0] + bytes[1] + bytes[2] + bytes[3] + bytes[4] + bytes[5] + bytes[6];
    if (d.wide.n < needWide || d.tris.n < needTris || d.fat.n < sg.host.fat.size() || d.instances.n < std::max<size_t>(h.instances.size(), 1)
        || d.lights.n < std::max<size_t>(h.lights.size(), 1) || d.jobs.n < std::max<size_t>(h.jobs.size(), 1) || d.instFold.n < std::max<size_t>(h.instFold.size(), 1)
        || d.instRootSrc.n < std::max<size_t>(h.instRootSrc.size(), 1) || d.stage.bytes < std::max<size_t>(total, 1)) {
        // growing frees device memory, which the runtime only does once nothing uses it: wait for both streams (rare: the first
        // uploads, or a state with more world-space copies than any before)
        HIPCHK(c, hipStreamSynchronize(c->copyStream));
        if (d.used)
            HIPCHK(c, hipEventSynchronize(d.lastUse));
        const bool regrown = d.wide.n < needWide || d.tris.n < needTris || d.fat.n < sg.host.fat.size();
        if ((rc = growTo(c, d.wide, needWide)) || (rc = growTo(c, d.tris, needTris)) || (rc = growTo(c, d.fat, sg.host.fat.size()))
            || (rc = growTo(c, d.instances, h.instances.size())) || (rc = growTo(c, d.lights, h.lights.size())) || (rc = growTo(c, d.jobs, h.jobs.size()))
            || (rc = growTo(c, d.instFold, h.instFold.size())) || (rc = growTo(c, d.instRootSrc, h.instRootSrc.size())))
            return rc;
        if (regrown)
            d.staticVersion = 0; // fresh buffers: the static arrays have to be put in again
        HIPCHK(c, d.stage.reserve(std::max<size_t>(total, 1), total + total / 8 + 4096)); // (new staging memory has no copies in flight)
    }
    HIPCHK(c, d.stage.wait()); // the staging memory of this set is about to be rewritten: its last copies (two ticks ago) must have been read
    tm.lap("grow");
    if (d.staticVersion != sg.host.version) { // device to device, from the master copy
        if (staticNodes)
            HIPCHK(c, hipMemcpyAsync(d.wide.p, sg.dWide.p, staticNodes * sizeof(WideNode), hipMemcpyDeviceToDevice, c->copyStream));
        HIPCHK(c, hipMemcpyAsync(d.tris.p, sg.dTris.p, staticTris * sizeof(TriIsect), hipMemcpyDeviceToDevice, c->copyStream));
        if (!sg.host.fat.empty())
            HIPCHK(c, hipMemcpyAsync(d.fat.p, sg.dFat.p, sg.host.fat.size() * sizeof(TriFat), hipMemcpyDeviceToDevice, c->copyStream));
        d.staticVersion = sg.host.version;
    }
    unsigned char* st = d.stage.mem.p;
    const void* src[7] = { h.topWide.data(), h.instances.data(), h.lights.data(), h.jobs.data(), h.instRoots.data(), h.instFold.data(), h.instRootSrc.data() };
    void* dst[7] = { d.wide.p + staticNodes, d.instances.p, d.lights.p, d.jobs.p, d.wide.p + h.instRootBase, d.instFold.p, d.instRootSrc.p };
    for (int k = 0; k < 7; k++) {
        if (bytes[k] == 0)
            continue;
        std::memcpy(st, src[k], bytes[k]);
        HIPCHK(c, hipMemcpyAsync(dst[k], st, bytes[k], hipMemcpyHostToDevice, c->copyStream));
        st += bytes[k];
    }
    if (total)
        HIPCHK(c, d.stage.recordRead(c->copyStream));
    if (!h.instRootSrc.empty()) { // the folded instances' copies of their meshes' root nodes, from the set's own (just refreshed) copy of the static nodes
        const uint32_t n = (uint32_t)h.instRootSrc.size();
        hipLaunchKernelGGL(k_inst_roots, dim3((n + 63u) / 64u), dim3(64), 0, c->copyStream, d.wide.p, d.instRootSrc.p, d.wide.p + h.instRootBase, n);
    }
    if (!h.jobs.empty()) { // the world-space copies: one thread per (copy, node) and per (copy, triangle reference)
        BakeArgs ba {};
        ba.srcWide = sg.dWide.p, ba.srcBoxes = sg.dBoxes.p, ba.srcLeafOfs = sg.dLeafOfs.p, ba.refTri = sg.dRefTri.p, ba.srcTris = sg.dTris.p;
        ba.dstWide = d.wide.p, ba.dstTris = d.tris.p, ba.emptyRef = sg.host.emptyRef;
        for (size_t first = 0; first < h.jobs.size(); first += 32768) {
            const uint32_t n = (uint32_t)std::min<size_t>(32768, h.jobs.size() - first);
            uint32_t maxNodes = 0, maxRefs = 0;
            for (uint32_t k = 0; k < n; k++)
                maxNodes = std::max(maxNodes, h.jobs[first + k].numNodes), maxRefs = std::max(maxRefs, h.jobs[first + k].numRefs);
            ba.jobs = d.jobs.p + first;
            if (maxNodes)
                hipLaunchKernelGGL(k_bake_nodes, dim3((maxNodes + 127) / 128, n), dim3(128), 0, c->copyStream, ba);
            if (maxRefs)
                hipLaunchKernelGGL(k_bake_tris, dim3((maxRefs + 255) / 256, n), dim3(256), 0, c->copyStream, ba);
        }
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(d.uploaded, c->copyStream));
    tm.lap("enqueue");
    d.numLights = h.numLights;
    d.rootRef = h.rootRef;
    d.staticIndex = (int)(c->st - c->stat);
    d.numTris = c->st->host.numTris, d.firstWorldNode = (uint32_t)sg.host.wide.size();
    d.rootRefFolded = h.rootRefFolded;
    d.foldedInstances = h.foldedInstances;
    d.instRootBase = h.instRootBase, d.numInstRoots = (uint32_t)h.instRoots.size(), d.instFoldCount = h.generalRoute ? h.enteredGeneral : (uint32_t)h.instFold.size(); // (the general route: how many entered instances want their 3 x 4 rows)
    d.packetOk = h.packetOk;
    d.stackNeed = h.stackNeed;
    d.hasInstances = h.hasInstances;
    d.generalRoute = h.generalRoute && h.hasInstances, d.enteredInstances = h.enteredInstances;
    d.instanceTopNode = std::move(h.instanceTopNode);
    d.hostInstances = std::move(h.instances); // (copied into the staging memory above)
    d.numTopNodes = nTop;
    c->pending = target;
    return PT_OK;
    });
}

// RayTracer::frameTick's flip (src/raytracer.cpp:183-189) with the barrier of transferDynamicData (:593): renders enqueued from
// now on wait for the pending upload and read the new set; nothing waits on the host.
int pt_frame_tick(pt_ctx* c)
{
    if (!c)
        return PT_ERR_INVALID;
    if (c->pending < 0)
        return PT_OK; // nothing was uploaded since the last tick
    HIPCHK(c, hipSetDevice(c->device));
    pt_ctx::DynamicSet& next = c->dyn[c->pending];
    HIPCHK(c, hipStreamWaitEvent(c->stream, next.uploaded, 0));
    if (c->pending != c->active) {
        pt_ctx::DynamicSet& old = c->dyn[c->active];
        HIPCHK(c, hipEventRecord(old.lastUse, c->stream)); // everything enqueued so far may still read the old set
        old.used = true;
    }
    next.used = true;
    HIPCHK(c, hipEventRecord(next.lastUse, c->stream));
    c->active = c->pending;
    newEpoch(c); // (what a batch's first pass emits belongs to the scene state it was measured on)
    c->pending = -1;
    c->haveDynamic = true;
    c->motion.set = false; // (its records are indexed by the state that was just replaced)
    c->motion.moving = 0;
    c->vertexMotion.set = false; // (its "then" is the state before the one that was just replaced)
    if (next.staticIndex != c->statCur) { // the state was built on a rebuilt scene (pt_upload_static_async): that scene is the current one from here on
        c->statCur = next.staticIndex;
        c->st = &c->stat[c->statCur];
    }
    if (c->statPending == c->statCur)
        c->statPending = -1;
    refreshSceneView(c);
    return PT_OK;
}

// the synchronous-looking form: the next pt_render sees the new state (still no host-side wait for the device)
int pt_upload_dynamic(pt_ctx* c, const pt_emissive_triangle* lights, uint32_t nL, const pt_top_bvh_node* topNodes, uint32_t nTop, uint32_t topRoot)
{
    const int rc = pt_upload_dynamic_async(c, lights, nL, topNodes, nTop, topRoot);
    return rc ? rc : pt_frame_tick(c);
}

int pt_upload_texture_array(pt_ctx* c, int kind, uint32_t width, uint32_t height, uint32_t layers, int format, const void* data)
{
    return guarded(c, "pt_upload_texture_array", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    if ((kind != 0 && kind != 1) || !data || width == 0 || height == 0 || layers == 0 || (format != PT_TEX_RGBA32F && format != PT_TEX_BGRA8_UNORM))
        return fail(c, PT_ERR_INVALID, "pt_upload_texture_array: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    DevBuf<uint8_t>& buf = kind == 0 ? c->texMaterial : c->texSky;
    const size_t bytes = (size_t)width * height * layers * (format == PT_TEX_RGBA32F ? sizeof(float4) : 4u);
    HIPCHK(c, buf.alloc(bytes));
    HIPCHK(c, hipMemcpy(buf.p, data, bytes, hipMemcpyHostToDevice));
    Texture& t = kind == 0 ? c->scene.materialTex : c->scene.sky;
    t.width = (int)width;
    t.height = (int)height;
    t.layers = (int)layers;
    t.format = format;
    refreshSceneView(c);
    newEpoch(c); // (an albedo map's alpha decides how many paths go on after a hit: the ratios the batches are sized by are measured again)
    return PT_OK;
    });
}

int pt_set_camera(pt_ctx* c, const pt_camera* cam)
{
    if (!c || !cam)
        return PT_ERR_INVALID;
    auto f4 = [](const float* p) { return make_float4(p[0], p[1], p[2], 0.f); };
    c->camera.eye = f4(cam->eyePoint);
    c->camera.screen = f4(cam->screenPoint);
    c->camera.u = f4(cam->u);
    c->camera.v = f4(cam->v);
    c->camera.uN = f4(cam->uNormalized);
    c->camera.vN = f4(cam->vNormalized);
    c->camera.focalDistance = cam->focalDistance;
    c->camera.apertureRadius = cam->apertureRadius;
    c->camera.relativeAperture = cam->relativeAperture;
    c->camera.shutterTime = cam->shutterTime;
    c->camera.ISO = cam->ISO;
    c->camera.thinLens = cam->thinLensEnabled ? 1u : 0u;
    c->haveCamera = true;
    newEpoch(c);
    return PT_OK;
}

} // extern "C"

namespace {

// The owned pixels of a context, from rects: pt_set_tiles' whole body, and how a round of pt_render_adaptive installs the pixels of its active blocks
// and puts the whole frame back.  n == 0: the whole frame.
int installPixelRects(pt_ctx* c, const pt_rect* rects, uint32_t n)
{
    const uint32_t W = c->cfg.width, H = c->cfg.height;
    pt_rect whole { 0, 0, W, H };
    if (n == 0 || !rects) {
        rects = &whole;
        n = 1;
    }
    const bool rowMajor = (c->cfg.flags & PT_FLAG_ROWMAJOR_PIXELS) || parityMode(c);
    std::vector<uint32_t> list;
    // position of every pixel in the list; doubles as the overlap check: the kernels deposit with a plain
    // read-modify-write that relies on ONE live path per (plane, pixel), so a pixel listed twice would race
    constexpr uint32_t kUnowned = 0xFFFFFFFFu;
    std::vector<uint32_t> ordinal((size_t)W * H, kUnowned);
    auto add = [&](uint32_t x, uint32_t y) {
        const uint32_t px = y * W + x;
        if (ordinal[px] != kUnowned)
            return false;
        ordinal[px] = (uint32_t)list.size();
        list.push_back(px);
        return true;
    };
    for (uint32_t r = 0; r < n; r++) {
        const pt_rect& q = rects[r];
        if (q.x0 >= q.x1 || q.y0 >= q.y1 || q.x1 > W || q.y1 > H)
            return fail(c, PT_ERR_INVALID, "pt_set_tiles: rect %u out of bounds", r);
        bool ok = true;
        if (rowMajor) {
            for (uint32_t y = q.y0; y < q.y1; y++)
                for (uint32_t x = q.x0; x < q.x1; x++)
                    ok = add(x, y) && ok;
        } else { // 8x8 pixel blocks: a 64-lane wave starts on a compact screen-space tile
            for (uint32_t by = q.y0; by < q.y1; by += 8)
                for (uint32_t bx = q.x0; bx < q.x1; bx += 8)
                    for (uint32_t y = by; y < std::min(by + 8, q.y1); y++)
                        for (uint32_t x = bx; x < std::min(bx + 8, q.x1); x++)
                            ok = add(x, y) && ok;
        }
        if (!ok)
            return fail(c, PT_ERR_INVALID, "pt_set_tiles: rect %u overlaps an earlier one", r);
    }
    if (c->queuesReady && list == c->hostPixelList)
        return PT_OK; // the same pixels in the same order: queues, planes and ordinals stay as they are
    c->identityPixels = rowMajor && n == 1 && rects[0].x0 == 0 && rects[0].y0 == 0 && rects[0].x1 == W && rects[0].y1 == H;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = uploadVec(c, c->pixelList, list);
    if (rc)
        return rc;
    if (list.size() == (size_t)W * H) { // whole frame: the extra accumulator planes are indexed by the pixel itself
        c->pixelOrdinal.release();
    } else if ((rc = uploadVec(c, c->pixelOrdinal, ordinal)))
        return rc;
    c->numOwned = (uint32_t)list.size();
    c->hostPixelList = std::move(list);
    c->queuesReady = false; // the ordinal of a pixel may have changed: queues and planes are re-made lazily (ensureQueues)
    return PT_OK;
}

// ---- adaptive sampling: the state and its one evaluation (pt_adaptive.h); the entry points stand behind the firefly clamp's

inline uint32_t adaptiveBlocksX(const pt_ctx* c) { return (c->cfg.width + 7u) / 8u; }
inline uint32_t adaptiveBlocks(const pt_ctx* c) { return adaptiveBlocksX(c) * ((c->cfg.height + 7u) / 8u); }
constexpr size_t kAdaptiveCounterWords = kAdaptiveStripes * sizeof(AdaptiveCounters) / sizeof(uint32_t);

// no samples: halves, counts and errors zero, every block active (a count of 0 is below any min_samples)
int clearAdaptive(pt_ctx* c)
{
    pt_ctx::Adaptive::Buffers& b = *c->adaptive.buf;
    HIPCHK(c, b.half[0].zero(c->stream));
    HIPCHK(c, b.half[1].zero(c->stream));
    HIPCHK(c, b.counts.zero(c->stream));
    HIPCHK(c, b.error.zero(c->stream));
    HIPCHK(c, b.blockError.zero(c->stream));
    HIPCHK(c, hipMemsetAsync(b.flags.p, 0x01, b.flags.n * sizeof(uint32_t), c->stream)); // (any non-zero word is a set flag)
    c->adaptive.stats = pt_adaptive_stats {};
    c->adaptive.stats.blocks = c->adaptive.stats.active_blocks = adaptiveBlocks(c);
    return PT_OK;
}

int ensureAdaptive(pt_ctx* c)
{
    if (c->adaptive.buf)
        return PT_OK;
    const size_t n = (size_t)c->cfg.width * c->cfg.height, nB = adaptiveBlocks(c);
    auto b = std::make_unique<pt_ctx::Adaptive::Buffers>(); // (the context gets it whole: a failure on the way frees what there is)
    HIPCHK(c, b->half[0].alloc(n));
    HIPCHK(c, b->half[1].alloc(n));
    HIPCHK(c, b->error.alloc(n));
    HIPCHK(c, b->blockError.alloc(nB));
    HIPCHK(c, b->flags.alloc(nB));
    HIPCHK(c, b->counters.alloc(kAdaptiveStripes));
    HIPCHK(c, b->back.alloc(nB + kAdaptiveCounterWords));
    HIPCHK(c, c->adaptive.events[0].create(true));
    HIPCHK(c, c->adaptive.events[1].create(true));
    HIPCHK(c, b->counts.alloc(n));
    c->adaptive.buf = std::move(b);
    return clearAdaptive(c);
}

// Steps 4 to 6 of a round: the blocks flagged on the device got `add` samples per pixel (0: judge the state as it stands); count, judge, publish the
// accumulator for `spp` = the largest count, read the flags and counters back behind a synchronisation.  One launch does all of it (DESIGN.md,
// section 10, has the two-launch form it was timed against).
int evaluateAdaptive(pt_ctx* c, uint32_t add, uint32_t spp)
{
    pt_ctx::Adaptive::Buffers& b = *c->adaptive.buf;
    const uint32_t W = c->cfg.width, H = c->cfg.height, nB = adaptiveBlocks(c);
    HIPCHK(c, b.counters.zero(c->stream));
    AdaptiveArgs a {};
    a.A = b.half[0].p, a.B = b.half[1].p, a.counts = b.counts.p, a.error = b.error.p;
    a.blockError = b.blockError.p, a.flags = b.flags.p, a.counters = b.counters.p, a.accum = c->accum;
    a.width = W, a.height = H, a.blocksX = adaptiveBlocksX(c), a.blocks = nB;
    a.add = add, a.spp = spp;
    a.minSamples = c->adaptive.prm.min_samples, a.maxSamples = c->adaptive.prm.max_samples, a.threshold = c->adaptive.prm.threshold;
    HIPCHK(c, hipEventRecord(c->adaptive.events[0], c->stream));
    hipLaunchKernelGGL(k_adaptive_eval, dim3((nB + 3u) / 4u), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->adaptive.events[1], c->stream));
    c->spp = spp;
    HIPCHK(c, b.flags.copyTo(b.back.p, c->stream));
    HIPCHK(c, b.counters.read(b.back.p + nB, c->stream));
    AdaptiveCounters k {};
    for (uint32_t s = 0; s < kAdaptiveStripes; s++) { // (the stripes the blocks spread their atomics over)
        AdaptiveCounters one;
        std::memcpy(&one, b.back.p + nB + s * (sizeof(AdaptiveCounters) / sizeof(uint32_t)), sizeof(one));
        k.active += one.active, k.nonfinite += one.nonfinite, k.total += one.total;
        k.maxErrorBits = std::max(k.maxErrorBits, one.maxErrorBits), k.maxNotCount = std::max(k.maxNotCount, one.maxNotCount);
    }
    pt_adaptive_stats& st = c->adaptive.stats;
    st.blocks = nB, st.active_blocks = k.active, st.nonfinite = k.nonfinite;
    st.min_count = ~k.maxNotCount, st.max_count = spp, st.samples_total = k.total;
    std::memcpy(&st.max_block_error, &k.maxErrorBits, sizeof(float));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->adaptive.events[0], c->adaptive.events[1]) == hipSuccess)
        c->adaptive.timing[0] += ms, c->adaptive.timing[1] += 1.0;
    else
        (void)hipGetLastError();
    return PT_OK;
}

} // namespace

extern "C" {

int pt_set_tiles(pt_ctx* c, const pt_rect* rects, uint32_t n)
{
    return guarded(c, "pt_set_tiles", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    if (c->adaptive.set && n != 0 && rects)
        return fail(c, PT_ERR_UNSUPPORTED, "pt_set_tiles: adaptive sampling is on (pt_set_adaptive) -- it owns the pixel list; sharded adaptive sampling is not supported");
    HIPCHK(c, hipSetDevice(c->device));
    return installPixelRects(c, rects, n);
    });
}

int pt_set_accum_buffer(pt_ctx* c, void* device_float4)
{
    if (!c)
        return PT_ERR_INVALID;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->accum = device_float4 ? (float4*)device_float4 : c->accumOwn.p;
    return PT_OK;
}

int pt_clear(pt_ctx* c)
{
    return guarded(c, "pt_clear", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->accum, 0, (size_t)c->cfg.width * c->cfg.height * sizeof(float4), c->stream));
    if (c->foldPlanes > 1 && c->accumPlanes.p) // samples of a pt_render that failed half-way: not to be folded into the fresh accumulator
        HIPCHK(c, hipMemsetAsync(c->accumPlanes.p, 0, c->accumPlanes.n * sizeof(float4), c->stream));
    c->foldPlanes = 0;
    c->spp = 0;
    int rc;
    if (c->guides[0] && (rc = c->guides.zero(c))) // the guide sums belong to the image they describe
        return rc;
    if (c->motionGuides[0] && (rc = c->motionGuides.zero(c))) // ... and so do the two motion sums (the motion itself stays set)
        return rc;
    c->guideSpp = 0;
    if (c->overflowPinned.p && *c->overflowPinned.p) { // a reported overflow is cleared with the image it spoiled (whatever set it has run: the word is only read after a synchronisation)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *c->overflowPinned.p = 0u;
        newEpoch(c); // the ratios learned since were measured on cut counts: the next render probes again
    }
    if (c->accumShadow.p) // (zero between pt_render calls unless one failed half-way)
        HIPCHK(c, hipMemsetAsync(c->accumShadow.p, 0, c->accumShadow.n * sizeof(float4), c->stream));
    c->mergePending = false;
    if (parityMode(c) && c->queuesReady && (rc = resetStreams(c)))
        return rc;
    if (c->adaptive.set && c->adaptive.buf && (rc = clearAdaptive(c))) // the halves, counts and errors belong to the image; the mode stays set
        return rc;
    return PT_OK;
    });
}

} // extern "C"

namespace {

// pt_render's body: `spp` more samples of every owned pixel into c->accum (pt_render_adaptive runs it twice per round, aimed at the two halves)
int renderSamples(pt_ctx* c, uint32_t spp)
{
    int rc;
    if ((rc = checkOverflow(c)))
        return rc;
    if (c->queuesReady && c->q0Small && !derivedPrimariesCapable(c))
        c->queuesReady = false; // (the first queue was sized for a pinhole's bundles: this camera / scene state queues whole camera rays)
    if ((rc = ensureQueues(c)) || (rc = ensureSpill(c)))
        return rc;
    Prof prof { c };
    HIPCHK(c, hipEventRecord(c->evStart, c->stream));
    const bool fixedSchedule = !parityMode(c) && c->cfg.max_active_rays == 0;
    for (uint32_t s = 0; s < spp;) {
        uint32_t batch = fixedSchedule ? std::min(c->planes, spp - s) : 1u;
        bool probe = false;
        if (fixedSchedule && smallQueues(c)) {
            // Queues smaller than the batch: how much of a batch goes on after the first hit, and how many shadow rays leave from there, is measured -- a report
            // of an earlier batch of this epoch, or a short PROBE batch whose report is waited for (16 samples per pixel: the queues hold at least what those
            // can emit, ensureQueues; its samples count like any others) -- and the batch is cut so that it fits with 3 % to spare.
            if (c->passCountsPending && hipEventQuery(c->passCountsCopied) == hipSuccess)
                adoptPassCounts(c);
            else
                (void)hipGetLastError();
            if (!c->ratiosKnown) {
                probe = true;
                const uint64_t room = std::min(c->capExt, c->capShadow);
                batch = std::min<uint32_t>(batch, (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(16, room / std::max(c->numOwned, 1u))));
                if (c->passCountsPending) { // an older report is still on its way: take it first, the probe needs the slot
                    HIPCHK(c, hipEventSynchronize(c->passCountsCopied));
                    adoptPassCounts(c);
                    probe = !c->ratiosKnown;
                }
            }
            if (!probe) // (16 samples per pixel always fit: ensureQueues' floor)
                batch = std::min(batch, std::max(safeBatch(c), std::min(16u, c->planes)));
        }
        if (fixedSchedule) {
            // Up to kGenInterleave samples of a pixel are queue neighbours only if the batch is a multiple of that power of two (k_gen,
            // primaryEntry): a batch of 2 046 would keep TWO together and lose the bundle kernel and every coherent launch behind it.
            // Cut the batch at the largest such multiple; what is left follows as smaller batches.
            uint32_t g = kGenInterleave;
            while (g > 1u && batch < g)
                g >>= 1;
            batch -= batch % g;
        }
        rc = fixedSchedule ? renderSampleFixed(c, c->sampleBase + c->spp, batch, prof) : renderSampleRefill(c, c->spp);
        if (rc) {
            foldPlanesNow(c); // what the earlier batches of this call deposited belongs to the samples already counted
            return rc;
        }
        c->spp += batch;
        s += batch;
        if (probe) { // wait for the probe's counters (a few ms of rendering) and learn the ratios
            c->probeBatches++;
            if (c->passCountsPending) {
                HIPCHK(c, hipEventSynchronize(c->passCountsCopied));
                adoptPassCounts(c);
            }
            if (!c->ratiosKnown) // (no report slot: cannot happen -- the probe took care of it above)
                return fail(c, PT_ERR_STATE, "the probe batch did not report its counters");
        }
    }
    foldPlanesNow(c); // the accumulator is complete when pt_render's work on the stream is: callers read it with their own tools
    HIPCHK(c, hipEventRecord(c->evStop, c->stream));
    if (c->profile) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        double fam[5] = { 0, 0, 0, 0, 0 };
        for (auto& m : prof.marks) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, c->profEvents[m.second], c->profEvents[m.second + 1]);
            fam[m.first] += ms;
        }
        c->msGen = fam[0], c->msIntersect = fam[1] + fam[4], c->msShade = fam[2], c->msShadow = fam[3], c->msPacket = fam[4];
    }
    return PT_OK;
}

} // namespace

extern "C" {

int pt_render(pt_ctx* c, uint32_t spp)
{
    return guarded(c, "pt_render", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    if (c->adaptive.set)
        return fail(c, PT_ERR_STATE, "pt_render: adaptive sampling is on -- pt_render_adaptive renders, or pt_clear and pt_set_adaptive(NULL)");
    if (!c->haveStatic || !c->haveDynamic || !c->haveCamera)
        return fail(c, PT_ERR_STATE, "pt_render: scene (static + dynamic) and camera must be set first");
    HIPCHK(c, hipSetDevice(c->device));
    return renderSamples(c, spp);
    });
}

int pt_synchronize(pt_ctx* c)
{
    if (!c)
        return PT_ERR_INVALID;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checkOverflow(c);
}

namespace {

// where pt_resolve, pt_resolve_device and pt_denoise_device write: the caller's image or, for null, the context's own (pt_resolve_device_ptr), allocated at
// first use -- once per context: this is the interactive getOutput() path
int resolveTarget(pt_ctx* c, void* device_rgba, float4** out)
{
    const uint32_t n = c->cfg.width * c->cfg.height;
    if (!device_rgba && c->resolveTmp.n != n)
        HIPCHK(c, c->resolveTmp.alloc(n));
    *out = device_rgba ? (float4*)device_rgba : c->resolveTmp.p;
    return PT_OK;
}

void launchResolve(pt_ctx* c, float4* out)
{
    const uint32_t n = c->cfg.width * c->cfg.height;
    hipLaunchKernelGGL(k_resolve, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->accum, out, n, (float)c->spp, c->camera.relativeAperture,
        c->camera.shutterTime, c->camera.ISO);
}

} // namespace

int pt_resolve(pt_ctx* c, float* rgba_out)
{
    return guarded(c, "pt_resolve", [&]() -> int {
    if (!c || !rgba_out)
        return PT_ERR_INVALID;
    if (!c->haveCamera || c->spp == 0)
        return fail(c, PT_ERR_STATE, "pt_resolve: nothing rendered yet");
    HIPCHK(c, hipSetDevice(c->device));
    float4* image;
    if (const int rc = resolveTarget(c, nullptr, &image))
        return rc;
    launchResolve(c, image);
    HIPCHK(c, c->resolveTmp.read(rgba_out, c->stream));
    return checkOverflow(c);
    });
}

int pt_resolve_device(pt_ctx* c, void* device_rgba)
{
    return guarded(c, "pt_resolve_device", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    if (!c->haveCamera || c->spp == 0)
        return fail(c, PT_ERR_STATE, "pt_resolve_device: nothing rendered yet");
    HIPCHK(c, hipSetDevice(c->device));
    float4* image;
    if (const int rc = resolveTarget(c, device_rgba, &image))
        return rc;
    launchResolve(c, image);
    HIPCHK(c, hipGetLastError());
    return PT_OK;
    });
}

// the image pt_resolve_device(ctx, NULL) writes: width * height float4, valid once the render stream has passed that call; NULL before
// the first one
void* pt_resolve_device_ptr(pt_ctx* c) { return c ? (void*)c->resolveTmp.p : nullptr; }

int pt_read_accum(pt_ctx* c, float* out)
{
    if (!c || !out)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->accum, (size_t)c->cfg.width * c->cfg.height * sizeof(float4), hipMemcpyDeviceToHost, c->stream)); // (not a DevBuf: the caller's memory, perhaps -- pt_set_accum_buffer)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checkOverflow(c);
}

int pt_write_accum(pt_ctx* c, const float* in, uint32_t spp)
{
    if (!c || !in)
        return PT_ERR_INVALID;
    if (c->adaptive.set)
        return fail(c, PT_ERR_STATE, "pt_write_accum: adaptive sampling is on -- the accumulator is made from the halves (pt_write_adaptive)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->accum, in, (size_t)c->cfg.width * c->cfg.height * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->spp = spp;
    return PT_OK;
}

void* pt_accum_device_ptr(pt_ctx* c) { return c ? (void*)c->accum : nullptr; }

uint32_t pt_samples_per_pixel(const pt_ctx* c) { return c ? c->spp : 0; }

// ---- first-hit guide buffers and the denoiser (pt_denoise.h) -----------------------------------

namespace {

// the guide pass, the sample base and the motion setters key the counter PRNG by sample index: the refusal they share (PT_OK where the schedule is the fixed one)
int fixedScheduleOnly(pt_ctx* c, const char* who)
{
    if (parityMode(c) || c->cfg.max_active_rays != 0)
        return fail(c, PT_ERR_UNSUPPORTED, "%s: the fixed schedule with PT_RNG_COUNTER only (not in parity / refill mode)", who);
    return PT_OK;
}

bool tilesSet(const pt_ctx* c) { return (uint64_t)c->numOwned != (uint64_t)c->cfg.width * c->cfg.height; }

// What the frame stages (filter, history, clamp) refuse alike, in two parts because the history asks for its camera between them: a context that owns
// part of the frame (`why`: what the stage needs the rest for, and what to do instead) ...
int wholeFrameOnly(pt_ctx* c, const char* who, const char* why)
{
    if (tilesSet(c))
        return fail(c, PT_ERR_UNSUPPORTED, "%s: tiles are set -- %s, on a context that owns the frame", who, why);
    return PT_OK;
}
// ... and an image without colour or guide samples
int samplesPresent(pt_ctx* c, const char* who)
{
    if (c->spp == 0)
        return fail(c, PT_ERR_STATE, "%s: no colour samples yet (pt_render)", who);
    if (c->guideSpp == 0)
        return fail(c, PT_ERR_STATE, "%s: no guide samples yet (pt_render_guides)", who);
    return PT_OK;
}

} // namespace

int pt_render_guides(pt_ctx* c, uint32_t spp)
{
    return guarded(c, "pt_render_guides", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    if (!c->haveStatic || !c->haveDynamic || !c->haveCamera)
        return fail(c, PT_ERR_STATE, "pt_render_guides: scene (static + dynamic) and camera must be set first");
    int rc;
    if ((rc = fixedScheduleOnly(c, "pt_render_guides")))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensureSpill(c)) || (rc = c->guides.ensure(c)))
        return rc;
    const uint32_t n = c->numOwned;
    if (c->guideRayO.n < n) { // a scratch queue of its own: one sample of the owned pixels (the render queues may be smaller than that, or hold directions only)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, c->guideRayO.alloc(n));
        HIPCHK(c, c->guideRayD.alloc(n));
        HIPCHK(c, c->guideHit.alloc(n));
        HIPCHK(c, c->guideHitInst.alloc(n));
    }
    if (!c->guideCtl.p) {
        HIPCHK(c, c->guideCtl.alloc(1));
        HIPCHK(c, hipMemsetAsync(c->guideCtl.p, 0, sizeof(Control), c->stream));
    }
    // the guide chain (pt_set_guide_chain), where the scene holds glass at all -- the conversion knows; without any, today's three kernels per sample.
    // With pt_set_guide_reflections a MIRROR is something to follow as well, and the chain's kernel is the reflecting instantiation.
    const ptconv::StaticHost& materialsOf = c->stat[c->dyn[c->active].staticIndex].host;
    const bool reflect = c->guideReflections && c->guideChain != 0u && (materialsOf.refractive || materialsOf.mirror);
    const uint32_t chain = materialsOf.refractive || reflect ? c->guideChain : 0u;
    if (chain && c->guideChainO.n < c->guideRayO.n) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, c->guideChainO.alloc(c->guideRayO.n));
        HIPCHK(c, c->guideChainD.alloc(c->guideRayO.n));
        HIPCHK(c, c->guideChainDist[0].alloc(c->guideRayO.n));
        HIPCHK(c, c->guideChainDist[1].alloc(c->guideRayO.n));
    }
    if (reflect && c->guideChainTint[0].n < c->guideRayO.n) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, c->guideChainTint[0].alloc(c->guideRayO.n));
        HIPCHK(c, c->guideChainTint[1].alloc(c->guideRayO.n));
    }
    // always the per-ray kernel: which kernel traces a launch must not depend on what the last render left in the context (the team kernel is chosen
    // by the previous batch's counters), and the launch is none of pt_stats' business
    const uint32_t batchEntries = c->batchEntries;
    const uint64_t teamLaunches = c->teamLaunches;
    c->batchEntries = 0;
    for (uint32_t s = 0; s < spp; s++) {
        const FrameParams fp = frameParams(c, c->sampleBase + c->guideSpp + s);
        hipLaunchKernelGGL(k_guide_gen, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, fp, c->guideRayO.p, c->guideRayD.p,
            c->identityPixels ? nullptr : c->pixelList.p, n, c->guideCtl.p);
        TraceArgs a = traceArgsBase(c);
        a.parityShadow = 0;
        a.rayO = c->guideRayO.p, a.rayD = c->guideRayD.p, a.rayC = nullptr;
        a.hit = c->guideHit.p, a.inst = c->guideHitInst.p, a.accum = AccumView { nullptr, nullptr, nullptr, 0u }, a.occluded = nullptr;
        a.ctl = c->guideCtl.p, a.pass = 0;
        if (chain) {
            // stages 1 .. K start empty, with their fetch cursors at zero (k_guide_gen arms stage 0 alone); an error shows in hipGetLastError below,
            // after the render's bookkeeping is back in place
            (void)hipMemsetAsync(&c->guideCtl.p->extCount[1], 0, chain * sizeof(uint32_t), c->stream);
            (void)hipMemsetAsync(&c->guideCtl.p->extCursor[1], 0, chain * sizeof(uint32_t), c->stream);
            GuideChainArgs g {};
            g.sc = c->scene, g.hit = c->guideHit.p, g.hitInst = c->guideHitInst.p, g.ctl = c->guideCtl.p;
            g.capacity = n, g.albedoHits = c->guides[0], g.normalDepth = c->guides[1], g.terminals = c->guideChainTerminals.p;
            for (uint32_t j = 0; j <= chain; j++) { // the counts of stages >= 1 are device words: every launch covers the queue, empty workgroups leave at once
                float4* const qO[2] = { c->guideRayO.p, c->guideChainO.p };
                float4* const qD[2] = { c->guideRayD.p, c->guideChainD.p };
                a.rayO = qO[j & 1u], a.rayD = qD[j & 1u], a.pass = j;
                launchTrace(c, false, a);
                g.qO = qO[j & 1u], g.qD = qD[j & 1u], g.qDist = c->guideChainDist[j & 1u].p;
                g.outO = qO[(j + 1u) & 1u], g.outD = qD[(j + 1u) & 1u], g.outDist = c->guideChainDist[(j + 1u) & 1u].p;
                g.stage = j, g.last = j == chain ? 1u : 0u, g.thinLens = j == 0u ? c->camera.thinLens : 0u;
                if (reflect) {
                    g.qTint = c->guideChainTint[j & 1u].p, g.outTint = c->guideChainTint[(j + 1u) & 1u].p;
                    hipLaunchKernelGGL(k_guide_chain<true>, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, g);
                } else {
                    hipLaunchKernelGGL(k_guide_chain<false>, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, g);
                }
            }
            continue;
        }
        launchTrace(c, false, a);
        if (c->vertexMotion.set && c->vertexMotion.deformed) // (the snapshot, never the inactive set: the next state may be on its way into that)
            launchGuides<2>(c, n, GuideMotionArgs { c->motion.records.p, c->motionGuides[0], c->motionGuides[1], c->vertexMotion.fatThen.p, c->vertexMotion.rows.p });
        else if (c->motion.set || c->vertexMotion.set) // (vertex motion with nothing deformed: identity records, exact zeros and the bits of N)
            launchGuides<1>(c, n, GuideMotionArgs { c->motion.records.p, c->motionGuides[0], c->motionGuides[1], nullptr, nullptr });
        else
            launchGuides<0>(c, n, GuideMotionArgs {});
    }
    c->batchEntries = batchEntries;
    c->teamLaunches = teamLaunches;
    HIPCHK(c, hipGetLastError());
    c->guideSpp += spp;
    return PT_OK;
    });
}

uint32_t pt_guide_samples(const pt_ctx* c) { return c ? c->guideSpp : 0; }

// ---- guide chain (k_guide_chain) ----------------------------------------------------------------
int pt_set_guide_chain(pt_ctx* c, uint32_t maxTransmissions)
{
    return guarded(c, "pt_set_guide_chain", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    if (maxTransmissions > PT_GUIDE_CHAIN_MAX)
        return fail(c, PT_ERR_INVALID, "pt_set_guide_chain: %u transmissions, at most PT_GUIDE_CHAIN_MAX = %u are followed", maxTransmissions, PT_GUIDE_CHAIN_MAX);
    if (maxTransmissions == c->guideChain)
        return PT_OK;
    if (maxTransmissions != 0u) {
        if (const int rc = fixedScheduleOnly(c, "pt_set_guide_chain"))
            return rc;
        if (c->motion.set || c->vertexMotion.set)
            return fail(c, PT_ERR_UNSUPPORTED, "pt_set_guide_chain: an instance or vertex motion is set -- motion deposits along a chain are not supported");
    }
    if (c->guideSpp != 0)
        return fail(c, PT_ERR_STATE, "pt_set_guide_chain: %u guide samples are in the sums already -- sums of two definitions must not mix: change it right after pt_clear", c->guideSpp);
    c->guideChain = maxTransmissions;
    return PT_OK;
    });
}

uint32_t pt_guide_chain(const pt_ctx* c) { return c ? c->guideChain : 0u; }

// ---- guide reflections (k_guide_chain<true>) ----------------------------------------------------
int pt_set_guide_reflections(pt_ctx* c, int enable)
{
    return guarded(c, "pt_set_guide_reflections", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    const bool on = enable != 0;
    if (on == c->guideReflections)
        return PT_OK;
    if (on) {
        if (const int rc = fixedScheduleOnly(c, "pt_set_guide_reflections"))
            return rc;
    }
    if (c->guideSpp != 0)
        return fail(c, PT_ERR_STATE, "pt_set_guide_reflections: %u guide samples are in the sums already -- sums of two definitions must not mix: change it right after pt_clear", c->guideSpp);
    c->guideReflections = on;
    return PT_OK;
    });
}

int pt_guide_reflections(const pt_ctx* c) { return c && c->guideReflections ? 1 : 0; }

// test hook: where the chain of each pixel's LAST guide sample ended
int pt_debug_guide_chain_terminals(pt_ctx* c, int enable)
{
    return guarded(c, "pt_debug_guide_chain_terminals", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (a guide pass in flight may be writing the records)
    const size_t n = (size_t)c->cfg.width * c->cfg.height;
    if (!enable) {
        c->guideChainTerminals.release();
        return PT_OK;
    }
    if (c->guideChainTerminals.n != n)
        HIPCHK(c, c->guideChainTerminals.alloc(n));
    HIPCHK(c, hipMemsetAsync(c->guideChainTerminals.p, 0xFF, n * sizeof(int4), c->stream)); // -1: no chain pass has written the pixel
    return PT_OK;
    });
}

int pt_debug_read_guide_chain_terminals(pt_ctx* c, int32_t* out4)
{
    return guarded(c, "pt_debug_read_guide_chain_terminals", [&]() -> int {
    if (!c || !out4)
        return PT_ERR_INVALID;
    if (!c->guideChainTerminals.p)
        return fail(c, PT_ERR_STATE, "pt_debug_read_guide_chain_terminals: the records are not enabled (pt_debug_guide_chain_terminals)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->guideChainTerminals.read(out4, c->stream));
    return PT_OK;
    });
}

int pt_read_guides(pt_ctx* c, float* albedo_hits, float* normal_depth)
{
    if (!c)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return c->guides.read(c, albedo_hits, normal_depth);
}

int pt_write_guides(pt_ctx* c, const float* albedo_hits, const float* normal_depth, uint32_t spp)
{
    if (!c || !albedo_hits || !normal_depth)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = c->guides.write(c, albedo_hits, normal_depth))
        return rc;
    c->guideSpp = spp;
    return PT_OK;
}

void* pt_guides_device_ptr(pt_ctx* c, int which) { return c && (which == 0 || which == 1) ? (void*)c->guides[which] : nullptr; }

namespace {

void resolveGuideSigmas(float k_normal, float sigma_depth, float* kNormal, float* invSigmaDepth) // 0 = the default, for the filter and the history's taps alike
{
    *kNormal = k_normal > 0.f ? k_normal : PT_DENOISE_DEFAULT_K_NORMAL;
    *invSigmaDepth = 1.0f / (sigma_depth > 0.f ? sigma_depth : PT_DENOISE_DEFAULT_SIGMA_DEPTH);
}

// the run-time switches of a call to the instantiation that has them as template flags: one table per kernel family, indexed by the switches as bits
// (clamped: `source` is the firefly plane, PT_DENOISE_INPUT_ACCUM alone)
void launchPrepare(pt_ctx* c, uint32_t input, bool clamped, const float4* source, const float* variance, uint32_t n)
{
    static_assert(PT_DENOISE_INPUT_ACCUM == 0 && PT_DENOISE_INPUT_TEMPORAL == 1 && PT_DENOISE_INPUT_TEMPORAL_VARIANCE == 2, "the table below is indexed by the input");
    static const decltype(&k_denoise_prepare<PT_DENOISE_INPUT_ACCUM>) table[4] = { k_denoise_prepare<PT_DENOISE_INPUT_ACCUM>, k_denoise_prepare<PT_DENOISE_INPUT_TEMPORAL>,
        k_denoise_prepare<PT_DENOISE_INPUT_TEMPORAL_VARIANCE>, k_denoise_prepare<PT_DENOISE_INPUT_ACCUM, true> };
    hipLaunchKernelGGL(table[clamped ? 3u : input], dim3((n + 255u) / 256u), dim3(256), 0, c->stream, source, variance, c->guides[0], c->guides[1], c->denoiseColour[0].p,
        c->denoiseGuide.p, n, (float)c->spp, (float)c->guideSpp);
}
void launchAtrous(hipStream_t stream, dim3 grid, dim3 block, bool inLds, bool guided, const AtrousArgs& a)
{
    static const decltype(&k_atrous<false>) table[4] = { k_atrous<false>, k_atrous<true>, k_atrous<false, true>, k_atrous<true, true> };
    hipLaunchKernelGGL(table[inLds | guided << 1], grid, block, 0, stream, a);
}
void launchTemporal(hipStream_t stream, dim3 grid, dim3 block, bool moved, bool variance, bool response, const TemporalArgs& a)
{
    static const decltype(&k_temporal<false>) table[16] = { // <moved, variance, response, firefly>
        k_temporal<false, false, false, false>, k_temporal<true, false, false, false>, k_temporal<false, true, false, false>, k_temporal<true, true, false, false>,
        k_temporal<false, false, true, false>, k_temporal<true, false, true, false>, k_temporal<false, true, true, false>, k_temporal<true, true, true, false>,
        k_temporal<false, false, false, true>, k_temporal<true, false, false, true>, k_temporal<false, true, false, true>, k_temporal<true, true, false, true>,
        k_temporal<false, false, true, true>, k_temporal<true, false, true, true>, k_temporal<false, true, true, true>, k_temporal<true, true, true, true> };
    const bool firefly = a.firefly != nullptr; // (pt_set_firefly_clamp: d comes from the clamped plane)
    hipLaunchKernelGGL(table[moved | variance << 1 | response << 2 | firefly << 3], grid, block, 0, stream, a);
}

// The firefly clamp's one launch (pt_firefly.h): the plane and the counters of the current accumulator and albedo sums, on the render stream.  The
// caller has checked that colour and guide samples exist and that no tiles are set.
int evaluateFirefly(pt_ctx* c)
{
    const uint32_t W = c->cfg.width, H = c->cfg.height;
    const size_t n = (size_t)W * H;
    if (c->firefly.plane.n != n) {
        HIPCHK(c, c->firefly.plane.alloc(n));
        HIPCHK(c, c->firefly.counts.alloc(2));
    }
    HIPCHK(c, c->firefly.counts.zero(c->stream));
    FireflyArgs f {};
    f.accum = c->accum, f.albedoHits = c->guides[0], f.plane = c->firefly.plane.p, f.counts = c->firefly.counts.p;
    f.width = W, f.height = H, f.spp = (float)c->spp, f.gspp = (float)c->guideSpp;
    f.rank = c->firefly.rank, f.scale = c->firefly.scale;
    hipLaunchKernelGGL(k_firefly, tileGrid(W, H, kAtrousTileW, kAtrousTileH), dim3(kAtrousTileW, kAtrousTileH), 0, c->stream, f);
    HIPCHK(c, hipGetLastError());
    c->firefly.evaluated = true;
    return PT_OK;
}

} // namespace

int pt_denoise_device(pt_ctx* c, const pt_denoise_params* prm, void* device_rgba)
{
    return guarded(c, "pt_denoise_device", [&]() -> int {
    if (!c || !prm)
        return PT_ERR_INVALID;
    if (prm->iterations > 6u)
        return fail(c, PT_ERR_INVALID, "pt_denoise: iterations = %u (0..6)", prm->iterations);
    if (prm->output != PT_DENOISE_TONEMAPPED && prm->output != PT_DENOISE_HDR)
        return fail(c, PT_ERR_INVALID, "pt_denoise: output = %u (PT_DENOISE_TONEMAPPED or PT_DENOISE_HDR)", prm->output);
    if (prm->k_normal < 0.f || prm->sigma_depth < 0.f || prm->sigma_lum < 0.f)
        return fail(c, PT_ERR_INVALID, "pt_denoise: negative filter parameter");
    int rc;
    if ((rc = wholeFrameOnly(c, "pt_denoise", "the filter needs every pixel's neighbours; denoise after the reduce")) || (rc = samplesPresent(c, "pt_denoise")))
        return rc;
    if (prm->input != PT_DENOISE_INPUT_ACCUM && prm->input != PT_DENOISE_INPUT_TEMPORAL && prm->input != PT_DENOISE_INPUT_TEMPORAL_VARIANCE)
        return fail(c, PT_ERR_INVALID, "pt_denoise: input = %u (PT_DENOISE_INPUT_ACCUM, PT_DENOISE_INPUT_TEMPORAL or PT_DENOISE_INPUT_TEMPORAL_VARIANCE)", prm->input);
    const bool guided = prm->input == PT_DENOISE_INPUT_TEMPORAL_VARIANCE; // the history, filtered under its variance
    const bool temporal = prm->input == PT_DENOISE_INPUT_TEMPORAL || guided;
    if (guided && !c->variance.set)
        return fail(c, PT_ERR_STATE, "pt_denoise: PT_DENOISE_INPUT_TEMPORAL_VARIANCE while the temporal variance is off (pt_set_temporal_variance)");
    if (temporal && c->temporalFrames == 0)
        return fail(c, PT_ERR_STATE, "pt_denoise: PT_DENOISE_INPUT_TEMPORAL%s without a history (pt_temporal_accumulate)", guided ? "_VARIANCE" : "");
    const bool tonemapped = prm->output == PT_DENOISE_TONEMAPPED;
    if (tonemapped && !c->haveCamera)
        return fail(c, PT_ERR_STATE, "pt_denoise: the tone-mapped output needs the camera's exposure (pt_set_camera)");
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t W = c->cfg.width, H = c->cfg.height, n = W * H;
    float4* image;
    if ((rc = resolveTarget(c, device_rgba, &image)))
        return rc;
    const PlanePair& history = c->temporal[c->temporalNewest];
    const dim3 lin((n + 255u) / 256u);
    if (prm->iterations == 0u) { // no filtering, no demodulation: pt_resolve's image, or the mean
        if (temporal) // ... over the history: d times the current albedo
            hipLaunchKernelGGL(k_temporal_resolve, lin, dim3(256), 0, c->stream, history[0], c->guides[0], image, n, (float)c->guideSpp, tonemapped ? 1u : 0u,
                c->camera.relativeAperture, c->camera.shutterTime, c->camera.ISO);
        else if (tonemapped)
            launchResolve(c, image);
        else
            hipLaunchKernelGGL(k_denoise_mean, lin, dim3(256), 0, c->stream, c->accum, image, n, (float)c->spp);
        HIPCHK(c, hipGetLastError());
        return PT_OK;
    }
    if (c->denoiseGuide.n != n) {
        HIPCHK(c, c->denoiseColour[0].alloc(n));
        HIPCHK(c, c->denoiseColour[1].alloc(n));
        HIPCHK(c, c->denoiseGuide.alloc(n));
    }
    const bool clamped = c->firefly.set && !temporal; // d_0 is the clamped plane, made afresh (the history was fed clamped frames already)
    if (clamped && (rc = evaluateFirefly(c)))
        return rc;
    launchPrepare(c, prm->input, clamped, temporal ? history[0] : (clamped ? c->firefly.plane.p : c->accum), guided ? c->variance.plane[c->temporalNewest].p : nullptr, n);
    AtrousArgs a {};
    a.guide = c->denoiseGuide.p;
    a.albedoHits = c->guides[0];
    a.width = W, a.height = H;
    resolveGuideSigmas(prm->k_normal, prm->sigma_depth, &a.kNormal, &a.invSigmaDepth);
    const float sigmaLum = prm->sigma_lum > 0.f ? prm->sigma_lum : PT_DENOISE_DEFAULT_SIGMA_LUM;
    a.gspp = (float)c->guideSpp;
    a.relativeAperture = c->camera.relativeAperture, a.shutterTime = c->camera.shutterTime, a.ISO = c->camera.ISO;
    a.history = history[0], a.sigmaVariance = c->variance.sigma, a.relativeFloor = c->variance.relativeFloor, a.invFullHistory = 1.0f / (c->variance.fullHistory - 1.0f); // (guided)
    const dim3 grid = tileGrid(W, H, kAtrousTileW, kAtrousTileH), block(kAtrousTileW, kAtrousTileH);
    for (uint32_t i = 0; i < prm->iterations; i++) {
        const bool last = i + 1u == prm->iterations;
        a.colour = c->denoiseColour[i & 1u].p;
        a.out = last ? image : c->denoiseColour[(i + 1u) & 1u].p;
        a.step = 1 << i;
        a.invSigmaLum = 1.0f / (sigmaLum * std::ldexp(1.0f, -(int)i));
        a.mode = !last ? ATROUS_MORE : (tonemapped ? ATROUS_LAST_TONEMAPPED : ATROUS_LAST_HDR);
        launchAtrous(c->stream, grid, block, 2 * a.step <= kAtrousMaxHalo, guided, a);
    }
    HIPCHK(c, hipGetLastError());
    return PT_OK;
    });
}

int pt_denoise(pt_ctx* c, const pt_denoise_params* prm, float* rgba_out, float* ms_out)
{
    if (!c || !prm || !rgba_out)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventRecord(c->evDenoise[0], c->stream));
    int rc = pt_denoise_device(c, prm, nullptr);
    if (rc)
        return rc;
    HIPCHK(c, hipEventRecord(c->evDenoise[1], c->stream));
    HIPCHK(c, c->resolveTmp.read(rgba_out, c->stream));
    if (ms_out)
        HIPCHK(c, hipEventElapsedTime(ms_out, c->evDenoise[0], c->evDenoise[1]));
    return checkOverflow(c);
}

// ---- sample base and temporal history (pt_temporal.h) -------------------------------------------

int pt_set_sample_base(pt_ctx* c, uint32_t base)
{
    if (!c)
        return PT_ERR_INVALID;
    if (const int rc = fixedScheduleOnly(c, "pt_set_sample_base"))
        return rc;
    c->sampleBase = base;
    return PT_OK;
}

uint32_t pt_sample_base(const pt_ctx* c) { return c ? c->sampleBase : 0; }

namespace {

// the two history sets: allocated (zeroed) at the first temporal call, both -- with their variance planes where that mode is on
int ensureTemporal(pt_ctx* c)
{
    int rc;
    if ((rc = c->temporal[0].ensure(c)) || (rc = c->temporal[1].ensure(c)))
        return rc;
    const size_t n = (size_t)c->cfg.width * c->cfg.height;
    if (c->variance.set)
        for (DevBuf<float>& plane : c->variance.plane)
            HIPCHK(c, plane.ensureZeroed(n, c->stream));
    if (c->response.set) {
        for (DevBuf<float4>& image : c->response.fast)
            HIPCHK(c, image.ensureZeroed(n, c->stream));
        HIPCHK(c, c->response.luminance.ensureZeroed(n, c->stream));
        HIPCHK(c, c->response.mix.ensureZeroed(n, c->stream));
    }
    return PT_OK;
}

// What the setters of the two temporal modes share: no parameter negative or non-finite ...
int nonNegativeFinite(pt_ctx* c, const char* who, std::initializer_list<float> given)
{
    for (const float f : given)
        if (!(f >= 0.0f) || !std::isfinite(f))
            return fail(c, PT_ERR_INVALID, "%s: negative or non-finite parameter", who);
    return PT_OK;
}
// ... and a mode that changes only while there is no history
int noHistoryOnly(pt_ctx* c, const char* who)
{
    if (c->temporalFrames != 0)
        return fail(c, PT_ERR_STATE, "%s: a history of %u frames exists -- set or forget the mode right after pt_temporal_reset", who, c->temporalFrames);
    return PT_OK;
}
// What the transfers of the two modes' planes share: PT_OK with the mode on (`set`; "variance" or "response"), a history there and the buffers allocated
int temporalModeReady(pt_ctx* c, const char* who, bool set, const char* mode)
{
    if (!set)
        return fail(c, PT_ERR_STATE, "%s: the temporal %s is off (pt_set_temporal_%s)", who, mode, mode);
    if (c->temporalFrames == 0)
        return fail(c, PT_ERR_STATE, "%s: no history (pt_temporal_accumulate, pt_write_temporal)", who);
    HIPCHK(c, hipSetDevice(c->device));
    return ensureTemporal(c);
}

struct D3 {
    double x, y, z;
};
D3 d3(float4 f) { return { f.x, f.y, f.z }; }
D3 crossD(D3 a, D3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
V3 scaledToV3(D3 a, double s) { return mk((float)(a.x * s), (float)(a.y * s), (float)(a.z * s)); }

} // namespace

int pt_temporal_accumulate(pt_ctx* c, const pt_temporal_params* prm)
{
    return guarded(c, "pt_temporal_accumulate", [&]() -> int {
    if (!c || !prm)
        return PT_ERR_INVALID;
    if (prm->max_history > 4096u)
        return fail(c, PT_ERR_INVALID, "pt_temporal_accumulate: max_history = %u (1..4096; 0 = 32)", prm->max_history);
    if (!(prm->k_normal >= 0.f) || !(prm->sigma_depth >= 0.f))
        return fail(c, PT_ERR_INVALID, "pt_temporal_accumulate: negative or NaN k_normal / sigma_depth");
    int rc;
    if ((rc = wholeFrameOnly(c, "pt_temporal_accumulate", "the history is reprojected across the whole frame; accumulate after the reduce")))
        return rc;
    if (!c->haveCamera)
        return fail(c, PT_ERR_STATE, "pt_temporal_accumulate: no camera yet (pt_set_camera)");
    if ((rc = samplesPresent(c, "pt_temporal_accumulate")))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensureTemporal(c)))
        return rc;
    const int from = c->temporalNewest, to = from ^ 1;
    TemporalArgs a {};
    a.accum = c->accum, a.albedoHits = c->guides[0], a.normalDepth = c->guides[1];
    a.outColour = c->temporal[to][0], a.outGuide = c->temporal[to][1];
    a.width = c->cfg.width, a.height = c->cfg.height;
    a.spp = (float)c->spp, a.gspp = (float)c->guideSpp;
    resolveGuideSigmas(prm->k_normal, prm->sigma_depth, &a.kNormal, &a.invSigmaDepth);
    a.maxHistory = (float)(prm->max_history ? prm->max_history : 32u);
    a.invW = 1.0f / (float)a.width, a.invH = 1.0f / (float)a.height;
    a.eye = xyz(c->camera.eye), a.screen = xyz(c->camera.screen), a.u = xyz(c->camera.u), a.v = xyz(c->camera.v);
    if (c->temporalFrames != 0) {
        const CameraDev& h = c->temporalCamera;
        const D3 e = d3(h.eye), sp = d3(h.screen), u = d3(h.u), v = d3(h.v);
        const D3 s0 { sp.x - e.x, sp.y - e.y, sp.z - e.z };
        const D3 uv = crossD(u, v), vs = crossD(v, s0), su = crossD(s0, u);
        const double det = s0.x * uv.x + s0.y * uv.y + s0.z * uv.z;
        if (det != 0.0 && std::isfinite(det)) { // (a degenerate camera has nothing to reproject into: the frame starts a history)
            a.histColour = c->temporal[from][0], a.histGuide = c->temporal[from][1];
            a.histEye = xyz(h.eye);
            a.rowLambda = scaledToV3(uv, 1.0 / det), a.rowAlpha = scaledToV3(vs, 1.0 / det), a.rowBeta = scaledToV3(su, 1.0 / det);
        }
    }
    const dim3 grid = tileGrid(a.width, a.height, kTemporalTileW, kTemporalTileH), block(kTemporalTileW, kTemporalTileH);
    const bool moved = c->motion.set || c->vertexMotion.set; // the history is met where the surfaces were (the two sums are there: the setters made them)
    if (moved)
        a.motion = c->motionGuides[0], a.prevNormal = c->motionGuides[1];
    a.histVariance = c->variance.plane[from].p, a.outVariance = c->variance.plane[to].p; // (varianceSet: the same arithmetic and one more plane)
    a.histFast = c->response.fast[from].p, a.outFast = c->response.fast[to].p, a.outLuminance = c->response.luminance.p, a.fastHistory = c->response.fastHistory; // (responseSet)
    if (c->firefly.set) { // the current frame's d comes clamped, from a plane made afresh
        if ((rc = evaluateFirefly(c)))
            return rc;
        a.firefly = c->firefly.plane.p;
    }
    launchTemporal(c->stream, grid, block, moved, c->variance.set, c->response.set, a);
    HIPCHK(c, hipGetLastError());
    if (c->response.set) {
        if (a.histColour) { // the two histories of every pixel are there: mix them where the window says so
            ResponseArgs r {};
            r.luminance = c->response.luminance.p, r.colour = a.outColour, r.fast = a.outFast, r.mix = c->response.mix.p;
            r.width = a.width, r.height = a.height, r.sigmaResponse = c->response.sigma, r.relativeFloor = c->response.relativeFloor;
            hipLaunchKernelGGL(k_temporal_response, grid, block, 0, c->stream, r);
            HIPCHK(c, hipGetLastError());
        } else // no history: fast = (d, 1) = colour_count, nothing to mix
            HIPCHK(c, c->response.mix.zero(c->stream));
    }
    c->temporalCamera = c->camera;
    c->temporalNewest = to;
    c->temporalFrames++;
    return PT_OK;
    });
}

int pt_temporal_reset(pt_ctx* c)
{
    if (!c)
        return PT_ERR_INVALID;
    c->temporalFrames = 0;
    return PT_OK;
}

uint32_t pt_temporal_frames(const pt_ctx* c) { return c ? c->temporalFrames : 0; }

int pt_read_temporal(pt_ctx* c, float* colour_count, float* normal_depth)
{
    if (!c)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = ensureTemporal(c))
        return rc;
    return c->temporal[c->temporalNewest].read(c, colour_count, normal_depth);
}

int pt_write_temporal(pt_ctx* c, const float* colour_count, const float* normal_depth, const pt_camera* made_under)
{
    if (!c || !colour_count || !normal_depth || !made_under)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensureTemporal(c)) || (rc = c->temporal[c->temporalNewest].write(c, colour_count, normal_depth)))
        return rc;
    if (c->variance.set) // nothing is known about these colours' spread: pt_write_temporal_variance restores it
        HIPCHK(c, c->variance.plane[c->temporalNewest].zero(c->stream));
    if (c->response.set) // the fast history restarts from the current frame: pt_write_temporal_fast restores it
        HIPCHK(c, c->response.fast[c->temporalNewest].zero(c->stream));
    auto f4 = [](const float* p) { return make_float4(p[0], p[1], p[2], 0.f); };
    c->temporalCamera = CameraDev {};
    c->temporalCamera.eye = f4(made_under->eyePoint), c->temporalCamera.screen = f4(made_under->screenPoint);
    c->temporalCamera.u = f4(made_under->u), c->temporalCamera.v = f4(made_under->v);
    c->temporalFrames = 1;
    return PT_OK;
}

void* pt_temporal_device_ptr(pt_ctx* c, int which) { return c && (which == 0 || which == 1) ? (void*)c->temporal[c->temporalNewest][which] : nullptr; }

// ---- temporal variance (k_temporal<., true>, k_atrous<., true>) ---------------------------------

int pt_set_temporal_variance(pt_ctx* c, const pt_variance_params* prm)
{
    if (!c)
        return PT_ERR_INVALID;
    if (const int rc = fixedScheduleOnly(c, "pt_set_temporal_variance"))
        return rc;
    int rc;
    if (prm) {
        if ((rc = nonNegativeFinite(c, "pt_set_temporal_variance", { prm->sigma_variance, prm->relative_floor, prm->full_history })))
            return rc;
        if (prm->full_history != 0.0f && prm->full_history < 2.0f)
            return fail(c, PT_ERR_INVALID, "pt_set_temporal_variance: full_history = %g (at least 2; 0 = %g)", (double)prm->full_history,
                (double)PT_VARIANCE_DEFAULT_FULL_HISTORY);
    }
    if ((rc = noHistoryOnly(c, "pt_set_temporal_variance")))
        return rc;
    c->variance.set = prm != nullptr;
    if (prm) {
        c->variance.sigma = prm->sigma_variance > 0.f ? prm->sigma_variance : PT_VARIANCE_DEFAULT_SIGMA_VARIANCE;
        c->variance.relativeFloor = prm->relative_floor > 0.f ? prm->relative_floor : PT_VARIANCE_DEFAULT_RELATIVE_FLOOR;
        c->variance.fullHistory = prm->full_history > 0.f ? prm->full_history : PT_VARIANCE_DEFAULT_FULL_HISTORY;
    }
    return PT_OK;
}

int pt_temporal_variance(const pt_ctx* c) { return c && c->variance.set ? 1 : 0; }

int pt_read_temporal_variance(pt_ctx* c, float* out)
{
    if (!c || !out)
        return PT_ERR_INVALID;
    if (const int rc = temporalModeReady(c, "pt_read_temporal_variance", c->variance.set, "variance"))
        return rc;
    HIPCHK(c, c->variance.plane[c->temporalNewest].read(out, c->stream));
    return PT_OK;
}

int pt_write_temporal_variance(pt_ctx* c, const float* in)
{
    if (!c || !in)
        return PT_ERR_INVALID;
    if (const int rc = temporalModeReady(c, "pt_write_temporal_variance", c->variance.set, "variance"))
        return rc;
    HIPCHK(c, c->variance.plane[c->temporalNewest].write(in, c->stream));
    return PT_OK;
}

void* pt_temporal_variance_device_ptr(pt_ctx* c) { return c && c->variance.set ? (void*)c->variance.plane[c->temporalNewest].p : nullptr; }

// ---- temporal response (k_temporal<., ., true>, k_temporal_response) ----------------------------

int pt_set_temporal_response(pt_ctx* c, const pt_response_params* prm)
{
    if (!c)
        return PT_ERR_INVALID;
    if (const int rc = fixedScheduleOnly(c, "pt_set_temporal_response"))
        return rc;
    if (prm) {
        if (prm->fast_history > 4096u)
            return fail(c, PT_ERR_INVALID, "pt_set_temporal_response: fast_history = %u (1..4096; 0 = %u)", prm->fast_history, PT_RESPONSE_DEFAULT_FAST_HISTORY);
        if (const int rc = nonNegativeFinite(c, "pt_set_temporal_response", { prm->sigma_response, prm->relative_floor }))
            return rc;
    }
    if (const int rc = noHistoryOnly(c, "pt_set_temporal_response"))
        return rc;
    c->response.set = prm != nullptr;
    if (prm) {
        c->response.fastHistory = (float)(prm->fast_history ? prm->fast_history : PT_RESPONSE_DEFAULT_FAST_HISTORY);
        c->response.sigma = prm->sigma_response > 0.f ? prm->sigma_response : PT_RESPONSE_DEFAULT_SIGMA_RESPONSE;
        c->response.relativeFloor = prm->relative_floor > 0.f ? prm->relative_floor : PT_RESPONSE_DEFAULT_RELATIVE_FLOOR;
    }
    return PT_OK;
}

int pt_temporal_response(const pt_ctx* c) { return c && c->response.set ? 1 : 0; }

int pt_read_temporal_fast(pt_ctx* c, float* colour_count)
{
    if (!c || !colour_count)
        return PT_ERR_INVALID;
    if (const int rc = temporalModeReady(c, "pt_read_temporal_fast", c->response.set, "response"))
        return rc;
    HIPCHK(c, c->response.fast[c->temporalNewest].read(colour_count, c->stream));
    return PT_OK;
}

int pt_write_temporal_fast(pt_ctx* c, const float* colour_count)
{
    if (!c || !colour_count)
        return PT_ERR_INVALID;
    if (const int rc = temporalModeReady(c, "pt_write_temporal_fast", c->response.set, "response"))
        return rc;
    HIPCHK(c, c->response.fast[c->temporalNewest].write(colour_count, c->stream));
    return PT_OK;
}

int pt_read_temporal_response(pt_ctx* c, float* s_out)
{
    if (!c || !s_out)
        return PT_ERR_INVALID;
    if (const int rc = temporalModeReady(c, "pt_read_temporal_response", c->response.set, "response"))
        return rc;
    HIPCHK(c, c->response.mix.read(s_out, c->stream));
    return PT_OK;
}

void* pt_temporal_fast_device_ptr(pt_ctx* c) { return c && c->response.set ? (void*)c->response.fast[c->temporalNewest].p : nullptr; }

// ---- firefly clamp (k_firefly, k_temporal<., ., ., true>, k_denoise_prepare<., true>) ------------

int pt_set_firefly_clamp(pt_ctx* c, const pt_firefly_params* prm)
{
    if (!c)
        return PT_ERR_INVALID;
    if (const int rc = fixedScheduleOnly(c, "pt_set_firefly_clamp"))
        return rc;
    if (prm) {
        if (prm->rank > PT_FIREFLY_MAX_RANK)
            return fail(c, PT_ERR_INVALID, "pt_set_firefly_clamp: rank = %u (1..%u; 0 = %u)", prm->rank, PT_FIREFLY_MAX_RANK, PT_FIREFLY_DEFAULT_RANK);
        if (!std::isfinite(prm->scale) || prm->scale < 0.0f || (prm->scale > 0.0f && prm->scale < 1.0f))
            return fail(c, PT_ERR_INVALID, "pt_set_firefly_clamp: scale = %g (at least 1; 0 = %g)", (double)prm->scale, (double)PT_FIREFLY_DEFAULT_SCALE);
    }
    c->firefly.set = prm != nullptr;
    if (prm) {
        c->firefly.rank = prm->rank ? prm->rank : PT_FIREFLY_DEFAULT_RANK;
        c->firefly.scale = prm->scale > 0.f ? prm->scale : PT_FIREFLY_DEFAULT_SCALE;
    }
    return PT_OK;
}

int pt_firefly_clamp(const pt_ctx* c) { return c && c->firefly.set ? 1 : 0; }

namespace {

// the plane and / or the counters of the last evaluation to the host, behind a synchronisation
int readFirefly(pt_ctx* c, float* d_s, uint32_t counts[2])
{
    HIPCHK(c, c->firefly.plane.copyTo(d_s, c->stream));
    HIPCHK(c, c->firefly.counts.read(counts, c->stream));
    return PT_OK;
}

} // namespace

int pt_read_firefly(pt_ctx* c, float* d_s, uint32_t counts[2])
{
    if (!c)
        return PT_ERR_INVALID;
    if (!c->firefly.set)
        return fail(c, PT_ERR_STATE, "pt_read_firefly: the firefly clamp is off (pt_set_firefly_clamp)");
    int rc;
    if ((rc = wholeFrameOnly(c, "pt_read_firefly", "the clamp needs every pixel's neighbours; evaluate after the reduce")) || (rc = samplesPresent(c, "pt_read_firefly")))
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = evaluateFirefly(c)))
        return rc;
    return readFirefly(c, d_s, counts);
}

int pt_firefly_counts(pt_ctx* c, uint32_t counts[2])
{
    if (!c || !counts)
        return PT_ERR_INVALID;
    if (!c->firefly.evaluated)
        return fail(c, PT_ERR_STATE, "pt_firefly_counts: the stage has not been evaluated yet (pt_temporal_accumulate, pt_denoise, pt_read_firefly with the mode on)");
    HIPCHK(c, hipSetDevice(c->device));
    return readFirefly(c, nullptr, counts);
}

void* pt_firefly_device_ptr(pt_ctx* c) { return c && c->firefly.set && c->firefly.evaluated ? (void*)c->firefly.plane.p : nullptr; }

// ---- adaptive sampling (k_adaptive_eval; the helpers stand before pt_set_tiles) -------------------

int pt_set_adaptive(pt_ctx* c, const pt_adaptive_params* prm)
{
    return guarded(c, "pt_set_adaptive", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    if (const int rc = fixedScheduleOnly(c, "pt_set_adaptive"))
        return rc;
    pt_adaptive_params p {};
    if (prm) {
        p.threshold = prm->threshold;
        p.min_samples = prm->min_samples ? prm->min_samples : 64u;
        p.round_samples = prm->round_samples ? prm->round_samples : 64u;
        p.max_samples = prm->max_samples ? prm->max_samples : 1024u;
        if (!std::isfinite(p.threshold) || p.threshold < 0.0f)
            return fail(c, PT_ERR_INVALID, "pt_set_adaptive: threshold = %g (finite, >= 0; 0 = never stop by error)", (double)prm->threshold);
        if ((p.min_samples | p.round_samples | p.max_samples) & 1u)
            return fail(c, PT_ERR_INVALID, "pt_set_adaptive: min_samples = %u, round_samples = %u, max_samples = %u must be even (a round is two equal halves)",
                p.min_samples, p.round_samples, p.max_samples);
        if (p.max_samples < p.min_samples || p.max_samples > (1u << 20))
            return fail(c, PT_ERR_INVALID, "pt_set_adaptive: max_samples = %u (min_samples = %u .. %u)", p.max_samples, p.min_samples, 1u << 20);
    }
    const bool on = prm != nullptr;
    if (on != c->adaptive.set) {
        if (on && tilesSet(c))
            return fail(c, PT_ERR_UNSUPPORTED, "pt_set_adaptive: tiles are set -- adaptive sampling owns the pixel list of a whole-frame context");
        if (c->spp != 0)
            return fail(c, PT_ERR_STATE, "pt_set_adaptive: the mode changes only while there are no samples (pt_clear first)");
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (!on) {
        if (c->adaptive.set) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->adaptive.buf.reset();
        }
        c->adaptive.set = false;
        return PT_OK;
    }
    const bool was = c->adaptive.set;
    c->adaptive.set = true;
    c->adaptive.prm = p;
    if (!was) {
        c->adaptive.stats = pt_adaptive_stats {};
        c->adaptive.stats.blocks = c->adaptive.stats.active_blocks = adaptiveBlocks(c);
    } else if (c->spp > 0 && c->adaptive.buf) { // the flags are a function of the state AND the parameters
        return evaluateAdaptive(c, 0, c->spp);
    }
    return PT_OK;
    });
}

int pt_adaptive(const pt_ctx* c) { return c && c->adaptive.set ? 1 : 0; }

int pt_adaptive_params_get(const pt_ctx* c, pt_adaptive_params* out)
{
    if (!c || !out)
        return PT_ERR_INVALID;
    if (!c->adaptive.set)
        return fail(const_cast<pt_ctx*>(c), PT_ERR_STATE, "pt_adaptive_params_get: adaptive sampling is off (pt_set_adaptive)");
    *out = c->adaptive.prm;
    return PT_OK;
}

int pt_render_adaptive(pt_ctx* c, uint32_t rounds)
{
    return guarded(c, "pt_render_adaptive", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    if (!c->adaptive.set)
        return fail(c, PT_ERR_STATE, "pt_render_adaptive: adaptive sampling is off (pt_set_adaptive)");
    if (!c->haveStatic || !c->haveDynamic || !c->haveCamera)
        return fail(c, PT_ERR_STATE, "pt_render_adaptive: scene (static + dynamic) and camera must be set first");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensureAdaptive(c);
    if (rc)
        return rc;
    const pt_adaptive_params& prm = c->adaptive.prm;
    const uint32_t W = c->cfg.width, H = c->cfg.height, bX = adaptiveBlocksX(c), nB = adaptiveBlocks(c);
    float4* const accum = c->accum;
    std::vector<pt_rect> rects;
    for (uint32_t r = 0; (rounds == 0 || r < rounds) && c->spp < prm.max_samples; r++) {
        const uint32_t S = c->spp;
        rects.clear();
        for (uint32_t b = 0; b < nB; b++) // (no samples yet: every block, whatever the read-back area holds)
            if (S == 0 || c->adaptive.buf->back.p[b]) {
                const uint32_t x = (b % bX) * 8u, y = (b / bX) * 8u;
                rects.push_back({ x, y, std::min(x + 8u, W), std::min(y + 8u, H) });
            }
        if (rects.empty())
            break;
        const uint32_t h = std::min(S == 0 ? prm.min_samples : prm.round_samples, prm.max_samples - S) / 2u;
        const auto t0 = std::chrono::steady_clock::now();
        if ((rc = installPixelRects(c, rects.data(), (uint32_t)rects.size())))
            break;
        const bool changed = !c->queuesReady; // (the same list as the one installed costs nothing)
        if ((rc = ensureQueues(c)))
            break;
        if (changed) {
            c->adaptive.timing[2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            c->adaptive.timing[3] += 1.0;
        }
        for (int half = 0; half < 2 && !rc; half++) { // sample indices base + S .. + h - 1 into A, the next h into B
            c->accum = c->adaptive.buf->half[half].p;
            rc = renderSamples(c, h);
        }
        c->accum = accum;
        if (rc) { // (the halves hold part of a round: pt_clear and render again, as after any failed pt_render)
            c->spp = S;
            break;
        }
        if ((rc = evaluateAdaptive(c, 2u * h, S + 2u * h)))
            break;
        c->adaptive.stats.rounds++;
    }
    const int whole = installPixelRects(c, nullptr, 0); // the context owns the whole frame again: guides, denoiser and history see no tiles
    return rc ? rc : whole;
    });
}

int pt_adaptive_stats_get(pt_ctx* c, pt_adaptive_stats* out)
{
    if (!c || !out)
        return PT_ERR_INVALID;
    if (!c->adaptive.set)
        return fail(c, PT_ERR_STATE, "pt_adaptive_stats_get: adaptive sampling is off (pt_set_adaptive)");
    *out = c->adaptive.stats;
    return PT_OK;
}

int pt_read_adaptive(pt_ctx* c, float* A, float* B, uint32_t* counts, float* error, float* block_error)
{
    if (!c)
        return PT_ERR_INVALID;
    if (!c->adaptive.set)
        return fail(c, PT_ERR_STATE, "pt_read_adaptive: adaptive sampling is off (pt_set_adaptive)");
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = ensureAdaptive(c))
        return rc;
    const pt_ctx::Adaptive::Buffers& b = *c->adaptive.buf;
    HIPCHK(c, b.half[0].copyTo(A, c->stream));
    HIPCHK(c, b.half[1].copyTo(B, c->stream));
    HIPCHK(c, b.counts.copyTo(counts, c->stream));
    HIPCHK(c, b.error.copyTo(error, c->stream));
    HIPCHK(c, b.blockError.read(block_error, c->stream));
    return PT_OK;
}

int pt_write_adaptive(pt_ctx* c, const float* A, const float* B, const uint32_t* counts)
{
    return guarded(c, "pt_write_adaptive", [&]() -> int {
    if (!c || !A || !B || !counts)
        return PT_ERR_INVALID;
    if (!c->adaptive.set)
        return fail(c, PT_ERR_STATE, "pt_write_adaptive: adaptive sampling is off (pt_set_adaptive)");
    const uint32_t W = c->cfg.width, H = c->cfg.height;
    uint32_t most = 0;
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const uint32_t n = counts[(size_t)y * W + x];
            if (n != counts[(size_t)(y & ~7u) * W + (x & ~7u)])
                return fail(c, PT_ERR_INVALID, "pt_write_adaptive: counts differ within the 8 x 8 block of pixel (%u, %u)", x, y);
            if ((n & 1u) || n > c->adaptive.prm.max_samples)
                return fail(c, PT_ERR_INVALID, "pt_write_adaptive: count %u at pixel (%u, %u) (even, <= max_samples = %u)", n, x, y, c->adaptive.prm.max_samples);
            most = std::max(most, n);
        }
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = ensureAdaptive(c))
        return rc;
    pt_ctx::Adaptive::Buffers& b = *c->adaptive.buf;
    HIPCHK(c, b.half[0].copyFrom(A, c->stream));
    HIPCHK(c, b.half[1].copyFrom(B, c->stream));
    HIPCHK(c, b.counts.copyFrom(counts, c->stream));
    return evaluateAdaptive(c, 0, most); // (synchronises: the caller's arrays are free again)
    });
}

void* pt_adaptive_device_ptr(pt_ctx* c, int which)
{
    if (!c || !c->adaptive.buf)
        return nullptr;
    switch (which) {
    case 0: return c->adaptive.buf->half[0].p;
    case 1: return c->adaptive.buf->half[1].p;
    case 2: return c->adaptive.buf->counts.p;
    case 3: return c->adaptive.buf->error.p;
    default: return nullptr;
    }
}

int pt_debug_adaptive_timing(pt_ctx* c, double out[4])
{
    if (!c || !out)
        return PT_ERR_INVALID;
    std::memcpy(out, c->adaptive.timing, sizeof(c->adaptive.timing));
    return PT_OK;
}

// ---- instance motion (k_guides<1>, k_temporal<true>) --------------------------------------------

namespace {

// The motion records' way to the device, on the render stream: the first `count` of them into a table of at least `capacity` entries (grown behind a
// synchronisation: a guide pass may still read the old one).  The host copy stays with the context.
int uploadMotionRecords(pt_ctx* c, std::vector<MotionRecord>& records, size_t capacity, size_t count)
{
    if (c->motion.records.n < capacity) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, c->motion.records.alloc(capacity));
    }
    c->motion.host = std::move(records);
    if (count)
        HIPCHK(c, hipMemcpyAsync(c->motion.records.p, c->motion.host.data(), count * sizeof(MotionRecord), hipMemcpyHostToDevice, c->stream));
    return PT_OK;
}

// Vertex motion's per-instance tables for the ACTIVE state, made again whenever either setter is called (so their order does not matter): the rows L of
// the world transform each instance had THEN -- from `records`' previous rows where an instance motion is set (withMotion), from the current rows
// otherwise -- and, without an instance motion, identity records (A = t = 0, the current rows).  Host only: nothing of the context changes.
int makeVertexTables(pt_ctx* c, bool withMotion, std::vector<MotionRecord>& records, std::vector<float4>& rows, const char* who)
{
    const pt_ctx::DynamicSet& d = c->dyn[c->active];
    const size_t nInst = d.hostInstances.size();
    if (!withMotion) {
        records.assign(std::max<size_t>(nInst, 1), MotionRecord {});
        for (size_t j = 0; j < nInst; j++)
            records[j].p0 = d.hostInstances[j].r0, records[j].p1 = d.hostInstances[j].r1, records[j].p2 = d.hostInstances[j].r2;
    }
    std::vector<float> inv(std::max<size_t>(nInst, 1) * 16);
    for (size_t j = 0; j < nInst; j++) {
        const float4 r[3] = { records[j].p0, records[j].p1, records[j].p2 };
        float* m = &inv[j * 16];
        for (int row = 0; row < 3; row++)
            m[row] = r[row].x, m[4 + row] = r[row].y, m[8 + row] = r[row].z, m[12 + row] = r[row].w;
        m[3] = m[7] = m[11] = 0.0f, m[15] = 1.0f;
    }
    rows.assign(std::max<size_t>(nInst, 1) * 3, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    std::string why;
    const int rc = ptconv::vertexMotionRows(inv.data(), (uint32_t)nInst, rows.data(), why);
    if (rc)
        return fail(c, rc, "%s: %s (entries count the state's instances, in the order of its top-level leaves)", who, why.c_str());
    return PT_OK;
}

// ... and their way to the device, on the render stream (the host copies stay with the context)
int commitVertexTables(pt_ctx* c, bool withMotion, std::vector<MotionRecord>& records, std::vector<float4>& rows)
{
    const pt_ctx::DynamicSet& d = c->dyn[c->active];
    int rc;
    if (!withMotion && (rc = uploadMotionRecords(c, records, std::max<size_t>(std::max<size_t>(d.numTopNodes, records.size()), 1), records.size())))
        return rc;
    if (c->vertexMotion.rows.n < rows.size()) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, c->vertexMotion.rows.alloc(rows.size() + rows.size() / 8));
    }
    c->vertexMotion.rowsHost = std::move(rows);
    HIPCHK(c, hipMemcpyAsync(c->vertexMotion.rows.p, c->vertexMotion.rowsHost.data(), c->vertexMotion.rowsHost.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    return PT_OK;
}

// What pt_set_vertex_motion and pt_set_rebuilt_motion make before they touch the device: the tables over the instance motion's records where one is
// set, and the two motion sums
int prepareVertexTables(pt_ctx* c, std::vector<MotionRecord>& records, std::vector<float4>& rows, const char* who)
{
    if (c->motion.set)
        records = c->motion.host;
    const int rc = makeVertexTables(c, c->motion.set, records, rows, who);
    return rc ? rc : c->motionGuides.ensure(c);
}

// What the three motion setters refuse alike, in the order they refuse it; `forget`: the call takes a motion away, which a guide chain does not mind
int motionSetterReady(pt_ctx* c, const char* who, bool forget)
{
    if (const int rc = fixedScheduleOnly(c, who))
        return rc;
    if (!c->haveDynamic)
        return fail(c, PT_ERR_STATE, "%s: no dynamic state is active yet (pt_upload_dynamic)", who);
    if (c->guideSpp != 0)
        return fail(c, PT_ERR_STATE, "%s: %u guide samples are in the sums already -- set or forget the motion right after pt_clear", who, c->guideSpp);
    if (!forget && c->guideChain)
        return fail(c, PT_ERR_UNSUPPORTED, "%s: a guide chain is set (pt_set_guide_chain) -- motion deposits along a chain are not supported", who);
    return PT_OK;
}

// ... and the two that need the previous state: it is still whole in the inactive set
int previousStateThere(pt_ctx* c, const char* who)
{
    if (c->pending >= 0)
        return fail(c, PT_ERR_STATE, "%s: an upload is pending (pt_upload_dynamic_async without its pt_frame_tick): it is overwriting the set that held the previous state", who);
    if (!c->dyn[1 - c->active].used)
        return fail(c, PT_ERR_STATE, "%s: there is no previous state (one pt_frame_tick adopted the only state so far)", who);
    return PT_OK;
}

} // namespace

int pt_set_instance_motion(pt_ctx* c, const float* prevInv, uint32_t nTop)
{
    return guarded(c, "pt_set_instance_motion", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    const bool forget = !prevInv || nTop == 0;
    int rc;
    if ((rc = motionSetterReady(c, "pt_set_instance_motion", forget)))
        return rc;
    if (forget) {
        if (c->vertexMotion.set) { // only the instance part goes: the vertex motion goes on from the current transforms
            HIPCHK(c, hipSetDevice(c->device));
            std::vector<MotionRecord> ident;
            std::vector<float4> rows;
            if ((rc = makeVertexTables(c, false, ident, rows, "pt_set_instance_motion")) || (rc = commitVertexTables(c, false, ident, rows)))
                return rc;
        }
        c->motion.set = false;
        c->motion.moving = 0;
        return PT_OK;
    }
    const pt_ctx::DynamicSet& d = c->dyn[c->active];
    if (nTop != d.numTopNodes)
        return fail(c, PT_ERR_INVALID, "pt_set_instance_motion: %u previous transforms for an active state of %u top-level nodes", nTop, d.numTopNodes);
    HIPCHK(c, hipSetDevice(c->device));
    // one record per INSTANCE (the index the guide pass meets a hit with); the fourth row of an invTransform is (0, 0, 0, 1) to the traversal, and here
    const size_t nInst = d.hostInstances.size();
    std::vector<float> prev(nInst * 16), cur(nInst * 16);
    for (size_t j = 0; j < nInst; j++) {
        const Instance& in = d.hostInstances[j];
        const float* p = prevInv + (size_t)in.topNode * 16;
        const float rows[3][4] = { { in.r0.x, in.r0.y, in.r0.z, in.r0.w }, { in.r1.x, in.r1.y, in.r1.z, in.r1.w }, { in.r2.x, in.r2.y, in.r2.z, in.r2.w } };
        float *pm = &prev[j * 16], *cm = &cur[j * 16];
        for (int col = 0; col < 4; col++) {
            for (int row = 0; row < 3; row++)
                pm[col * 4 + row] = p[col * 4 + row], cm[col * 4 + row] = rows[row][col];
            pm[col * 4 + 3] = cm[col * 4 + 3] = col == 3 ? 1.0f : 0.0f;
        }
    }
    std::vector<MotionRecord> records(std::max<size_t>(nInst, 1));
    uint32_t moving = 0;
    std::string why;
    if ((rc = ptconv::motionRecords(prev.data(), cur.data(), (uint32_t)nInst, nullptr, records.data(), &moving, why)))
        return fail(c, rc, "pt_set_instance_motion: %s (entries count the state's instances, in the order of its top-level leaves)", why.c_str());
    std::vector<float4> rows;
    if (c->vertexMotion.set && (rc = makeVertexTables(c, true, records, rows, "pt_set_instance_motion")))
        return rc;
    if ((rc = c->motionGuides.ensure(c)) || (rc = uploadMotionRecords(c, records, std::max<size_t>(nTop, 1), nInst))) // n_top entries: never fewer than the state has instances
        return rc;
    c->motion.set = true;
    c->motion.moving = moving;
    if (c->vertexMotion.set && (rc = commitVertexTables(c, true, c->motion.host, rows)))
        return rc;
    return PT_OK;
    });
}

int pt_instance_motion(const pt_ctx* c, uint32_t* movingOut)
{
    if (movingOut)
        *movingOut = c && c->motion.set ? c->motion.moving : 0u;
    return c && c->motion.set ? 1 : 0;
}

// ---- vertex motion (k_guides<2>) ------------------------------------------------------------------
int pt_set_vertex_motion(pt_ctx* c, int enable)
{
    return guarded(c, "pt_set_vertex_motion", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    int rc;
    if ((rc = motionSetterReady(c, "pt_set_vertex_motion", !enable)))
        return rc;
    if (!enable) {
        c->vertexMotion.set = false;
        return PT_OK;
    }
    if ((rc = previousStateThere(c, "pt_set_vertex_motion")))
        return rc;
    pt_ctx::DynamicSet &cur = c->dyn[c->active], &old = c->dyn[1 - c->active];
    if (old.staticIndex != cur.staticIndex)
        return fail(c, PT_ERR_UNSUPPORTED, "pt_set_vertex_motion: the previous state was built on another static scene (pt_upload_static_async): a rebuilt tree numbers its triangles anew -- hand the correspondence to pt_set_rebuilt_motion");
    if (old.numTris != cur.numTris)
        return fail(c, PT_ERR_UNSUPPORTED, "pt_set_vertex_motion: the previous state has %u triangles, the active one %u", old.numTris, cur.numTris);
    HIPCHK(c, hipSetDevice(c->device));
    const bool deformed = old.staticVersion != cur.staticVersion && cur.numTris != 0;
    if (deformed && (old.fat.n < cur.numTris || cur.fat.n < cur.numTris))
        return fail(c, PT_ERR_STATE, "pt_set_vertex_motion: the states hold no shading records for %u triangles", cur.numTris);
    std::vector<MotionRecord> records;
    std::vector<float4> rows;
    if ((rc = prepareVertexTables(c, records, rows, "pt_set_vertex_motion")))
        return rc;
    if (deformed) {
        if (c->vertexMotion.fatThen.n < cur.numTris) {
            HIPCHK(c, hipStreamSynchronize(c->stream)); // (growing frees what an earlier guide pass may still read)
            HIPCHK(c, c->vertexMotion.fatThen.alloc(cur.numTris));
        }
        // "then": the inactive set still holds the previous state's records.  Taken on the render stream, which has waited for that set's upload at its tick;
        // the next pt_upload_dynamic_async writes the set on the copy stream after the set's lastUse event, which therefore moves behind this copy.
        HIPCHK(c, hipMemcpyAsync(c->vertexMotion.fatThen.p, old.fat.p, (size_t)cur.numTris * sizeof(TriFat), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipEventRecord(old.lastUse, c->stream));
    }
    if ((rc = commitVertexTables(c, c->motion.set, records, rows)))
        return rc;
    c->vertexMotion.set = true;
    c->vertexMotion.deformed = deformed;
    c->rebuiltMotion.set = false;
    return PT_OK;
    });
}

int pt_vertex_motion(const pt_ctx* c, uint32_t* deformedOut)
{
    if (deformedOut)
        *deformedOut = c && c->vertexMotion.set && c->vertexMotion.deformed ? 1u : 0u;
    return c && c->vertexMotion.set ? 1 : 0;
}

// test hook, no device needed: the rows pt_set_vertex_motion makes of n invTransforms (12 floats each)
int pt_debug_vertex_motion_rows(const float* invTransforms, uint32_t n, float* out12)
{
    return guarded(nullptr, "pt_debug_vertex_motion_rows", [&]() -> int {
    if (!invTransforms || !out12)
        return fail(nullptr, PT_ERR_INVALID, "pt_debug_vertex_motion_rows: null argument");
    std::vector<float4> rows(std::max<size_t>((size_t)n * 3, 1));
    std::string why;
    const int rc = ptconv::vertexMotionRows(invTransforms, n, rows.data(), why);
    if (rc)
        return fail(nullptr, rc, "pt_debug_vertex_motion_rows: %s", why.c_str());
    std::memcpy(out12, rows.data(), (size_t)n * 3 * sizeof(float4));
    return PT_OK;
    });
}

// ---- rebuilt motion (k_gather_then, then k_guides<2>) ---------------------------------------------
namespace {

void launchGatherThen(hipStream_t s, const TriFat* then, uint32_t nThen, const TriFat* now, const uint32_t* map, TriFat* out, uint32_t nNow)
{
    hipLaunchKernelGGL(ptd::k_gather_then, dim3((nNow + 31u) / 32u), dim3(256), 0, s, then, nThen, now, map, out, nNow); // (eight lanes per record)
}

} // namespace

int pt_set_rebuilt_motion(pt_ctx* c, const uint32_t* prevTriangle, uint32_t nTris)
{
    return guarded(c, "pt_set_rebuilt_motion", [&]() -> int {
    if (!c)
        return PT_ERR_INVALID;
    const bool forget = !prevTriangle || nTris == 0;
    int rc;
    if ((rc = motionSetterReady(c, "pt_set_rebuilt_motion", forget)))
        return rc;
    if (forget) {
        c->vertexMotion.set = false;
        return PT_OK;
    }
    if ((rc = previousStateThere(c, "pt_set_rebuilt_motion")))
        return rc;
    pt_ctx::DynamicSet &cur = c->dyn[c->active], &old = c->dyn[1 - c->active];
    if (old.fat.n < old.numTris || cur.fat.n < cur.numTris)
        return fail(c, PT_ERR_STATE, "pt_set_rebuilt_motion: the states hold no shading records for their %u and %u triangles", old.numTris, cur.numTris);
    if (nTris != cur.numTris)
        return fail(c, PT_ERR_INVALID, "pt_set_rebuilt_motion: a map of %u entries for an active state of %u triangles", nTris, cur.numTris);
    HIPCHK(c, hipSetDevice(c->device));
    // the one pass over the map: validated, counted and copied into pinned memory of the context's own, which the asynchronous upload reads (the caller's
    // array is free again when the call returns; the previous call's upload out of that memory has long been read)
    HIPCHK(c, c->rebuiltMotion.stage.read.create());
    HIPCHK(c, c->rebuiltMotion.stage.wait());
    HIPCHK(c, c->rebuiltMotion.stage.reserve((size_t)nTris * sizeof(uint32_t), ((size_t)nTris + nTris / 8) * sizeof(uint32_t)));
    uint32_t* const map = (uint32_t*)c->rebuiltMotion.stage.mem.p;
    uint32_t followed = 0;
    for (uint32_t i = 0; i < nTris; i++) {
        const uint32_t j = prevTriangle[i];
        if (j != PT_NO_PREVIOUS_TRIANGLE) {
            if (j >= old.numTris)
                return fail(c, PT_ERR_INVALID, "pt_set_rebuilt_motion: entry %u names triangle %u of a previous state of %u triangles", i, j, old.numTris);
            followed++;
        }
        map[i] = j;
    }
    std::vector<MotionRecord> records;
    std::vector<float4> rows;
    if ((rc = prepareVertexTables(c, records, rows, "pt_set_rebuilt_motion")))
        return rc;
    if (c->vertexMotion.fatThen.n < nTris || c->rebuiltMotion.map.n < nTris) {
        HIPCHK(c, hipStreamSynchronize(c->stream)); // (growing frees what an earlier guide pass or gather may still read)
        if (c->vertexMotion.fatThen.n < nTris)
            HIPCHK(c, c->vertexMotion.fatThen.alloc(nTris));
        if (c->rebuiltMotion.map.n < nTris)
            HIPCHK(c, c->rebuiltMotion.map.alloc(nTris));
    }
    // "then", through the map: the inactive set still holds the previous state's records, the active set the current ones.  On the render stream, which has
    // waited for both sets' uploads at their ticks and on which every earlier gather has read the map; the inactive set's lastUse moves behind the
    // gather as it moves behind pt_set_vertex_motion's copy, so the next upload into that set may be started at once.
    HIPCHK(c, hipMemcpyAsync(c->rebuiltMotion.map.p, map, (size_t)nTris * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, c->rebuiltMotion.stage.recordRead(c->stream));
    launchGatherThen(c->stream, old.fat.p, old.numTris, cur.fat.p, c->rebuiltMotion.map.p, c->vertexMotion.fatThen.p, nTris);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(old.lastUse, c->stream));
    if ((rc = commitVertexTables(c, c->motion.set, records, rows)))
        return rc;
    c->vertexMotion.set = c->vertexMotion.deformed = c->rebuiltMotion.set = true;
    c->rebuiltMotion.followed = followed;
    return PT_OK;
    });
}

int pt_rebuilt_motion(const pt_ctx* c, uint32_t* followedOut)
{
    const bool set = c && c->vertexMotion.set && c->rebuiltMotion.set;
    if (followedOut)
        *followedOut = set ? c->rebuiltMotion.followed : 0u;
    return set ? 1 : 0;
}

// test hook (tests/test_gpu_rebuilt_motion.py): k_gather_then over host arrays
int pt_debug_gather_records(pt_ctx* c, const void* then128, uint32_t nThen, const void* now128, uint32_t nNow, const uint32_t* map, void* out128)
{
    return guarded(c, "pt_debug_gather_records", [&]() -> int {
    if (!c || !now128 || !map || !out128 || nNow == 0 || (nThen != 0 && !then128))
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<TriFat> dThen, dNow, dOut;
    DevBuf<uint32_t> dMap;
    HIPCHK(c, dThen.alloc(std::max<uint32_t>(nThen, 1)));
    HIPCHK(c, dNow.alloc(nNow));
    HIPCHK(c, dOut.alloc(nNow));
    HIPCHK(c, dMap.alloc(nNow));
    if (nThen)
        HIPCHK(c, hipMemcpy(dThen.p, then128, (size_t)nThen * sizeof(TriFat), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dNow.p, now128, (size_t)nNow * sizeof(TriFat), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dMap.p, map, (size_t)nNow * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(dOut.p, 0, (size_t)nNow * sizeof(TriFat), c->stream));
    launchGatherThen(c->stream, dThen.p, nThen, dNow.p, dMap.p, dOut.p, nNow);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out128, dOut.p, (size_t)nNow * sizeof(TriFat), hipMemcpyDeviceToHost));
    return PT_OK;
    });
}

int pt_read_motion_guides(pt_ctx* c, float* motion, float* prevNormal)
{
    if (!c)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return c->motionGuides.read(c, motion, prevNormal);
}

int pt_write_motion_guides(pt_ctx* c, const float* motion, const float* prevNormal)
{
    if (!c || !motion || !prevNormal)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return c->motionGuides.write(c, motion, prevNormal);
}

void* pt_motion_guides_device_ptr(pt_ctx* c, int which) { return c && (which == 0 || which == 1) ? (void*)c->motionGuides[which] : nullptr; }

// test hook, no device needed: the host conversion behind pt_set_instance_motion, entry by entry (24 floats each)
int pt_debug_motion_records(const float* prevInv, const float* curInv, uint32_t n, float* out24)
{
    return guarded(nullptr, "pt_debug_motion_records", [&]() -> int {
    if (!prevInv || !curInv || !out24)
        return fail(nullptr, PT_ERR_INVALID, "pt_debug_motion_records: null argument");
    std::vector<MotionRecord> records(std::max<uint32_t>(n, 1u));
    std::string why;
    const int rc = ptconv::motionRecords(prevInv, curInv, n, nullptr, records.data(), nullptr, why);
    if (rc)
        return fail(nullptr, rc, "pt_debug_motion_records: %s", why.c_str());
    std::memcpy(out24, records.data(), (size_t)n * sizeof(MotionRecord));
    return PT_OK;
    });
}

int pt_stats_get(pt_ctx* c, pt_stats* out)
{
    if (!c || !out)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    Totals t {};
    HIPCHK(c, hipMemcpy(&t, c->totals.p, sizeof(Totals), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof(*out));
    out->rays_extension = t.raysExtension;
    out->rays_shadow = t.raysShadow;
    out->rays_generated = t.raysGenerated;
    out->shade_hits = t.shadeHits;
    out->deposits = t.deposits;
    out->deposits_shadow = t.depositsShadow;
    out->samples = c->spp;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->evStart, c->evStop) == hipSuccess)
        c->msLastRender = ms;
    else
        (void)hipGetLastError(); // nothing rendered yet: the events were never recorded; do not leave that error for the next call to find
    out->ms_last_render = c->msLastRender;
    out->ms_intersect = c->msIntersect;
    out->ms_shade = c->msShade;
    out->ms_shadow = c->msShadow;
    out->ms_gen = c->msGen;
    out->packet_launches = c->packetLaunches;
    out->gen_launches = c->genLaunches;
    out->bundle_launches = c->bundleLaunches;
    out->ms_packet = c->msPacket;
    out->stack_need = c->dyn[c->active].stackNeed;
    out->folded_instances = c->dyn[c->active].foldedInstances;
    out->entered_instances = c->dyn[c->active].enteredInstances;
    out->batch_samples = c->batchSamples;
    out->probe_batches = c->probeBatches;
    out->first_pass_ext_ratio = (float)c->ratioExt, out->first_pass_shadow_ratio = (float)c->ratioShadowFirst;
    out->general_route = c->dyn[c->active].generalRoute ? 1u : 0u;
    out->team_launches = c->teamLaunches;
    return PT_OK;
}

int pt_stats_reset(pt_ctx* c)
{
    if (!c)
        return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->totals.p, 0, sizeof(Totals), c->stream));
    c->packetLaunches = c->genLaunches = c->bundleLaunches = c->teamLaunches = 0;
    return PT_OK;
}

int pt_profile_kernels(pt_ctx* c, int enable)
{
    if (!c)
        return PT_ERR_INVALID;
    c->profile = enable != 0;
    return PT_OK;
}

int pt_reduce_accum(pt_ctx* c, void* nccl_comm, int root)
{
    if (!c || !nccl_comm)
        return PT_ERR_INVALID;
    // RCCL is bound at first use, and to the copy the process has ALREADY loaded if there is one (the
    // communicator comes from the caller's RCCL; a second copy of the library would not know it).
    // PTAMD_RCCL_LIB names a library explicitly.
    typedef int (*reduce_fn)(const void*, void*, size_t, int, int, int, void*, hipStream_t);
    static reduce_fn reduce = nullptr;
    if (!reduce) {
        void* lib = nullptr;
        if (const char* path = getenv("PTAMD_RCCL_LIB"))
            lib = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
        const char* names[] = { "librccl.so.1", "librccl.so" };
        for (int pass = 0; pass < 2 && !lib; pass++)
            for (const char* n : names)
                if (!lib)
                    lib = dlopen(n, RTLD_NOW | (pass == 0 ? RTLD_NOLOAD : RTLD_GLOBAL));
        if (lib)
            reduce = (reduce_fn)dlsym(lib, "ncclReduce");
        if (!reduce)
            return fail(c, PT_ERR_UNSUPPORTED, "pt_reduce_accum: librccl not found (%s)", dlerror() ? dlerror() : "no ncclReduce symbol");
    }
    HIPCHK(c, hipSetDevice(c->device));
    float* buf = (float*)c->accum; // in place on the root (sendbuff == recvbuff is allowed there), send-only elsewhere
    const size_t count = (size_t)c->cfg.width * c->cfg.height * 4;
#ifdef PT_HAVE_RCCL_HEADER
    constexpr int kFloat = (int)ncclFloat, kSum = (int)ncclSum;
    static_assert(kFloat == 7 && kSum == 0, "the values this file falls back to where rccl.h is absent at build time");
#else
    constexpr int kFloat = 7, kSum = 0; // ncclFloat, ncclSum (rccl.h: ncclDataType_t / ncclRedOp_t)
#endif
    // (all four floats of every pixel travel, although w is unused: the accumulator is one contiguous float4 array and a strided reduce
    // would be three collectives instead of one; 33 MB at 1080p is 0.2 ms on one xGMI link)
    const int rc = reduce(buf, buf, count, kFloat, kSum, root, nccl_comm, c->stream);
    if (rc != 0)
        return fail(c, PT_ERR_HIP, "pt_reduce_accum: ncclReduce returned %d", rc);
    return PT_OK;
}

// ---- kernel-granular hooks ---------------------------------------------------------------------

namespace {

// queue entries read back, as the hooks' callers see them: rays (the pixel is the bits of the origin's w; any output may be null) ...
void unpackRays(const std::vector<float4>& o, const std::vector<float4>& d, float* ox, float* oy, float* oz, float* dx, float* dy, float* dz, uint32_t* pixel)
{
    for (size_t i = 0; i < o.size(); i++) {
        if (ox) ox[i] = o[i].x;
        if (oy) oy[i] = o[i].y;
        if (oz) oz[i] = o[i].z;
        if (dx) dx[i] = d[i].x;
        if (dy) dy[i] = d[i].y;
        if (dz) dz[i] = d[i].z;
        if (pixel)
            std::memcpy(&pixel[i], &o[i].w, 4);
    }
}

// ... and closest-hit records (the primitive is the bits of w; the instance is reported as its top-level leaf)
void unpackHits(const pt_ctx* c, const std::vector<float4>& h, const std::vector<int32_t>& in, pt_hits_soa* hits)
{
    const std::vector<uint32_t>& top = c->dyn[c->active].instanceTopNode;
    for (size_t i = 0; i < h.size(); i++) {
        hits->t[i] = h[i].x, hits->u[i] = h[i].y, hits->v[i] = h[i].z;
        int32_t prim;
        std::memcpy(&prim, &h[i].w, 4);
        hits->prim[i] = prim;
        hits->inst[i] = (in[i] >= 0 && (size_t)in[i] < top.size()) ? (int32_t)top[in[i]] : -1;
    }
}

} // namespace

int pt_intersect(pt_ctx* c, const pt_rays_soa* rays, uint32_t n, int any_hit, pt_hits_soa* hits, uint32_t repeat, float* ms_out)
{
    return guarded(c, "pt_intersect", [&]() -> int {
    if (!c || !rays || !hits || n == 0)
        return PT_ERR_INVALID;
    if (!c->haveStatic || !c->haveDynamic)
        return fail(c, PT_ERR_STATE, "pt_intersect: upload the scene first");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensureSpill(c);
    if (rc)
        return rc;
    std::vector<float4> hO(n), hD(n), hC(n);
    for (uint32_t i = 0; i < n; i++) {
        hO[i] = make_float4(rays->ox[i], rays->oy[i], rays->oz[i], any_hit ? rays->tmax[i] : 0.f);
        hD[i] = make_float4(rays->dx[i], rays->dy[i], rays->dz[i], 0.f); // pixel / flags = 0
        hC[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    DevBuf<float4> dO, dD, dC, dH, dAcc;
    DevBuf<int32_t> dI;
    DevBuf<uint32_t> dOcc;
    DevBuf<Control> dCtl;
    HIPCHK(c, allocPlanes(dO, dD, dC, n));
    HIPCHK(c, dH.alloc(n));
    HIPCHK(c, dI.alloc(n));
    HIPCHK(c, dOcc.alloc(n));
    HIPCHK(c, dAcc.alloc(1));
    HIPCHK(c, dCtl.alloc(1));
    HIPCHK(c, hipMemcpy(dO.p, hO.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dD.p, hD.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dC.p, hC.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(dAcc.p, 0, sizeof(float4), c->stream));
    // sentinels: an entry no lane wrote comes back as t = NaN (closest hit; a miss is +inf) or as verdict -1 (any hit; 0 / 1 otherwise)
    HIPCHK(c, hipMemsetAsync(dH.p, 0xFF, n * sizeof(float4), c->stream));
    HIPCHK(c, hipMemsetAsync(dI.p, 0xFF, n * sizeof(int32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(dOcc.p, 0xFF, n * sizeof(uint32_t), c->stream));
    float msTotal = 0;
    repeat = std::max(repeat, 1u);
    Event e0, e1;
    HIPCHK(c, e0.create(true));
    HIPCHK(c, e1.create(true));
    for (uint32_t r = 0; r < repeat; r++) {
        Control ctl {}; // a control block of its own: n entries in pass 0's queue, cursors at zero
        ctl.extCount[0] = ctl.shadowCount[0] = n;
        HIPCHK(c, hipMemcpyAsync(dCtl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); // `ctl` is a stack object
        TraceArgs a = traceArgsBase(c);
        a.parityShadow = 0;
        a.rayO = dO.p, a.rayD = dD.p, a.rayC = dC.p;
        a.hit = dH.p, a.inst = dI.p, a.accum = AccumView { dAcc.p, nullptr, nullptr, 0u }, a.occluded = dOcc.p;
        a.ctl = dCtl.p, a.pass = 0;
        HIPCHK(c, hipEventRecord(e0, c->stream));
        if (c->dyn[c->active].packetOk && (c->packetUse & 4u))
            launchPacket(c, any_hit != 0, a);
        else
            launchTrace(c, any_hit != 0, a);
        HIPCHK(c, hipEventRecord(e1, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
        msTotal += ms;
    }
    if (any_hit) {
        std::vector<uint32_t> occ(n);
        HIPCHK(c, hipMemcpy(occ.data(), dOcc.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++)
            hits->prim[i] = (int32_t)occ[i];
    } else {
        std::vector<float4> h(n);
        std::vector<int32_t> in(n);
        HIPCHK(c, hipMemcpy(h.data(), dH.p, n * sizeof(float4), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(in.data(), dI.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        unpackHits(c, h, in, hits);
    }
    if (ms_out)
        *ms_out = msTotal / (float)repeat;
    return PT_OK;
    });
}

int pt_gen_rays(pt_ctx* c, uint32_t sample, uint32_t n, float* ox, float* oy, float* oz, float* dx, float* dy, float* dz, uint32_t* pixel)
{
    return guarded(c, "pt_gen_rays", [&]() -> int {
    if (!c || n == 0)
        return PT_ERR_INVALID;
    if (!c->haveCamera)
        return fail(c, PT_ERR_STATE, "pt_gen_rays: set the camera first");
    if (n > c->numOwned)
        return fail(c, PT_ERR_INVALID, "pt_gen_rays: n exceeds the owned pixels");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensureQueues(c);
    if (rc)
        return rc;
    if (n > (c->q0Small ? c->capExt : c->capacity))
        return fail(c, PT_ERR_INVALID, "pt_gen_rays: n exceeds the queue capacity");
    FrameParams fp = frameParams(c, sample);
    launchGen(c, fp, 0, 0, n, 0, 0);
    std::vector<float4> o(n), d(n);
    HIPCHK(c, hipMemcpyAsync(o.data(), c->rays[0].o.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(d.data(), c->rays[0].d.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(c->control.p, 0, sizeof(Control), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unpackRays(o, d, ox, oy, oz, dx, dy, dz, pixel);
    return PT_OK;
    });
}

// The first pass of one batch exactly as pt_render issues it -- camera rays generated inside the traversal kernel where pt_render does
// that, walked as bundles where it does that -- with the rays and the hit records read back in queue order.
int pt_primary_pass(pt_ctx* c, uint32_t sample, uint32_t batch, uint32_t n, float* ox, float* oy, float* oz, float* dx, float* dy, float* dz, uint32_t* pixel,
    pt_hits_soa* hits)
{
    return guarded(c, "pt_primary_pass", [&]() -> int {
    if (!c || !hits || batch == 0 || n == 0)
        return PT_ERR_INVALID;
    if (!c->haveStatic || !c->haveDynamic || !c->haveCamera)
        return fail(c, PT_ERR_STATE, "pt_primary_pass: scene (static + dynamic) and camera must be set first");
    if (parityMode(c) || c->cfg.max_active_rays != 0)
        return fail(c, PT_ERR_UNSUPPORTED, "pt_primary_pass: the fixed schedule only");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensureQueues(c)) || (rc = ensureSpill(c)))
        return rc;
    if (batch > c->planes || n != c->numOwned * batch)
        return fail(c, PT_ERR_INVALID, "pt_primary_pass: batch exceeds samples_in_flight, or n != owned pixels * batch");
    if (c->q0Small)
        return fail(c, PT_ERR_UNSUPPORTED, "pt_primary_pass: the hook queues whole camera rays; this context's first queue holds directions only (pt_config.ext_queue_fraction)");
    if (n > (1u << 26)) // every entry comes back to the host (68 B each): a hook for tests, not for 531 M-entry batches
        return fail(c, PT_ERR_INVALID, "pt_primary_pass: %u entries -- the hook reads everything back, use it on small frames (<= 64 M entries)", n);
    FrameParams fp = batchFrameParams(c, sample, batch);
    BatchPlan plan = planBatch(c, fp, batch);
    plan.derived = false; // (the origins are read back below: the one thing that differs from pt_render's first pass)
    if (plan.fused)
        hipLaunchKernelGGL(k_begin_batch, dim3(1), dim3(64), 0, c->stream, &c->control.p->extCount[0], &c->control.p->generated, n);
    else
        launchGen(c, fp, 0, 0, n, 0, 0);
    launchIntersect(c, 0, 0, plan, fp);
    std::vector<float4> o(n), d(n), h(n);
    std::vector<int32_t> in(n);
    HIPCHK(c, hipMemcpyAsync(o.data(), c->rays[0].o.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(d.data(), c->rays[0].d.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h.data(), c->hitH.p, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(in.data(), c->hitInst.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(c->control.p, 0, sizeof(Control), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    unpackRays(o, d, ox, oy, oz, dx, dy, dz, pixel);
    unpackHits(c, h, in, hits);
    return PT_OK;
    });
}

int pt_shade_batch(pt_ctx* c, pt_shade_batch_io* io)
{
    return guarded(c, "pt_shade_batch", [&]() -> int {
    if (!c || !io || io->n == 0)
        return PT_ERR_INVALID;
    if (!c->haveStatic || !c->haveDynamic)
        return fail(c, PT_ERR_STATE, "pt_shade_batch: upload the scene first");
    if (parityMode(c))
        return fail(c, PT_ERR_UNSUPPORTED, "pt_shade_batch uses the counter PRNG keying");
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t n = io->n;
    // instance index from the reported top-level leaf
    std::vector<int32_t> topToInst;
    const std::vector<uint32_t>& instanceTopNode = c->dyn[c->active].instanceTopNode;
    for (size_t k = 0; k < instanceTopNode.size(); k++) {
        if (instanceTopNode[k] >= topToInst.size())
            topToInst.resize(instanceTopNode[k] + 1, -1);
        topToInst[instanceTopNode[k]] = (int32_t)k;
    }
    std::vector<float4> hO(n), hD(n), hT(n), hH(n);
    std::vector<int32_t> hI(n);
    for (uint32_t i = 0; i < n; i++) {
        float fp, ff, fprim;
        uint32_t px = io->pixel[i], fl = (io->flags[i] & 0xFFu) | (io->bounce[i] << 8);
        int32_t prim = io->prim[i];
        std::memcpy(&fp, &px, 4), std::memcpy(&ff, &fl, 4), std::memcpy(&fprim, &prim, 4);
        hO[i] = make_float4(io->ox[i], io->oy[i], io->oz[i], fp);
        hD[i] = make_float4(io->dx[i], io->dy[i], io->dz[i], ff);
        hT[i] = make_float4(io->thr_r[i], io->thr_g[i], io->thr_b[i], io->in_pdf ? io->in_pdf[i] : 0.f);
        hH[i] = make_float4(prim >= 0 ? io->t[i] : INFINITY, io->u[i], io->v[i], fprim);
        int32_t ti = io->inst[i];
        hI[i] = (ti >= 0 && (size_t)ti < topToInst.size()) ? topToInst[ti] : -1;
        if (prim >= 0 && (hI[i] < 0 || (uint32_t)prim >= c->st->host.numTris))
            return fail(c, PT_ERR_INVALID, "pt_shade_batch: entry %u has an invalid prim/inst", i);
    }
    RayQueueBuf in, out;
    ShadowQueueBuf sh;
    DevBuf<float4> dH, dAcc;
    DevBuf<int32_t> dI;
    DevBuf<uint32_t> dCtl;
    HIPCHK(c, in.alloc(n));
    HIPCHK(c, out.alloc(n));
    HIPCHK(c, sh.alloc(n));
    HIPCHK(c, dH.alloc(n));
    HIPCHK(c, dI.alloc(n));
    HIPCHK(c, dCtl.alloc(5));
    HIPCHK(c, dAcc.alloc((size_t)c->cfg.width * c->cfg.height));
    // per-entry outputs are needed, so every entry is shaded as its own 1-entry queue slice
    HIPCHK(c, hipMemcpy(in.o.p, hO.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(in.d.p, hD.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(in.thr.p, hT.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dH.p, hH.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dI.p, hI.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    FrameParams fp = frameParams(c, io->sample);
    for (uint32_t i = 0; i < n; i++) {
        // pixel-indexed accumulator: clear only the touched pixel
        uint32_t ctl[5] = { 1, 0, 0, 0, 0 }; // inCount, outCount, shadowCount, shadeHits, deposits
        HIPCHK(c, hipMemcpyAsync(dCtl.p, ctl, sizeof(ctl), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(dAcc.p + io->pixel[i], 0, sizeof(float4), c->stream));
        ShadeArgs a {};
        a.sc = c->scene;
        a.fp = fp;
        a.in = { in.o.p + i, in.d.p + i, in.thr.p + i };
        a.hits = { dH.p + i, dI.p + i };
        a.out = { out.o.p + i, out.d.p + i, out.thr.p + i };
        a.shadow = { sh.o.p + i, sh.d.p + i, sh.c.p + i };
        a.accum = AccumView { dAcc.p, nullptr, nullptr, 0u };
        a.inCount = dCtl.p, a.outCount = dCtl.p + 1, a.shadowCount = dCtl.p + 2, a.shadeHits = dCtl.p + 3, a.deposits = dCtl.p + 4;
        a.outCap = a.shadowCap = 0xFFFFFFFFu; // (the hook's own queues: one slot per entry)
        hipLaunchKernelGGL(kShadeKernels[0][generalShading(c) ? 1 : 0][kShadeTile], dim3(1), dim3(64), 0, c->stream, a);
        uint32_t back[4];
        float4 px;
        HIPCHK(c, hipMemcpyAsync(back, dCtl.p, sizeof(back), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&px, dAcc.p + io->pixel[i], sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        io->out_alive[i] = back[1];
        io->shadow_alive[i] = back[2];
        io->radiance[3 * i] = px.x, io->radiance[3 * i + 1] = px.y, io->radiance[3 * i + 2] = px.z;
    }
    std::vector<float4> o(n), d(n), t(n), so(n), sd(n), sc(n);
    HIPCHK(c, hipMemcpy(o.data(), out.o.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(d.data(), out.d.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(t.data(), out.thr.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(so.data(), sh.o.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(sd.data(), sh.d.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(sc.data(), sh.c.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        if (io->out_alive[i]) {
            io->nox[i] = o[i].x, io->noy[i] = o[i].y, io->noz[i] = o[i].z;
            io->ndx[i] = d[i].x, io->ndy[i] = d[i].y, io->ndz[i] = d[i].z;
            io->nthr_r[i] = t[i].x, io->nthr_g[i] = t[i].y, io->nthr_b[i] = t[i].z;
            uint32_t fl;
            std::memcpy(&fl, &d[i].w, 4);
            io->nflags[i] = fl & 0xFFu;
            if (io->npdf)
                io->npdf[i] = t[i].w;
        }
        if (io->shadow_alive[i]) {
            io->sox[i] = so[i].x, io->soy[i] = so[i].y, io->soz[i] = so[i].z, io->slen[i] = so[i].w;
            io->sdx[i] = sd[i].x, io->sdy[i] = sd[i].y, io->sdz[i] = sd[i].z;
            io->sc_r[i] = sc[i].x, io->sc_g[i] = sc[i].y, io->sc_b[i] = sc[i].z;
        }
    }
    return PT_OK;
    });
}

} // extern "C"
