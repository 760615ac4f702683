// Scene conversion of the C-ABI (pt_convert.cpp): the caller's reference-layout arrays (include/ptamd.h) validated and turned into the HBM layouts of
// pt_device.h --
//   * the static part (pt_upload_static / _async, pt_update_geometry, pt_refit_vertices): pair nodes, the SAH-optimal collapse to 4-wide nodes, breadth-first
//     packing and quantisation, leaf cuts, triangle records, refit tables;
//   * the dynamic part (pt_upload_dynamic_async): the top level, the instance table and its routes (copied / folded / general / parked), lights, copy jobs.
// pt_convert.cpp is host code built apart from the kernels: no device call, no kernel, no environment -- what it makes is a function of its arguments.
// ptamd.hip reads the options (convertOptions), hands the latest arrays in, and uploads what comes out.  This header is what the two units share.
// Reference: RayTracer::initBuffersAndTransferStaticData / transferDynamicData, src/raytracer.cpp:201-287, 497-621.
#pragma once
#include "../../include/ptamd.h"
#include "pt_hostdev.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

namespace ptconv {

using namespace ptd;

// Leaf formation inside the collapse (round 5).  The reference's builders stop at <= 3 triangles per leaf with Ct 1.5 / Ci 1.0 tuned for a binary tree
// (src/bvh/bvh_build.cpp:15-18); for THIS traversal a visit of a 4-wide node costs ~105 vector instructions and a triangle test ~35, and a leaf step runs
// to the longest leaf among its lanes.  So the collapse may turn a whole subtree into ONE leaf where that is cheaper:
//   asLeaf[n] = area(n) * (leaf0 + tri * (alpha * tris(n) + (1 - alpha) * cap))      (alpha 1: cost per triangle; alpha 0: every leaf visit costs the cap)
//   asRoot[n] = area(n) * inner + cheapest distribution of its (up to four) slots
// possible only where the subtree's triangle references are one contiguous run (the reference's builders emit leaves depth first: always) of <= cap.
// cap 0 = the leaves are given (rounds 1-4).  PTAMD_LEAF_FORMATION="cap[,inner,leaf0,tri,alpha]" overrides at run time (sweeps).
#ifndef PT_LEAF_CAP
#define PT_LEAF_CAP 0
#endif
struct CollapseCosts {
    uint32_t cap = PT_LEAF_CAP;
    double inner = 105.0, leaf0 = 20.0, tri = 35.0, alpha = 1.0;
    double leaf(uint32_t n) const { return leaf0 + tri * (alpha * (double)n + (1.0 - alpha) * (double)std::max(cap, 1u)); }
};

// Everything that steers a conversion besides the caller's arrays: pt_config, the diagnostic variables of tools/README.md and EXPERIMENTS.md (read once
// per upload call by convertOptions, ptamd.hip), and the limits of the kernels the result is for.
struct ConvertOptions {
    uint32_t flags = 0; // pt_config.flags
    bool parity = false; // pt_config.rng_mode == PT_RNG_LFSR113_PARITY: the reference's routes to the letter
    CollapseCosts costs; // PTAMD_LEAF_FORMATION
    uint32_t maxLeaf = 0; // PTAMD_MAX_LEAF (0: PT_MAX_LEAF, the caller's leaves in parity mode)
    uint64_t bakeBudgetBytes = 2ull << 30; // PTAMD_BAKE_BUDGET_GB: the bytes world-space copies of instances may take
    bool noFoldedInstances = false; // PTAMD_NO_FOLDED_INSTANCES: every entered instance takes the parked route (rounds 2-4)
    int generalRoute = -1; // PTAMD_GENERAL_ROUTE=1 / 0: the general route for every scene with entered instances / never (-1: by the scene)
    bool sequential = false; // PTAMD_BUILD_THREADS=1: everything on the calling thread
    bool hostRecords = true; // the host makes the records (pt_upload_static_async leaves them to the device unless PTAMD_HOST_RECORDS is set)
    bool timing = false; // PTAMD_UPLOAD_TIMING
    bool collapseReport = false; // PTAMD_COLLAPSE_REPORT
    uint32_t stackMax = 0, packetStack = 0, foldTable = 0; // the kernels' traversal stack, packet stack and fold table (pt_trace.h, pt_packet.h)
};

// PTAMD_UPLOAD_TIMING=1: host time of the stages of an upload, one line per call on stderr (diagnostics; tools/r5_upload_timing.sh)
struct StageTimer {
    const char* what;
    bool on;
    std::chrono::steady_clock::time_point t0, last;
    std::string line;
    StageTimer(const char* w, bool timing)
        : what(w)
        , on(timing)
    {
        if (on)
            t0 = last = std::chrono::steady_clock::now();
    }
    void lap(const char* name)
    {
        if (!on)
            return;
        const auto now = std::chrono::steady_clock::now();
        char buf[96];
        snprintf(buf, sizeof buf, " %s %.3f", name, std::chrono::duration<double, std::milli>(now - last).count());
        line += buf;
        last = now;
    }
    ~StageTimer()
    {
        if (on)
            fprintf(stderr, "[ptamd] %s: total %.3f ms;%s\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), line.c_str());
    }
};

// The host half of a static scene -- what the conversion reads and writes (StaticScene, pt_context.h, adds the device's master copies).  The bottom-level
// trees as packed 4-wide nodes, object-space triangles and shading records, converted once per pt_upload_static / pt_update_geometry (buildStaticGeom),
// and the host's mirrors of the caller's arrays.
struct StaticHost {
    std::vector<WideNode> wide; // packed, object space
    std::vector<WideBoxes> boxes; // exact child boxes of every packed node
    std::vector<uint32_t> leafOfs; // [node][child]: offset of a leaf child's first triangle reference in its mesh's run
    std::vector<uint32_t> refTri; // triangle references in leaf order, mesh by mesh -> caller's triangle index
    std::vector<uint32_t> stackNeed; // per packed node
    // what a REFIT needs of the conversion and cannot change: which pair-node child the box of every packed child slot is, which
    // slots are unused (the collapse's split choices and the packing order stay as they are)
    std::vector<uint32_t> kidSrc; // [node][child]: (pair node << 1) | side
    std::vector<uint8_t> kidEmpty; // [node][child]
    std::vector<uint32_t> kidBoxNode; // [node][child]: the same as a caller's node index (k_refit_nodes, pt_bake.h), 0x80000000 | i: extra box i, ~0: unused
    std::vector<TriFat> fat;
    struct Root {
        uint32_t ref; // device reference of the mesh root (a packed node, or a leaf)
        uint32_t nodeBase, numNodes, refBase, numRefs;
        bool bakeable; // its nodes are one run of their own
    };
    std::vector<Root> roots;
    std::vector<int32_t> rootOfNode; // caller's node index -> roots[] slot, -1: not a root
    std::vector<uint32_t> extraRoots; // interior nodes a top-level leaf has named
    uint32_t emptyRef = 0;
    uint64_t version = 0; // drawn from the context's counter (a dynamic set compares the one it holds with the scene's)
    uint64_t topology = 0; // the version of the last buildStaticGeom
    // pt_upload_static_async (a rebuilt tree per frame): the host makes the topology only -- child references, the slots' box sources, the triangle
    // references -- and the device makes the records from the caller's own arrays, as after a refit (k_refit_nodes: exact boxes and quantised planes;
    // k_refit_tris: intersection and shading records).  The host's `wide` planes, `boxes` and `fat` are then not filled in (nothing reads them: a
    // conversion that runs again makes everything anew, refitWideOnHost / buildFat re-make them from the pair boxes where a host-side refit needs them).
    bool deviceMakesRecords = false;

    std::vector<VertexShade> hostVerts;
    std::vector<pt_vertex> rawVerts; // the caller's vertices as last handed in (pt_upload_static / pt_update_geometry)
    std::vector<uint32_t> denseOfNode; // caller's sub-BVH node -> pair node (0xFFFFFFFF: a leaf or a pad)
    uint32_t numDensePairs = 0; // pair nodes [0, numDensePairs) mirror the caller's inner nodes; the rest split leaves of more than kMaxLeafTris
    std::vector<TriIsect> hostTris; // object-space intersection triangles
    std::vector<PairNode> hostBottomNodes; // bottom-level pair nodes
    std::vector<uint32_t> nodeRef; // reference sub-BVH node index -> device child reference
    std::vector<uint32_t> subtreeDepth; // per reference node (roots queried)
    std::vector<TriShade> hostTriShade; // vertex indices + material of every triangle (kept for pt_update_geometry)
    std::vector<pt_material> hostMaterials;
    std::vector<pt_sub_bvh_node> hostSubNodes; // the caller's sub-BVH as uploaded (topology; boxes are replaced by pt_update_geometry)
    uint32_t numVerts = 0;
    uint32_t numRefNodes = 0, numTris = 0;
    bool hostNodeBoxesStale = false; // the boxes in hostSubNodes are older than rawVerts (pt_refit_vertices: the device refitted its own tree, nobody handed nodes in)
    bool hostGeomStale = false; // hostTris / hostVerts / hostBottomNodes' boxes / wide / boxes / fat are older than the caller's latest arrays (a refit
                                // re-makes the device's copies on the device only; the host's are refreshed if the whole conversion ever runs again)
    bool materialBins = false; // the surfaces are of more than one material type: k_shade shades its tiles in material order
    bool refractive = false; // some triangle is REFRACTIVE or BASIC_REFRACTIVE: a guide chain has something to follow (pt_set_guide_chain)
    bool mirror = false; // some triangle is a MIRROR -- PBR, metallic, smoothness > 0.94: with pt_set_guide_reflections a guide chain follows those too
};

// The caller's latest vertices and nodes where they are not rawVerts / hostSubNodes: after a refit on the device (pt_update_geometry) they sit in its
// pinned staging memory (vertices first), and a conversion that runs then takes them over.  Null: the host vectors are the latest.
struct Latest {
    const pt_vertex* verts = nullptr;
    const pt_sub_bvh_node* nodes = nullptr;
};

// What the host-side conversion of one dynamic state produces: the top level, the instance table, the lights,
// and the list of world-space copies the device is to make.  Everything below the top level is static (StaticHost).
struct DynamicHost {
    std::vector<WideNode> topWide; // goes to wide[staticNodes ...]
    std::vector<Instance> instances;
    std::vector<Light> lights;
    std::vector<BakeJob> jobs;
    std::vector<uint32_t> instanceTopNode;
    uint32_t numLights = 0, rootRef = 0, rootRefFolded = 0;
    uint32_t foldedInstances = 0; // instances the per-ray kernels walk without parking (translation + uniform scale, pt_trace.h)
    std::vector<WideNode> instRoots; // their copies of their meshes' root nodes (one slot per instance), stored at instRootBase: the last run of the node array
    std::vector<uint32_t> instRootSrc; // per instance: the packed node its root copy is made from ON THE DEVICE (k_inst_roots), ~0: instRoots[k] holds it already
    std::vector<float4> instFold; // entry 1 + k: (1 / s, w) of instance k; entry 0 and the instances on the general route: the identity
    uint32_t instRootBase = 0;
    uint32_t topSlots = 0; // node slots reserved for the top level (the copies start behind them)
    uint32_t bakedNodes = 0, bakedTris = 0;
    bool packetOk = false, hasInstances = false, generalRoute = false;
    uint32_t stackNeed = 0, enteredInstances = 0, enteredGeneral = 0; // (... of which not a translation + uniform scale)
};

// A refused conversion returns its PT_* code and leaves the message in `why` (the entry point passes it to fail()).  `versions` is the context's
// counter the scene's version is drawn from.  `tm` (pt_upload_static's timer) takes the stages.
int convertStatic(StaticHost& s, const ConvertOptions& o, uint64_t& versions, const pt_vertex* verts, uint32_t nV, const pt_triangle* tris, uint32_t nT,
    const pt_material* mats, uint32_t nM, const pt_sub_bvh_node* nodes, uint32_t nN, StageTimer& tm, std::string& why);
// The dynamic state on top of `s`; a top-level leaf that names an interior node makes it a root of its own, and the static part is converted again.
int convertDynamic(StaticHost& s, const ConvertOptions& o, uint64_t& versions, Latest latest, const pt_emissive_triangle* lights, uint32_t nL,
    const pt_top_bvh_node* topNodes, uint32_t nTop, uint32_t topRoot, DynamicHost& out, std::string& why);

// Instance motion (pt_set_instance_motion, pt_debug_motion_records): entry i of `out` from the previous and the current invTransform of entry i, 16 floats
// each, column-major.  In double, P = inverse(prev) * cur (world now -> world then); the record holds P - I and the translation, rounded to float once, and
// prev's rows 0..2.  Where prev has cur's bits the displacement is written as exact zeros (no inverse involved).  `use` (optional): entries whose byte is 0
// are skipped (their record is all zero).  `moving` (optional): entries whose matrices differ in any bit.  A previous matrix that is singular or not finite
// is refused (PT_ERR_INVALID, `why`).
int motionRecords(const float* prevInv, const float* curInv, uint32_t n, const uint8_t* use, MotionRecord* out, uint32_t* moving, std::string& why);

// Vertex motion (pt_set_vertex_motion, pt_debug_vertex_motion_rows): entry i of `out` is three float4 rows (w = 0), the linear part of the WORLD transform
// whose inverse entry i of `inv` is (16 floats, column-major): the 3 x 3 of inverse(inv) in double, rounded to float once.  It takes an object-space
// displacement of a deformed mesh to world space.  A matrix that is singular or not finite is refused (PT_ERR_INVALID, `why`).
int vertexMotionRows(const float* inv, uint32_t n, float4* out, std::string& why);

// refits on the host (pt_update_geometry before the master copy reached the device, or a conversion after a refit on the device)
void refitPairBoxes(StaticHost& s, const pt_vertex* verts, const pt_sub_bvh_node* nodes, bool onlyExtra);
void refitWideOnHost(StaticHost& s);
void refreshHostGeometry(StaticHost& s, Latest latest);
void buildFat(StaticHost& s);
// boxes of the pair nodes that cut an oversized leaf, 12 floats each (k_refit_nodes: entry (pair - numDensePairs) * 2 + side)
std::vector<float> extraBoxes(const StaticHost& s);

} // namespace ptconv
