// Scene conversion of the C-ABI: the definitions behind pt_convert.h.  Host code alone, built apart from the kernels (ptamd/build.py): no device call,
// no kernel, no environment -- the options arrive in ConvertOptions, the caller's latest arrays as pointers, and tests/test_convert.py holds what comes out
// against recorded digests without a GPU.
#include "pt_convert.h"
#include "../host/parallel.h" // (header only: the worker threads the host library uses, here for the conversion of an upload)
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstring>

namespace ptconv {

// the records travel between this unit and the kernels' one, which another compiler driver builds: their layouts must agree
static_assert(sizeof(float4) == 16 && alignof(float4) == 16 && sizeof(PairNode) == 64 && sizeof(WideNode) == 64 && sizeof(TriFat) == 128 && sizeof(BakeJob) == 128 && sizeof(MotionRecord) == 96,
    "record layouts of pt_device.h");

// a refusal: its PT_* code, and the message formatted as the entry points' fail() formats it
static int refuse(std::string& why, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    why = buf;
    return code;
}

// Collapse the pair-node tree into 4-wide nodes (pt_device.h, WideNode): which descendants of pair node i become the (up to four)
// children of its wide node.  kids[i] describes the same subtree as pair[i], so child references keep their indices; the boxes are the
// exact ones (quantiseWideNode, pt_bake.h, makes the 8-bit planes; the world-space copies of instances are re-fitted from the exact boxes).
#ifndef PT_COLLAPSE_OPTIMAL
#define PT_COLLAPSE_OPTIMAL 1
#endif
struct WideKids {
    float lo[4][3], hi[4][3];
    uint32_t ref[4];
    uint32_t src[4]; // where the box of child k comes from: (pair node << 1) | side -- what a refit re-reads (refitStaticGeom)
    bool empty[4];
};

static std::vector<WideKids> collapseKids(const std::vector<PairNode>& pair, const CollapseCosts& costs, bool sequential)
{
    std::vector<WideKids> out(pair.size());
    const bool pooled = pair.size() >= 4096 && !sequential; // (sequential: everything on the calling thread, as the host library's builders do -- tests compare the two)
    struct Child {
        float lo[3], hi[3];
        uint32_t ref;
        uint32_t src;
    };
    auto childOf = [&pair](const PairNode& n, int side) {
        Child c;
        c.src = ((uint32_t)(&n - pair.data()) << 1) | (uint32_t)side;
        const float* bx = &n.bx.x;
        const float* by = &n.by.x;
        const float* bz = &n.bz.x;
        c.lo[0] = bx[side * 2], c.hi[0] = bx[side * 2 + 1];
        c.lo[1] = by[side * 2], c.hi[1] = by[side * 2 + 1];
        c.lo[2] = bz[side * 2], c.hi[2] = bz[side * 2 + 1];
        c.ref = side ? n.right : n.left;
        return c;
    };
    auto area = [](const Child& c) {
        const float dx = c.hi[0] - c.lo[0], dy = c.hi[1] - c.lo[1], dz = c.hi[2] - c.lo[2];
        return dx >= 0.f && dy >= 0.f && dz >= 0.f ? dx * dy + dy * dz + dz * dx : -1.f;
    };
    // Which descendants become the (up to four) children of the wide node made from pair node i?  The cost of a wide tree is the
    // sum over its inner nodes of the chance a ray visits them ~ their surface area (the leaves are given).  Minimised exactly by
    // dynamic programming over the binary tree (as in Ylitie et al. 2017 for 8-wide trees):
    //   asRoot[n]   = area(n) + min over i of  atMost[left][i] + atMost[right][4 - i]          (n becomes a wide node)
    //   atMost[n][k] = cheapest way to hand subtree n to a parent that has k child slots for it:
    //                  n itself as one child (asRoot[n]), or split between its two children (i and k - i slots)
    // Round 1 opened the child of largest area until four were collected (surface-area greedy): 3 % more inner-node area on the
    // benchmark's meshes (17.67 vs 17.12 / 16.49 vs 16.02 root areas).
#if PT_COLLAPSE_OPTIMAL
    const size_t N = pair.size();
    auto isInner = [&](uint32_t r) { return r != kRefNone && refCount(r) == 0u && refIndex(r) < N; };
    struct Dp {
        double atMost[5]; // [1..4]
        uint8_t split[5]; // 0: the node itself, i: i slots to the left child
        uint8_t rootSplit, done;
        uint8_t asLeaf; // as ONE child the subtree is a leaf of [leafFirst, leafFirst + leafCount)
        uint32_t leafFirst, leafCount; // the subtree's triangle references, when they are one run of <= cap (leafCount 0: not)
    };
    const bool leafCosts = costs.cap > 0u; // the leaves are no longer given: they enter the cost
    auto childArea = [&](const PairNode& n, int side) {
        const Child c = childOf(n, side);
        const double dx = (double)c.hi[0] - c.lo[0], dy = (double)c.hi[1] - c.lo[1], dz = (double)c.hi[2] - c.lo[2];
        return dx >= 0.0 && dy >= 0.0 && dz >= 0.0 ? dx * dy + dy * dz + dz * dx : 0.0;
    };
    std::vector<Dp> dp(N);
    for (Dp& d : dp)
        d.done = 0;
    auto nodeArea = [&](size_t n) { // box of pair node n = union of its two child boxes
        const Child a = childOf(pair[n], 0), b = childOf(pair[n], 1);
        double lo[3], hi[3];
        bool any = false;
        for (const Child* c : { &a, &b }) {
            if (!(c->lo[0] <= c->hi[0]) || c->ref == kRefNone)
                continue;
            for (int ax = 0; ax < 3; ax++) {
                lo[ax] = any ? std::min(lo[ax], (double)c->lo[ax]) : c->lo[ax];
                hi[ax] = any ? std::max(hi[ax], (double)c->hi[ax]) : c->hi[ax];
            }
            any = true;
        }
        if (!any)
            return 0.0;
        const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    };
    {
        // post-order over the subtree below `root` (a stack of its own per caller: subtrees are disjoint, so several can be solved side by side)
        auto solve = [&](size_t root, std::vector<uint32_t>& stack) {
            if (dp[root].done)
                return;
            stack.push_back((uint32_t)root);
            while (!stack.empty()) {
                const uint32_t n = stack.back();
                if (dp[n].done == 2) {
                    stack.pop_back();
                    continue;
                }
                const uint32_t kids[2] = { pair[n].left, pair[n].right };
                if (dp[n].done == 0) { // first visit: children first (done = 1 marks 'on the stack': a cycle cannot loop forever)
                    dp[n].done = 1;
                    for (uint32_t r : kids)
                        if (isInner(r) && dp[refIndex(r)].done == 0)
                            stack.push_back(refIndex(r));
                    continue;
                }
                // children are final (or n sits on a cycle, which upload validation has already excluded): combine.  What either side costs with k slots,
                // looked up once: the child's own table, or one number for every k (a given leaf: what a visit of it costs; nothing where the leaves are given)
                double flat[2][5];
                const double* cost[2];
                for (int side = 0; side < 2; side++) {
                    const uint32_t r = kids[side];
                    if (isInner(r) && dp[refIndex(r)].done == 2) {
                        cost[side] = dp[refIndex(r)].atMost;
                        continue;
                    }
                    const double v = leafCosts && r != kRefNone && refCount(r) >= 1u && refCount(r) <= kMaxLeafTris ? costs.leaf(refCount(r)) * childArea(pair[n], side) : 0.0;
                    for (int k = 1; k <= 4; k++)
                        flat[side][k] = v;
                    cost[side] = flat[side];
                }
                auto costSide = [&](int side, int k) { return cost[side][k]; };
                Dp& d = dp[n];
                // the subtree's triangle references as one run?
                d.asLeaf = 0, d.leafFirst = 0, d.leafCount = 0;
                if (leafCosts) {
                    uint32_t first[2] = { 0, 0 }, cnt[2] = { 0, 0 };
                    for (int side = 0; side < 2; side++) {
                        const uint32_t r = kids[side];
                        if (isInner(r) && dp[refIndex(r)].done == 2)
                            first[side] = dp[refIndex(r)].leafFirst, cnt[side] = dp[refIndex(r)].leafCount;
                        else if (r != kRefNone && refCount(r) >= 1u && refCount(r) <= kMaxLeafTris)
                            first[side] = refIndex(r), cnt[side] = refCount(r);
                    }
                    if (cnt[0] && cnt[1] && cnt[0] + cnt[1] <= costs.cap && (first[0] + cnt[0] == first[1] || first[1] + cnt[1] == first[0]))
                        d.leafFirst = std::min(first[0], first[1]), d.leafCount = cnt[0] + cnt[1];
                }
                double best = 1e300;
                for (int i = 1; i <= 3; i++) {
                    const double v = costSide(0, i) + costSide(1, 4 - i);
                    if (v < best)
                        best = v, d.rootSplit = (uint8_t)i;
                }
                const double ownArea = nodeArea(n);
                d.atMost[1] = (leafCosts ? costs.inner : 1.0) * ownArea + best;
                if (d.leafCount) {
                    const double asLeaf = costs.leaf(d.leafCount) * ownArea;
                    if (asLeaf < d.atMost[1])
                        d.atMost[1] = asLeaf, d.asLeaf = 1;
                }
                d.split[1] = 0;
                for (int k = 2; k <= 4; k++) {
                    d.atMost[k] = d.atMost[1];
                    d.split[k] = 0;
                    for (int i = 1; i < k; i++) {
                        const double v = costSide(0, i) + costSide(1, k - i);
                        if (v < d.atMost[k])
                            d.atMost[k] = v, d.split[k] = (uint8_t)i;
                    }
                }
                d.done = 2;
                stack.pop_back();
            }
        };
        // A rebuilt tree per frame: the subtrees five levels below the roots of large trees are solved on the host library's worker pool, the tops on the
        // calling thread afterwards.  The recurrence has one solution per node whatever the order: the same tree, byte for byte.  (Built once before, on the
        // pool of four threads that parked between loops, and reverted: the NEXT Mesh build on that pool paid 0.9 ms for the 0.2 this saved -- EXPERIMENTS.md.
        // The pool of eight that polls before it parks does not show that.)
        std::vector<uint32_t> tasks;
        if (pooled) {
            std::vector<uint8_t> isChild(N, 0);
            for (size_t n = 0; n < N; n++)
                for (uint32_t r : { pair[n].left, pair[n].right })
                    if (isInner(r))
                        isChild[refIndex(r)] = 1;
            std::vector<uint32_t> level, next;
            for (size_t n = 0; n < N; n++)
                if (!isChild[n])
                    level.push_back((uint32_t)n);
            for (int depth = 0; depth < 5 && !level.empty() && level.size() < 64; depth++) {
                next.clear();
                for (uint32_t n : level)
                    for (uint32_t r : { pair[n].left, pair[n].right })
                        if (isInner(r) && refIndex(r) != n)
                            next.push_back(refIndex(r));
                level.swap(next);
            }
            std::sort(level.begin(), level.end());
            level.erase(std::unique(level.begin(), level.end()), level.end()); // (a shared subtree -- refused by the upload's validation anyway -- is solved once)
            tasks = level;
        }
        if (tasks.size() >= 2) {
            std::atomic<size_t> nextTask { 0 };
            raytracer::WorkerPool& pool = raytracer::WorkerPool::get();
            pool.parallelFor(pool.threads(), 1, [&](size_t, size_t) {
                std::vector<uint32_t> stack;
                for (size_t t; (t = nextTask.fetch_add(1)) < tasks.size();)
                    solve(tasks[t], stack);
            });
        }
        std::vector<uint32_t> stack;
        for (size_t root = 0; root < N; root++)
            solve(root, stack);
    }
#endif
    raytracer::WorkerPool::get().parallelFor(pair.size(), pooled ? 2048 : pair.size() + 1, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; i++) {
        Child kids[4];
        int n = 0;
#if PT_COLLAPSE_OPTIMAL
        {
            struct Item {
                Child c;
                int slots;
            };
            Item todo[8];
            int nt = 0;
            const int ls = dp[i].rootSplit;
            todo[nt++] = { childOf(pair[i], 1), 4 - ls }; // right first: the stack pops the left one first, slot order = tree order
            todo[nt++] = { childOf(pair[i], 0), ls };
            while (nt > 0) {
                const Item it = todo[--nt];
                const uint32_t r = it.c.ref;
                const int sp = isInner(r) && refIndex(r) != i ? dp[refIndex(r)].split[it.slots] : 0;
                if (sp == 0) {
                    kids[n] = it.c;
                    if (isInner(r) && refIndex(r) != i && dp[refIndex(r)].asLeaf) // the whole subtree as ONE leaf: same box, its run of triangles
                        kids[n].ref = makeRef(dp[refIndex(r)].leafFirst, dp[refIndex(r)].leafCount);
                    n++;
                    continue;
                }
                const PairNode& g = pair[refIndex(r)];
                todo[nt++] = { childOf(g, 1), it.slots - sp };
                todo[nt++] = { childOf(g, 0), sp };
            }
        }
#else
        // the two children of the binary node, then (surface-area greedy) the largest inner child is replaced
        // by its own two children until four are collected: the expensive-to-miss boxes are the ones opened up
        kids[n++] = childOf(pair[i], 0);
        kids[n++] = childOf(pair[i], 1);
        while (n < 4) {
            int best = -1;
            float bestArea = -1.f;
            for (int k = 0; k < n; k++) {
                const uint32_t r = kids[k].ref;
                if (r != kRefNone && refCount(r) == 0u && refIndex(r) < pair.size() && refIndex(r) != i && area(kids[k]) > bestArea) {
                    best = k;
                    bestArea = area(kids[k]);
                }
            }
            if (best < 0)
                break;
            const PairNode& g = pair[refIndex(kids[best].ref)];
            kids[best] = childOf(g, 0);
            kids[n++] = childOf(g, 1);
        }
#endif
        WideKids wk {};
        for (int k = 0; k < 4; k++) {
            wk.empty[k] = k >= n || !(kids[k].lo[0] <= kids[k].hi[0]) || kids[k].ref == kRefNone;
            wk.ref[k] = wk.empty[k] ? kRefNone : kids[k].ref;
            wk.src[k] = k < n ? kids[k].src : 0u;
            for (int a = 0; a < 3; a++) {
                wk.lo[k][a] = wk.empty[k] ? 1.f : kids[k].lo[a];
                wk.hi[k][a] = wk.empty[k] ? -1.f : kids[k].hi[a];
            }
        }
        out[i] = wk;
    }
    });
    return out;
}

// world = inverse(invTransform) by Gauss-Jordan in double; m is column-major (TopBvhNode::invTransform).
// On success w[r][4 + c] holds element (r, c) of the world transform.
static bool invertTransform(const float* m, double w[4][8])
{
    for (int r = 0; r < 4; r++)
        for (int col = 0; col < 4; col++) {
            w[r][col] = m[col * 4 + r];
            w[r][col + 4] = (r == col) ? 1.0 : 0.0;
        }
    for (int col = 0; col < 4; col++) {
        int piv = col;
        for (int r = col + 1; r < 4; r++)
            if (std::fabs(w[r][col]) > std::fabs(w[piv][col]))
                piv = r;
        if (std::fabs(w[piv][col]) < 1e-300)
            return false;
        for (int k = 0; k < 8; k++)
            std::swap(w[piv][k], w[col][k]);
        const double dv = w[col][col];
        for (int k = 0; k < 8; k++)
            w[col][k] /= dv;
        for (int r = 0; r < 4; r++)
            if (r != col) {
                const double f = w[r][col];
                for (int k = 0; k < 8; k++)
                    w[r][k] -= f * w[col][k];
            }
    }
    return true;
}

// ---- the static part of a scene: bottom-level trees, converted once per pt_upload_static / pt_update_geometry -----------------------
// Collapse every mesh tree to 4-wide nodes and pack them breadth-first root by root: the four children of a node get neighbouring
// slots (half the footprint in the 4 MB-per-XCD L2, siblings share 128-byte lines) and a mesh's nodes are ONE contiguous run, which is
// what a world-space copy of an instance (pt_bake.h) is made from.  Roots are the caller's nodes no other node refers to, plus any
// node a top-level leaf has ever named (`extraRoots`).
// pair-node boxes of a refit: the caller's refitted boxes for the pairs that mirror its inner nodes (`onlyExtra`: skipped) and, for the pairs that
// split a leaf of more than kMaxLeafTris triangles (appended children first), the bounds of their triangles
void refitPairBoxes(StaticHost& s, const pt_vertex* verts, const pt_sub_bvh_node* nodes, bool onlyExtra)
{
    std::vector<PairNode>& pair = s.hostBottomNodes;
    if (!onlyExtra)
        for (uint32_t i = 0; i < s.numRefNodes; i++) {
            const uint32_t d = s.denseOfNode[i];
            if (d == 0xFFFFFFFFu)
                continue;
            const uint32_t l = nodes[i].leftChildOrFirstTriangle;
            const pt_sub_bvh_node &L = nodes[l], &R = nodes[l + 1];
            pair[d].bx = make_float4(L.min[0], L.max[0], R.min[0], R.max[0]);
            pair[d].by = make_float4(L.min[1], L.max[1], R.min[1], R.max[1]);
            pair[d].bz = make_float4(L.min[2], L.max[2], R.min[2], R.max[2]);
        }
    if (pair.size() <= s.numDensePairs)
        return;
    auto boxOf = [&](uint32_t ref, V3& lo, V3& hi) {
        lo = mk(FLT_MAX), hi = mk(-FLT_MAX);
        if (refCount(ref) != 0u) {
            for (uint32_t t = refIndex(ref); t < refIndex(ref) + refCount(ref); t++) {
                const TriShade& ts = s.hostTriShade[t];
                for (uint32_t vi : { ts.i0, ts.i1, ts.i2 }) {
                    const V3 p = mk(verts[vi].vertex[0], verts[vi].vertex[1], verts[vi].vertex[2]);
                    lo = mk(fminf(lo.x, p.x), fminf(lo.y, p.y), fminf(lo.z, p.z));
                    hi = mk(fmaxf(hi.x, p.x), fmaxf(hi.y, p.y), fmaxf(hi.z, p.z));
                }
            }
        } else {
            const PairNode& n = pair[refIndex(ref)];
            lo = mk(fminf(n.bx.x, n.bx.z), fminf(n.by.x, n.by.z), fminf(n.bz.x, n.bz.z));
            hi = mk(fmaxf(n.bx.y, n.bx.w), fmaxf(n.by.y, n.by.w), fmaxf(n.bz.y, n.bz.w));
        }
    };
    for (size_t j = s.numDensePairs; j < pair.size(); j++) {
        V3 llo, lhi, rlo, rhi;
        boxOf(pair[j].left, llo, lhi);
        boxOf(pair[j].right, rlo, rhi);
        pair[j].bx = make_float4(llo.x, lhi.x, rlo.x, rhi.x);
        pair[j].by = make_float4(llo.y, lhi.y, rlo.y, rhi.y);
        pair[j].bz = make_float4(llo.z, lhi.z, rlo.z, rhi.z);
    }
}

// the packed 4-wide nodes of a refit on the host: same children in the same slots, new boxes (what k_refit_nodes does on the device)
void refitWideOnHost(StaticHost& s)
{
    const std::vector<PairNode>& pair = s.hostBottomNodes;
    for (size_t q = 0; q < s.wide.size(); q++) {
        float lo[4][3], hi[4][3];
        uint32_t refs[4];
        bool empty[4];
        for (int k = 0; k < 4; k++) {
            empty[k] = s.kidEmpty[q * 4 + k] != 0u;
            refs[k] = s.wide[q].child[k];
            if (empty[k]) {
                for (int a = 0; a < 3; a++)
                    lo[k][a] = 1.f, hi[k][a] = -1.f;
                continue;
            }
            const uint32_t src = s.kidSrc[q * 4 + k];
            const PairNode& n = pair[src >> 1];
            const int side = (int)(src & 1u);
            const float *bx = &n.bx.x, *by = &n.by.x, *bz = &n.bz.x;
            lo[k][0] = bx[side * 2], hi[k][0] = bx[side * 2 + 1];
            lo[k][1] = by[side * 2], hi[k][1] = by[side * 2 + 1];
            lo[k][2] = bz[side * 2], hi[k][2] = bz[side * 2 + 1];
        }
        for (int k = 0; k < 4; k++)
            for (int a = 0; a < 3; a++)
                s.boxes[q].lo[k][a] = lo[k][a], s.boxes[q].hi[k][a] = hi[k][a];
        quantiseWideNode(lo, hi, refs, empty, s.emptyRef, &s.wide[q]);
    }
}

// The host's mirrors from the caller's arrays as last handed in (a refit re-makes the device's records on the device and leaves these behind): pair-node
// boxes, the packed nodes, hostTris / hostVerts.
// the caller's node boxes recomputed from the latest vertices (what refitBVH leaves, reference src/bvh/refit_bvh.cpp:6-34): after a refit on
// the device alone nobody handed refitted nodes in.  Children lie after their parent (validated at upload): one reverse sweep.
static void refitHostNodeBoxes(StaticHost& s)
{
    const pt_vertex* verts = s.rawVerts.data();
    std::vector<pt_sub_bvh_node>& nodes = s.hostSubNodes;
    for (size_t i = nodes.size(); i-- > 0;) {
        pt_sub_bvh_node& n = nodes[i];
        float lo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, hi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
        if (n.triangleCount != 0) {
            for (uint32_t t = n.leftChildOrFirstTriangle; t < n.leftChildOrFirstTriangle + n.triangleCount; t++) {
                const TriShade& ts = s.hostTriShade[t];
                for (uint32_t vi : { ts.i0, ts.i1, ts.i2 })
                    for (int a = 0; a < 3; a++)
                        lo[a] = fminf(lo[a], verts[vi].vertex[a]), hi[a] = fmaxf(hi[a], verts[vi].vertex[a]);
            }
        } else {
            if (s.denseOfNode[i] == 0xFFFFFFFFu)
                continue; // an unused pad
            const pt_sub_bvh_node &L = nodes[n.leftChildOrFirstTriangle], &R = nodes[n.leftChildOrFirstTriangle + 1];
            for (int a = 0; a < 3; a++)
                lo[a] = fminf(L.min[a], R.min[a]), hi[a] = fmaxf(L.max[a], R.max[a]);
        }
        for (int a = 0; a < 3; a++)
            n.min[a] = lo[a], n.max[a] = hi[a];
    }
    s.hostNodeBoxesStale = false;
}

void refreshHostGeometry(StaticHost& s, Latest latest)
{
    if (!s.hostGeomStale)
        return;
    if (s.hostNodeBoxesStale) { // (rawVerts is current then: pt_refit_vertices keeps it so)
        refitHostNodeBoxes(s);
        refitPairBoxes(s, s.rawVerts.data(), s.hostSubNodes.data(), false);
        if (s.wide.size() == s.kidEmpty.size() / 4)
            refitWideOnHost(s);
    }
    const pt_vertex* verts = latest.verts ? latest.verts : s.rawVerts.data();
    if (latest.verts) {
        refitPairBoxes(s, verts, latest.nodes, false);
        if (s.wide.size() == s.kidEmpty.size() / 4)
            refitWideOnHost(s);
    }
    auto P = [&](uint32_t vi) { return mk(verts[vi].vertex[0], verts[vi].vertex[1], verts[vi].vertex[2]); };
    for (size_t t = 0; t < s.hostTriShade.size(); t++) {
        const TriShade& ts = s.hostTriShade[t];
        const V3 v0 = P(ts.i0);
        const V3 e1 = P(ts.i1) - v0, e2 = P(ts.i2) - v0; // shapes.cl:37-38
        s.hostTris[t].a = make_float4(v0.x, v0.y, v0.z, e1.x);
        s.hostTris[t].b = make_float4(e1.y, e1.z, e2.x, e2.y);
        s.hostTris[t].c = make_float4(e2.z, 0.f, 0.f, 0.f);
    }
    for (size_t v = 0; v < s.numVerts; v++) {
        s.hostVerts[v].n_u = make_float4(verts[v].normal[0], verts[v].normal[1], verts[v].normal[2], verts[v].texCoord[0]);
        s.hostVerts[v].v_pad = make_float4(verts[v].texCoord[1], 0.f, 0.f, 0.f);
    }
    if (latest.verts) { // the host vectors take the latest arrays over (the staging memory is rewritten by the next refit)
        s.rawVerts.assign(verts, verts + s.numVerts);
        s.hostSubNodes.assign(latest.nodes, latest.nodes + s.numRefNodes);
    }
    s.hostGeomStale = false;
}

// shading records of the caller's triangles: one 128-byte line per triangle (TriFat, pt_device.h)
void buildFat(StaticHost& s)
{
    s.fat.resize(s.hostTriShade.size());
    for (size_t t = 0; t < s.hostTriShade.size(); t++) {
        const TriShade& ts = s.hostTriShade[t];
        const VertexShade &a0 = s.hostVerts[ts.i0], &a1 = s.hostVerts[ts.i1], &a2 = s.hostVerts[ts.i2];
        const TriIsect& ti = s.hostTris[t];
        TriFat f {};
        f.n0u = a0.n_u, f.n1u = a1.n_u, f.n2u = a2.n_u;
        float mbits;
        std::memcpy(&mbits, &ts.material, 4);
        f.vvvm = make_float4(a0.v_pad.x, a1.v_pad.x, a2.v_pad.x, mbits);
        f.e1e = make_float4(ti.a.w, ti.b.x, ti.b.y, ti.b.z); // edge1.xyz, edge2.x
        f.e2v = make_float4(ti.b.w, ti.c.x, ti.a.x, ti.a.y); // edge2.yz, v0.xy
        float m[12]; // the caller's 48-byte material record: colour (16 B), parameters (16 B), type (+ padding)
        std::memcpy(m, &s.hostMaterials[ts.material], sizeof m);
        f.v0c = make_float4(ti.a.z, m[0], m[1], m[2]);
        f.mat = make_float4(m[4], m[5], m[6], m[8]);
        s.fat[t] = f;
    }
}

static void buildStaticGeom(StaticHost& s, const ConvertOptions& o, uint64_t& versions, Latest latest, bool deviceMakesRecords)
{
    StageTimer tm("buildStaticGeom", o.timing);
    s.deviceMakesRecords = deviceMakesRecords;
    refreshHostGeometry(s, latest);
    tm.lap("refreshHostGeometry");
    const uint32_t nN = s.numRefNodes, nT = s.numTris;
    const std::vector<WideKids> kids = collapseKids(s.hostBottomNodes, o.costs, o.sequential);
    tm.lap("collapseKids");
    const uint32_t emptyRef = makeRef(nT, 1u); // the all-zero triangle stored right after the caller's triangles (det == 0: never hit)
    std::vector<uint8_t> isChild(nN, 0);
    for (uint32_t i = 0; i < nN; i++) {
        const pt_sub_bvh_node& n = s.hostSubNodes[i];
        const uint32_t l = n.leftChildOrFirstTriangle;
        if (n.triangleCount == 0 && s.nodeRef[i] != kRefNone && (uint64_t)l + 1 < nN)
            isChild[l] = isChild[l + 1] = 1;
    }
    std::vector<uint32_t> rootNodes;
    for (uint32_t i = 0; i < nN; i++)
        if (s.nodeRef[i] != kRefNone && (!isChild[i] || std::find(s.extraRoots.begin(), s.extraRoots.end(), i) != s.extraRoots.end()))
            rootNodes.push_back(i);
    s.wide.clear(), s.leafOfs.clear(), s.refTri.clear(), s.roots.clear(), s.kidSrc.clear(), s.kidEmpty.clear(), s.kidBoxNode.clear();
    std::vector<uint32_t> pairLeft(s.numDensePairs, 0u); // pair node -> the caller's node that is its left child
    for (uint32_t i = 0; i < nN; i++)
        if (s.denseOfNode[i] != 0xFFFFFFFFu)
            pairLeft[s.denseOfNode[i]] = s.hostSubNodes[i].leftChildOrFirstTriangle;
    s.rootOfNode.assign(nN, -1);
    tm.lap("roots");
    constexpr uint32_t kUnset = 0xFFFFFFFFu;
    std::vector<uint32_t> newIndex(kids.size(), kUnset), order;
    auto isInner = [&](uint32_t r) { return r != kRefNone && refCount(r) == 0u && refIndex(r) < kids.size(); };
    for (uint32_t rn : rootNodes) {
        StaticHost::Root root {};
        const uint32_t rref = s.nodeRef[rn];
        root.nodeBase = (uint32_t)order.size();
        root.refBase = (uint32_t)s.refTri.size();
        root.bakeable = true;
        if (isInner(rref)) {
            if (newIndex[refIndex(rref)] != kUnset) { // reachable from an earlier root too (a top-level leaf names an interior node): shares its run
                root.ref = makeRef(newIndex[refIndex(rref)], 0u);
                root.bakeable = false;
            } else {
                const size_t first = order.size();
                newIndex[refIndex(rref)] = (uint32_t)order.size();
                order.push_back(refIndex(rref));
                for (size_t q = first; q < order.size(); q++) // breadth first
                    for (int k = 0; k < 4; k++) {
                        const uint32_t r = kids[order[q]].ref[k];
                        if (kids[order[q]].empty[k] || !isInner(r))
                            continue;
                        if (newIndex[refIndex(r)] != kUnset) {
                            root.bakeable = false; // shares nodes with another tree: not one run
                            continue;
                        }
                        newIndex[refIndex(r)] = (uint32_t)order.size();
                        order.push_back(refIndex(r));
                    }
                root.ref = makeRef(root.nodeBase, 0u);
            }
            root.numNodes = (uint32_t)order.size() - root.nodeBase;
        } else {
            root.ref = rref; // the mesh is a single leaf
            for (uint32_t k = 0; k < refCount(rref); k++)
                s.refTri.push_back(refIndex(rref) + k);
        }
        // nodes of this run: remapped references, exact boxes, triangle-reference offsets of the leaves
        s.wide.resize(order.size());
        s.boxes.resize(order.size()); // (every slot is written below -- or, where the device makes the records, never read)
        s.leafOfs.resize(order.size() * 4, 0u);
        s.kidSrc.resize(order.size() * 4, 0u);
        s.kidEmpty.resize(order.size() * 4, 1u);
        s.kidBoxNode.resize(order.size() * 4, 0xFFFFFFFFu);
        for (size_t q = root.nodeBase; q < order.size(); q++) { // the leaves' runs in the table of triangle references: in node order, one after the other
            const WideKids& wk = kids[order[q]];
            for (int k = 0; k < 4; k++)
                if (!wk.empty[k] && !isInner(wk.ref[k])) {
                    s.leafOfs[q * 4 + k] = (uint32_t)s.refTri.size() - root.refBase;
                    for (uint32_t t = 0; t < refCount(wk.ref[k]); t++)
                        s.refTri.push_back(refIndex(wk.ref[k]) + t);
                }
        }
        // ... everything else per node on its own (the quantiser is most of a conversion's time): the host library's worker threads take ranges of them
        raytracer::WorkerPool::get().parallelFor(order.size() - root.nodeBase, 512, [&](size_t q0, size_t q1) {
            for (size_t q = root.nodeBase + q0; q < root.nodeBase + q1; q++) {
                const WideKids& wk = kids[order[q]];
                uint32_t refs[4];
                for (int k = 0; k < 4; k++) {
                    s.kidSrc[q * 4 + k] = wk.src[k], s.kidEmpty[q * 4 + k] = wk.empty[k] ? 1u : 0u;
                    if (!wk.empty[k]) { // the caller's node whose box this slot takes: the left / right child of the node its pair mirrors
                        const uint32_t pr = wk.src[k] >> 1, side = wk.src[k] & 1u;
                        s.kidBoxNode[q * 4 + k] = pr < s.numDensePairs ? pairLeft[pr] + side : (0x80000000u | ((pr - s.numDensePairs) * 2u + side));
                    }
                    refs[k] = wk.empty[k] ? emptyRef : (isInner(wk.ref[k]) ? makeRef(newIndex[refIndex(wk.ref[k])], 0u) : wk.ref[k]);
                    if (!deviceMakesRecords)
                        for (int a = 0; a < 3; a++)
                            s.boxes[q].lo[k][a] = wk.lo[k][a], s.boxes[q].hi[k][a] = wk.hi[k][a];
                }
                if (deviceMakesRecords) { // the references only: k_refit_nodes gathers the boxes and makes the planes (uploadStaticGeom)
                    WideNode w {};
                    for (int k = 0; k < 4; k++)
                        w.child[k] = refs[k];
                    s.wide[q] = w;
                } else {
                    quantiseWideNode(wk.lo, wk.hi, refs, wk.empty, emptyRef, &s.wide[q]);
                }
            }
        });
        root.numRefs = (uint32_t)s.refTri.size() - root.refBase;
        s.rootOfNode[rn] = (int32_t)s.roots.size();
        s.roots.push_back(root);
    }
    // worst-case number of pending stack entries below every packed node: visiting a node can leave all its other children on the
    // stack (children are visited nearest first, so any order can occur: the bound takes the deepest child first).  Inside a run the
    // children sit after their parent; a child that lies in ANOTHER run (a top-level leaf named an interior node, whose subtree an
    // earlier root had packed already) lies in an earlier one.  So: run by run in ascending order, each run in reverse -- every child
    // is final when its parent is reached.  (One reverse sweep over everything took 0 for the shared children: too small a bound.)
    tm.lap("pack");
    s.stackNeed.assign(s.wide.size(), 0u);
    for (const StaticHost::Root& root : s.roots)
        for (size_t q = (size_t)root.nodeBase + root.numNodes; q-- > root.nodeBase;) {
            if (refCount(root.ref) != 0u || refIndex(root.ref) != root.nodeBase)
                break; // no run of its own (a single leaf, or the root sits inside an earlier run)
            uint32_t n = 0, deepest = 0;
            for (uint32_t r : s.wide[q].child) {
                if (r == emptyRef)
                    continue;
                n++;
                if (refCount(r) == 0u && refIndex(r) < s.wide.size())
                    deepest = std::max(deepest, s.stackNeed[refIndex(r)]);
            }
            s.stackNeed[q] = (n > 0 ? n - 1 : 0u) + deepest;
        }
    if (o.collapseReport) { // what the collapse made: packed nodes, leaves by size (tools / sweeps of PTAMD_LEAF_FORMATION)
        uint64_t hist[kMaxLeafTris + 1] = {}, leaves = 0, refs = 0, used = 0;
        for (const WideNode& w : s.wide)
            for (uint32_t r : w.child)
                if (r != emptyRef) {
                    used++;
                    if (refCount(r) >= 1u && refCount(r) <= kMaxLeafTris)
                        hist[refCount(r)]++, leaves++, refs += refCount(r);
                }
        const CollapseCosts& k = o.costs;
        fprintf(stderr, "[ptamd] collapse: cap %u costs %.0f/%.0f/%.0f alpha %.2f -> %zu wide nodes, %.2f used slots per node, %llu leaves, %.2f triangles per leaf; by size:", k.cap, k.inner,
            k.leaf0, k.tri, k.alpha, s.wide.size(), s.wide.empty() ? 0.0 : (double)used / (double)s.wide.size(), (unsigned long long)leaves, leaves ? (double)refs / (double)leaves : 0.0);
        for (uint32_t n = 1; n <= kMaxLeafTris; n++)
            if (hist[n])
                fprintf(stderr, " %u:%llu", n, (unsigned long long)hist[n]);
        fprintf(stderr, "\n");
    }
    tm.lap("stackNeed");
    if (deviceMakesRecords)
        s.fat.resize(s.hostTriShade.size()); // (its size is what the dynamic sets allocate by)
    else
        buildFat(s);
    tm.lap("buildFat");
    s.emptyRef = emptyRef;
    s.version = ++versions;
    s.topology = s.version;
}

int convertStatic(StaticHost& s, const ConvertOptions& o, uint64_t& versions, const pt_vertex* verts, uint32_t nV, const pt_triangle* tris, uint32_t nT,
    const pt_material* mats, uint32_t nM, const pt_sub_bvh_node* nodes, uint32_t nN, StageTimer& tm, std::string& why)
{
    if (!verts || !tris || !mats || !nodes || nV == 0 || nT == 0 || nM == 0 || nN == 0)
        return refuse(why, PT_ERR_INVALID, "pt_upload_static: empty or null scene array");
    if (nT > kRefIndexMask || nN > kRefIndexMask)
        return refuse(why, PT_ERR_UNSUPPORTED, "pt_upload_static: more than 2^27 triangle references or nodes");
    // ---- validate: every index in range, children after their parent (rules out cycles) -----
    for (uint32_t t = 0; t < nT; t++) {
        if (tris[t].indices[0] >= nV || tris[t].indices[1] >= nV || tris[t].indices[2] >= nV)
            return refuse(why, PT_ERR_INVALID, "triangle %u: vertex index out of range", t);
        if (tris[t].materialIndex >= nM)
            return refuse(why, PT_ERR_INVALID, "triangle %u: material index out of range", t);
    }
    // An inner node whose children do not lie strictly after it is an unused pad (the reference's pair
    // allocator leaves one next to every root); pads may not be referenced.
    auto isPad = [&](uint32_t i) {
        const uint32_t l = nodes[i].leftChildOrFirstTriangle;
        return nodes[i].triangleCount == 0 && (l <= i || (uint64_t)l + 1 >= nN);
    };
    for (uint32_t i = 0; i < nN; i++) {
        const pt_sub_bvh_node& n = nodes[i];
        if (n.triangleCount != 0 && (uint64_t)n.leftChildOrFirstTriangle + n.triangleCount > nT)
            return refuse(why, PT_ERR_INVALID, "sub-BVH leaf %u: triangle range out of bounds", i);
    }

    tm.lap("validate");
    // ---- triangles / vertices / materials ------------------------------------------------------
    std::vector<TriIsect> hTris(nT);
    std::vector<TriShade> hShade(nT);
    auto P = [&](uint32_t vi) { return mk(verts[vi].vertex[0], verts[vi].vertex[1], verts[vi].vertex[2]); };
    for (uint32_t t = 0; t < nT; t++) {
        const V3 v0 = P(tris[t].indices[0]);
        const V3 e1 = P(tris[t].indices[1]) - v0, e2 = P(tris[t].indices[2]) - v0; // shapes.cl:37-38
        hTris[t].a = make_float4(v0.x, v0.y, v0.z, e1.x);
        hTris[t].b = make_float4(e1.y, e1.z, e2.x, e2.y);
        hTris[t].c = make_float4(e2.z, 0.f, 0.f, 0.f);
        hShade[t] = { tris[t].indices[0], tris[t].indices[1], tris[t].indices[2], tris[t].materialIndex };
    }
    std::vector<VertexShade> hVerts(nV);
    for (uint32_t v = 0; v < nV; v++) {
        hVerts[v].n_u = make_float4(verts[v].normal[0], verts[v].normal[1], verts[v].normal[2], verts[v].texCoord[0]);
        hVerts[v].v_pad = make_float4(verts[v].texCoord[1], 0.f, 0.f, 0.f);
    }

    tm.lap("records");
    // ---- pair nodes ----------------------------------------------------------------------------
    std::vector<uint32_t> dense(nN, 0xFFFFFFFFu);
    uint32_t numInner = 0;
    for (uint32_t i = 0; i < nN; i++)
        if (nodes[i].triangleCount == 0 && !isPad(i))
            dense[i] = numInner++;
    std::vector<PairNode> hNodes(numInner);
    auto triBox = [&](uint32_t t, V3& lo, V3& hi) {
        for (int k = 0; k < 3; k++) {
            const V3 p = P(tris[t].indices[k]);
            lo = mk(fminf(lo.x, p.x), fminf(lo.y, p.y), fminf(lo.z, p.z));
            hi = mk(fmaxf(hi.x, p.x), fmaxf(hi.y, p.y), fmaxf(hi.z, p.z));
        }
    };
    // Leaves larger than `maxLeaf` triangles become a small subtree over their triangle range.  Round 5: maxLeaf = 2, not the 30 a reference can
    // address -- the reference's builders stop at <= 3 triangles (src/bvh/bvh_build.cpp:15: 60 % of the benchmark meshes' leaves hold two, 39 % three),
    // and a leaf step of the traversal kernels runs to the LONGEST leaf among its lanes: with the three-triangle leaves cut into 1 + 2 at the cheaper
    // of the two places (the pieces go into free slots of the 4-wide nodes where there are any: 27 k -> 37 k nodes for 82 k triangles) every leaf step
    // is two trips at most.  Measured on the benchmark (one box, A / B / A): 10 868 -> 11 012 -> 10 832 Mrays/s (+1.5 %; leaves of ONE triangle: -0.7 %;
    // merging subtrees into leaves of up to 4 / 6 / 8 instead: -1.0 / -3.3 / -3.4 %, profiles/round5/r5_tree_shape.txt).  Parity mode keeps the caller's
    // leaves (its order of triangle tests is the reference's).  PTAMD_MAX_LEAF=n overrides (diagnostics).
#ifndef PT_MAX_LEAF
#define PT_MAX_LEAF 2
#endif
    const uint32_t maxLeaf = o.maxLeaf ? o.maxLeaf : o.parity ? kMaxLeafTris : std::min<uint32_t>(PT_MAX_LEAF, kMaxLeafTris);
    struct Range {
        uint32_t first, count;
    };
    auto rangeBox = [&](Range r, V3& lo, V3& hi) {
        lo = mk(FLT_MAX), hi = mk(-FLT_MAX);
        for (uint32_t t = 0; t < r.count; t++)
            triBox(r.first + t, lo, hi);
    };
    auto halfArea = [](V3 lo, V3 hi) {
        const float dx = hi.x - lo.x, dy = hi.y - lo.y, dz = hi.z - lo.z;
        return dx * dy + dy * dz + dz * dx;
    };
    auto leafRefImpl = [&](auto& leafRef, Range r, V3& lo, V3& hi) -> uint32_t {
        lo = mk(FLT_MAX), hi = mk(-FLT_MAX);
        if (r.count <= maxLeaf) {
            for (uint32_t t = 0; t < r.count; t++)
                triBox(r.first + t, lo, hi);
            return makeRef(r.first, r.count);
        }
        // the range stays in the caller's order (a leaf is a run of it): cut where the two runs' surface-area cost is smallest
        uint32_t half = r.count / 2;
        if (r.count <= 8u) {
            float best = FLT_MAX;
            for (uint32_t cut = 1; cut < r.count; cut++) {
                V3 alo, ahi, blo, bhi;
                rangeBox({ r.first, cut }, alo, ahi);
                rangeBox({ r.first + cut, r.count - cut }, blo, bhi);
                const float cost = halfArea(alo, ahi) * (float)cut + halfArea(blo, bhi) * (float)(r.count - cut);
                if (cost < best)
                    best = cost, half = cut;
            }
        }
        V3 llo, lhi, rlo, rhi;
        const uint32_t l = leafRef(leafRef, { r.first, half }, llo, lhi);
        const uint32_t rr = leafRef(leafRef, { r.first + half, r.count - half }, rlo, rhi);
        PairNode pn {};
        pn.bx = make_float4(llo.x, lhi.x, rlo.x, rhi.x);
        pn.by = make_float4(llo.y, lhi.y, rlo.y, rhi.y);
        pn.bz = make_float4(llo.z, lhi.z, rlo.z, rhi.z);
        pn.left = l;
        pn.right = rr;
        lo = mk(fminf(llo.x, rlo.x), fminf(llo.y, rlo.y), fminf(llo.z, rlo.z));
        hi = mk(fmaxf(lhi.x, rhi.x), fmaxf(lhi.y, rhi.y), fmaxf(lhi.z, rhi.z));
        hNodes.push_back(pn);
        return makeRef((uint32_t)hNodes.size() - 1, 0);
    };
    s.nodeRef.assign(nN, kRefNone);
    for (uint32_t i = 0; i < nN; i++) {
        if (nodes[i].triangleCount != 0) {
            if (nodes[i].triangleCount <= maxLeaf) {
                s.nodeRef[i] = makeRef(nodes[i].leftChildOrFirstTriangle, nodes[i].triangleCount);
            } else {
                V3 lo, hi;
                s.nodeRef[i] = leafRefImpl(leafRefImpl, { nodes[i].leftChildOrFirstTriangle, nodes[i].triangleCount }, lo, hi);
            }
        } else if (dense[i] != 0xFFFFFFFFu) {
            s.nodeRef[i] = makeRef(dense[i], 0);
        }
    }
    for (uint32_t i = 0; i < nN; i++) {
        if (dense[i] == 0xFFFFFFFFu)
            continue;
        const uint32_t l = nodes[i].leftChildOrFirstTriangle;
        const pt_sub_bvh_node& L = nodes[l];
        const pt_sub_bvh_node& R = nodes[l + 1];
        PairNode pn {};
        pn.bx = make_float4(L.min[0], L.max[0], R.min[0], R.max[0]);
        pn.by = make_float4(L.min[1], L.max[1], R.min[1], R.max[1]);
        pn.bz = make_float4(L.min[2], L.max[2], R.min[2], R.max[2]);
        pn.left = s.nodeRef[l];
        pn.right = s.nodeRef[l + 1];
        if (pn.left == kRefNone || pn.right == kRefNone)
            return refuse(why, PT_ERR_INVALID, "sub-BVH node %u: child is an unused pad node", i);
        hNodes[dense[i]] = pn;
    }
    // depth of every subtree (children have larger indices: one reverse sweep), for the stack bound
    s.subtreeDepth.assign(nN, 0);
    for (uint32_t i = nN; i-- > 0;) {
        if (dense[i] == 0xFFFFFFFFu) {
            uint32_t extra = 0;
            for (uint32_t cnt = nodes[i].triangleCount; cnt > maxLeaf; cnt = cnt > 8u ? (cnt + 1) / 2 : cnt - 1) // (the cost-driven cut of a short run may peel one triangle off per level)
                extra++;
            s.subtreeDepth[i] = extra;
        } else {
            const uint32_t l = nodes[i].leftChildOrFirstTriangle;
            s.subtreeDepth[i] = 1 + std::max(s.subtreeDepth[l], s.subtreeDepth[l + 1]);
        }
    }
    if (hNodes.size() > kRefIndexMask)
        return refuse(why, PT_ERR_UNSUPPORTED, "too many BVH nodes");

    tm.lap("pairNodes");
    s.hostTris = std::move(hTris);
    s.hostBottomNodes = std::move(hNodes);
    s.rawVerts.assign(verts, verts + nV);
    s.hostGeomStale = false;
    s.denseOfNode = std::move(dense);
    s.numDensePairs = numInner;
    s.hostTriShade = std::move(hShade);
    s.hostMaterials.assign(mats, mats + nM);
    s.hostSubNodes.assign(nodes, nodes + nN);
    s.hostVerts = std::move(hVerts);
    s.numVerts = nV;
    s.numRefNodes = nN;
    s.numTris = nT;
    s.hostNodeBoxesStale = false;
    {   // material types in use (emissive surfaces end a path in a few instructions: they do not count)
        uint32_t types = 0;
        bool mirror = false;
        for (uint32_t t = 0; t < nT; t++) {
            const char* const record = (const char*)&mats[tris[t].materialIndex];
            uint32_t ty;
            std::memcpy(&ty, record + 32, 4); // the type word of the 48-byte record (Material::typeAndPad.x)
            types |= 1u << std::min(ty, 31u);
            if (ty == (uint32_t)MAT_PBR) { // a MIRROR as k_shade and k_guide_chain<true> read the record: the smoothness float, the metallic byte
                float smoothness;
                std::memcpy(&smoothness, record + 16, 4);
                mirror = mirror || (record[24] != 0 && smoothness > 0.94f); // kMaxSmoothness (pt_shade.h)
            }
        }
        s.mirror = mirror;
        s.refractive = (types & ((1u << MAT_REFRACTIVE) | (1u << MAT_BASIC_REFRACTIVE))) != 0u;
        types &= ~(1u << MAT_EMISSIVE);
        s.materialBins = (types & (types - 1u)) != 0u && (o.flags & PT_FLAG_MATERIAL_BINS) != 0u; // opt-in: measured slower (pt_shade.h)
    }
    s.extraRoots.clear();
    tm.lap("mirrors");
    buildStaticGeom(s, o, versions, Latest {}, !o.hostRecords);
    tm.lap("buildStaticGeom");
    return PT_OK;
}

// boxes of the pair nodes that cut an oversized leaf, in the order k_refit_nodes reads them (entry (pair - numDensePairs) * 2 + side)
std::vector<float> extraBoxes(const StaticHost& s)
{
    std::vector<float> extra;
    for (size_t j = s.numDensePairs; j < s.hostBottomNodes.size(); j++) {
        const PairNode& n = s.hostBottomNodes[j];
        const float b[12] = { n.bx.x, n.by.x, n.bz.x, n.bx.y, n.by.y, n.bz.y, n.bx.z, n.by.z, n.bz.z, n.bx.w, n.by.w, n.bz.w };
        extra.insert(extra.end(), b, b + 12);
    }
    return extra;
}

int convertDynamic(StaticHost& s, const ConvertOptions& o, uint64_t& versions, Latest latest, const pt_emissive_triangle* lights, uint32_t nL,
    const pt_top_bvh_node* topNodes, uint32_t nTop, uint32_t topRoot, DynamicHost& out, std::string& why)
{
    if (!topNodes || nTop == 0 || topRoot >= nTop)
        return refuse(why, PT_ERR_INVALID, "pt_upload_dynamic: bad top-level BVH");
    if (nL > 0 && !lights)
        return refuse(why, PT_ERR_INVALID, "pt_upload_dynamic: null light array");
    // a top-level leaf may name any node of the caller's sub-BVH array; the ones that are not mesh roots become roots of their own
    {
        bool grown = false;
        for (uint32_t i = 0; i < nTop; i++) {
            const pt_top_bvh_node& n = topNodes[i];
            if (!n.isLeaf)
                continue;
            if (n.a >= s.numRefNodes || s.nodeRef[n.a] == kRefNone)
                return refuse(why, PT_ERR_INVALID, "top-level leaf %u: sub-BVH root %u is not a valid node", i, n.a);
            if (s.rootOfNode[n.a] < 0 && std::find(s.extraRoots.begin(), s.extraRoots.end(), n.a) == s.extraRoots.end()) {
                s.extraRoots.push_back(n.a);
                grown = true;
            }
        }
        if (grown)
            buildStaticGeom(s, o, versions, latest, false);
    }
    const uint32_t staticNodes = (uint32_t)s.wide.size();
    const uint32_t staticTris = s.numTris + 1u; // the caller's triangles + the all-zero one
    // ---- instances (one per top-level leaf) and top-level pair nodes (one per top-level inner node)
    std::vector<Instance>& hInst = out.instances;
    hInst.clear();
    std::vector<uint32_t> topRef(nTop, kRefNone); // reference of top node i as a child
    std::vector<int32_t> instRoot; // instance -> roots[] slot
    out.instanceTopNode.clear();
    out.jobs.clear();
    uint32_t numTopInner = 0, maxBottomDepth = 0;
    for (uint32_t i = 0; i < nTop; i++) {
        const pt_top_bvh_node& n = topNodes[i];
        if (n.isLeaf) {
            maxBottomDepth = std::max(maxBottomDepth, s.subtreeDepth[n.a] + 1);
            const StaticHost::Root& root = s.roots[s.rootOfNode[n.a]];
            Instance in {};
            const float* m = n.invTransform; // column-major
            in.r0 = make_float4(m[0], m[4], m[8], m[12]);
            in.r1 = make_float4(m[1], m[5], m[9], m[13]);
            in.r2 = make_float4(m[2], m[6], m[10], m[14]);
            in.rootRef = root.ref;
            in.topNode = i;
            {   // a translation + uniform scale?  (parity mode follows the reference's route to the letter)
                const float a = in.r0.x;
                in.simple = (!o.parity && !(o.flags & PT_FLAG_PARKED_INSTANCES) && a > 0.f && std::isfinite(a) && in.r1.y == a && in.r2.z == a && in.r0.y == 0.f
                                && in.r0.z == 0.f && in.r1.x == 0.f && in.r1.z == 0.f && in.r2.x == 0.f && in.r2.y == 0.f && std::isfinite(in.r0.w) && std::isfinite(in.r1.w)
                                && std::isfinite(in.r2.w))
                    ? 1u : 0u;
            }
            if (hInst.size() >= kSpecialIdle) // (the indices from there on are the markers of pt_device.h)
                return refuse(why, PT_ERR_UNSUPPORTED, "too many instances");
            topRef[i] = makeRef((uint32_t)hInst.size(), kRefSpecial);
            hInst.push_back(in);
            instRoot.push_back(s.rootOfNode[n.a]);
            out.instanceTopNode.push_back(i);
        } else {
            if (n.a >= nTop || n.b >= nTop)
                return refuse(why, PT_ERR_INVALID, "top-level node %u: child out of range", i);
            topRef[i] = makeRef(staticNodes + numTopInner, 0u);
            numTopInner++;
        }
    }
    // node slots of the top level: [the top level with instance references (<= numTopInner nodes) | the same top level for the per-ray kernels, which
    // walk translated + uniformly scaled instances without parking (<= numTopInner)]; the world-space copies start behind them, the instances' root
    // copies (one slot per instance) come last
    const uint32_t foldedBase = staticNodes + numTopInner;
    out.topSlots = 2u * numTopInner;
    // ---- instances copied to world space --------------------------------------------------------------------
    // An instance costs every ray that enters it a transform in and a restore out on top of the traversal proper.  With 288 GB of
    // HBM the instanced geometry of scenes like the benchmark's (12 x 82 k triangles: ~110 MB of nodes and triangles) simply fits
    // as world-space copies, so instances are copied while a byte budget lasts -- single-leaf meshes (a ground quad, an area light)
    // first, they cost almost nothing -- and the rest stay two-level.  (t,u,v) are the same in both spaces (the reference never
    // renormalises the transformed direction, scene.cl:118-121); the traversal kernels map a hit on a copy back to (original
    // triangle, instance).  The copies themselves are made on the device (pt_bake.h); this only lays them out.
    {
        const uint64_t budgetBytes = o.bakeBudgetBytes;
        uint64_t usedBytes = 0;
        uint32_t nextNode = staticNodes + out.topSlots, nextTri = staticTris;
        // Whole trees: ALL of them or none (round 6).  A scene that is partly copied pays for both: every ray runs the kernels that can enter instances,
        // and the copies' bytes push the shared trees out of the caches (432 instances of the 82 k-triangle meshes, 421 copied + 13 entered: 8 481 Mrays/s
        // against 9 089 with all of them entered and 9 017 with all of them copied: profiles/round6/).
        uint64_t allBytes = 0;
        for (uint32_t k = 0; k < hInst.size(); k++) {
            const StaticHost::Root& root = s.roots[instRoot[k]];
            if (refCount(root.ref) == 0u)
                allBytes += (uint64_t)root.numNodes * sizeof(WideNode) + (uint64_t)root.numRefs * sizeof(TriIsect);
        }
        const bool copiesAllowed = !(o.flags & PT_FLAG_NO_BAKED_INSTANCES), wholeTreesFit = allBytes <= budgetBytes;
        auto mayBake = [&](uint32_t instIndex) { // by the mesh alone (the byte budget and the index range are the layout's business, below)
            const StaticHost::Root& root = s.roots[instRoot[instIndex]];
            if (refCount(root.ref) != 0u)
                return true; // the mesh is one leaf
            return wholeTreesFit && root.bakeable && root.numNodes != 0u && !(o.flags & PT_FLAG_TWO_LEVEL_ONLY) && !o.parity; // parity mode follows the reference to the letter
        };
        // the world transforms of the instances that may be copied: a 4 x 4 inversion in double each -- ten thousand instances moved per tick are ten thousand of
        // them: on the host library's worker pool
        struct World {
            double m[12];
            bool ok;
        };
        std::vector<World> world(copiesAllowed ? hInst.size() : 0);
        raytracer::WorkerPool::get().parallelFor(world.size(), 256, [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; k++) {
                world[k].ok = false;
                if (!mayBake((uint32_t)k))
                    continue;
                double w[4][8]; // [r][4..7] = row r of the world transform
                if (!invertTransform(topNodes[hInst[k].topNode].invTransform, w))
                    continue; // singular: stays an instance
                for (int r = 0; r < 3; r++)
                    for (int col = 0; col < 4; col++)
                        world[k].m[r * 4 + col] = w[r][4 + col];
                world[k].ok = true;
            }
        });
        auto tryBake = [&](uint32_t instIndex, bool wholeTrees) {
            const StaticHost::Root& root = s.roots[instRoot[instIndex]];
            const bool single = refCount(root.ref) != 0u; // the mesh is one leaf
            if (single != !wholeTrees)
                return;
            if (!world[instIndex].ok)
                return; // not a mesh that is copied, or a singular transform
            const uint64_t bytes = (uint64_t)root.numNodes * sizeof(WideNode) + (uint64_t)root.numRefs * sizeof(TriIsect);
            if ((!single && usedBytes + bytes > budgetBytes) || (uint64_t)nextNode + root.numNodes >= kRefIndexMask - 4u
                || (uint64_t)nextTri + root.numRefs >= kRefIndexMask - 4u)
                return;
            usedBytes += bytes;
            BakeJob j {};
            std::memcpy(j.m, world[instIndex].m, sizeof j.m);
            j.srcNode = root.nodeBase, j.numNodes = root.numNodes, j.dstNode = nextNode;
            j.srcRef = root.refBase, j.numRefs = root.numRefs, j.dstTri = nextTri;
            j.instance = instIndex;
            out.jobs.push_back(j);
            topRef[hInst[instIndex].topNode] = single ? makeRef(nextTri, refCount(root.ref)) : makeRef(nextNode, 0u);
            nextNode += root.numNodes;
            nextTri += root.numRefs;
        };
        if (copiesAllowed) {
            for (uint32_t k = 0; k < hInst.size(); k++) // single leaves first
                tryBake(k, false);
            if (wholeTreesFit)
                for (uint32_t k = 0; k < hInst.size(); k++)
                    tryBake(k, true);
        }
        out.bakedNodes = nextNode - (staticNodes + out.topSlots);
        out.bakedTris = nextTri - staticTris;
    }
    uint32_t topDepth = 0;
    { // depth / cycle check from the root
        std::vector<std::pair<uint32_t, uint32_t>> st { { topRoot, 1u } };
        size_t visited = 0;
        while (!st.empty()) {
            auto [ni, depth] = st.back();
            st.pop_back();
            if (++visited > nTop)
                return refuse(why, PT_ERR_INVALID, "top-level BVH is not a tree");
            topDepth = std::max(topDepth, depth);
            if (!topNodes[ni].isLeaf) {
                st.push_back({ topNodes[ni].a, depth + 1 });
                st.push_back({ topNodes[ni].b, depth + 1 });
            }
        }
    }
    // one pending entry per level of either tree + the leave-instance sentinel
    if (topDepth + 1 + maxBottomDepth > o.stackMax)
        return refuse(why, PT_ERR_UNSUPPORTED, "BVH depth %u (top) + %u (bottom) exceeds the traversal stack (%d)", topDepth, maxBottomDepth, (int)o.stackMax);
    if ((uint64_t)staticNodes + out.topSlots + out.bakedNodes + hInst.size() > kRefIndexMask)
        return refuse(why, PT_ERR_UNSUPPORTED, "too many BVH nodes");
    // ---- the top level: pair nodes -> 4-wide, packed breadth-first into the slots behind the static nodes -----------------
    std::vector<PairNode> topPairs(numTopInner);
    auto local = [&](uint32_t ref) { return refIndex(ref) - staticNodes; }; // top-level inner reference -> index into topPairs
    auto isTopInner = [&](uint32_t ref) { return ref != kRefNone && refCount(ref) == 0u && refIndex(ref) >= staticNodes && refIndex(ref) < staticNodes + numTopInner; };
    for (uint32_t i = 0; i < nTop; i++) {
        const pt_top_bvh_node& n = topNodes[i];
        if (n.isLeaf)
            continue;
        const pt_top_bvh_node& L = topNodes[n.a];
        const pt_top_bvh_node& R = topNodes[n.b];
        PairNode pn {};
        pn.bx = make_float4(L.min[0], L.max[0], R.min[0], R.max[0]);
        pn.by = make_float4(L.min[1], L.max[1], R.min[1], R.max[1]);
        pn.bz = make_float4(L.min[2], L.max[2], R.min[2], R.max[2]);
        // inside the collapse the top-level children are indices into topPairs; every other reference is opaque to it (instance
        // references and leaves by their count, the roots of world-space copies by an index beyond the array: they start behind the
        // top level's slots)
        pn.left = isTopInner(topRef[n.a]) ? makeRef(local(topRef[n.a]), 0u) : topRef[n.a];
        pn.right = isTopInner(topRef[n.b]) ? makeRef(local(topRef[n.b]), 0u) : topRef[n.b];
        topPairs[local(topRef[i])] = pn;
    }
    const std::vector<WideKids> kids = collapseKids(topPairs, CollapseCosts { 0u }, o.sequential);
    // breadth-first packing of the top-level nodes the collapse kept
    uint32_t rootRef = topRef[topRoot];
    constexpr uint32_t kUnset = 0xFFFFFFFFu;
    std::vector<uint32_t> newIndex(numTopInner, kUnset), order;
    auto isKept = [&](uint32_t r) { return r != kRefNone && refCount(r) == 0u && refIndex(r) < numTopInner; };
    if (isTopInner(rootRef)) {
        newIndex[local(rootRef)] = 0;
        order.push_back(local(rootRef));
        for (size_t q = 0; q < order.size(); q++)
            for (int k = 0; k < 4; k++) {
                const uint32_t r = kids[order[q]].ref[k];
                if (!kids[order[q]].empty[k] && isKept(r) && newIndex[refIndex(r)] == kUnset) {
                    newIndex[refIndex(r)] = (uint32_t)order.size();
                    order.push_back(refIndex(r));
                }
            }
        rootRef = makeRef(staticNodes, 0u);
    }
    out.topWide.resize(order.size());
    raytracer::WorkerPool::get().parallelFor(order.size(), 512, [&](size_t q0, size_t q1) {
        for (size_t q = q0; q < q1; q++) {
            const WideKids& wk = kids[order[q]];
            uint32_t refs[4];
            for (int k = 0; k < 4; k++)
                refs[k] = wk.empty[k] ? s.emptyRef : (isKept(wk.ref[k]) ? makeRef(staticNodes + newIndex[refIndex(wk.ref[k])], 0u) : wk.ref[k]);
            quantiseWideNode(wk.lo, wk.hi, refs, wk.empty, s.emptyRef, &out.topWide[q]);
        }
    });
    out.hasInstances = refCount(rootRef) == kRefSpecial;
    for (size_t q = 0; q < order.size() && !out.hasInstances; q++)
        for (uint32_t r : out.topWide[q].child)
            if (r != s.emptyRef && refCount(r) == kRefSpecial)
                out.hasInstances = true;
    // ---- worst-case traversal stack: the top level on top of the deepest thing below it (an entered instance adds its sentinel)
    std::vector<uint32_t> topNeed(order.size(), 0u);
    // the copies' roots are looked up by node index: a map for scenes with many of them
    std::vector<std::pair<uint32_t, uint32_t>> copyRoots;
    for (const BakeJob& j : out.jobs)
        if (j.numNodes)
            copyRoots.push_back({ j.dstNode, s.stackNeed[j.srcNode] });
    std::sort(copyRoots.begin(), copyRoots.end());
    auto needOf = [&](uint32_t ref) -> uint32_t {
        if (refCount(ref) == 0u && refIndex(ref) >= staticNodes && refIndex(ref) < staticNodes + order.size())
            return topNeed[refIndex(ref) - staticNodes];
        if (refCount(ref) == 0u) {
            auto it = std::lower_bound(copyRoots.begin(), copyRoots.end(), std::make_pair(refIndex(ref), 0u));
            return it != copyRoots.end() && it->first == refIndex(ref) ? it->second : 0u;
        }
        if (refCount(ref) == kRefSpecial) { // an entered instance: its sentinel + its mesh tree
            const uint32_t rr = hInst[refIndex(ref)].rootRef;
            return 1u + (refCount(rr) == 0u ? s.stackNeed[refIndex(rr)] : 0u);
        }
        return 0u;
    };
    for (size_t q = order.size(); q-- > 0;) {
        uint32_t n = 0, deepest = 0;
        for (uint32_t r : out.topWide[q].child)
            if (r != s.emptyRef)
                n++, deepest = std::max(deepest, needOf(r));
        topNeed[q] = (n > 0 ? n - 1 : 0u) + deepest;
    }
    const uint32_t stackNeed = needOf(rootRef);
    if (stackNeed > o.stackMax)
        return refuse(why, PT_ERR_UNSUPPORTED, "BVH needs %u traversal stack entries, %d are available", stackNeed, (int)o.stackMax);
    // k_trace_packet keeps its stack in the 64 lanes of a register (instance references are entered there too, pt_packet.h)
    out.packetOk = stackNeed <= o.packetStack;
    out.stackNeed = stackNeed;
    // ---- the top level once more, for the per-ray kernels: instances whose transform is a translation + uniform scale (the reference's own scenes,
    // BASELINE configs 4 / 5) are walked WITHOUT parking (pt_trace.h).  In this copy of the top level such an instance is an ordinary inner reference
    // -- to the instance's own copy of its mesh's ROOT node (object space, 64 bytes; the copies are the LAST run of the node array, copy k = instance
    // k) -- and (1 / s, w = -t / s) of its inverse transform sits in a table the kernel keeps in LDS.  Same pairs, same boxes, hence the same
    // collapse and a worst-case stack no larger than the one computed above (no sentinel).
    out.rootRefFolded = rootRef;
    out.foldedInstances = 0;
    out.instRoots.clear();
    out.instRootSrc.clear();
    out.instFold.clear();
    out.instRootBase = staticNodes + out.topSlots + out.bakedNodes;
    {
        const bool parked = o.noFoldedInstances || (o.flags & PT_FLAG_PARKED_INSTANCES) != 0u || o.parity; // (parity mode follows the reference to the letter)
        auto simple = [](const Instance& in) { return in.simple != 0u; };
        // Which route for the instances that are entered?  Every one a translation + uniform scale and few enough for the LDS table: folded (no entry step at
        // all).  Otherwise -- a rotation, a non-uniform scale, a shear, or instance number 96 -- the general route (round 6): every instance is entered as a
        // leaf-kind step, nothing is parked (pt_trace.h, LEVELS 2).  PTAMD_GENERAL_ROUTE=1 / 0 (diagnostics): the general route for every scene with entered
        // instances / never (rounds 2-5: such scenes park).
        uint32_t entered = 0, enteredGeneral = 0;
        for (size_t k = 0; k < hInst.size(); k++)
            if (refCount(topRef[hInst[k].topNode]) == kRefSpecial)
                entered++, enteredGeneral += simple(hInst[k]) ? 0u : 1u;
        out.enteredInstances = entered, out.enteredGeneral = enteredGeneral;
        // A scene with FEW such instances among many translated + uniformly scaled ones (at most a quarter) that fits the table keeps the folded route
        // for those -- no entry step at all -- and parks the few.
        const bool tableHolds = hInst.size() + 1 <= o.foldTable;
        const bool mostlySimple = enteredGeneral * 4u <= entered;
        out.generalRoute = !parked && entered > 0u && (o.generalRoute >= 0 ? o.generalRoute != 0 : (!mostlySimple || !tableHolds));
        const bool noFold = parked || out.generalRoute || !tableHolds;
        if (out.generalRoute) { // the entry records of the general route (pt_trace.h): 32 bytes per instance
            out.instFold.assign(hInst.size() * 2, make_float4(0.f, 0.f, 0.f, 0.f));
            for (size_t k = 0; k < hInst.size(); k++) {
                const Instance& in = hInst[k];
                const bool sim = simple(in);
                out.instFold[2 * k] = sim ? make_float4(in.r0.x, in.r0.w, in.r1.w, in.r2.w) : make_float4(1.f, 0.f, 0.f, 0.f);
                float4 tail = make_float4(0.f, 0.f, sim ? 1.0f / in.r0.x : 1.f, 0.f);
                std::memcpy(&tail.x, &in.rootRef, 4);
                const uint32_t flag = sim ? 1u : 0u;
                std::memcpy(&tail.y, &flag, 4);
                out.instFold[2 * k + 1] = tail;
            }
        }
        std::vector<uint8_t> folded(hInst.size(), 0);
        for (size_t k = 0; k < hInst.size() && !noFold; k++)
            if (refCount(topRef[hInst[k].topNode]) == kRefSpecial && simple(hInst[k]))
                folded[k] = 1, out.foldedInstances++;
        if (out.foldedInstances) {
            const uint32_t instRootBase = out.instRootBase;
            auto foldRef = [&](uint32_t r) { return refCount(r) == kRefSpecial && refIndex(r) < hInst.size() && folded[refIndex(r)] ? makeRef(instRootBase + refIndex(r), 0u) : r; };
            std::vector<PairNode> pairsB = topPairs;
            for (PairNode& pn : pairsB)
                pn.left = foldRef(pn.left), pn.right = foldRef(pn.right);
            const std::vector<WideKids> kidsB = collapseKids(pairsB, CollapseCosts { 0u }, o.sequential);
            std::vector<uint32_t> newB(numTopInner, kUnset), orderB;
            uint32_t rootB = foldRef(topRef[topRoot]);
            if (isTopInner(topRef[topRoot])) {
                newB[local(topRef[topRoot])] = 0;
                orderB.push_back(local(topRef[topRoot]));
                for (size_t q = 0; q < orderB.size(); q++)
                    for (int k = 0; k < 4; k++) {
                        const uint32_t r = kidsB[orderB[q]].ref[k];
                        if (!kidsB[orderB[q]].empty[k] && isKept(r) && newB[refIndex(r)] == kUnset) {
                            newB[refIndex(r)] = (uint32_t)orderB.size();
                            orderB.push_back(refIndex(r));
                        }
                    }
                rootB = makeRef(foldedBase, 0u);
            }
            out.topWide.resize((size_t)numTopInner + orderB.size()); // (the gap behind the first top level stays zero: never referenced)
            raytracer::WorkerPool::get().parallelFor(orderB.size(), 512, [&](size_t q0, size_t q1) {
                for (size_t q = q0; q < q1; q++) {
                    const WideKids& wk = kidsB[orderB[q]];
                    uint32_t refs[4];
                    for (int k = 0; k < 4; k++)
                        refs[k] = wk.empty[k] ? s.emptyRef : (isKept(wk.ref[k]) ? makeRef(foldedBase + newB[refIndex(wk.ref[k])], 0u) : wk.ref[k]);
                    quantiseWideNode(wk.lo, wk.hi, refs, wk.empty, s.emptyRef, &out.topWide[(size_t)numTopInner + q]);
                }
            });
            out.rootRefFolded = rootB;
            // the instances' root copies and the table of their transforms (entry 0: the identity; instances on the general route: the identity too --
            // their lanes hold the instance-space ray in registers)
            out.instRoots.assign(hInst.size(), WideNode {});
            out.instRootSrc.assign(hInst.size(), 0xFFFFFFFFu);
            out.instFold.assign(hInst.size() + 1, make_float4(1.f, 0.f, 0.f, 0.f));
            for (size_t k = 0; k < hInst.size(); k++) {
                if (!folded[k])
                    continue;
                Instance& in = hInst[k];
                out.instFold[k + 1] = make_float4(in.r0.x, in.r0.w, in.r1.w, in.r2.w);
                in.folded = 1u;
                if (refCount(in.rootRef) == 0u) {
                    out.instRootSrc[k] = refIndex(in.rootRef); // the mesh's packed root node as the device holds it (the host's mirror goes stale with a refit): object space, children in the shared tree
                } else { // the mesh is a single leaf: a one-child node around it -- the top-level leaf's box taken into object space, a few ulps outwards
                    const pt_top_bvh_node& leaf = topNodes[in.topNode];
                    float lo[4][3], hi[4][3];
                    const uint32_t refs[4] = { in.rootRef, s.emptyRef, s.emptyRef, s.emptyRef };
                    const bool empty[4] = { false, true, true, true };
                    const float w[3] = { in.r0.w, in.r1.w, in.r2.w };
                    for (int a = 0; a < 3; a++) {
                        const double l = (double)leaf.min[a] * in.r0.x + w[a], h = (double)leaf.max[a] * in.r0.x + w[a];
                        lo[0][a] = nextafterf(nextafterf((float)l, -INFINITY), -INFINITY), hi[0][a] = nextafterf(nextafterf((float)h, INFINITY), INFINITY);
                        for (int q = 1; q < 4; q++)
                            lo[q][a] = 1.f, hi[q][a] = -1.f;
                    }
                    quantiseWideNode(lo, hi, refs, empty, s.emptyRef, &out.instRoots[k]);
                }
            }
        }
    }
    std::vector<Light>& hLights = out.lights;
    hLights.resize(nL);
    for (uint32_t i = 0; i < nL; i++) {
        const pt_emissive_triangle& e = lights[i];
        const V3 v0 = mk(e.vertices[0][0], e.vertices[0][1], e.vertices[0][2]);
        const V3 v1 = mk(e.vertices[1][0], e.vertices[1][1], e.vertices[1][2]);
        const V3 v2 = mk(e.vertices[2][0], e.vertices[2][1], e.vertices[2][2]);
        // Heron's formula (shading_helper.cl:204-214)
        const V3 A = v1 - v0, B = v2 - v1, C = v0 - v2;
        const float la = sqrtf(dot(A, A)), lb = sqrtf(dot(B, B)), lc = sqrtf(dot(C, C));
        const float s = (la + lb + lc) / 2.0f;
        const float area = sqrtf(s * (s - la) * (s - lb) * (s - lc));
        const V3 nrm = normalize(cross(v1 - v0, v2 - v0));
        hLights[i].v0 = make_float4(v0.x, v0.y, v0.z, area);
        hLights[i].v1 = make_float4(v1.x, v1.y, v1.z, 0.f);
        hLights[i].v2 = make_float4(v2.x, v2.y, v2.z, 0.f);
        hLights[i].normal = make_float4(nrm.x, nrm.y, nrm.z, 0.f);
        hLights[i].colour = make_float4(e.material.u.emissive.emissiveColour[0], e.material.u.emissive.emissiveColour[1], e.material.u.emissive.emissiveColour[2], 0.f);
    }
    out.numLights = nL;
    out.rootRef = rootRef;
    return PT_OK;
}

// ---- instance motion ------------------------------------------------------------------------------------------------------------------
int motionRecords(const float* prevInv, const float* curInv, uint32_t n, const uint8_t* use, MotionRecord* out, uint32_t* moving, std::string& why)
{
    uint32_t moved = 0;
    for (uint32_t i = 0; i < n; i++) {
        MotionRecord r {};
        if (use && !use[i]) {
            out[i] = r;
            continue;
        }
        const float *p = prevInv + (size_t)i * 16, *c = curInv + (size_t)i * 16;
        for (int k = 0; k < 16; k++)
            if (!std::isfinite(p[k]))
                return refuse(why, PT_ERR_INVALID, "instance motion: the previous invTransform of entry %u is not finite", i);
        r.p0 = make_float4(p[0], p[4], p[8], p[12]);
        r.p1 = make_float4(p[1], p[5], p[9], p[13]);
        r.p2 = make_float4(p[2], p[6], p[10], p[14]);
        double w[4][8];
        if (!invertTransform(p, w)) // (also where the bits are the current ones: a state that cannot be inverted has no "then" to go to)
            return refuse(why, PT_ERR_INVALID, "instance motion: the previous invTransform of entry %u is singular", i);
        if (std::memcmp(p, c, 16 * sizeof(float)) != 0) {
            moved++;
            float4* rows[3] = { &r.a0, &r.a1, &r.a2 };
            for (int row = 0; row < 3; row++) {
                double e[4];
                for (int col = 0; col < 4; col++) {
                    double s = 0.0;
                    for (int k = 0; k < 4; k++)
                        s += w[row][4 + k] * (double)c[col * 4 + k]; // element (row, k) of inverse(prev) times element (k, col) of cur
                    e[col] = s - (row == col ? 1.0 : 0.0);
                }
                *rows[row] = make_float4((float)e[0], (float)e[1], (float)e[2], (float)e[3]);
            }
        }
        out[i] = r;
    }
    if (moving)
        *moving = moved;
    return PT_OK;
}

// ---- vertex motion --------------------------------------------------------------------------------------------------------------------
int vertexMotionRows(const float* inv, uint32_t n, float4* out, std::string& why)
{
    for (uint32_t i = 0; i < n; i++) {
        const float* m = inv + (size_t)i * 16;
        for (int k = 0; k < 16; k++)
            if (!std::isfinite(m[k]))
                return refuse(why, PT_ERR_INVALID, "vertex motion: the invTransform of entry %u is not finite", i);
        double w[4][8];
        if (!invertTransform(m, w))
            return refuse(why, PT_ERR_INVALID, "vertex motion: the invTransform of entry %u is singular", i);
        for (int row = 0; row < 3; row++) {
            const float4 r = make_float4((float)w[row][4], (float)w[row][5], (float)w[row][6], 0.0f);
            if (!std::isfinite(r.x) || !std::isfinite(r.y) || !std::isfinite(r.z)) // (a pivot above the threshold by round-off alone)
                return refuse(why, PT_ERR_INVALID, "vertex motion: the invTransform of entry %u is singular", i);
            out[(size_t)i * 3 + row] = r;
        }
    }
    return PT_OK;
}

} // namespace ptconv
