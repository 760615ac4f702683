// A REBUILT tree per frame through the kept C++ API -- the other branch of the reference's MeshSequence::buildBvh (src/model/mesh_sequence.cpp:89-96:
// `buildBinnedFastBVH` on the frame's triangles instead of a refit), whose arrays transferDynamicData re-uploads every tick (src/raytracer.cpp:510-568).
// A sequence-like IMesh makes a new Mesh (fast binned builder) per frame; RayTracer::rebuildGeometry hands the re-flattened scene to the device library's
// second static set (pt_upload_static_async: the host converts the topology, the device makes the records), RayTracer::frameTick adopts it with the new
// top level, frames keep rendering meanwhile.  Prints the median milliseconds of every stage and checks the last frame against a RayTracer that only ever
// saw that frame: the two accumulators must be identical.
//      usage: rebuild_loop [level] [frames]        (icosphere level: 5 = 20 480 triangles, bench.py's `rebuild_20k`)
#include "cornell.h"
#include "meshes.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace raytracer;
using namespace cornell;
using namespace meshes;
using Clock = std::chrono::steady_clock;

static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2];
}

static void deformed(const std::vector<float>& unit, int k, std::vector<float>& pos)
{
    pos.resize(unit.size());
    for (size_t i = 0; i < unit.size(); i += 3) {
        const float s = 0.5f * (1.0f + 0.1f * std::sin((float)k + 1.0f + 5.0f * unit[i]));
        pos[i] = unit[i] * s, pos[i + 1] = unit[i + 1] * s, pos[i + 2] = unit[i + 2] * s;
    }
}

int main(int argc, char** argv)
{
    const int level = argc > 1 ? std::atoi(argv[1]) : 5, frames = argc > 2 ? std::atoi(argv[2]) : 12;
    const int W = 1280, H = 720;
    try {
        std::vector<float> unit, pos;
        std::vector<uint32_t> idx;
        icosphere(level, unit, idx);
        const Material white = Material::Diffuse(vec3(0.73f)), blobMaterial = Material::PBRDielectric(vec3(0.75f, 0.2f, 0.15f), 0.7f);
        auto makeScene = [&](std::shared_ptr<RebuiltMesh>* out, int frame) {
            auto scene = std::make_shared<Scene>();
            scene->addNode(quadMesh({ -1, 0, -1 }, { -1, 0, 1 }, { 1, 0, 1 }, { 1, 0, -1 }, white));
            scene->addNode(quadMesh({ -1, 0, 1 }, { -1, 2, 1 }, { 1, 2, 1 }, { 1, 0, 1 }, white));
            scene->addNode(ceilingLight());
            auto seq = std::make_shared<RebuiltMesh>(idx, blobMaterial);
            deformed(unit, frame, pos);
            seq->goToFrame(pos);
            Transform t;
            t.location = vec3(0.0f, 0.8f, 0.1f);
            t.scale = vec3(1.2f);
            scene->addNode(seq, t);
            *out = seq;
            return scene;
        };
        const TextureArray noTextures, sky = greySky();
        Transform camT(vec3(0.0f, 1.0f, -3.9f));
        Camera camera(camT, 50.0f, (float)W / H, 3.9f);
        camera.m_thinLens = false;
        auto check = [](int rc, pt_ctx* c) {
            if (rc != PT_OK)
                throw std::runtime_error(pt_last_error(c));
        };

        std::shared_ptr<RebuiltMesh> seq;
        RayTracer rt(W, H, makeScene(&seq, 0), noTextures, sky);
        rt.rayTrace(camera);
        std::vector<double> tBuild, tRebuild, tTick, tAdopted;
        for (int k = 1; k <= frames + 2; k++) {
            check(pt_render(rt.context(), 1), rt.context()); // a frame of the old scene is in flight while the host builds
            deformed(unit, k, pos);
            const auto t0 = Clock::now();
            seq->goToFrame(pos);
            const auto t1 = Clock::now();
            check(pt_render(rt.context(), 1), rt.context()); // ... and another one while the host converts
            rt.rebuildGeometry();
            const auto t2 = Clock::now();
            rt.frameTick();
            const auto t3 = Clock::now();
            check(pt_render(rt.context(), 1), rt.context()); // the first frame of the new scene
            check(pt_synchronize(rt.context()), rt.context());
            const auto t4 = Clock::now();
            if (k > 2) // the first two rebuilds size the two static sets
                tBuild.push_back(ms(t0, t1)), tRebuild.push_back(ms(t1, t2)), tTick.push_back(ms(t2, t3)), tAdopted.push_back(ms(t0, t4));
        }
        // the last frame against a RayTracer that only ever saw it
        check(pt_clear(rt.context()), rt.context());
        for (int s = 0; s < 4; s++)
            rt.rayTrace(camera);
        const std::vector<float> got = rt.getAccumulator();
        std::shared_ptr<RebuiltMesh> seq2;
        RayTracer fresh(W, H, makeScene(&seq2, frames + 2), noTextures, sky);
        for (int s = 0; s < 4; s++)
            fresh.rayTrace(camera);
        const std::vector<float> want = fresh.getAccumulator();
        const bool same = got.size() == want.size() && std::memcmp(got.data(), want.data(), got.size() * sizeof(float)) == 0;
        std::printf("triangles=%zu frames=%d mesh_build_ms=%.3f rebuild_geometry_ms=%.3f frame_tick_ms=%.3f until_first_new_frame_ms=%.3f same_as_fresh=%d\n", idx.size() / 3, frames,
            median(tBuild), median(tRebuild), median(tTick), median(tAdopted), same ? 1 : 0);
        return same ? 0 : 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
