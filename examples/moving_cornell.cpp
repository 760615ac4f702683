// A moving instance at one sample per pixel under a static camera: a diffuse box slides and turns through the Cornell room of denoise_cornell.cpp,
// one frameTick per frame, every frame cleared and traced anew with the sample base set to the frame number and blended into the temporal history
// (getTemporalOutput).  The loop runs twice: without instance motion -- the box's pixels look up where that world point WAS SEEN and lose their
// history, or blend in the wall that used to be there -- and with it (RayTracer::setInstanceMotion, the default), where the history follows the box.
// The last frame is written three times as a PPM: filtered alone (getDenoisedOutput), filtered over the history without motion, and with motion.
//     usage: moving_cornell [frames] [filtered.ppm] [temporal_plain.ppm] [temporal_motion.ppm]
#include "cornell.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace raytracer;
using namespace cornell;

// a box about the origin, four vertices of its own per face (flat normals), wound outwards
static std::shared_ptr<Mesh> boxMesh(vec3 h, const Material& m)
{
    const float s[6][4][3] = { { { -1, -1, -1 }, { -1, 1, -1 }, { 1, 1, -1 }, { 1, -1, -1 } }, { { -1, -1, 1 }, { 1, -1, 1 }, { 1, 1, 1 }, { -1, 1, 1 } },
        { { -1, -1, -1 }, { -1, -1, 1 }, { -1, 1, 1 }, { -1, 1, -1 } }, { { 1, -1, -1 }, { 1, 1, -1 }, { 1, 1, 1 }, { 1, -1, 1 } },
        { { -1, 1, -1 }, { -1, 1, 1 }, { 1, 1, 1 }, { 1, 1, -1 } }, { { -1, -1, -1 }, { 1, -1, -1 }, { 1, -1, 1 }, { -1, -1, 1 } } };
    std::vector<float> pos;
    std::vector<uint32_t> idx;
    for (int f = 0; f < 6; f++) {
        for (int k = 0; k < 4; k++) {
            pos.push_back(s[f][k][0] * h.x);
            pos.push_back(s[f][k][1] * h.y);
            pos.push_back(s[f][k][2] * h.z);
        }
        const uint32_t b = (uint32_t)f * 4;
        for (uint32_t i : { b, b + 1, b + 2, b, b + 2, b + 3 })
            idx.push_back(i);
    }
    return std::make_shared<Mesh>(pos.data(), nullptr, nullptr, 24, idx.data(), nullptr, 12, std::vector<Material> { m }, BvhBuilder::BinnedSAH);
}

static const vec3 kHalf(0.28f, 0.45f, 0.28f);

static Transform boxPose(int frame)
{
    const float deg = 3.14159265f / 180.0f;
    return Transform(vec3(-0.35f + 0.05f * (float)frame, 0.46f, 0.0f), quat::angleAxis(3.0f * deg * (float)frame, vec3(0.0f, 1.0f, 0.0f)));
}

struct Result {
    std::vector<float> temporal, filtered;
    int spp = 0;
    unsigned temporalFrames = 0, moving = 0;
};

static Result run(int frames, bool instanceMotion, const Camera& camera, int W, int H)
{
    auto scene = std::make_shared<Scene>();
    addWalls(*scene); // floor, ceiling, back, left, right
    scene->addNode(ceilingLight());
    SceneNode& box = scene->addNode(boxMesh(kHalf, Material::Diffuse(vec3(0.2f, 0.3f, 0.7f))), boxPose(0));

    const TextureArray noTextures, sky = greySky();
    RayTracer rt(W, H, scene, noTextures, sky);
    rt.setInstanceMotion(instanceMotion);
    Result r;
    for (int f = 0; f < frames; f++) {
        if (f) {
            box.transform = boxPose(f);
            rt.frameTick(); // the new pose; with instance motion on, the pose the history was made under is kept
            if (pt_clear(rt.context()) != PT_OK) // the camera stands still: rayTrace would go on accumulating
                throw std::runtime_error(pt_last_error(rt.context()));
        }
        rt.setSampleBase((uint32_t)f);
        rt.rayTrace(camera); // the first sample after a tick: sets the motion, then one sample per pixel
        r.temporal = rt.getTemporalOutput();
    }
    uint32_t moving = 0;
    pt_instance_motion(rt.context(), &moving);
    r.moving = moving;
    r.filtered = rt.getDenoisedOutput();
    r.spp = rt.getSamplesPerPixel();
    r.temporalFrames = pt_temporal_frames(rt.context());
    return r;
}

int main(int argc, char** argv)
{
    const int frames = argc > 1 ? std::atoi(argv[1]) : 12;
    const char* filteredPath = argc > 2 ? argv[2] : "moving_filtered.ppm";
    const char* plainPath = argc > 3 ? argv[3] : "moving_temporal_plain.ppm";
    const char* motionPath = argc > 4 ? argv[4] : "moving_temporal_motion.ppm";
    const int W = 256, H = 256;
    if (frames < 1) {
        std::fprintf(stderr, "error: frames must be at least 1\n");
        return 1;
    }
    try {
        const Camera camera = frontCamera(W, H);
        const Result plain = run(frames, false, camera, W, H), motion = run(frames, true, camera, W, H);
        writePPM(filteredPath, motion.filtered, W, H);
        writePPM(plainPath, plain.temporal, W, H);
        writePPM(motionPath, motion.temporal, W, H);
        // the box's screen rectangle in its final pose: its corners through the camera, X - E = lambda (S - E + u fx + v fy)
        const CameraData c = camera.get_camera_data();
        const vec3 E(c.eyePoint[0], c.eyePoint[1], c.eyePoint[2]), S(c.screenPoint[0], c.screenPoint[1], c.screenPoint[2]);
        const vec3 u(c.u[0], c.u[1], c.u[2]), v(c.v[0], c.v[1], c.v[2]), s0 = S - E;
        const float det = dot(s0, cross(u, v));
        const Transform last = boxPose(frames - 1);
        float x0 = (float)W, y0 = (float)H, x1 = 0.0f, y1 = 0.0f;
        for (int k = 0; k < 8; k++) {
            const vec3 corner((k & 1 ? 1.0f : -1.0f) * kHalf.x, (k & 2 ? 1.0f : -1.0f) * kHalf.y, (k & 4 ? 1.0f : -1.0f) * kHalf.z);
            const vec3 q = last.location + last.transformDirection(corner) - E;
            const float lambda = dot(q, cross(u, v)) / det;
            const float fx = (float)W * dot(s0, cross(q, v)) / det / lambda, fy = (float)H * dot(s0, cross(u, q)) / det / lambda;
            x0 = std::min(x0, fx), x1 = std::max(x1, fx), y0 = std::min(y0, fy), y1 = std::max(y1, fy);
        }
        const int rx0 = std::max(0, (int)std::floor(x0)), ry0 = std::max(0, (int)std::floor(y0)), rx1 = std::min(W, (int)std::ceil(x1)), ry1 = std::min(H, (int)std::ceil(y1));
        std::printf("frames=%d spp=%d temporal_frames=%u moving=%u blob_rect=%d,%d,%d,%d -> %s %s %s\n", frames, motion.spp, motion.temporalFrames, motion.moving,
            rx0, ry0, rx1, ry1, filteredPath, plainPath, motionPath);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
