// A deforming mesh at one sample per pixel under a static camera: a lumpy blob leans over and sways in the Cornell room of moving_cornell.cpp, refitted
// every frame (Mesh::refit, RayTracer::updateGeometry: the device refits its own trees), one frameTick per frame, every frame cleared and traced anew
// with the sample base set to the frame number and blended into the temporal history (getTemporalOutput).  The loop runs twice: without vertex motion --
// the blob's pixels look up where that world point WAS SEEN and lose their history, or blend in the wall that used to be there -- and with it
// (RayTracer::setVertexMotion, the default), where the history follows the surface.  The last frame is written three times as a PPM: filtered alone
// (getDenoisedOutput), filtered over the history without vertex motion, and with it.
//     usage: deforming_cornell [frames] [filtered.ppm] [temporal_plain.ppm] [temporal_motion.ppm]
#include "cornell.h"
#include "meshes.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace raytracer;
using namespace cornell;
using namespace meshes;

struct Result {
    std::vector<float> temporal, filtered;
    int spp = 0;
    unsigned temporalFrames = 0, deformed = 0;
};

static Result run(int frames, bool vertexMotion, const Camera& camera, int W, int H)
{
    auto scene = std::make_shared<Scene>();
    addWalls(*scene); // floor, ceiling, back, left, right
    scene->addNode(ceilingLight());
    std::vector<float> rest, pos;
    blobRest(rest);
    const std::vector<uint32_t> idx = blobIndices();
    auto blob = std::make_shared<Mesh>(rest.data(), nullptr, nullptr, rest.size() / 3, idx.data(), nullptr, idx.size() / 3,
        std::vector<Material> { Material::Diffuse(vec3(0.2f, 0.3f, 0.7f)) }, BvhBuilder::BinnedSAH);
    scene->addNode(blob, Transform(kBlobAt));

    const TextureArray noTextures, sky = greySky();
    RayTracer rt(W, H, scene, noTextures, sky);
    rt.setVertexMotion(vertexMotion);
    Result r;
    for (int f = 0; f < frames; f++) {
        if (f) {
            blobShape(rest, f, pos);
            blob->refit(pos.data(), nullptr);
            rt.updateGeometry(); // the vertices go to the device, which refits its trees
            rt.frameTick(); // the new shape; with vertex motion on, the shape the history was made under stays on the device as "then"
            if (pt_clear(rt.context()) != PT_OK) // the camera stands still: rayTrace would go on accumulating
                throw std::runtime_error(pt_last_error(rt.context()));
        }
        rt.setSampleBase((uint32_t)f);
        rt.rayTrace(camera); // the first sample after a tick: sets the motion, then one sample per pixel
        r.temporal = rt.getTemporalOutput();
    }
    uint32_t deformed = 0;
    pt_vertex_motion(rt.context(), &deformed);
    r.deformed = deformed;
    r.filtered = rt.getDenoisedOutput();
    r.spp = rt.getSamplesPerPixel();
    r.temporalFrames = pt_temporal_frames(rt.context());
    return r;
}

int main(int argc, char** argv)
{
    const int frames = argc > 1 ? std::atoi(argv[1]) : 12;
    const char* filteredPath = argc > 2 ? argv[2] : "deforming_filtered.ppm";
    const char* plainPath = argc > 3 ? argv[3] : "deforming_temporal_plain.ppm";
    const char* motionPath = argc > 4 ? argv[4] : "deforming_temporal_motion.ppm";
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
        // the blob's screen rectangle in its final shape: its vertices through the camera, X - E = lambda (S - E + u fx + v fy)
        const CameraData c = camera.get_camera_data();
        const vec3 E(c.eyePoint[0], c.eyePoint[1], c.eyePoint[2]), S(c.screenPoint[0], c.screenPoint[1], c.screenPoint[2]);
        const vec3 u(c.u[0], c.u[1], c.u[2]), v(c.v[0], c.v[1], c.v[2]), s0 = S - E;
        const float det = dot(s0, cross(u, v));
        std::vector<float> rest, last;
        blobRest(rest);
        blobShape(rest, frames - 1, last);
        float x0 = (float)W, y0 = (float)H, x1 = 0.0f, y1 = 0.0f;
        for (size_t k = 0; k < last.size(); k += 3) {
            const vec3 q = kBlobAt + vec3(last[k], last[k + 1], last[k + 2]) - E;
            const float lambda = dot(q, cross(u, v)) / det;
            const float fx = (float)W * dot(s0, cross(q, v)) / det / lambda, fy = (float)H * dot(s0, cross(u, q)) / det / lambda;
            x0 = std::min(x0, fx), x1 = std::max(x1, fx), y0 = std::min(y0, fy), y1 = std::max(y1, fy);
        }
        const int rx0 = std::max(0, (int)std::floor(x0)), ry0 = std::max(0, (int)std::floor(y0)), rx1 = std::min(W, (int)std::ceil(x1)), ry1 = std::min(H, (int)std::ceil(y1));
        std::printf("frames=%d spp=%d temporal_frames=%u deformed=%u blob_rect=%d,%d,%d,%d -> %s %s %s\n", frames, motion.spp, motion.temporalFrames, motion.deformed,
            rx0, ry0, rx1, ry1, filteredPath, plainPath, motionPath);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
