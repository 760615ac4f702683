// What the firefly clamp buys a frame loop in a room with specular paths: the Cornell room with a polished metal blob (a lumpy sphere, PBR metal of
// reflectance (0.95, 0.8, 0.5) and smoothness 1) under a static camera.  Twelve frames of one sample per pixel, each blended into the temporal history
// and filtered (getTemporalOutput, guides through the chain with reflections) -- once with the clamp off, once with RayTracer::setFireflyClamp(true).
// Printed: the RMSE of the last frame's output against 256 samples per pixel (both through pt_resolve's tone curve), the pixels the last frame clamped
// and the share of that frame's demodulated luminance the clamp kept -- what it removes is real light (include/ptamd.h, "firefly clamp").
//     usage: firefly_cornell [frames] [reference spp]
#include "cornell.h"
#include "meshes.h"
#include <cstdio>
#include <cstdlib>

using namespace raytracer;
using namespace cornell;

static std::shared_ptr<Scene> room()
{
    auto scene = std::make_shared<Scene>();
    addWalls(*scene); // floor, ceiling, back, left, right
    scene->addNode(ceilingLight());
    std::vector<float> pos;
    meshes::blobRest(pos);
    const std::vector<uint32_t> idx = meshes::blobIndices();
    scene->addNode(std::make_shared<Mesh>(pos.data(), nullptr, nullptr, pos.size() / 3, idx.data(), nullptr, idx.size() / 3,
                       std::vector<Material> { Material::PBRMetal(vec3(0.95f, 0.8f, 0.5f), 1.0f) }, BvhBuilder::BinnedSAH),
        Transform(vec3(0.1f, 0.6f, 0.1f)));
    return scene;
}

int main(int argc, char** argv)
{
    const int frames = argc > 1 ? std::atoi(argv[1]) : 12;
    const int referenceSpp = argc > 2 ? std::atoi(argv[2]) : 256;
    const int W = 64, H = 64;
    if (frames < 1 || referenceSpp < 1) {
        std::fprintf(stderr, "error: frames and reference spp must be at least 1\n");
        return 1;
    }
    try {
        const Camera camera = frontCamera(W, H);
        const TextureArray noTextures, sky = greySky();
        auto rgb = [](const std::vector<float>& rgba) { // (the fourth component is no colour)
            std::vector<double> out;
            for (size_t i = 0; i < rgba.size(); i++)
                if (i % 4 != 3)
                    out.push_back(rgba[i]);
            return out;
        };

        std::vector<double> want; // the converged view, from random numbers no frame below draws
        {
            RayTracer rt(W, H, room(), noTextures, sky);
            rt.setSampleBase(1000000u);
            for (int s = 0; s < referenceSpp; s++)
                rt.rayTrace(camera);
            want = rgb(rt.getOutput());
        }

        double e[2];
        uint32_t counts[2] = { 0, 0 };
        double kept = 1.0;
        for (int mode = 0; mode < 2; mode++) {
            RayTracer rt(W, H, room(), noTextures, sky);
            rt.setGuideChain(PT_GUIDE_CHAIN_MAX);
            rt.setGuideReflections(true);
            rt.setFireflyClamp(mode == 1);
            std::vector<float> out;
            for (int f = 0; f < frames; f++) {
                if (pt_clear(rt.context()) != PT_OK) // the camera stands still: rayTrace would go on accumulating
                    throw std::runtime_error(pt_last_error(rt.context()));
                rt.setSampleBase((uint32_t)f);
                rt.rayTrace(camera);
                out = rt.getTemporalOutput(5);
            }
            e[mode] = rmse(rgb(out), want);
            if (pt_firefly_clamp(rt.context()) != mode)
                throw std::runtime_error("the firefly clamp is not in the mode it was set to");
            if (mode == 1) { // the last frame's plane: d_out = d s where s > 0
                std::vector<float> plane((size_t)W * H * 4);
                if (pt_read_firefly(rt.context(), plane.data(), counts) != PT_OK)
                    throw std::runtime_error(pt_last_error(rt.context()));
                double after = 0.0, before = 0.0;
                for (size_t i = 0; i < plane.size(); i += 4)
                    if (plane[i + 3] > 0.0f) {
                        const double l = 0.2126 * plane[i] + 0.7152 * plane[i + 1] + 0.0722 * plane[i + 2];
                        after += l, before += l / plane[i + 3];
                    }
                kept = before > 0.0 ? after / before : 1.0;
            }
        }
        std::printf("frames=%d rmse_off=%.4e rmse_on=%.4e ratio=%.3f\n", frames, e[0], e[1], e[1] / e[0]);
        std::printf("clamped=%u nonfinite=%u luminance_kept=%.4f\n", counts[0], counts[1], kept);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 1;
    }
    return 0;
}
