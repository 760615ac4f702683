// A light that moves under a static camera, at one sample per pixel and frame: the Cornell room of converge_cornell.cpp with its ceiling light as an
// instance of its own, which stands at x = -0.5 for a while and then swings to x = +0.5 (one frameTick).  A moving light has no motion vector -- the
// surfaces its shadows move over stand still -- so the temporal history keeps the old lighting and fades it over max_history frames.  The loop runs
// twice, without and with the temporal response (RayTracer::setTemporalResponse), and at three frames after the jump the unfiltered history is
// measured against a converged render of the new state (tone-mapped RMSE, before gamma).  Every frame takes 16 guide samples (first hits alone: cheap next
// to the frame): how long the history grows is the guides' doing, and with one jittered guide sample per frame the history of this small room stays so
// short that it forgets the old light by itself.
//     usage: moving_light [frames before the jump] [reference spp]
#include "cornell.h"
#include <cstdio>
#include <cstdlib>

using namespace raytracer;
using namespace cornell;

static const int kAfter[3] = { 4, 16, 32 }; // frames after the jump at which the history is measured
static const uint32_t kGuideSamples = 16;
static const float kLightBefore = -0.5f, kLightAfter = 0.5f;

struct Room {
    std::shared_ptr<Scene> scene = std::make_shared<Scene>();
    SceneNode* light = nullptr;
    Room()
    {
        addWalls(*scene); // floor, ceiling, back, left, right
        scene->addNode(bluePlate(), Transform(vec3(0.2f, 0.0f, 0.1f)));
        light = &scene->addNode(quadMesh({ -0.25f, 0.0f, -0.25f }, { 0.25f, 0.0f, -0.25f }, { 0.25f, 0.0f, 0.25f }, { -0.25f, 0.0f, 0.25f },
                                    Material::Emissive(vec3(1.0f, 0.92f, 0.8f), 12.0f)),
            Transform(vec3(kLightBefore, 1.98f, 0.0f)));
    }
};

// the unfiltered history (the newest d times the current albedo), linear
static std::vector<float> history(RayTracer& rt, int W, int H)
{
    std::vector<float> image((size_t)W * H * 4);
    pt_denoise_params prm {};
    prm.iterations = 0u;
    prm.output = PT_DENOISE_HDR;
    prm.input = PT_DENOISE_INPUT_TEMPORAL;
    if (pt_denoise(rt.context(), &prm, image.data(), nullptr) != PT_OK)
        throw std::runtime_error(pt_last_error(rt.context()));
    return image;
}

int main(int argc, char** argv)
{
    const int before = argc > 1 ? std::atoi(argv[1]) : 16;
    const int referenceSpp = argc > 2 ? std::atoi(argv[2]) : 256;
    const int W = 64, H = 64;
    if (before < 1 || referenceSpp < 1) {
        std::fprintf(stderr, "error: frames before the jump and reference spp must be at least 1\n");
        return 1;
    }
    try {
        const Camera camera = frontCamera(W, H);
        const CameraData cam = camera.get_camera_data();
        const TextureArray noTextures, sky = greySky();

        std::vector<double> want; // the converged view of the state after the jump, from random numbers no frame below draws
        {
            Room room;
            room.light->transform = Transform(vec3(kLightAfter, 1.98f, 0.0f));
            RayTracer rt(W, H, room.scene, noTextures, sky);
            rt.setSampleBase(1000000u);
            for (int s = 0; s < referenceSpp; s++)
                rt.rayTrace(camera);
            want = tonemapped(rt.getAccumulator(), 1.0 / referenceSpp, cam);
        }

        double e[2][3];
        unsigned temporalFrames = 0;
        for (int mode = 0; mode < 2; mode++) {
            Room room;
            RayTracer rt(W, H, room.scene, noTextures, sky);
            rt.setTemporalResponse(mode == 1);
            const int frames = before + kAfter[2];
            for (int f = 0; f < frames; f++) {
                if (f == before) {
                    room.light->transform = Transform(vec3(kLightAfter, 1.98f, 0.0f)); // the swing: one re-posed instance, one tick
                    rt.frameTick();
                }
                if (pt_clear(rt.context()) != PT_OK) // the camera stands still: rayTrace would go on accumulating
                    throw std::runtime_error(pt_last_error(rt.context()));
                rt.setSampleBase((uint32_t)f);
                rt.rayTrace(camera);
                if (pt_render_guides(rt.context(), kGuideSamples) != PT_OK) // (getTemporalOutput would take one: as many as the frame has samples)
                    throw std::runtime_error(pt_last_error(rt.context()));
                rt.getTemporalOutput(0); // blends this frame into the history (and, with the mode on, into the fast one)
                for (int k = 0; k < 3; k++)
                    if (f + 1 == before + kAfter[k])
                        e[mode][k] = rmse(tonemapped(history(rt, W, H), 1.0, cam), want);
            }
            temporalFrames = pt_temporal_frames(rt.context());
            if (pt_temporal_response(rt.context()) != mode)
                throw std::runtime_error("the temporal response is not in the mode it was set to");
        }
        for (int k = 0; k < 3; k++)
            std::printf("after=%d plain=%.4e response=%.4e ratio=%.3f\n", kAfter[k], e[0][k], e[1][k], e[1][k] / e[0][k]);
        std::printf("before=%d temporal_frames=%u\n", before, temporalFrames);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
