// A static camera at one sample per pixel and frame: the Cornell box of orbit_cornell.cpp, every frame cleared and traced anew with the sample base
// set to the frame number and blended into the temporal history with the luminance variance on (RayTracer::setTemporalVariance).  At frames 1, 8 and
// the last one the history is measured three ways against a converged render of the same view (tone-mapped RMSE, before gamma): as it is, through
// the plain a-trous filter (PT_DENOISE_INPUT_TEMPORAL) and through the variance-guided one (PT_DENOISE_INPUT_TEMPORAL_VARIANCE).
//     usage: converge_cornell [frames] [reference spp]
#include "cornell.h"
#include <cstdio>
#include <cstdlib>

using namespace raytracer;
using namespace cornell;

int main(int argc, char** argv)
{
    const int frames = argc > 1 ? std::atoi(argv[1]) : 32;
    const int referenceSpp = argc > 2 ? std::atoi(argv[2]) : 256;
    const int W = 64, H = 64;
    if (frames < 1 || referenceSpp < 1) {
        std::fprintf(stderr, "error: frames and reference spp must be at least 1\n");
        return 1;
    }
    try {
        auto scene = std::make_shared<Scene>();
        addWalls(*scene); // floor, ceiling, back, left, right
        scene->addNode(ceilingLight());
        scene->addNode(bluePlate(), Transform(vec3(0.2f, 0.0f, 0.1f)));

        const TextureArray noTextures, sky = greySky();
        RayTracer rt(W, H, scene, noTextures, sky);

        const Camera camera = frontCamera(W, H);
        const CameraData cam = camera.get_camera_data();

        // the converged view, from random numbers no frame below draws
        rt.setSampleBase(1000000u);
        for (int s = 0; s < referenceSpp; s++)
            rt.rayTrace(camera);
        const std::vector<double> want = tonemapped(rt.getAccumulator(), 1.0 / referenceSpp, cam);

        rt.setTemporalVariance(true);
        std::vector<float> image((size_t)W * H * 4);
        for (int f = 0; f < frames; f++) {
            if (pt_clear(rt.context()) != PT_OK) // (a static camera: rayTrace clears only when the camera changed)
                throw std::runtime_error("pt_clear failed");
            rt.setSampleBase((uint32_t)f);
            rt.rayTrace(camera);
            rt.getTemporalOutput(0); // blends this frame and its variance into the history
            if (f + 1 != 1 && f + 1 != 8 && f + 1 != frames)
                continue;
            double e[3];
            const uint32_t inputs[3] = { PT_DENOISE_INPUT_TEMPORAL, PT_DENOISE_INPUT_TEMPORAL, PT_DENOISE_INPUT_TEMPORAL_VARIANCE };
            for (int k = 0; k < 3; k++) {
                pt_denoise_params prm {};
                prm.iterations = k == 0 ? 0u : 5u;
                prm.output = PT_DENOISE_HDR;
                prm.input = inputs[k];
                if (pt_denoise(rt.context(), &prm, image.data(), nullptr) != PT_OK)
                    throw std::runtime_error(pt_last_error(rt.context()));
                e[k] = rmse(tonemapped(image, 1.0, cam), want);
            }
            std::printf("frame=%d history=%.4e plain=%.4e guided=%.4e\n", f + 1, e[0], e[1], e[2]);
        }
        std::printf("frames=%d temporal_frames=%u variance=%d\n", frames, pt_temporal_frames(rt.context()), pt_temporal_variance(rt.context()));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
