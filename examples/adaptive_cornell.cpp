// Adaptive sampling on the Cornell room seen from far enough back that grey sky surrounds it: RayTracer::setAdaptive, then rayTraceAdaptive to
// completion -- rounds of `round` samples per pixel that go only to the 8 x 8 blocks whose two half images still differ by `threshold` or more
// (include/ptamd.h, "adaptive sampling").  The sky and the directly seen light stop at min_samples, the penumbrae and the colour bleeding go on.
// Written: adaptive_cornell.ppm, the image, and adaptive_cornell_counts.ppm, a heat map of the samples each pixel got (black = min_samples, white =
// max_samples).  Printed: the samples spent against the uniform budget W H max_samples.
//     usage: adaptive_cornell [threshold] [max_samples]
#include "cornell.h"
#include <cstdio>
#include <cstdlib>

using namespace raytracer;
using namespace cornell;

int main(int argc, char** argv)
{
    const float threshold = argc > 1 ? (float)std::atof(argv[1]) : 0.02f;
    const int maxSamples = argc > 2 ? std::atoi(argv[2]) : 256;
    const int W = 96, H = 64;
    if (!(threshold >= 0.0f) || maxSamples < 16 || maxSamples % 2) {
        std::fprintf(stderr, "error: threshold >= 0, max_samples even and at least 16\n");
        return 1;
    }
    try {
        auto scene = std::make_shared<Scene>();
        addWalls(*scene);
        scene->addNode(ceilingLight());
        scene->addNode(bluePlate(), Transform(vec3(0.2f, 0.0f, 0.1f)));
        Camera camera(Transform(vec3(0.0f, 1.0f, -8.0f)), 40.0f, (float)W / H, 8.0f); // (frontCamera stands at -3.9, where the room fills the frame)
        camera.m_thinLens = false;
        camera.m_shutterTime = 1.0f;
        const TextureArray noTextures, sky = greySky();
        RayTracer rt(W, H, scene, noTextures, sky);

        pt_adaptive_params prm {};
        prm.threshold = threshold;
        prm.min_samples = 16, prm.round_samples = 16, prm.max_samples = (uint32_t)maxSamples;
        rt.setAdaptive(&prm);
        const pt_adaptive_stats st = rt.rayTraceAdaptive(camera, 0);

        writePPM("adaptive_cornell.ppm", rt.getOutput(), W, H);
        const std::vector<uint32_t> counts = rt.getAdaptiveCounts();
        std::vector<float> heat((size_t)W * H * 4, 1.0f);
        for (size_t i = 0; i < counts.size(); i++) {
            const float v = st.max_count > st.min_count ? (float)(counts[i] - st.min_count) / (float)(st.max_count - st.min_count) : 0.0f;
            heat[i * 4] = heat[i * 4 + 1] = heat[i * 4 + 2] = v;
        }
        writePPM("adaptive_cornell_counts.ppm", heat, W, H);

        const double uniform = (double)W * H * maxSamples;
        std::printf("rounds=%u blocks=%u active_blocks=%u min_count=%u max_count=%u max_block_error=%.4g nonfinite=%u\n", st.rounds, st.blocks, st.active_blocks,
            st.min_count, st.max_count, (double)st.max_block_error, st.nonfinite);
        std::printf("samples_total=%llu uniform=%.0f share=%.3f\n", (unsigned long long)st.samples_total, uniform, (double)st.samples_total / uniform);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 1;
    }
    return 0;
}
