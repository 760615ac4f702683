// A few samples per pixel made presentable: the Cornell box of render_cornell.cpp through the kept Scene / Mesh / Material / Camera / RayTracer
// API, the raw tone-mapped image (getOutput) and the same frame through the edge-avoiding a-trous filter under first-hit guides
// (getDenoisedOutput), each written as a PPM.     usage: denoise_cornell [spp] [raw.ppm] [denoised.ppm]
#include "cornell.h"
#include <cstdio>
#include <cstdlib>

using namespace raytracer;
using namespace cornell;

int main(int argc, char** argv)
{
    const int spp = argc > 1 ? std::atoi(argv[1]) : 4;
    const char* rawPath = argc > 2 ? argv[2] : "cornell_raw.ppm";
    const char* denoisedPath = argc > 3 ? argv[3] : "cornell_denoised.ppm";
    const int W = 256, H = 256;
    try {
        auto scene = std::make_shared<Scene>();
        addWalls(*scene); // floor, ceiling, back, left, right
        scene->addNode(ceilingLight());
        scene->addNode(bluePlate(), Transform(vec3(0.2f, 0.0f, 0.1f)));

        const TextureArray noTextures, sky = greySky();
        RayTracer rt(W, H, scene, noTextures, sky);

        const Camera camera = frontCamera(W, H);
        for (int i = 0; i < spp; i++)
            rt.rayTrace(camera);
        const std::vector<float> raw = rt.getOutput(), denoised = rt.getDenoisedOutput();
        const RayTracer::Guides g = rt.getGuides();
        writePPM(rawPath, raw, W, H);
        writePPM(denoisedPath, denoised, W, H);
        double covered = 0;
        for (int i = 0; i < W * H; i++)
            covered += g.albedoHits[i * 4 + 3];
        std::printf("spp=%d guide_samples=%d coverage=%.4f -> %s %s\n", rt.getSamplesPerPixel(), g.samples, covered / ((double)W * H * g.samples), rawPath,
            denoisedPath);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
