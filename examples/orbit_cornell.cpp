// A moving camera at one sample per pixel: the Cornell box of denoise_cornell.cpp seen from a short orbit about the room's centre, every frame
// cleared and traced anew (RayTracer::rayTrace does that when the camera changed) with the sample base set to the frame number, and blended
// into the temporal history reprojected into its camera (getTemporalOutput).  The last frame is written three times as a PPM: raw (getOutput),
// filtered alone (getDenoisedOutput), filtered over the history (getTemporalOutput).
//     usage: orbit_cornell [frames] [raw.ppm] [filtered.ppm] [temporal.ppm]
#include "cornell.h"
#include <cstdio>
#include <cstdlib>

using namespace raytracer;
using namespace cornell;

int main(int argc, char** argv)
{
    const int frames = argc > 1 ? std::atoi(argv[1]) : 12;
    const char* rawPath = argc > 2 ? argv[2] : "orbit_raw.ppm";
    const char* filteredPath = argc > 3 ? argv[3] : "orbit_filtered.ppm";
    const char* temporalPath = argc > 4 ? argv[4] : "orbit_temporal.ppm";
    const int W = 256, H = 256;
    if (frames < 1) {
        std::fprintf(stderr, "error: frames must be at least 1\n");
        return 1;
    }
    try {
        auto scene = std::make_shared<Scene>();
        addWalls(*scene); // floor, ceiling, back, left, right
        scene->addNode(ceilingLight());
        scene->addNode(bluePlate(), Transform(vec3(0.2f, 0.0f, 0.1f)));

        const TextureArray noTextures, sky = greySky();
        RayTracer rt(W, H, scene, noTextures, sky);

        const float step = 1.5f * 3.14159265f / 180.0f; // 1.5 degrees per frame about the vertical axis through the room's centre
        std::vector<float> temporal;
        for (int f = 0; f < frames; f++) {
            rt.setSampleBase((uint32_t)f); // every frame restarts at sample 0 of ITS OWN random numbers
            rt.rayTrace(orbitCamera(step * (float)(f - frames + 1), W, H)); // the camera changed: clears, then one sample per pixel.  The last frame is denoise_cornell's view
            temporal = rt.getTemporalOutput(); // blends this frame into the reprojected history, then filters the history
        }
        const std::vector<float> raw = rt.getOutput(), filtered = rt.getDenoisedOutput();
        writePPM(rawPath, raw, W, H);
        writePPM(filteredPath, filtered, W, H);
        writePPM(temporalPath, temporal, W, H);
        std::printf("frames=%d spp=%d temporal_frames=%u -> %s %s %s\n", frames, rt.getSamplesPerPixel(), pt_temporal_frames(rt.context()), rawPath,
            filteredPath, temporalPath);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
