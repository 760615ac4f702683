// The reference's main loop (src/main.cpp:34-121) without the window: build a Scene through the kept
// Scene / Mesh / Material / Camera / RayTracer API, call rayTrace() N times, write the tone-mapped
// image as a PPM.     usage: render_cornell [spp] [out.ppm]
#include "cornell.h"
#include <cstdio>
#include <cstdlib>

using namespace raytracer;
using namespace cornell;

int main(int argc, char** argv)
{
    const int spp = argc > 1 ? std::atoi(argv[1]) : 64;
    const char* out = argc > 2 ? argv[2] : "cornell.ppm";
    const int W = 256, H = 256;
    try {
        auto scene = std::make_shared<Scene>();
        addWalls(*scene); // floor, ceiling, back, left, right
        scene->addNode(ceilingLight());
        // a copper sphere-ish blob would come from Mesh::fromPLY(".../bun_zipper.ply", Material::PBRMetal(...)) (src/main.cpp:143-155)
        auto box = quadMesh({ -0.3f, 0.6f, -0.3f }, { -0.3f, 0.6f, 0.3f }, { 0.3f, 0.6f, 0.3f }, { 0.3f, 0.6f, -0.3f },
            Material::PBRMetal(vec3(0.955f, 0.638f, 0.538f), 0.8f));
        Transform t;
        t.location = vec3(0.2f, 0.0f, 0.1f);
        scene->addNode(box, t);

        const TextureArray noTextures, sky = greySky();
        RayTracer rt(W, H, scene, noTextures, sky);

        Transform camT(vec3(0.0f, 1.0f, -3.9f)); // identity orientation looks down +z
        Camera camera(camT, 40.0f, (float)W / H, 3.9f);
        camera.m_thinLens = false;
        for (int i = 0; i < spp; i++)
            rt.rayTrace(camera);
        std::vector<float> img = rt.getOutput();
        pt_stats st = rt.getStats();
        writePPM(out, img, W, H);
        double mean = 0;
        for (int i = 0; i < W * H; i++)
            mean += img[i * 4] + img[i * 4 + 1] + img[i * 4 + 2];
        std::printf("spp=%d rays=%llu mean=%.5f -> %s\n", rt.getSamplesPerPixel(), (unsigned long long)(st.rays_extension + st.rays_shadow),
            mean / (3.0 * W * H), out);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
