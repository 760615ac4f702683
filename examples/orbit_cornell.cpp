// A moving camera at one sample per pixel: the Cornell box of denoise_cornell.cpp seen from a short orbit about the room's centre, every frame
// cleared and traced anew (RayTracer::rayTrace does that when the camera changed) with the sample base set to the frame number, and blended
// into the temporal history reprojected into its camera (getTemporalOutput).  The last frame is written three times as a PPM: raw (getOutput),
// filtered alone (getDenoisedOutput), filtered over the history (getTemporalOutput).
//     usage: orbit_cornell [frames] [raw.ppm] [filtered.ppm] [temporal.ppm]
#include "../opencl-path-tracer_amd/host/raytracer.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace raytracer;

static std::shared_ptr<Mesh> quadMesh(vec3 a, vec3 b, vec3 c, vec3 d, const Material& m)
{
    const float pos[12] = { a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, d.x, d.y, d.z };
    const uint32_t idx[6] = { 0, 1, 2, 0, 2, 3 };
    return std::make_shared<Mesh>(pos, nullptr, nullptr, 4, idx, nullptr, 2, std::vector<Material> { m }, BvhBuilder::BinnedSAH);
}

static void writePPM(const char* path, const std::vector<float>& img, int W, int H)
{
    FILE* f = std::fopen(path, "wb");
    if (!f)
        throw std::runtime_error("cannot write output");
    std::fprintf(f, "P6\n%d %d\n255\n", W, H);
    for (int i = 0; i < W * H; i++)
        for (int k = 0; k < 3; k++)
            std::fputc((int)(std::fmin(1.0f, std::fmax(0.0f, img[i * 4 + k])) * 255.0f + 0.5f), f);
    std::fclose(f);
}

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
        const Material white = Material::Diffuse(vec3(0.73f)), green = Material::Diffuse(vec3(0.12f, 0.45f, 0.15f)),
                       red = Material::Diffuse(vec3(0.65f, 0.05f, 0.05f));
        scene->addNode(quadMesh({ -1, 0, -1 }, { -1, 0, 1 }, { 1, 0, 1 }, { 1, 0, -1 }, white)); // floor
        scene->addNode(quadMesh({ -1, 2, -1 }, { 1, 2, -1 }, { 1, 2, 1 }, { -1, 2, 1 }, white)); // ceiling
        scene->addNode(quadMesh({ -1, 0, 1 }, { -1, 2, 1 }, { 1, 2, 1 }, { 1, 0, 1 }, white)); // back
        scene->addNode(quadMesh({ -1, 0, -1 }, { -1, 2, -1 }, { -1, 2, 1 }, { -1, 0, 1 }, green)); // left
        scene->addNode(quadMesh({ 1, 0, -1 }, { 1, 0, 1 }, { 1, 2, 1 }, { 1, 2, -1 }, red)); // right
        scene->addNode(quadMesh({ -0.25f, 1.98f, -0.25f }, { 0.25f, 1.98f, -0.25f }, { 0.25f, 1.98f, 0.25f }, { -0.25f, 1.98f, 0.25f },
            Material::Emissive(vec3(1.0f, 0.92f, 0.8f), 12.0f)));
        auto plate = quadMesh({ -0.3f, 0.6f, -0.3f }, { -0.3f, 0.6f, 0.3f }, { 0.3f, 0.6f, 0.3f }, { 0.3f, 0.6f, -0.3f }, Material::Diffuse(vec3(0.2f, 0.3f, 0.7f)));
        Transform t;
        t.location = vec3(0.2f, 0.0f, 0.1f);
        scene->addNode(plate, t);

        TextureArray noTextures, sky;
        const float grey[4] = { 0.4f, 0.4f, 0.4f, 1.0f };
        sky.add(grey, 1, 1);
        RayTracer rt(W, H, scene, noTextures, sky);

        const vec3 centre(0.0f, 1.0f, 0.0f);
        const float step = 1.5f * 3.14159265f / 180.0f; // 1.5 degrees per frame about the vertical axis through the room's centre
        std::vector<float> temporal;
        for (int f = 0; f < frames; f++) {
            Transform camT(centre, quat::angleAxis(step * (float)(f - frames + 1), vec3(0.0f, 1.0f, 0.0f)));
            camT.location = centre + camT.transformDirection(vec3(0.0f, 0.0f, -3.9f)); // identity orientation looks down +z: the last frame is denoise_cornell's view
            Camera camera(camT, 40.0f, (float)W / H, 3.9f);
            camera.m_thinLens = false;
            camera.m_shutterTime = 1.0f;
            rt.setSampleBase((uint32_t)f); // every frame restarts at sample 0 of ITS OWN random numbers
            rt.rayTrace(camera); // the camera changed: clears, then one sample per pixel
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
