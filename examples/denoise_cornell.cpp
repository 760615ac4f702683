// A few samples per pixel made presentable: the Cornell box of render_cornell.cpp through the kept Scene / Mesh / Material / Camera / RayTracer
// API, the raw tone-mapped image (getOutput) and the same frame through the edge-avoiding a-trous filter under first-hit guides
// (getDenoisedOutput), each written as a PPM.     usage: denoise_cornell [spp] [raw.ppm] [denoised.ppm]
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
    const int spp = argc > 1 ? std::atoi(argv[1]) : 4;
    const char* rawPath = argc > 2 ? argv[2] : "cornell_raw.ppm";
    const char* denoisedPath = argc > 3 ? argv[3] : "cornell_denoised.ppm";
    const int W = 256, H = 256;
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

        Transform camT(vec3(0.0f, 1.0f, -3.9f)); // identity orientation looks down +z
        Camera camera(camT, 40.0f, (float)W / H, 3.9f);
        camera.m_thinLens = false;
        camera.m_shutterTime = 1.0f; // a long exposure (the default 1/32 s leaves the room a few 8-bit levels above black: nothing to look at, noisy or not)
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
