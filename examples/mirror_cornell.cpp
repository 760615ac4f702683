// What guide reflections buy a frame loop in front of a mirror: the Cornell room with a blue plate and a polished metal wall (the quad x in [-0.8, 0.8],
// y in [0.2, 1.8] at z = 0.99, PBR metal of reflectance 0.9 and smoothness 1) from a camera that orbits the room's centre, 2 degrees per frame.  Twelve
// frames of one sample per pixel, each blended into the temporal history and filtered (getTemporalOutput) -- once with first-hit guides, once with
// RayTracer::setGuideChain(K) and setGuideReflections(true).  Printed for both: the RMSE of the last frame's output against 256 samples per pixel from
// the same camera (both through pt_resolve's tone curve) over the pixels that show the mirror and over the rest, and the mean history count in both
// regions -- with first-hit guides the mirror keeps a history it should lose (it reprojects where the mirror was, not where the reflection was).  These
// are measurements, not a gate.
//     usage: mirror_cornell [frames] [chain K] [first_hit.ppm] [reflections.ppm]
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

static Camera orbitCamera(float angle, int W, int H)
{
    const vec3 centre(0.0f, 1.0f, 0.0f);
    Transform camT(centre, quat::angleAxis(angle, vec3(0.0f, 1.0f, 0.0f)));
    camT.location = centre + camT.transformDirection(vec3(0.0f, 0.0f, -3.9f)); // identity orientation looks down +z
    Camera camera(camT, 40.0f, (float)W / H, 3.9f);
    camera.m_thinLens = false;
    camera.m_shutterTime = 1.0f;
    return camera;
}

struct Run {
    std::vector<float> image, depth, count; // the last frame's output; its guides' distance; the history count N
};

// `frames` 1-spp frames along the orbit (the last one at angle 0), history + filter
static Run frameLoop(RayTracer& rt, unsigned chain, int frames, int W, int H)
{
    const float step = 2.0f * 3.14159265f / 180.0f;
    rt.setGuideChain(chain);
    rt.setGuideReflections(chain != 0u);
    rt.resetTemporalHistory();
    Run r;
    for (int f = 0; f < frames; f++) {
        rt.setSampleBase((uint32_t)f);
        rt.rayTrace(orbitCamera(step * (float)(f - frames + 1), W, H)); // the camera changed: clears, then one sample per pixel
        r.image = rt.getTemporalOutput();
    }
    const RayTracer::Guides g = rt.getGuides();
    std::vector<float> history((size_t)W * H * 4);
    if (pt_read_temporal(rt.context(), history.data(), nullptr) != PT_OK)
        throw std::runtime_error("pt_read_temporal failed");
    r.depth.resize((size_t)W * H), r.count.resize((size_t)W * H);
    for (int i = 0; i < W * H; i++)
        r.depth[i] = g.normalDepth[i * 4 + 3] / (float)g.samples, r.count[i] = history[i * 4 + 3];
    return r;
}

int main(int argc, char** argv)
{
    const int frames = argc > 1 ? std::atoi(argv[1]) : 12;
    const int chain = argc > 2 ? std::atoi(argv[2]) : 2;
    const char* firstPath = argc > 3 ? argv[3] : "mirror_first_hit.ppm";
    const char* chainPath = argc > 4 ? argv[4] : "mirror_reflections.ppm";
    const int W = 256, H = 256;
    if (frames < 1 || chain < 1 || chain > (int)PT_GUIDE_CHAIN_MAX) {
        std::fprintf(stderr, "error: frames must be at least 1, the chain 1..%u\n", PT_GUIDE_CHAIN_MAX);
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
        scene->addNode(quadMesh({ -0.8f, 0.2f, 0.99f }, { -0.8f, 1.8f, 0.99f }, { 0.8f, 1.8f, 0.99f }, { 0.8f, 0.2f, 0.99f }, Material::PBRMetal(vec3(0.9f), 1.0f))); // the mirror, into the room

        TextureArray noTextures, sky;
        const float grey[4] = { 0.4f, 0.4f, 0.4f, 1.0f };
        sky.add(grey, 1, 1);
        RayTracer rt(W, H, scene, noTextures, sky);

        const Run first = frameLoop(rt, 0u, frames, W, H), through = frameLoop(rt, (unsigned)chain, frames, W, H);
        // the reference: 256 samples per pixel from the last frame's camera
        rt.setGuideChain(0u);
        rt.setGuideReflections(false);
        rt.setSampleBase(1000u);
        const Camera last = orbitCamera(0.0f, W, H);
        for (int s = 0; s < 256; s++)
            rt.rayTrace(last);
        const std::vector<float> ref = rt.getOutput();

        // in the mirror: where the chain's distance lies behind the first hit's
        double err[2][2] = {}, count[2][2] = {};
        size_t pixels[2] = {};
        for (int i = 0; i < W * H; i++) {
            const int region = through.depth[i] > first.depth[i] + 1e-3f ? 0 : 1;
            pixels[region]++;
            for (int k = 0; k < 3; k++) {
                const double a = first.image[i * 4 + k] - ref[i * 4 + k], b = through.image[i * 4 + k] - ref[i * 4 + k];
                err[0][region] += a * a, err[1][region] += b * b;
            }
            count[0][region] += first.count[i], count[1][region] += through.count[i];
        }
        const char* names[2] = { "in the mirror", "outside the mirror" };
        for (int region = 0; region < 2; region++) {
            const double n = (double)(pixels[region] ? pixels[region] : 1);
            std::printf("%s (%zu pixels): RMSE against 256 spp  first-hit guides %.5f  reflections K=%d %.5f  ratio %.3f;  mean history count  %.2f  %.2f\n", names[region],
                pixels[region], std::sqrt(err[0][region] / (3.0 * n)), chain, std::sqrt(err[1][region] / (3.0 * n)),
                std::sqrt(err[1][region] / (err[0][region] > 0 ? err[0][region] : 1.0)), count[0][region] / n, count[1][region] / n);
        }
        writePPM(firstPath, first.image, W, H);
        writePPM(chainPath, through.image, W, H);
        std::printf("frames=%d chain=%d -> %s %s\n", frames, chain, firstPath, chainPath);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
