// A static camera at one sample per pixel and frame: the Cornell box of orbit_cornell.cpp, every frame cleared and traced anew with the sample base
// set to the frame number and blended into the temporal history with the luminance variance on (RayTracer::setTemporalVariance).  At frames 1, 8 and
// the last one the history is measured three ways against a converged render of the same view (tone-mapped RMSE, before gamma): as it is, through
// the plain a-trous filter (PT_DENOISE_INPUT_TEMPORAL) and through the variance-guided one (PT_DENOISE_INPUT_TEMPORAL_VARIANCE).
//     usage: converge_cornell [frames] [reference spp]
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

// linear radiance -> exposure -> Reinhard, before gamma: the space the image gates of the tests measure in
static std::vector<double> tonemapped(const std::vector<float>& rgba, double scale, const CameraData& cam)
{
    const double ev = std::log2((double)cam.relativeAperture * cam.relativeAperture / cam.shutterTime * 100.0 / cam.ISO);
    const double exposure = 1.0 / (1.2 * std::exp2(ev));
    std::vector<double> out(rgba.size() / 4 * 3);
    for (size_t i = 0; i < rgba.size() / 4; i++)
        for (int k = 0; k < 3; k++) {
            const double l = rgba[i * 4 + k] * scale * exposure;
            out[i * 3 + k] = l / (1.0 + l);
        }
    return out;
}

static double rmse(const std::vector<double>& a, const std::vector<double>& b)
{
    double s = 0.0;
    for (size_t i = 0; i < a.size(); i++)
        s += (a[i] - b[i]) * (a[i] - b[i]);
    return std::sqrt(s / (double)a.size());
}

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

        Transform camT;
        camT.location = vec3(0.0f, 1.0f, -3.9f); // identity orientation looks down +z
        Camera camera(camT, 40.0f, (float)W / H, 3.9f);
        camera.m_thinLens = false;
        camera.m_shutterTime = 1.0f;
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
