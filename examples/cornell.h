// What the examples share: the quad they build everything from, the Cornell room's fixed parts, its two cameras, the grey sky, the PPM writer and the
// tone-mapped RMSE.  Plain inline C++ on the kept Scene / Mesh / Material / Camera / RayTracer API -- no scene description, nothing configurable: an example
// whose room, camera or output differs from these writes its own out.  The order of Scene::addNode calls decides instance and light indices, so every
// example adds the parts itself, in its own order.
#pragma once
#include "../opencl-path-tracer_amd/host/raytracer.h"
#include <cmath>
#include <cstdio>

namespace cornell {
using namespace raytracer;

inline std::shared_ptr<Mesh> quadMesh(vec3 a, vec3 b, vec3 c, vec3 d, const Material& m)
{
    const float pos[12] = { a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, d.x, d.y, d.z };
    const uint32_t idx[6] = { 0, 1, 2, 0, 2, 3 };
    return std::make_shared<Mesh>(pos, nullptr, nullptr, 4, idx, nullptr, 2, std::vector<Material> { m }, BvhBuilder::BinnedSAH);
}

// the room x, z in [-1, 1], y in [0, 2], open towards -z: white floor, ceiling and back wall, green left, red right -- five nodes in that order
inline void addWalls(Scene& scene)
{
    const Material white = Material::Diffuse(vec3(0.73f)), green = Material::Diffuse(vec3(0.12f, 0.45f, 0.15f)), red = Material::Diffuse(vec3(0.65f, 0.05f, 0.05f));
    scene.addNode(quadMesh({ -1, 0, -1 }, { -1, 0, 1 }, { 1, 0, 1 }, { 1, 0, -1 }, white)); // floor
    scene.addNode(quadMesh({ -1, 2, -1 }, { 1, 2, -1 }, { 1, 2, 1 }, { -1, 2, 1 }, white)); // ceiling
    scene.addNode(quadMesh({ -1, 0, 1 }, { -1, 2, 1 }, { 1, 2, 1 }, { 1, 0, 1 }, white)); // back
    scene.addNode(quadMesh({ -1, 0, -1 }, { -1, 2, -1 }, { -1, 2, 1 }, { -1, 0, 1 }, green)); // left
    scene.addNode(quadMesh({ 1, 0, -1 }, { 1, 0, 1 }, { 1, 2, 1 }, { 1, 2, -1 }, red)); // right
}

// the half-metre light just under the ceiling's centre, in world coordinates
inline std::shared_ptr<Mesh> ceilingLight()
{
    return quadMesh({ -0.25f, 1.98f, -0.25f }, { 0.25f, 1.98f, -0.25f }, { 0.25f, 1.98f, 0.25f }, { -0.25f, 1.98f, 0.25f }, Material::Emissive(vec3(1.0f, 0.92f, 0.8f), 12.0f));
}

// the blue plate, 0.6 x 0.6 at y = 0.6 about the vertical axis; the examples stand it at (0.2, 0, 0.1)
inline std::shared_ptr<Mesh> bluePlate()
{
    return quadMesh({ -0.3f, 0.6f, -0.3f }, { -0.3f, 0.6f, 0.3f }, { 0.3f, 0.6f, 0.3f }, { 0.3f, 0.6f, -0.3f }, Material::Diffuse(vec3(0.2f, 0.3f, 0.7f)));
}

// a 1 x 1 skydome of grey 0.4
inline TextureArray greySky()
{
    TextureArray sky;
    const float grey[4] = { 0.4f, 0.4f, 0.4f, 1.0f };
    sky.add(grey, 1, 1);
    return sky;
}

// a pinhole camera 3.9 from the room's centre (0, 1, 0), turned about the vertical axis through it, 40 degrees, a 1 s exposure (the default 1/32 s leaves
// the room a few 8-bit levels above black)
inline Camera orbitCamera(float angle, int W, int H)
{
    const vec3 centre(0.0f, 1.0f, 0.0f);
    Transform camT(centre, quat::angleAxis(angle, vec3(0.0f, 1.0f, 0.0f)));
    camT.location = centre + camT.transformDirection(vec3(0.0f, 0.0f, -3.9f)); // identity orientation looks down +z
    Camera camera(camT, 40.0f, (float)W / H, 3.9f);
    camera.m_thinLens = false;
    camera.m_shutterTime = 1.0f;
    return camera;
}

// the same camera in front of the opening, at (0, 1, -3.9)
inline Camera frontCamera(int W, int H)
{
    Camera camera(Transform(vec3(0.0f, 1.0f, -3.9f)), 40.0f, (float)W / H, 3.9f); // identity orientation looks down +z
    camera.m_thinLens = false;
    camera.m_shutterTime = 1.0f;
    return camera;
}

// float RGBA in [0, 1] (getOutput and its kin) as an 8-bit binary PPM
inline void writePPM(const char* path, const std::vector<float>& img, int W, int H)
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

// linear radiance -> exposure -> Reinhard, before gamma: the space the image gates of the tests measure in
inline std::vector<double> tonemapped(const std::vector<float>& rgba, double scale, const CameraData& cam)
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

inline double rmse(const std::vector<double>& a, const std::vector<double>& b)
{
    double s = 0.0;
    for (size_t i = 0; i < a.size(); i++)
        s += (a[i] - b[i]) * (a[i] - b[i]);
    return std::sqrt(s / (double)a.size());
}

} // namespace cornell
