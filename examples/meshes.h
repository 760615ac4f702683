// The meshes more than one example builds: an IMesh that is a NEW Mesh (a new tree) every frame, the unit icosphere, and the leaning blob of
// deforming_cornell.cpp / rebuilt_cornell.cpp.  Plain inline C++ on the kept Mesh / IMesh API, like cornell.h.
#pragma once
#include "../opencl-path-tracer_amd/host/raytracer.h"
#include <algorithm>
#include <cmath>
#include <map>

namespace meshes {
using namespace raytracer;

// what the reference's MeshSequence is to its RayTracer: an IMesh whose arrays are another frame's after goToFrame
class RebuiltMesh : public IMesh {
public:
    RebuiltMesh(std::vector<uint32_t> indices, Material material, BvhBuilder builder = BvhBuilder::BinnedFast)
        : m_indices(std::move(indices)), m_material(material), m_builder(builder) {}
    void goToFrame(const std::vector<float>& positions)
    {
        m_mesh = std::make_shared<Mesh>(positions.data(), nullptr, nullptr, positions.size() / 3, m_indices.data(), nullptr, m_indices.size() / 3,
            std::vector<Material> { m_material }, m_builder);
    }
    const std::vector<VertexSceneData>& getVertices() const override { return m_mesh->getVertices(); }
    const std::vector<TriangleSceneData>& getTriangles() const override { return m_mesh->getTriangles(); }
    const std::vector<Material>& getMaterials() const override { return m_mesh->getMaterials(); }
    const std::vector<SubBVHNode>& getBvhNodes() const override { return m_mesh->getBvhNodes(); }
    const std::vector<uint32_t>& getEmissiveTriangles() const override { return m_mesh->getEmissiveTriangles(); }
    AABB getBounds() const override { return m_mesh->getBounds(); }
    bool isDynamic() const override { return true; }
    uint32_t maxNumVertices() const override { return m_mesh->maxNumVertices(); }
    uint32_t maxNumTriangles() const override { return m_mesh->maxNumTriangles(); }
    uint32_t maxNumMaterials() const override { return m_mesh->maxNumMaterials(); }
    uint32_t maxNumBvhNodes() const override { return m_mesh->maxNumBvhNodes(); }
    void buildBvh() override {}
    uint32_t getBvhRootNode() const override { return m_mesh->getBvhRootNode(); }
    // every frame is built from the same index buffer: the inner mesh's input numbering follows a triangle from tree to tree (RayTracer::setRebuiltMotion)
    const std::vector<uint32_t>* getOriginalTriangles() const override { return m_mesh->getOriginalTriangles(); }

private:
    std::vector<uint32_t> m_indices;
    Material m_material;
    BvhBuilder m_builder;
    std::shared_ptr<Mesh> m_mesh;
};

// unit icosphere, `level` subdivisions (20 * 4^level triangles)
inline void icosphere(int level, std::vector<float>& pos, std::vector<uint32_t>& idx)
{
    const float t = (1.0f + std::sqrt(5.0f)) / 2.0f;
    const float v[12][3] = { { -1, t, 0 }, { 1, t, 0 }, { -1, -t, 0 }, { 1, -t, 0 }, { 0, -1, t }, { 0, 1, t }, { 0, -1, -t }, { 0, 1, -t }, { t, 0, -1 }, { t, 0, 1 }, { -t, 0, -1 }, { -t, 0, 1 } };
    const uint32_t f[20][3] = { { 0, 11, 5 }, { 0, 5, 1 }, { 0, 1, 7 }, { 0, 7, 10 }, { 0, 10, 11 }, { 1, 5, 9 }, { 5, 11, 4 }, { 11, 10, 2 }, { 10, 7, 6 }, { 7, 1, 8 },
        { 3, 9, 4 }, { 3, 4, 2 }, { 3, 2, 6 }, { 3, 6, 8 }, { 3, 8, 9 }, { 4, 9, 5 }, { 2, 4, 11 }, { 6, 2, 10 }, { 8, 6, 7 }, { 9, 8, 1 } };
    auto push = [&](float x, float y, float z) {
        const float n = std::sqrt(x * x + y * y + z * z);
        pos.push_back(x / n), pos.push_back(y / n), pos.push_back(z / n);
        return (uint32_t)(pos.size() / 3 - 1);
    };
    pos.clear(), idx.clear();
    for (const auto& p : v)
        push(p[0], p[1], p[2]);
    for (const auto& tri : f)
        idx.insert(idx.end(), tri, tri + 3);
    for (int l = 0; l < level; l++) {
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> mid;
        auto middle = [&](uint32_t a, uint32_t b) {
            const auto key = std::make_pair(std::min(a, b), std::max(a, b));
            auto it = mid.find(key);
            if (it != mid.end())
                return it->second;
            const uint32_t m = push(pos[3 * a] + pos[3 * b], pos[3 * a + 1] + pos[3 * b + 1], pos[3 * a + 2] + pos[3 * b + 2]);
            mid.emplace(key, m);
            return m;
        };
        std::vector<uint32_t> next;
        for (size_t i = 0; i < idx.size(); i += 3) {
            const uint32_t a = idx[i], b = idx[i + 1], c = idx[i + 2], ab = middle(a, b), bc = middle(b, c), ca = middle(c, a);
            const uint32_t t4[12] = { a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca };
            next.insert(next.end(), t4, t4 + 12);
        }
        idx.swap(next);
    }
}

// a lumpy sphere of radius ~0.45 about the origin: kLat x kLon quads, one vertex per pole and ring position
static const int kLat = 24, kLon = 48;
static const vec3 kBlobAt(-0.15f, 0.55f, 0.0f);

inline void blobRest(std::vector<float>& pos)
{
    const float pi = 3.14159265f;
    pos.clear();
    for (int i = 0; i <= kLat; i++)
        for (int j = 0; j < kLon; j++) {
            const float th = pi * (float)i / kLat, ph = 2.0f * pi * (float)j / kLon;
            const float r = 0.45f * (1.0f + 0.12f * std::sin(3.0f * th) * std::cos(4.0f * ph));
            pos.push_back(r * std::sin(th) * std::cos(ph));
            pos.push_back(r * std::cos(th));
            pos.push_back(r * std::sin(th) * std::sin(ph));
        }
}

inline std::vector<uint32_t> blobIndices()
{
    std::vector<uint32_t> idx;
    for (int i = 0; i < kLat; i++)
        for (int j = 0; j < kLon; j++) {
            const uint32_t a = (uint32_t)(i * kLon + j), b = (uint32_t)((i + 1) * kLon + j), c = (uint32_t)((i + 1) * kLon + (j + 1) % kLon),
                           d = (uint32_t)(i * kLon + (j + 1) % kLon);
            if (i + 1 < kLat) // (at the poles a ring has shrunk to a point: one triangle per quad)
                idx.insert(idx.end(), { a, c, b });
            if (i > 0)
                idx.insert(idx.end(), { a, d, c });
        }
    return idx;
}

// frame f: the blob leans along x by 0.05 per frame at its top and sways along z -- a shear that grows with the square of the height above its foot
inline void blobShape(const std::vector<float>& rest, int frame, std::vector<float>& pos)
{
    pos = rest;
    for (size_t k = 0; k < rest.size(); k += 3) {
        const float h = rest[k + 1] + 0.5f;
        pos[k] += 0.05f * (float)frame * h * h;
        pos[k + 2] += 0.12f * std::sin(0.5f * (float)frame) * h * h;
    }
}

} // namespace meshes
