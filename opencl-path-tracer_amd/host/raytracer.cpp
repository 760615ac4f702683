#include "raytracer.h"
#include <cstring>

namespace raytracer {

void RayTracer::check(int rc, const char* what)
{
    if (rc != PT_OK)
        throw std::runtime_error(std::string(what) + ": " + pt_last_error(m_ctx));
}

RayTracer::RayTracer(int width, int height, std::shared_ptr<Scene> scene, const TextureArray& materialTextures, const TextureArray& skydomeTextures,
    int device, uint32_t seed)
    : m_scene(std::move(scene)), m_width(width), m_height(height)
{
    pt_config cfg {};
    cfg.width = (uint32_t)width;
    cfg.height = (uint32_t)height;
    cfg.device = device;
    cfg.seed = seed;
    cfg.samples_in_flight = 1; // rayTrace() adds exactly one sample per call, like the reference
    if (pt_create(&cfg, &m_ctx) != PT_OK)
        throw std::runtime_error(std::string("pt_create: ") + pt_last_error(nullptr));
    try {
        upload(materialTextures, skydomeTextures);
    } catch (...) { // the destructor does not run for a partially constructed object: release the context here
        pt_destroy(m_ctx);
        m_ctx = nullptr;
        throw;
    }
}

void RayTracer::upload(const TextureArray& materialTextures, const TextureArray& skydomeTextures)
{
    // static geometry once (reference: initBuffersAndTransferStaticData, src/raytracer.cpp:201-287) ...
    flattenStatic(*m_scene, m_flat);
    for (MeshBvhPair& pair : m_scene->getMeshes())
        pair.uploadedGeneration = pair.meshPtr->generation();
    check(pt_upload_static(m_ctx, m_flat.vertices.data(), (uint32_t)m_flat.vertices.size(), m_flat.triangles.data(), (uint32_t)m_flat.triangles.size(),
              m_flat.materials.data(), (uint32_t)m_flat.materials.size(), m_flat.subBvhNodes.data(), (uint32_t)m_flat.subBvhNodes.size()),
        "pt_upload_static");
    if (materialTextures.layers)
        check(pt_upload_texture_array(m_ctx, 0, materialTextures.width, materialTextures.height, materialTextures.layers,
                  materialTextures.storeAsFloat() ? PT_TEX_RGBA32F : PT_TEX_BGRA8_UNORM, materialTextures.data()),
            "pt_upload_texture_array(material)");
    if (skydomeTextures.layers)
        check(pt_upload_texture_array(m_ctx, 1, skydomeTextures.width, skydomeTextures.height, skydomeTextures.layers,
                  skydomeTextures.storeAsFloat() ? PT_TEX_RGBA32F : PT_TEX_BGRA8_UNORM, skydomeTextures.data()),
            "pt_upload_texture_array(skydome)");
    // ... then the dynamic part (lights + top-level BVH), as the reference's constructor ends with frameTick()
    frameTick();
}

RayTracer::~RayTracer() { pt_destroy(m_ctx); }

// transferDynamicData + the flip (reference src/raytracer.cpp:183-189,497-595): lights and top-level BVH from the scene graph as
// it stands, converted and copied into the inactive device buffers on the copy stream while frames enqueued so far keep
// rendering, then adopted by everything enqueued from here on.  No wait on the host.
void RayTracer::frameTick()
{
    // instance motion: the state about to be replaced is the one the newest history was made under if getTemporalOutput blended a frame of it; if not
    // (several ticks without a blend) the transforms kept before stay: the oldest.  The leaves of the top level are nodes [0, instances) in scene-graph
    // order (buildTopBVHOver), so index i names the same instance across ticks while the graph's structure is unchanged.
    if (m_rebuilt && !m_rebuiltMotion) {
        m_prevLeafValid = false; // other meshes: nothing to follow
    } else if (m_blendedThisState) { // (rebuilt meshes that are followed: setInstanceMotionAfterTick's leaf count decides)
        size_t leaves = 0;
        while (leaves < m_flat.topBvhNodes.size() && m_flat.topBvhNodes[leaves].isLeaf)
            leaves++;
        m_prevLeafInv.resize(leaves * 16);
        for (size_t i = 0; i < leaves; i++)
            std::memcpy(&m_prevLeafInv[i * 16], m_flat.topBvhNodes[i].invTransform, 16 * sizeof(float));
        m_prevLeafValid = true;
    }
    // vertex motion: the device library takes the state about to be replaced as "then", which is the history's only under the same condition
    m_vertexDue = m_refitted && m_blendedThisState && !m_rebuilt;
    // rebuilt motion, under the same condition: the map rebuildGeometry made leads from the scene this tick adopts to the one it replaces.  The origins kept
    // are those of the ADOPTED flat scene -- of two rebuildGeometry calls before one tick the second replaced the first on the device too, and its map.
    m_rebuiltDue = m_rebuiltMotion && m_rebuilt && m_blendedThisState && m_rebuiltMapValid;
    if (m_rebuiltDue)
        m_rebuiltMapDue.swap(m_rebuiltMap);
    m_rebuiltMapValid = false;
    if (m_rebuiltMotion && (m_rebuilt || !m_adoptedValid))
        keepAdoptedOrigins();
    m_refitted = false;
    m_blendedThisState = false;
    m_rebuilt = false;
    m_motionDue = true;
    flattenDynamic(*m_scene, m_flat);
    check(pt_upload_dynamic_async(m_ctx, m_flat.emissiveTriangles.data(), (uint32_t)m_flat.emissiveTriangles.size(), m_flat.topBvhNodes.data(),
              (uint32_t)m_flat.topBvhNodes.size(), m_flat.topBvhRoot),
        "pt_upload_dynamic_async");
    check(pt_frame_tick(m_ctx), "pt_frame_tick");
}

// Deformed meshes (Mesh::refit: same topology, new vertices -- the reference rewrites the dynamic tail of its vertex and sub-BVH buffers in
// transferDynamicData, :510-568, after refitting the boxes on the host, src/bvh/refit_bvh.cpp:6-34): every mesh that changed since the last
// call hands its vertices to the device library, which refits its own copy of the trees (pt_refit_vertices) -- no node array travels, the
// host never runs refitBVH in a frame loop (Mesh::refit leaves the boxes to whoever asks for them).  The following frameTick adopts it.
void RayTracer::updateGeometry()
{
    bool hostRoute = false;
    for (MeshBvhPair& pair : m_scene->getMeshes()) {
        const uint64_t gen = pair.meshPtr->generation();
        if (gen == IMesh::kUntracked) { // the mesh does not say when it changes: a dynamic one has changed, a static one never does
            if (pair.meshPtr->isDynamic()) {
                hostRoute = true;
                break;
            }
            continue;
        }
        if (gen == pair.uploadedGeneration)
            continue;
        const auto& verts = pair.meshPtr->getVertices();
        const int rc = pt_refit_vertices(m_ctx, pair.vertexIndexOffset, verts.data(), (uint32_t)verts.size());
        if (rc == PT_ERR_UNSUPPORTED) { // (roots of the sub-BVH array that share a subtree: the bottom-up pass on the device does not apply)
            hostRoute = true;
            break;
        }
        check(rc, "pt_refit_vertices");
        pair.uploadedGeneration = gen;
        m_refitted = true;
    }
    if (hostRoute) { // the reference's way: boxes refitted on the host, the whole vertex and node arrays handed over
        flattenStatic(*m_scene, m_flat);
        check(pt_update_geometry(m_ctx, m_flat.vertices.data(), (uint32_t)m_flat.vertices.size(), m_flat.subBvhNodes.data(), (uint32_t)m_flat.subBvhNodes.size()),
            "pt_update_geometry");
        m_refitted = true;
        for (MeshBvhPair& pair : m_scene->getMeshes())
            pair.uploadedGeneration = pair.meshPtr->generation();
    }
}

// A rebuilt scene (meshes replaced, topology changed -- the else branch of MeshSequence::buildBvh, reference src/model/mesh_sequence.cpp:89-96):
// everything static is flattened again and handed to the device library's second static set on the copy stream; frames keep rendering the old scene
// until the next frameTick, which uploads the new scene's lights and top level and adopts both.
void RayTracer::rebuildGeometry()
{
    flattenStatic(*m_scene, m_flat);
    for (MeshBvhPair& pair : m_scene->getMeshes())
        pair.uploadedGeneration = pair.meshPtr->generation();
    check(pt_upload_static_async(m_ctx, m_flat.vertices.data(), (uint32_t)m_flat.vertices.size(), m_flat.triangles.data(), (uint32_t)m_flat.triangles.size(),
              m_flat.materials.data(), (uint32_t)m_flat.materials.size(), m_flat.subBvhNodes.data(), (uint32_t)m_flat.subBvhNodes.size()),
        "pt_upload_static_async");
    m_rebuilt = true;
    m_rebuiltMapValid = m_rebuiltMotion && m_adoptedValid;
    if (m_rebuiltMapValid)
        m_rebuiltMap = triangleHistory(m_flat.triangleMesh.data(), m_flat.triangleOriginal.data(), m_flat.triangleMesh.size(), m_adoptedMesh.data(),
            m_adoptedOriginal.data(), m_adoptedMesh.size());
}

void RayTracer::keepAdoptedOrigins()
{
    m_adoptedMesh = m_flat.triangleMesh;
    m_adoptedOriginal = m_flat.triangleOriginal;
    m_adoptedValid = true;
}

void RayTracer::setRebuiltMotion(bool on)
{
    m_rebuiltMotion = on;
    m_rebuiltDue = m_rebuiltMapValid = m_adoptedValid = false;
    if (on && !m_rebuilt) // (a rebuilt scene that waits for its tick: m_flat is no longer the adopted one, the origins are kept from that tick on)
        keepAdoptedOrigins();
}

// The first rayTrace on a cleared accumulator after a tick: hand the device library the transforms the leaves had when the newest history was made
// (pt_set_instance_motion wants them before the first guide sample).  Nothing is set without a history, with another number of leaves, or when switched off.
// Next to it the vertex motion, when a mesh was refitted (updateGeometry) since the previous tick and the history is of the state that tick replaced; or,
// under the same condition, the map of a scene that was rebuilt (rebuildGeometry, setRebuiltMotion).
void RayTracer::setMotionAfterTick()
{
    m_motionDue = false;
    setInstanceMotionAfterTick();
    const bool deformed = m_vertexMotion && !m_guideChain && m_vertexDue && pt_temporal_frames(m_ctx) != 0;
    const bool rebuilt = m_rebuiltMotion && !m_guideChain && m_rebuiltDue && !m_rebuiltMapDue.empty() && pt_temporal_frames(m_ctx) != 0;
    m_vertexDue = m_rebuiltDue = false;
    if (deformed)
        check(pt_set_vertex_motion(m_ctx, 1), "pt_set_vertex_motion");
    else if (rebuilt)
        check(pt_set_rebuilt_motion(m_ctx, m_rebuiltMapDue.data(), (uint32_t)m_rebuiltMapDue.size()), "pt_set_rebuilt_motion");
    else if (pt_vertex_motion(m_ctx, nullptr)) // set for an earlier frame of this state: the history has caught up since
        check(pt_set_vertex_motion(m_ctx, 0), "pt_set_vertex_motion");
}

void RayTracer::setInstanceMotionAfterTick()
{
    const std::vector<TopBVHNode>& top = m_flat.topBvhNodes;
    size_t leaves = 0;
    while (leaves < top.size() && top[leaves].isLeaf)
        leaves++;
    bool follow = m_instanceMotion && !m_guideChain && m_prevLeafValid && pt_temporal_frames(m_ctx) != 0 && leaves * 16 == m_prevLeafInv.size();
    for (size_t i = leaves; i < top.size(); i++)
        follow = follow && !top[i].isLeaf; // (leaves behind an inner node: not the host library's top level, the indices mean something else)
    if (!follow) {
        if (pt_instance_motion(m_ctx, nullptr)) // a motion set for an earlier frame of this state: the history has caught up since
            check(pt_set_instance_motion(m_ctx, nullptr, 0), "pt_set_instance_motion");
        return;
    }
    std::vector<float> prev(top.size() * 16, 0.0f); // (entries of inner nodes are ignored)
    std::memcpy(prev.data(), m_prevLeafInv.data(), m_prevLeafInv.size() * sizeof(float));
    check(pt_set_instance_motion(m_ctx, prev.data(), (uint32_t)top.size()), "pt_set_instance_motion");
}

void RayTracer::rayTrace(const Camera& camera)
{
    const CameraData cam = camera.get_camera_data();
    if (!m_haveCamera || std::memcmp(&cam, &m_prevCamera, sizeof(CameraData)) != 0) { // src/raytracer.cpp:99-105
        m_prevCamera = cam;
        m_haveCamera = true;
        check(pt_set_camera(m_ctx, &cam), "pt_set_camera");
        check(pt_clear(m_ctx), "pt_clear");
    }
    if (getSamplesPerPixel() >= getMaxSamplesPerPixel())
        return;
    if (m_motionDue && pt_samples_per_pixel(m_ctx) == 0 && pt_guide_samples(m_ctx) == 0)
        setMotionAfterTick();
    check(pt_render(m_ctx, 1), "pt_render");
    m_temporalDirty = true;
    check(pt_synchronize(m_ctx), "pt_synchronize"); // queue.finish(), src/raytracer.cpp:117-118
}

int RayTracer::getSamplesPerPixel() const { return (int)pt_samples_per_pixel(m_ctx); }

std::vector<float> RayTracer::getOutput()
{
    std::vector<float> out((size_t)m_width * m_height * 4);
    check(pt_resolve(m_ctx, out.data()), "pt_resolve");
    return out;
}

std::vector<float> RayTracer::getAccumulator()
{
    std::vector<float> out((size_t)m_width * m_height * 4);
    check(pt_read_accum(m_ctx, out.data()), "pt_read_accum");
    return out;
}

void RayTracer::renderMissingGuides()
{
    const uint32_t want = pt_samples_per_pixel(m_ctx), have = pt_guide_samples(m_ctx);
    if (have < want)
        check(pt_render_guides(m_ctx, want - have), "pt_render_guides");
}

std::vector<float> RayTracer::getDenoisedOutput(int iterations)
{
    renderMissingGuides();
    pt_denoise_params prm {};
    prm.iterations = (uint32_t)iterations;
    prm.output = PT_DENOISE_TONEMAPPED;
    std::vector<float> out((size_t)m_width * m_height * 4);
    check(pt_denoise(m_ctx, &prm, out.data(), nullptr), "pt_denoise");
    return out;
}

std::vector<float> RayTracer::getTemporalOutput(int iterations)
{
    renderMissingGuides();
    if (m_temporalDirty || pt_temporal_frames(m_ctx) == 0) {
        pt_temporal_params tp {};
        check(pt_temporal_accumulate(m_ctx, &tp), "pt_temporal_accumulate");
        m_temporalDirty = false;
        m_blendedThisState = true; // the newest history is of this scene state: the next frameTick keeps its transforms
        m_prevLeafValid = false;
        if (pt_instance_motion(m_ctx, nullptr) || pt_vertex_motion(m_ctx, nullptr))
            m_motionDue = true; // ... and a further frame of this state must not be moved again
    }
    pt_denoise_params prm {};
    prm.iterations = (uint32_t)iterations;
    prm.output = PT_DENOISE_TONEMAPPED;
    prm.input = m_temporalVariance ? PT_DENOISE_INPUT_TEMPORAL_VARIANCE : PT_DENOISE_INPUT_TEMPORAL;
    std::vector<float> out((size_t)m_width * m_height * 4);
    check(pt_denoise(m_ctx, &prm, out.data(), nullptr), "pt_denoise");
    return out;
}

void RayTracer::setTemporalVariance(bool on)
{
    check(pt_temporal_reset(m_ctx), "pt_temporal_reset");
    const pt_variance_params defaults {};
    check(pt_set_temporal_variance(m_ctx, on ? &defaults : nullptr), "pt_set_temporal_variance");
    m_temporalVariance = on;
}

void RayTracer::setTemporalResponse(bool on)
{
    check(pt_temporal_reset(m_ctx), "pt_temporal_reset");
    const pt_response_params defaults {};
    check(pt_set_temporal_response(m_ctx, on ? &defaults : nullptr), "pt_set_temporal_response");
}

void RayTracer::setFireflyClamp(bool on)
{
    const pt_firefly_params defaults {};
    check(pt_set_firefly_clamp(m_ctx, on ? &defaults : nullptr), "pt_set_firefly_clamp");
}

void RayTracer::setAdaptive(const pt_adaptive_params* params)
{
    if ((params != nullptr) != (pt_adaptive(m_ctx) != 0)) // the mode changes only while there are no samples
        check(pt_clear(m_ctx), "pt_clear");
    check(pt_set_adaptive(m_ctx, params), "pt_set_adaptive");
}

pt_adaptive_stats RayTracer::rayTraceAdaptive(const Camera& camera, unsigned rounds)
{
    const CameraData cam = camera.get_camera_data();
    if (!m_haveCamera || std::memcmp(&cam, &m_prevCamera, sizeof(CameraData)) != 0) { // as rayTrace
        m_prevCamera = cam;
        m_haveCamera = true;
        check(pt_set_camera(m_ctx, &cam), "pt_set_camera");
        check(pt_clear(m_ctx), "pt_clear");
    }
    check(pt_render_adaptive(m_ctx, rounds), "pt_render_adaptive"); // (synchronous at the end of every round)
    m_temporalDirty = true;
    pt_adaptive_stats st {};
    check(pt_adaptive_stats_get(m_ctx, &st), "pt_adaptive_stats_get");
    return st;
}

std::vector<uint32_t> RayTracer::getAdaptiveCounts()
{
    std::vector<uint32_t> out((size_t)m_width * m_height);
    check(pt_read_adaptive(m_ctx, nullptr, nullptr, out.data(), nullptr, nullptr), "pt_read_adaptive");
    return out;
}

void RayTracer::setGuideChain(unsigned maxTransmissions)
{
    check(pt_clear(m_ctx), "pt_clear"); // (the chain changes, and a motion is forgotten, only while no guide samples are in the sums)
    if (maxTransmissions != 0) {
        if (pt_instance_motion(m_ctx, nullptr))
            check(pt_set_instance_motion(m_ctx, nullptr, 0), "pt_set_instance_motion");
        if (pt_vertex_motion(m_ctx, nullptr))
            check(pt_set_vertex_motion(m_ctx, 0), "pt_set_vertex_motion");
    }
    check(pt_set_guide_chain(m_ctx, maxTransmissions), "pt_set_guide_chain");
    m_guideChain = maxTransmissions;
}

void RayTracer::setGuideReflections(bool on)
{
    check(pt_clear(m_ctx), "pt_clear"); // (like the chain: it changes only while no guide samples are in the sums)
    check(pt_set_guide_reflections(m_ctx, on ? 1 : 0), "pt_set_guide_reflections");
}

void RayTracer::resetTemporalHistory() { check(pt_temporal_reset(m_ctx), "pt_temporal_reset"); }

void RayTracer::setSampleBase(uint32_t base) { check(pt_set_sample_base(m_ctx, base), "pt_set_sample_base"); }

RayTracer::Guides RayTracer::getGuides()
{
    renderMissingGuides();
    Guides g;
    g.albedoHits.resize((size_t)m_width * m_height * 4);
    g.normalDepth.resize((size_t)m_width * m_height * 4);
    check(pt_read_guides(m_ctx, g.albedoHits.data(), g.normalDepth.data()), "pt_read_guides");
    g.samples = (int)pt_guide_samples(m_ctx);
    return g;
}

pt_stats RayTracer::getStats()
{
    pt_stats s;
    check(pt_stats_get(m_ctx, &s), "pt_stats_get");
    return s;
}

} // namespace raytracer
