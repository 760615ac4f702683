// RayTracer with the reference's public surface (src/raytracer.h:20-30) on top of the HIP C-ABI
// (include/ptamd.h).  Differences a caller sees: no GL target (the image is fetched with
// getOutput()/getAccumulator() -- the GPU box is headless), texture arrays are plain float RGBA
// arrays (filled from memory or from Radiance .hdr files, host/image.h) instead of FreeImage-loaded files.
#pragma once
#include "../../include/ptamd.h"
#include "camera.h"
#include "image.h"
#include "scene.h"
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace raytracer {

// what UniqueTextureArray / CLTextureArray hold after loading (src/opencl/texture.h:18-49):
// `layers` RGBA float images of one size, already linear and brightness-scaled
struct TextureArray {
    uint32_t width = 0, height = 0, layers = 0;
    std::vector<float> rgba; // storeAsFloat = true (skydome): r g b a floats
    std::vector<uint8_t> bgra8; // storeAsFloat = false (material textures): b g r a bytes, as the reference uploads them
    bool storeAsFloat() const { return bgra8.empty(); }
    const void* data() const { return storeAsFloat() ? (const void*)rgba.data() : (const void*)bgra8.data(); }
    int add(const float* texels, uint32_t w, uint32_t h)
    {
        if (layers == 0)
            width = w, height = h;
        if (w != width || h != height)
            throw std::invalid_argument("TextureArray: all layers must have the same size");
        if (!bgra8.empty())
            throw std::invalid_argument("TextureArray: float and 8-bit layers cannot be mixed");
        rgba.insert(rgba.end(), texels, texels + (size_t)w * h * 4);
        return (int)layers++;
    }
    // UniqueTextureArray::add(filePath, isLinear = true, brightnessMultiplier) for Radiance .hdr files
    // (src/opencl/texture.cpp:18-49,72-120): the first file fixes the layer size unless one was set, later ones
    // are rescaled to it
    int add(const std::string& hdrFile, float brightnessMultiplier = 1.0f)
    {
        ImageRGBAF img = loadRadianceHDR(hdrFile);
        if (layers == 0 && width == 0)
            width = img.width, height = img.height;
        img = loadSkydomeLayer(hdrFile, width, height, brightnessMultiplier);
        return add(img.rgba.data(), img.width, img.height);
    }
    // CLTextureArray(files, ..., width, height, storeAsFloat = false): every registered file as a layer of that size
    static TextureArray fromFiles(const UniqueTextureFiles& files, uint32_t w, uint32_t h)
    {
        TextureArray t;
        t.width = w, t.height = h;
        for (const TextureFile& f : files.files())
            t.addMaterial(f.path, f.isLinear);
        return t;
    }
    // UniqueTextureArray::add(filePath, isLinear) for the 8-bit material array (PNG files: every texture the reference ships)
    int addMaterial(const std::string& pngFile, bool isLinear = false)
    {
        if (!rgba.empty())
            throw std::invalid_argument("TextureArray: float and 8-bit layers cannot be mixed");
        const ImageRGBA8 img = loadMaterialLayerBGRA8(pngFile, width, height, isLinear); // 0 x 0: the first file fixes the layer size
        if (layers == 0)
            width = img.width, height = img.height;
        if (img.width != width || img.height != height)
            throw std::invalid_argument("TextureArray: all layers must have the same size");
        bgra8.insert(bgra8.end(), img.rgba.begin(), img.rgba.end());
        return (int)layers++;
    }
};

class RayTracer {
public:
    RayTracer(int width, int height, std::shared_ptr<Scene> scene, const TextureArray& materialTextures, const TextureArray& skydomeTextures,
        int device = 0, uint32_t seed = 1);
    ~RayTracer();
    RayTracer(const RayTracer&) = delete;
    RayTracer& operator=(const RayTracer&) = delete;

    void rayTrace(const Camera& camera); // one sample per pixel; resets the accumulation when the camera changed
    void frameTick(); // re-flatten lights + top-level BVH after scene-graph transforms changed (asynchronous upload + flip)
    void updateGeometry(); // after Mesh::refit: new vertices (the device refits its trees); takes effect with the next frameTick.  Not between rebuildGeometry() and
                           // its frameTick(): the device library refuses a refit while a rebuilt scene waits to be adopted (PT_ERR_STATE -> std::runtime_error)
    void rebuildGeometry(); // after meshes of the scene were REPLACED (a new tree per frame, MeshSequence's other branch): converted and copied beside the scene that is rendering; adopted by the next frameTick
    int getSamplesPerPixel() const;
    int getMaxSamplesPerPixel() const { return 20000000; } // MAX_SAMPLES_PER_PIXEL, src/raytracer.cpp:38

    std::vector<float> getOutput(); // width*height RGBA in [0,1]: the `accumulate` kernel's image
    std::vector<float> getAccumulator(); // width*height float4 HDR sums
    // the image of getOutput() through the edge-avoiding a-trous filter (include/ptamd.h, "guides and denoiser"): renders as many guide samples as are
    // missing to match getSamplesPerPixel(), then filters `iterations` times (0..6; 0: getOutput())
    std::vector<float> getDenoisedOutput(int iterations = 5);
    // the same over the temporal history (include/ptamd.h, "temporal history"): blends the frame just traced into the history reprojected into its
    // camera (once per frame: a second call for the same frame filters the same history again), then filters the history `iterations` times.  For a
    // frame loop that moves the camera every frame: setSampleBase(frame); rayTrace(camera); getTemporalOutput().
    std::vector<float> getTemporalOutput(int iterations = 5);
    // Motion vectors for instances re-posed by frameTick (include/ptamd.h, "instance motion"): frameTick keeps the leaves' transforms of the state the last
    // getTemporalOutput blended (the oldest, if several ticks passed since), and the first rayTrace on a cleared accumulator after the tick hands them to
    // the device library -- so the guide samples getTemporalOutput renders carry the motion, and the history follows the instances.  Only while the scene
    // graph's structure is unchanged (same number of leaves: index i then names the same instance), and across rebuildGeometry only with setRebuiltMotion.  On by default; it acts
    // for getTemporalOutput users alone (without a history nothing is set): getOutput / getDenoisedOutput are what they were.  A frame loop with a static
    // camera clears by itself (pt_clear(context())) after its frameTick: rayTrace only clears when the camera changed.
    void setInstanceMotion(bool on) { m_instanceMotion = on; }
    // Motion vectors for meshes refitted between two ticks (include/ptamd.h, "vertex motion"): when updateGeometry handed a refitted mesh over since the
    // previous frameTick, and getTemporalOutput blended a frame of the state that tick replaced, the first rayTrace on a cleared accumulator after the tick
    // sets pt_set_vertex_motion next to the instance motion -- the history follows the deforming surface.  Not across rebuildGeometry (setRebuiltMotion).  On by
    // default.
    void setVertexMotion(bool on) { m_vertexMotion = on; }
    // Motion vectors across rebuildGeometry (include/ptamd.h, "rebuilt motion"): frameTick keeps where every triangle of the flat scene it adopts comes
    // from (its mesh's place in the scene, its input triangle: IMesh::getOriginalTriangles), rebuildGeometry maps the new scene's triangles onto those
    // (triangleHistory, scene.h), and the first rayTrace on a cleared accumulator after the tick hands the map to pt_set_rebuilt_motion -- under
    // setVertexMotion's condition: getTemporalOutput blended a frame of the state the tick replaced.  For meshes that keep their place in the scene and
    // their input numbering from frame to frame (a deforming surface rebuilt every frame); a triangle without a predecessor, and every triangle of a
    // mesh that does not report its origins, keeps or loses its history by depth and normal.  The instance motion then survives a rebuild as well, while
    // the number of leaves stays.  Off by default: the class then does what it did without this call.
    void setRebuiltMotion(bool on);
    // The luminance variance of every pixel's history beside it, and the filter guided by it (include/ptamd.h, "temporal variance"): resets the history
    // (the mode changes only while there is none); from then on getTemporalOutput filters with PT_DENOISE_INPUT_TEMPORAL_VARIANCE -- a static camera's
    // image keeps converging where the fixed-strength filter stops at its own blur.  Off by default.
    void setTemporalVariance(bool on);
    // A short, fast history beside the long one, and a fall-back to it where the lighting changed (include/ptamd.h, "temporal response"): a moving light
    // has no motion vector, and its old shadows would fade over max_history frames.  Resets the history like setTemporalVariance, of which it is
    // independent.  Off by default.
    void setTemporalResponse(bool on);
    // Every frame's demodulated colour bounded by its 5 x 5 neighbourhood before the history and the filter see it (include/ptamd.h, "firefly clamp"):
    // one outlier of a 1-spp frame no longer enters the history at full weight, and a non-finite pixel no longer stays in it.  Acts on getTemporalOutput
    // and getDenoisedOutput (iterations > 0); getOutput and the accumulator are what they were.  Trades energy for variance: single-pixel highlights
    // and caustics lose light.  May change at any time, the history is kept.  Off by default.
    void setFireflyClamp(bool on);
    // Adaptive sampling (include/ptamd.h, "adaptive sampling"): rayTraceAdaptive renders in rounds of params->round_samples and stops the 8 x 8 blocks
    // whose two half images agree to within params->threshold; the accumulator then holds every pixel's mean times getSamplesPerPixel(), so getOutput,
    // getDenoisedOutput and getAccumulator are used as ever.  Turning the mode on or off restarts the accumulation; null turns it off.  While it is on,
    // rayTrace() is refused (std::runtime_error).  rayTraceAdaptive: up to `rounds` rounds, 0 = until every block has stopped or holds max_samples.
    void setAdaptive(const pt_adaptive_params* params);
    pt_adaptive_stats rayTraceAdaptive(const Camera& camera, unsigned rounds = 0);
    std::vector<uint32_t> getAdaptiveCounts(); // width*height: the samples each pixel holds
    // Guide rays follow up to `maxTransmissions` refractions (0..PT_GUIDE_CHAIN_MAX; 0, the default: off) to the first surface that is not glass
    // (include/ptamd.h, "guide chain"): the filter and the history then see the edges and albedos behind a pane or inside a glass body.  Restarts the
    // accumulation (pt_clear: guide sums of two definitions must not mix).  While it is on no instance or vertex motion is handed to the device library
    // (motion deposits along a chain are not supported): moving surfaces keep or lose their history by depth and normal alone.
    void setGuideChain(unsigned maxTransmissions);
    // The guide chain also follows mirrors -- PBR metal of smoothness > 0.94 -- and total internal reflection, within setGuideChain's budget, and
    // tints the terminal's albedo by the mirrors on the way (include/ptamd.h, "guide reflections"): a planar mirror then shows the filter the edges
    // of what it reflects and keeps a history under camera motion that follows the virtual image.  Inert while setGuideChain is 0; small or curved
    // mirrors gain nothing.  Restarts the accumulation like setGuideChain.  Off by default.
    void setGuideReflections(bool on);
    void resetTemporalHistory(); // forget the history: after a cut, or when the scene changed beyond what depth and normal can tell
    void setSampleBase(uint32_t base); // pt_set_sample_base: frames that restart at sample 0 draw other random numbers each
    struct Guides {
        std::vector<float> albedoHits, normalDepth; // width*height float4 sums over `samples` guide samples
        int samples = 0;
    };
    Guides getGuides(); // what the filter is guided by (rendered up to getSamplesPerPixel() like getDenoisedOutput does)
    pt_stats getStats();
    pt_ctx* context() { return m_ctx; }

private:
    void check(int rc, const char* what);
    void renderMissingGuides();
    void upload(const TextureArray& materialTextures, const TextureArray& skydomeTextures); // constructor body proper
    pt_ctx* m_ctx = nullptr;
    std::shared_ptr<Scene> m_scene;
    FlattenedScene m_flat;
    CameraData m_prevCamera;
    bool m_haveCamera = false;
    bool m_temporalDirty = false; // samples were traced since the last getTemporalOutput
    unsigned m_guideChain = 0; // setGuideChain
    bool m_temporalVariance = false; // setTemporalVariance: getTemporalOutput's filter reads the variance plane
    // instance motion: the leaves' invTransform (16 floats each, scene-graph order) of the state the newest history was made under
    bool m_instanceMotion = true;
    std::vector<float> m_prevLeafInv;
    bool m_prevLeafValid = false; // m_prevLeafInv is that state's (false: no history yet, or the geometry was rebuilt since without setRebuiltMotion)
    bool m_blendedThisState = false; // getTemporalOutput blended a frame of the current scene state
    bool m_motionDue = false; // a tick happened: the next rayTrace on a cleared accumulator sets (or leaves unset) the motion
    bool m_rebuilt = false; // rebuildGeometry since the last frameTick
    bool m_vertexMotion = true;
    bool m_refitted = false; // updateGeometry handed a refitted mesh to the device library since the last frameTick
    bool m_vertexDue = false; // ... and that tick replaced the state the newest history was made under: the device library's "then" is the history's
    // rebuilt motion: the triangle origins of the flat scene the last tick adopted, the map rebuildGeometry made against them, the map the last tick owes
    bool m_rebuiltMotion = false;
    std::vector<uint32_t> m_adoptedMesh, m_adoptedOriginal;
    bool m_adoptedValid = false;
    std::vector<uint32_t> m_rebuiltMap, m_rebuiltMapDue;
    bool m_rebuiltMapValid = false; // m_rebuiltMap leads from m_flat to the adopted scene
    bool m_rebuiltDue = false; // ... and the last tick replaced the state the newest history was made under: m_rebuiltMapDue goes to the device library
    void keepAdoptedOrigins();
    void setMotionAfterTick();
    void setInstanceMotionAfterTick();
    int m_width, m_height;
};

} // namespace raytracer
