// The loop of deforming_cornell.cpp with the blob REBUILT every frame: a new Mesh and a new tree per frame (a RebuiltMesh, the fast binned builder),
// RayTracer::rebuildGeometry and frameTick, every frame cleared, traced at one sample per pixel with the sample base set to the frame number and blended
// into the temporal history.  A rebuilt tree numbers its triangles anew, so nothing followed such a surface before; with RayTracer::setRebuiltMotion the
// class maps every triangle onto the one it was in the tree before (the builder's originalTriangle) and the history follows the surface.  The loop runs
// twice, without and with it, and prints for both: the mean history count over the blob's pixels of the last frame and the tone-mapped RMSE of the
// filtered history against `reference spp` of the last shape.  Exit status 2 unless the count is larger and the RMSE smaller with the motion.
//     usage: rebuilt_cornell [frames] [size] [reference spp]
#include "cornell.h"
#include "meshes.h"
#include <cstdio>
#include <cstdlib>

using namespace raytracer;
using namespace cornell;
using namespace meshes;

static const vec3 kBlobColour(0.2f, 0.3f, 0.7f);

struct Room {
    std::shared_ptr<Scene> scene = std::make_shared<Scene>();
    std::shared_ptr<RebuiltMesh> blob = std::make_shared<RebuiltMesh>(blobIndices(), Material::Diffuse(kBlobColour));
    std::vector<float> rest, pos;
    explicit Room(int frame)
    {
        addWalls(*scene); // floor, ceiling, back, left, right
        scene->addNode(ceilingLight());
        blobRest(rest);
        shape(frame);
        scene->addNode(blob, Transform(kBlobAt));
    }
    void shape(int frame)
    {
        blobShape(rest, frame, pos);
        blob->goToFrame(pos); // a new mesh: a new tree, its triangles in a new order
    }
};

static void check(int rc, RayTracer& rt)
{
    if (rc != PT_OK)
        throw std::runtime_error(pt_last_error(rt.context()));
}

struct Result {
    std::vector<float> filtered, count; // the filtered history, linear; the history count per pixel
    std::vector<char> blob; // the pixels whose first hit is the blob, by its albedo
    uint32_t followed = 0; // triangles the last frame's map followed
};

static Result run(int frames, bool rebuiltMotion, const Camera& camera, int W, int H)
{
    Room room(0);
    const TextureArray noTextures, sky = greySky();
    RayTracer rt(W, H, room.scene, noTextures, sky);
    rt.setRebuiltMotion(rebuiltMotion);
    Result r;
    for (int f = 0; f < frames; f++) {
        if (f) {
            room.shape(f);
            rt.rebuildGeometry(); // the new tree goes beside the one that is rendering ...
            rt.frameTick(); // ... and is adopted; the records of the tree before stay on the device as "then"
            check(pt_clear(rt.context()), rt); // the camera stands still: rayTrace would go on accumulating
        }
        rt.setSampleBase((uint32_t)f);
        rt.rayTrace(camera); // the first sample after a tick: hands the map over, then one sample per pixel
        pt_rebuilt_motion(rt.context(), &r.followed);
        rt.getTemporalOutput(0); // blends this frame into the history
    }
    const size_t n = (size_t)W * H;
    r.filtered.resize(n * 4);
    pt_denoise_params prm {};
    prm.iterations = 5u;
    prm.output = PT_DENOISE_HDR;
    prm.input = PT_DENOISE_INPUT_TEMPORAL;
    check(pt_denoise(rt.context(), &prm, r.filtered.data(), nullptr), rt);
    std::vector<float> colourCount(n * 4);
    check(pt_read_temporal(rt.context(), colourCount.data(), nullptr), rt);
    const RayTracer::Guides g = rt.getGuides();
    r.count.resize(n), r.blob.resize(n);
    for (size_t i = 0; i < n; i++) {
        r.count[i] = colourCount[i * 4 + 3];
        const float* a = &g.albedoHits[i * 4];
        const float s = (float)g.samples;
        r.blob[i] = a[3] == s && std::fabs(a[0] / s - kBlobColour.x) < 1e-3f && std::fabs(a[1] / s - kBlobColour.y) < 1e-3f && std::fabs(a[2] / s - kBlobColour.z) < 1e-3f;
    }
    return r;
}

int main(int argc, char** argv)
{
    const int frames = argc > 1 ? std::atoi(argv[1]) : 12, size = argc > 2 ? std::atoi(argv[2]) : 256, referenceSpp = argc > 3 ? std::atoi(argv[3]) : 256;
    if (frames < 2 || size < 16 || referenceSpp < 1) {
        std::fprintf(stderr, "error: at least 2 frames, 16 pixels and 1 reference sample\n");
        return 1;
    }
    const int W = size, H = size;
    try {
        const Camera camera = frontCamera(W, H);
        const CameraData cam = camera.get_camera_data();
        std::vector<double> want; // the converged view of the last shape, from random numbers no frame draws
        {
            Room room(frames - 1);
            const TextureArray noTextures, sky = greySky();
            RayTracer rt(W, H, room.scene, noTextures, sky);
            rt.setSampleBase(1000000u);
            for (int s = 0; s < referenceSpp; s++)
                rt.rayTrace(camera);
            want = tonemapped(rt.getAccumulator(), 1.0 / referenceSpp, cam);
        }
        const Result plain = run(frames, false, camera, W, H), motion = run(frames, true, camera, W, H);
        if (plain.blob != motion.blob)
            throw std::runtime_error("the two loops do not see the blob in the same pixels");
        double count[2] = { 0.0, 0.0 }, e[2] = { 0.0, 0.0 };
        size_t pixels = 0;
        const Result* both[2] = { &plain, &motion };
        for (int k = 0; k < 2; k++) {
            const std::vector<double> got = tonemapped(both[k]->filtered, 1.0, cam);
            pixels = 0;
            for (size_t i = 0; i < plain.blob.size(); i++)
                if (plain.blob[i]) {
                    pixels++;
                    count[k] += both[k]->count[i];
                    for (int ch = 0; ch < 3; ch++)
                        e[k] += (got[i * 3 + ch] - want[i * 3 + ch]) * (got[i * 3 + ch] - want[i * 3 + ch]);
                }
            if (pixels == 0)
                throw std::runtime_error("no pixel sees the blob");
            count[k] /= (double)pixels, e[k] = std::sqrt(e[k] / (3.0 * (double)pixels));
        }
        std::printf("frames=%d size=%d blob_pixels=%zu followed=%u followed_without=%u count_with_motion=%.3f count_without=%.3f rmse_with_motion=%.4e rmse_without=%.4e ratio=%.3f\n",
            frames, size, pixels, motion.followed, plain.followed, count[1], count[0], e[1], e[0], e[1] / e[0]);
        return count[1] > count[0] && e[1] < e[0] ? 0 : 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
