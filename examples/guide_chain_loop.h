// The program glass_cornell.cpp and mirror_cornell.cpp share: the Cornell room with the blue plate and one more quad of theirs, seen from a camera that
// orbits the room's centre by 2 degrees per frame.  `frames` frames of one sample per pixel, each blended into the temporal history and filtered
// (getTemporalOutput) -- once with first-hit guides, once with RayTracer::setGuideChain(K), with or without setGuideReflections.  Printed for both: the
// RMSE of the last frame's output against 256 samples per pixel from the same camera (both through pt_resolve's tone curve) over the pixels where the
// chain looks further than the first hit and over the rest, and the mean history count in both regions.
//     usage: <example> [frames] [chain K] [first_hit.ppm] [chain.ppm]
#pragma once
#include "cornell.h"
#include <cstdlib>

namespace cornell {

struct GuideChainLoop {
    std::shared_ptr<Mesh> (*extraQuad)(); // added after the plate
    bool reflections; // setGuideReflections goes with the chain
    const char *firstPath, *chainPath; // the default file names
    const char *inside, *outside, *guides; // the report's words: the two regions, and what the second run's guides follow
};

struct Run {
    std::vector<float> image, depth, count; // the last frame's output; its guides' distance; the history count N
};

// `frames` 1-spp frames along the orbit (the last one at angle 0), history + filter
inline Run frameLoop(RayTracer& rt, unsigned chain, bool reflections, int frames, int W, int H)
{
    const float step = 2.0f * 3.14159265f / 180.0f;
    rt.setGuideChain(chain);
    if (reflections)
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

inline int guideChainLoop(int argc, char** argv, const GuideChainLoop& ex)
{
    const int frames = argc > 1 ? std::atoi(argv[1]) : 12;
    const int chain = argc > 2 ? std::atoi(argv[2]) : 2;
    const char* firstPath = argc > 3 ? argv[3] : ex.firstPath;
    const char* chainPath = argc > 4 ? argv[4] : ex.chainPath;
    const int W = 256, H = 256;
    if (frames < 1 || chain < 1 || chain > (int)PT_GUIDE_CHAIN_MAX) {
        std::fprintf(stderr, "error: frames must be at least 1, the chain 1..%u\n", PT_GUIDE_CHAIN_MAX);
        return 1;
    }
    try {
        auto scene = std::make_shared<Scene>();
        addWalls(*scene); // floor, ceiling, back, left, right
        scene->addNode(ceilingLight());
        scene->addNode(bluePlate(), Transform(vec3(0.2f, 0.0f, 0.1f)));
        scene->addNode(ex.extraQuad());

        const TextureArray noTextures, sky = greySky();
        RayTracer rt(W, H, scene, noTextures, sky);

        const Run first = frameLoop(rt, 0u, ex.reflections, frames, W, H), through = frameLoop(rt, (unsigned)chain, ex.reflections, frames, W, H);
        // the reference: 256 samples per pixel from the last frame's camera
        rt.setGuideChain(0u);
        if (ex.reflections)
            rt.setGuideReflections(false);
        rt.setSampleBase(1000u);
        const Camera last = orbitCamera(0.0f, W, H);
        for (int s = 0; s < 256; s++)
            rt.rayTrace(last);
        const std::vector<float> ref = rt.getOutput();

        // region 0: where the chain's distance lies behind the first hit's
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
        for (int region = 0; region < 2; region++) {
            const double n = (double)(pixels[region] ? pixels[region] : 1);
            std::printf("%s (%zu pixels): RMSE against 256 spp  first-hit guides %.5f  %s K=%d %.5f  ratio %.3f;  mean history count  %.2f  %.2f\n", region == 0 ? ex.inside : ex.outside,
                pixels[region], std::sqrt(err[0][region] / (3.0 * n)), ex.guides, chain, std::sqrt(err[1][region] / (3.0 * n)),
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

} // namespace cornell
