// What the guide chain buys a frame loop behind glass: the Cornell room with a blue plate seen through a pane of glass (the quad x in [-0.6, 0.6],
// y in [0.2, 1.8] at z = -0.6, BASIC_REFRACTIVE of index 1.5) from a camera that orbits the room's centre, 2 degrees per frame.  Twelve frames of one
// sample per pixel, each blended into the temporal history and filtered (getTemporalOutput) -- once with first-hit guides, once with
// RayTracer::setGuideChain(K).  Printed for both: the RMSE of the last frame's output against 256 samples per pixel from the same camera (both through
// pt_resolve's tone curve) over the pixels seen through the glass and over the rest, and the mean history count in both regions.  These are measurements,
// not a gate.
//     usage: glass_cornell [frames] [chain K] [first_hit.ppm] [chain.ppm]
#include "guide_chain_loop.h"

using namespace raytracer;
using namespace cornell;

int main(int argc, char** argv)
{
    GuideChainLoop glass;
    glass.extraQuad = [] { // the pane, towards the camera
        return quadMesh({ -0.6f, 0.2f, -0.6f }, { -0.6f, 1.8f, -0.6f }, { 0.6f, 1.8f, -0.6f }, { 0.6f, 0.2f, -0.6f }, Material::BasicRefractive(1.5f));
    };
    glass.reflections = false;
    glass.firstPath = "glass_first_hit.ppm", glass.chainPath = "glass_chain.ppm";
    glass.inside = "through the glass", glass.outside = "outside the glass", glass.guides = "chain"; // seen through the glass: where the chain's distance lies behind the first hit's
    return guideChainLoop(argc, argv, glass);
}
