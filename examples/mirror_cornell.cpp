// What guide reflections buy a frame loop in front of a mirror: the Cornell room with a blue plate and a polished metal wall (the quad x in [-0.8, 0.8],
// y in [0.2, 1.8] at z = 0.99, PBR metal of reflectance 0.9 and smoothness 1) from a camera that orbits the room's centre, 2 degrees per frame.  Twelve
// frames of one sample per pixel, each blended into the temporal history and filtered (getTemporalOutput) -- once with first-hit guides, once with
// RayTracer::setGuideChain(K) and setGuideReflections(true).  Printed for both: the RMSE of the last frame's output against 256 samples per pixel from
// the same camera (both through pt_resolve's tone curve) over the pixels that show the mirror and over the rest, and the mean history count in both
// regions -- with first-hit guides the mirror keeps a history it should lose (it reprojects where the mirror was, not where the reflection was).  These
// are measurements, not a gate.
//     usage: mirror_cornell [frames] [chain K] [first_hit.ppm] [reflections.ppm]
#include "guide_chain_loop.h"

using namespace raytracer;
using namespace cornell;

int main(int argc, char** argv)
{
    GuideChainLoop mirror;
    mirror.extraQuad = [] { // the mirror, into the room
        return quadMesh({ -0.8f, 0.2f, 0.99f }, { -0.8f, 1.8f, 0.99f }, { 0.8f, 1.8f, 0.99f }, { 0.8f, 0.2f, 0.99f }, Material::PBRMetal(vec3(0.9f), 1.0f));
    };
    mirror.reflections = true;
    mirror.firstPath = "mirror_first_hit.ppm", mirror.chainPath = "mirror_reflections.ppm";
    mirror.inside = "in the mirror", mirror.outside = "outside the mirror", mirror.guides = "reflections"; // in the mirror: where the chain's distance lies behind the first hit's
    return guideChainLoop(argc, argv, mirror);
}
