"""The scene conversion (csrc/pt_convert.cpp) on the CPU.  pt_debug_convert runs what pt_upload_static (records made on the host) and pt_upload_dynamic
make of a scene's arrays, without a context or a device, and returns one line: a hash of every array the static part makes | a hash of every array of the
dynamic state and the figures of its instance route.  tests/golden/conversion_digests.json holds the lines of the library as it was before the conversion
left the device library's translation unit; a change to the conversion that is meant to keep its result keeps them."""
import functools
import json
import os
import re

import numpy as np
import pytest

from gpu_util import parse_digest
from ptamd import device as D, host as H, scenes

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "conversion_digests.json")
NO_BAKED, PARKED = D.FLAG_NO_BAKED_INSTANCES, D.FLAG_PARKED_INSTANCES
SKY = (8, 4)  # (the conversion never reads the sky)


def _grid(level):
    return scenes.instanced_grid(64, 64, level=level, sky_size=SKY).flat


def _crowd(transform="general"):
    return scenes.instanced_crowd(64, 64, nx=4, nz=3, level=3, transform=transform, sky_size=SKY).flat


def _few_general():
    """22 entered instances (20 blobs, the ground, the light), two of them not a translation + uniform scale: few enough (a quarter at most) that the others
    stay folded while the two are parked.  No generator makes such a crowd: two of the blobs' inverse transforms get a non-uniform scale."""
    f = scenes.instanced_crowd(64, 64, nx=5, nz=4, level=3, transform="uniform", sky_size=SKY).flat
    top = f.top_nodes.copy()
    scaled = [i for i in np.flatnonzero(top["isLeaf"] != 0) if top["invTransform"][i][0] != 1.0]
    for i in scaled[:2]:
        top["invTransform"][i][0] *= 1.25
    return H.FlatScene(f.vertices, f.triangles, f.materials, f.sub_nodes, f.lights, top, f.top_root, f.num_instances)


# name -> (arrays, pt_config flags, RNG mode).  The first eight: every builder, leaves of one to three triangles, an SBVH with duplicated references,
# parity mode.  The rest: one scene for each route an instance can take (copied to world space, folded, general, parked).
SCENES = {
    "cornell": (lambda: scenes.cornell_box(64, 64).flat, 0, D.RNG_COUNTER),
    "blob_room_4_binned": (lambda: scenes.blob_room(64, 64, level=4, builder=H.BVH_BINNED_SAH).flat, 0, D.RNG_COUNTER),
    "blob_room_4_fast": (lambda: scenes.blob_room(64, 64, level=4, builder=H.BVH_BINNED_FAST).flat, 0, D.RNG_COUNTER),
    "blob_room_4_spatial": (lambda: scenes.blob_room(64, 64, level=4, builder=H.BVH_SPATIAL_SPLIT).flat, 0, D.RNG_COUNTER),
    "grid_4x3_level5": (lambda: _grid(5), 0, D.RNG_COUNTER),
    "grid_parity": (lambda: _grid(3), 0, D.RNG_LFSR113_PARITY),
    "crowd": (_crowd, 0, D.RNG_COUNTER),
    "mixed": (lambda: scenes.mixed_material_room(64, 64, level=4).flat, 0, D.RNG_COUNTER),
    "grid_folded": (lambda: _grid(3), NO_BAKED, D.RNG_COUNTER),
    "crowd_general": (_crowd, NO_BAKED, D.RNG_COUNTER),
    "field_1000_general": (lambda: scenes.instance_field(64, 64, n=1000, sky_size=SKY).flat, NO_BAKED, D.RNG_COUNTER),
    "crowd_parked": (_crowd, PARKED | NO_BAKED, D.RNG_COUNTER),
    "crowd_few_general": (_few_general, NO_BAKED, D.RNG_COUNTER),
}


@functools.lru_cache(maxsize=None)
def flat(name):
    return SCENES[name][0]()


def convert(name):
    _, flags, rng = SCENES[name]
    return D.debug_convert(flat(name), flags=flags, rng_mode=rng)


parse = parse_digest  # (tests/gpu_util.py: tests/test_transforms_cpu.py reads the same lines)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("threads", ["pool", "1"])
@pytest.mark.parametrize("name", list(SCENES))
def test_conversion_matches_the_recorded_digests(name, threads, monkeypatch):
    """Byte for byte what the library made before (every packed node, box, triangle reference and record; the top level, the instance table, the copies'
    jobs), on the worker pool and on the calling thread alone (PTAMD_BUILD_THREADS=1)."""
    if threads == "1":
        monkeypatch.setenv("PTAMD_BUILD_THREADS", "1")
    else:
        monkeypatch.delenv("PTAMD_BUILD_THREADS", raising=False)
    got, want = parse(convert(name)), golden()[name]
    for half in ("static", "dynamic"):
        for key in want[half]:
            assert got[half].get(key) == want[half][key], f"{name}: {half} {key}"
    assert got == want


def test_each_instance_route_is_taken_where_it_belongs():
    """Which route the instances that are not copied to world space take: folded (translation + uniform scale, few enough for the fold table), general
    (a rotation or a non-uniform scale among more than a quarter of them, or more instances than the table holds), parked (asked for, parity mode, or the
    few general ones beside folded ones)."""
    d = {n: parse(convert(n))["dynamic"] for n in ("grid_4x3_level5", "grid_folded", "crowd_general", "field_1000_general", "crowd_parked", "grid_parity",
                                                   "crowd_few_general")}
    num = {n: {k: int(v, 10) for k, v in f.items() if k in ("hasInstances", "enteredInstances", "enteredGeneral", "foldedInstances", "generalRoute", "bakedNodes")}
           for n, f in d.items()}
    copied = num["grid_4x3_level5"]  # 12 blobs, the ground and the light: all copied
    assert copied["hasInstances"] == 0 and copied["enteredInstances"] == 0 and copied["bakedNodes"] > 0
    folded = num["grid_folded"]
    assert folded["enteredInstances"] == 14 and folded["foldedInstances"] == 14 and folded["generalRoute"] == 0
    for name, entered in (("crowd_general", 14), ("field_1000_general", 1002)):
        general = num[name]
        assert general["enteredInstances"] == entered and general["generalRoute"] == 1 and general["foldedInstances"] == 0, name
    for name, entered in (("crowd_parked", 14), ("grid_parity", 12)):  # (parity mode still copies the two single-leaf meshes)
        parked = num[name]
        assert parked["hasInstances"] == 1 and parked["enteredInstances"] == entered, name
        assert parked["generalRoute"] == 0 and parked["foldedInstances"] == 0 and parked["bakedNodes"] == 0, name
    few = num["crowd_few_general"]
    assert few["enteredInstances"] == 22 and few["enteredGeneral"] == 2
    assert few["generalRoute"] == 0 and few["foldedInstances"] == 20


def _with(f, **arrays):
    a = dict(vertices=f.vertices, triangles=f.triangles, materials=f.materials, sub_nodes=f.sub_nodes, lights=f.lights, top_nodes=f.top_nodes)
    a.update(arrays)
    return H.FlatScene(a["vertices"], a["triangles"], a["materials"], a["sub_nodes"], a["lights"], a["top_nodes"], f.top_root, f.num_instances)


def test_invalid_arrays_are_refused_with_the_upload_messages():
    """The upload's validation runs in the conversion: an out-of-range vertex index and a leaf whose triangles run past the array are refused with the
    messages pt_upload_static gives (tests/test_gpu_intersect.py checks that nothing is traversed after them)."""
    f = flat("cornell")
    bad = f.triangles.copy()
    bad["indices"][5, 1] = len(f.vertices)
    with pytest.raises(D.PtError, match=re.escape("failed (-1): triangle 5: vertex index out of range")):
        D.debug_convert(_with(f, triangles=bad))
    nodes = f.sub_nodes.copy()
    leaf = int(np.flatnonzero(nodes["count"] != 0)[0])
    nodes["left"][leaf] = len(f.triangles)
    with pytest.raises(D.PtError, match=re.escape(f"failed (-1): sub-BVH leaf {leaf}: triangle range out of bounds")):
        D.debug_convert(_with(f, sub_nodes=nodes))
