"""Rebuilt motion without a device (include/ptamd.h "rebuilt motion"; host/scene.h triangleHistory): where the triangles of a flattened scene come from,
and the map between two rebuilt trees of one mesh against an independent statement of it and against the meshes' own topology."""
import numpy as np
import pytest

import rebuilt_motion_ref as RB
import vertex_motion_ref as V
from ptamd import device as D, host as H

NONE = RB.NONE
BUILDERS = ["BVH_BINNED_FAST", "BVH_SPATIAL_SPLIT"]


def test_the_marker_is_one_value_everywhere():
    assert D.NO_PREVIOUS_TRIANGLE == H.NO_PREVIOUS_TRIANGLE == NONE == 0xFFFFFFFF
    for name in ("pt_set_rebuilt_motion", "pt_rebuilt_motion", "pt_debug_gather_records"):
        assert name in D.EXPORTS and hasattr(D.lib(), name)


@pytest.fixture(scope="module", params=BUILDERS)
def two_frames(request):
    room = RB.RebuiltRoom(getattr(H, request.param))
    a = room.twisted(0)
    blob_a = room.blob
    b = room.twisted(1)
    return request.param, room, a, b, blob_a, room.blob


def test_origins_are_the_meshes_own(two_frames):
    """flatten() reports, per triangle, its mesh's place in the scene and the builder's originalTriangle"""
    _, room, (flat_a, org_a), (flat_b, org_b), blob_a, blob_b = two_frames
    for flat, (mesh, original), blob in ((flat_a, org_a, blob_a), (flat_b, org_b, blob_b)):
        assert mesh.shape == original.shape == (len(flat.triangles),) and mesh.dtype == original.dtype == np.uint32
        walls = room.walls.bvh()[2]
        assert np.array_equal(mesh, np.r_[np.zeros(len(walls), np.uint32), np.ones(len(mesh) - len(walls), np.uint32)])
        assert np.array_equal(original, np.r_[walls, blob.bvh()[2]])
        assert sorted(set(original[mesh == 1].tolist())) == list(range(len(room.faces)))  # every input triangle is somewhere


def test_history_of_two_rebuilt_trees(two_frames):
    builder, room, (flat_a, org_a), (flat_b, org_b), _, _ = two_frames
    if builder == "BVH_SPATIAL_SPLIT":  # the splits of the two frames differ: the map is no permutation, the test means something
        assert room.chords and len(flat_a.triangles) != len(flat_b.triangles) and len(flat_a.triangles) > len(room.faces) + 12 + 50
    else:
        assert len(flat_a.triangles) == len(flat_b.triangles)
        assert not np.array_equal(org_a[1], org_b[1])  # another leaf order
    for now, then in ((org_b, org_a), (org_a, org_b)):
        got = H.triangle_history(now, then)
        assert got.dtype == np.uint32 and np.array_equal(got, RB.triangle_history(now, then))
        assert not (got == NONE).any()  # both frames hold every input triangle
        assert np.array_equal(then[0][got], now[0]) and np.array_equal(then[1][got], now[1])
    assert np.array_equal(H.triangle_history(org_a, org_a)[org_a[0] == 0], np.flatnonzero(org_a[0] == 0))  # the walls: where they were


def test_the_map_leads_to_the_same_vertices(two_frames):
    """the topology check that makes the map right whatever a kernel does with it: frame 0's triangle map[i] has the vertex indices of frame 1's
    triangle i (the two scenes share the vertex numbering: the same meshes in the same order)"""
    _, _, (flat_a, org_a), (flat_b, org_b), _, _ = two_frames
    m = H.triangle_history(org_b, org_a)
    assert np.array_equal(flat_a.triangles["indices"][m], flat_b.triangles["indices"])
    assert np.array_equal(flat_a.triangles["materialIndex"][m], flat_b.triangles["materialIndex"])


@pytest.mark.parametrize("builder", BUILDERS)
def test_history_when_triangles_come_and_go(builder):
    """a frame without the last 200 input triangles, in both directions: none-entries exactly for the triangles that are missing"""
    room = RB.RebuiltRoom(getattr(H, builder))
    full, org_full = room.twisted(0)
    n_in = len(room.faces)
    less, org_less = room.twisted(1, triangles=n_in - 200)
    assert len(less.triangles) < len(full.triangles)
    fewer = H.triangle_history(org_less, org_full)  # now: the smaller frame -- everything has a predecessor
    assert np.array_equal(fewer, RB.triangle_history(org_less, org_full)) and not (fewer == NONE).any()
    assert np.array_equal(org_full[1][fewer], org_less[1]) and np.array_equal(org_full[0][fewer], org_less[0])
    assert np.array_equal(full.triangles["indices"][fewer], less.triangles["indices"])
    more = H.triangle_history(org_full, org_less)  # now: the full frame -- its last 200 input triangles are new
    assert np.array_equal(more, RB.triangle_history(org_full, org_less))
    new = (org_full[0] == 1) & (org_full[1] >= n_in - 200)
    assert len(set(org_full[1][new].tolist())) == 200 and np.array_equal(more == NONE, new)  # (200 input triangles, and every reference to one of them)
    assert np.array_equal(org_less[1][more[~new]], org_full[1][~new]) and np.array_equal(org_less[0][more[~new]], org_full[0][~new])
    assert np.array_equal(less.triangles["indices"][more[~new]], full.triangles["indices"][~new])


def test_a_mesh_without_origins_has_no_history():
    """what flattenStatic reports of a mesh whose IMesh::getOriginalTriangles is the default (unknown): every entry the marker, on either side"""
    room = RB.RebuiltRoom()
    (_, org_a), (_, org_b) = room.twisted(0), room.twisted(1)
    blob = org_b[0] == 1
    unknown_b = (org_b[0], np.where(blob, NONE, org_b[1]).astype(np.uint32))
    got = H.triangle_history(unknown_b, org_a)
    assert np.array_equal(got, RB.triangle_history(unknown_b, org_a)) and np.all(got[blob] == NONE) and not (got[~blob] == NONE).any()
    unknown_a = (org_a[0], np.where(org_a[0] == 1, NONE, org_a[1]).astype(np.uint32))
    got = H.triangle_history(org_b, unknown_a)
    assert np.all(got[blob] == NONE) and not (got[~blob] == NONE).any()
    everything = (org_a[0], np.full_like(org_a[1], NONE))
    assert np.all(H.triangle_history(everything, everything) == NONE)
    assert len(H.triangle_history((np.zeros(0, np.uint32),) * 2, org_a)) == 0
    assert np.all(H.triangle_history(org_b, (np.zeros(0, np.uint32),) * 2) == NONE)


def test_history_is_the_lowest_duplicate_and_refuses_what_are_no_origins():
    then = (np.array([0, 0, 0, 1, 1], np.uint32), np.array([2, 0, 2, 0, 0], np.uint32))
    now = (np.array([1, 0, 0, 0, 2], np.uint32), np.array([0, 2, 1, 0, 0], np.uint32))
    assert H.triangle_history(now, then).tolist() == [3, 0, NONE, 1, NONE]
    with pytest.raises(RuntimeError):
        H.triangle_history(now, (then[0], np.array([2, 0, 0xFFFFFFF0, 0, 0], np.uint32)))
    with pytest.raises(ValueError):
        H.triangle_history((now[0], now[1][:3]), then)
