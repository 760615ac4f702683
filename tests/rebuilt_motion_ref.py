"""numpy restatement of the rebuilt motion (include/ptamd.h, "rebuilt motion"): the triangle map of two rebuilt trees, the snapshot the gather makes of
it, and the two guide deposits -- vertex_motion_ref.deposits with the "then" geometry read through the map.  Also the room the rebuilt-motion tests
share: vertex_motion_ref.DeformingRoom's, its sphere a NEW mesh (a new tree) every frame."""
import numpy as np

import vertex_motion_ref as V
from ptamd import host as H, layout as L, scenes

NONE = 0xFFFFFFFF  # PT_NO_PREVIOUS_TRIANGLE


# ---------------------------------------------------------------- the map
def triangle_history(now, then):
    """An independent statement of H.triangle_history: per triangle of `now` the lowest index in `then` of the same (mesh, original), NONE where there
    is none or the original is unknown.  now, then: (mesh, original) uint32 arrays."""
    first = {}
    for j, key in enumerate(zip(then[0].tolist(), then[1].tolist())):
        if key[1] != NONE:
            first.setdefault(key, j)
    return np.array([NONE if o == NONE else first.get((m, o), NONE) for m, o in zip(now[0].tolist(), now[1].tolist())], np.uint32).reshape(-1)


def gather(then, now, prev_triangle):
    """what k_gather_then leaves: then[map[i]] where the entry is below len(then), else now[i] -- numpy fancy indexing"""
    prev_triangle = np.asarray(prev_triangle, np.uint32)
    follow = prev_triangle < len(then)
    out = now.copy()
    out[follow] = then[prev_triangle[follow]]
    return out


# ---------------------------------------------------------------- the two guide deposits
class _Then:
    """the geometry `then` seen through the map, in the numbering of `now`: what vertex_motion_ref.deposits reads of a flattened scene"""

    def __init__(self, flat_now, flat_then, prev_triangle):
        prev_triangle = np.asarray(prev_triangle, np.uint32)
        assert prev_triangle.shape == (len(flat_now.triangles),)
        follow = prev_triangle != NONE
        assert np.all(prev_triangle[follow] < len(flat_then.triangles))
        nv = len(flat_then.vertices)
        self.vertices = np.concatenate([flat_then.vertices, flat_now.vertices])  # a new triangle reads the current geometry
        self.triangles = flat_now.triangles.copy()
        self.triangles["indices"] = self.triangles["indices"] + nv
        self.triangles["indices"][follow] = flat_then.triangles["indices"][prev_triangle[follow]]


def deposits_rebuilt(flat_now, flat_then, prev_triangle, prev_top, o, d, hits, dtype=np.float64, thin_lens=False):
    """vertex_motion_ref.deposits for a state whose tree was rebuilt: the "then" geometry of hit triangle prim is triangle prev_triangle[prim] of
    flat_then; where the map says none it is the current geometry (delta == 0, the current normal)."""
    return V.deposits(flat_now, _Then(flat_now, flat_then, prev_triangle), prev_top, o, d, hits, dtype, thin_lens)


# ---------------------------------------------------------------- the room whose sphere is rebuilt
class RebuiltRoom:
    """DeformingRoom's room and camera; frame(p) makes a NEW H.Mesh of the sphere (the same index buffer, or its first `triangles`) with `builder`,
    in a new scene, and returns (flat, origins) -- origins as Scene.triangle_origins gives them.  The spatial-split builder never splits the sphere's
    small triangles on their own, so under it the index buffer BEGINS with `chords` triangles between far-apart vertices (seeded; inside the sphere
    while it is round): with those it splits, differently in every frame, and the trees hold duplicates."""

    def __init__(self, builder=H.BVH_BINNED_FAST, width=V.W, height=V.Hh, fov=None, chords=None):
        v, f = scenes.icosphere(3)
        self.p0 = (v * 0.5).astype(np.float32)
        self.chords = (16 if builder == H.BVH_SPATIAL_SPLIT else 0) if chords is None else chords
        rng = np.random.default_rng(5)
        far = [rng.choice(len(v), 3, replace=False) for _ in range(self.chords)]
        self.faces = np.concatenate([np.array(far, np.uint32).reshape(-1, 3), f.astype(np.uint32)])
        self.builder = builder
        self.mat = L.material_pbr_dielectric((0.75, 0.2, 0.15), 0.7)
        mb, mats = scenes._MeshBuilder(), scenes._room_materials()
        scenes._room(mb, mats)
        self.walls = mb.build(mats, H.BVH_BINNED_SAH)
        self.width, self.height = width, height
        fov = min(40.0 * (width / height) ** 0.5, 75.0) if fov is None else fov
        self.camera = scenes._camera(width, height, (0.0, 1.0, -3.9), (0.0, 1.0, 0.0), fov)
        self.blob = None  # the newest sphere

    def frame(self, p, triangles=None, builder=None, location=(0.0, 0.8, 0.1), orientation_wxyz=(1, 0, 0, 0), walls_at=(0, 0, 0)):
        f = self.faces if triangles is None else self.faces[:triangles]
        self.blob = H.Mesh(np.ascontiguousarray(p, np.float32), f, [self.mat], builder=self.builder if builder is None else builder)
        scene = H.Scene()
        scene.add_node(self.walls, location=walls_at)
        scene.add_node(self.blob, location=location, orientation_wxyz=orientation_wxyz, scale=V.BLOB_SCALE)
        flat = scene.flatten()
        return flat, scene.triangle_origins()

    def twisted(self, frame, **kw):
        return self.frame(V.twist_and_squash(self.p0, frame), **kw)
