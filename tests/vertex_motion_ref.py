"""numpy restatement of the vertex motion (include/ptamd.h, "vertex motion"): the host's rows L and the two guide deposits of a refitted mesh,
parameterised by dtype like motion_ref -- float64 is the reference the device is held against, float32 measures what single precision costs the
same arithmetic on the same input.  Also the deforming room the vertex-motion tests share."""
import numpy as np

import denoise_ref as R
import motion_ref as M
from ptamd import host as H, layout as L, scenes

W, Hh = 64, 36  # the deposit tests' image


# ---------------------------------------------------------------- the host's rows
def vertex_motion_rows(inv):
    """(n, 3, 4) float64 from (n, 16) float32 invTransforms: the linear part of inverse(inv), before the rounding; w = 0"""
    inv = np.ascontiguousarray(inv, np.float32).reshape(-1, 16)
    out = np.zeros((len(inv), 3, 4), np.float64)
    for i, m in enumerate(inv):
        out[i, :, :3] = np.linalg.inv(M._matrix(m))[:3, :3]
    return out


# ---------------------------------------------------------------- the two guide deposits
def _object_points(flat, prim, u, v, dt):
    """x = v0 + e1 u + e2 v of the hit triangles, the edges formed in float32 as the library's shading records hold them, then cast"""
    idx = flat.triangles[prim]["indices"]
    p = flat.vertices["vertex"][:, :3].astype(np.float32)
    v0, e1, e2 = p[idx[:, 0]], p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]]
    assert e1.dtype == np.float32
    return v0.astype(dt) + e1.astype(dt) * u + e2.astype(dt) * v


def deposits(flat_now, flat_then, prev_top_nodes, o, d, hits, dtype=np.float64, thin_lens=False):
    """What ONE guide sample deposits into the two motion sums with vertex motion set, for rays (o, d) with hit records `hits` on the state flat_now,
    whose static arrays were flat_then's before the refit and whose instances had prev_top_nodes' invTransform (None: no instance motion is set):
    (motion (n, 4), prev_normal (n, 4), extra) -- extra as motion_ref.motion_deposits returns it, then_unflipped from the geometry then."""
    dt = dtype
    then_top = flat_now.top_nodes if prev_top_nodes is None else prev_top_nodes
    motion, pn, extra = M.motion_deposits(flat_now, then_top, o, d, hits, dt, thin_lens)  # (A X + t, the flip of N; zeros without an instance motion)
    prim = np.asarray(hits["prim"])
    k = np.flatnonzero(prim >= 0)
    if k.size == 0:
        return motion, pn, extra
    inst = np.asarray(hits["inst"])[k]
    u, v = np.asarray(hits["u"], np.float32).astype(dt)[k, None], np.asarray(hits["v"], np.float32).astype(dt)[k, None]
    delta = _object_points(flat_then, prim[k], u, v, dt) - _object_points(flat_now, prim[k], u, v, dt)
    rows = vertex_motion_rows(then_top["invTransform"][inst]).astype(np.float32).astype(dt)  # rounded once, as the host rounds them
    motion[k, :3] = motion[k, :3] + np.einsum("kij,kj->ki", rows[:, :, :3], delta)
    idx = flat_then.triangles[prim[k]]["indices"]
    vn = flat_then.vertices["normal"][:, :3].astype(dt)
    n0, n1, n2 = vn[idx[:, 0]], vn[idx[:, 1]], vn[idx[:, 2]]
    sn = R._unit(n0 + (n1 - n0) * u + (n2 - n0) * v)  # object space, then
    m = then_top["invTransform"][inst].astype(dt).reshape(-1, 4, 4)
    n_then = R._unit(np.einsum("kji,ki->kj", m[:, :3, :3], sn))  # normalTransform, as motion_ref spells it
    pn[k, :3] = np.where(extra["n_dot_d"][k, None] > 0, -n_then, n_then)  # flipped if and only if N is
    extra["then_unflipped"][k] = n_then
    assert motion.dtype == dt and pn.dtype == dt
    return motion, pn, extra


# ---------------------------------------------------------------- the deforming room
BLOB_LEAF = 1  # (leaves of the host library's top level are the scene nodes, in order)
BLOB_SCALE = (1.2, 0.9, 1.5)  # non-uniform


def twist_and_squash(p0, frame):
    """the deformation of tests/test_gpu_dynamic.py::test_deforming_mesh_through_refit"""
    if frame == 0:
        return p0.copy()
    ang = 0.9 * frame * p0[:, 1]
    return np.stack([np.cos(ang) * p0[:, 0] - np.sin(ang) * p0[:, 2], (1 - 0.2 * frame) * p0[:, 1] + 0.05 * frame * np.sin(5 * p0[:, 0]),
                     np.sin(ang) * p0[:, 0] + np.cos(ang) * p0[:, 2]], 1).astype(np.float32)


class DeformingRoom:
    """The room of test_deforming_mesh_through_refit -- five walls, a light, an icosphere of level 3 (1280 triangles) of radius 0.5 -- with the sphere
    under a non-uniform scale.  shape(p) refits the sphere and returns the flattened scene (a copy: earlier ones stay what they were)."""

    def __init__(self, builder=H.BVH_BINNED_SAH, width=W, height=Hh, thin_lens=False, eye=(0.0, 1.0, -3.9), fov=None, location=(0.0, 0.8, 0.1),
                 scale=BLOB_SCALE):
        v, f = scenes.icosphere(3)
        self.p0 = (v * 0.5).astype(np.float32)
        mat = L.material_pbr_dielectric((0.75, 0.2, 0.15), 0.7)
        self.blob = H.Mesh(self.p0, f.astype(np.uint32), [mat], builder=builder)
        self.scene = H.Scene()
        mb, mats = scenes._MeshBuilder(), scenes._room_materials()
        scenes._room(mb, mats)
        self.scene.add_node(mb.build(mats, H.BVH_BINNED_SAH))
        self.node = self.scene.add_node(self.blob, location=location, scale=scale)
        self.width, self.height = width, height
        fov = min(40.0 * (width / height) ** 0.5, 75.0) if fov is None else fov  # scenes.blob_room's
        kw = dict(thin_lens=True, focal_length_mm=50.0, aperture_fstops=2.0) if thin_lens else {}  # (scenes.instanced_grid's lens)
        self.camera = scenes._camera(width, height, eye, (0.0, 1.0, 0.0), fov, **kw)
        self.flat0 = self.scene.flatten()

    def shape(self, p):
        self.blob.refit(np.ascontiguousarray(p, np.float32))
        return self.scene.flatten()

    def frame(self, frame):
        return self.shape(twist_and_squash(self.p0, frame))

    def refit_on(self, ctx, route, flat):
        """hand the sphere's current shape (flat: its flattened scene) to a context and make it the active state"""
        self.hand_over(ctx, route, flat)
        ctx.frame_tick()

    def hand_over(self, ctx, route, flat):
        """... without the tick"""
        if route == "device":
            first_vertex, _ = self.scene.mesh_offsets(self.blob)
            ctx.refit_vertices(first_vertex, self.blob.vertices_view())
            ctx.upload_dynamic_async(self.scene.flatten_dynamic_only()[0])
        else:
            ctx.update_geometry(flat)
            ctx.upload_dynamic_async(flat)

    def blob_triangles(self, flat):
        """mask over flat.triangles: the sphere's (the room's come first)"""
        first_vertex, _ = self.scene.mesh_offsets(self.blob)
        return flat.triangles["indices"].min(1) >= first_vertex


def pixel_centre_rays(camera, width, height):
    """(o, d) float32: the pinhole rays through the pixel centres, row-major -- the guide rays up to their sub-pixel jitter"""
    import temporal_ref as T
    E, S, u, v = T.camera_vectors(camera, np.float64)
    yy, xx = np.mgrid[0:height, 0:width]
    dirv = S + u * ((xx + 0.5) / width)[..., None] + v * ((yy + 0.5) / height)[..., None] - E
    d = (dirv / np.linalg.norm(dirv, axis=-1, keepdims=True)).reshape(-1, 3)
    return np.broadcast_to(E, d.shape).astype(np.float32).copy(), d.astype(np.float32)


def scene_extent(flat):
    root = flat.top_nodes[flat.top_root]
    return float(max(np.abs(root["min"][:3]).max(), np.abs(root["max"][:3]).max()))
