"""A float64 brute-force ray / triangle intersector over a flattened scene: every instance's triangles taken to world space, every ray against
every triangle (Moeller-Trumbore, two-sided, t > 0).  No tree, no fp32, no tricks: what the oracle and the kernels are held against where the
scene leaves the region the reference was written for (tests/test_transforms_cpu.py)."""
import numpy as np


def _triangles_under(flat, root):
    out, stack = [], [int(root)]
    while stack:
        nd = flat.sub_nodes[stack.pop()]
        if nd["count"]:
            out.extend(range(int(nd["left"]), int(nd["left"]) + int(nd["count"])))
        else:
            stack += [int(nd["left"]), int(nd["left"]) + 1]
    return np.asarray(out, np.int64)


def world_triangles(flat):
    """(corners [n, 3, 3] float64 in world space, triangle index, top-level leaf) of every triangle reference reachable through every instance."""
    pos = flat.vertices["vertex"][:, :3].astype(np.float64)
    corners, prim, inst = [], [], []
    for leaf in np.flatnonzero(flat.top_nodes["isLeaf"] != 0):
        inv = flat.top_nodes["invTransform"][leaf].astype(np.float64).reshape(4, 4).T  # column-major
        world = np.linalg.inv(inv)
        tris = _triangles_under(flat, flat.top_nodes["a"][leaf])
        p = pos[flat.triangles["indices"][tris].astype(np.int64)]  # [n, 3, 3]
        corners.append(p @ world[:3, :3].T + world[:3, 3])
        prim.append(tris)
        inst.append(np.full(len(tris), leaf, np.int64))
    return np.concatenate(corners), np.concatenate(prim), np.concatenate(inst)


def intersect(flat, o, d, chunk=128):
    """Closest hit per ray: dict(t, u, v, prim, inst) like orclib.intersect_batch (t = inf, prim = inst = -1 for a miss), all float64 / int64."""
    corners, prim, inst = world_triangles(flat)
    v0, e1, e2 = corners[:, 0], corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = len(o)
    out = dict(t=np.full(n, np.inf), u=np.zeros(n), v=np.zeros(n), prim=np.full(n, -1, np.int64), inst=np.full(n, -1, np.int64))
    for s in range(0, n, chunk):
        oo, dd = o[s:s + chunk, None, :], d[s:s + chunk, None, :]
        P = np.cross(dd, e2[None])
        det = (e1[None] * P).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            T = oo - v0[None]
            u = (T * P).sum(-1) * inv
            Q = np.cross(T, e1[None])
            v = (dd * Q).sum(-1) * inv
            t = (e2[None] * Q).sum(-1) * inv
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)  # (a zero-area triangle: det = 0, NaN or inf everywhere, never ok)
        t = np.where(ok, t, np.inf)
        best = t.argmin(1)
        rows = np.arange(len(best))
        hit = np.isfinite(t[rows, best])
        sl = slice(s, s + len(best))
        out["t"][sl] = t[rows, best]
        out["u"][sl], out["v"][sl] = np.where(hit, u[rows, best], 0.0), np.where(hit, v[rows, best], 0.0)
        out["prim"][sl], out["inst"][sl] = np.where(hit, prim[best], -1), np.where(hit, inst[best], -1)
    return out


def barycentrics(flat, o, d, prim, inst):
    """float64 (u, v) of rays against the triangle (prim, inst) each names: how close to that triangle's boundary a disputed hit lies."""
    pos = flat.vertices["vertex"][:, :3].astype(np.float64)
    u, v = np.zeros(len(prim)), np.zeros(len(prim))
    for k in range(len(prim)):
        inv = flat.top_nodes["invTransform"][inst[k]].astype(np.float64).reshape(4, 4).T
        world = np.linalg.inv(inv)
        p = pos[flat.triangles["indices"][prim[k]].astype(np.int64)] @ world[:3, :3].T + world[:3, 3]
        e1, e2, T = p[1] - p[0], p[2] - p[0], np.asarray(o[k], np.float64) - p[0]
        P = np.cross(np.asarray(d[k], np.float64), e2)
        det = e1 @ P
        u[k], v[k] = (T @ P) / det, (np.asarray(d[k], np.float64) @ np.cross(T, e1)) / det
    return u, v
