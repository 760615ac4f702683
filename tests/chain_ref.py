"""numpy restatement of the guide chain (include/ptamd.h, "guide chain"): a guide ray follows refraction through REFRACTIVE / BASIC_REFRACTIVE
surfaces to the first surface that is not glass, and that surface makes the deposits.  Parameterised by dtype like tests/denoise_ref.py: float64 is
the reference the device is held against, float32 measures what single precision costs the same arithmetic.  The intersections are the oracle's
(O.intersect_batch, float32 rays: each segment's origin and direction are rounded to float32 once, as a queue entry is), the deposits of the
terminal surface are denoise_ref.guide_deposits' own."""
import numpy as np

import denoise_ref as R
import orclib as O
from ptamd import layout as L

CHAIN_MAX = 4  # PT_GUIDE_CHAIN_MAX
EPS = 1e-4     # kEPS, the shading's constant (shading_helper.cl:15)


def _unit(v):
    return v / np.sqrt((v * v).sum(1, keepdims=True))


def _real_normal(flat, prim, inst, dt):
    """shadeHit's real normal up to its (positive) length: normalTransform(instance, cross(edge1, edge2))"""
    idx = flat.triangles["indices"][prim]
    p = flat.vertices["vertex"][:, :3].astype(dt)
    g = np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]])
    m = flat.top_nodes["invTransform"][inst].astype(dt).reshape(-1, 4, 4)
    return _unit(np.einsum("kji,ki->kj", m[:, :3, :3], g))


def chain(flat, scene, o, d, K, material_textures=None, dtype=np.float64, thin_lens=False, threads=8):
    """One guide sample of the rays (o, d) ((n, 3) each, as the camera made them: a thin lens hands in un-normalised directions) with
    max_transmissions = K.  Returns (albedo_hits (n, 4), normal_depth (n, 4), info): the deposits of each ray's terminal surface, and
    info = dict(prim, inst: the terminal primitive and top-level leaf (-1: a miss), depth: the stage the ray ended at, tir: it ended in total
    internal reflection, first_glass: its stage-0 hit was glass, segments: depth + 1, dir: the unit direction of the last segment, point: the
    terminal hit point (nan: a miss))."""
    dt = dtype
    n = len(d)
    ah, nd = np.zeros((n, 4), dt), np.zeros((n, 4), dt)
    info = dict(prim=np.full(n, -1, np.int64), inst=np.full(n, -1, np.int64), depth=np.zeros(n, np.int64), tir=np.zeros(n, bool),
                first_glass=np.zeros(n, bool), dir=np.zeros((n, 3), dt), point=np.full((n, 3), np.nan, dt))
    live = np.arange(n)
    co, cd = np.asarray(o, np.float32), np.asarray(d, np.float32)
    dist = np.zeros(n, dt)
    for j in range(K + 1):
        if live.size == 0:
            break
        hits = O.intersect_batch(scene, co, cd, threads=threads)
        lens = thin_lens and j == 0
        a, g = R.guide_deposits(flat, cd, hits, material_textures, dtype=dt, thin_lens=lens)
        Do = cd.astype(dt)
        scale = np.sqrt((Do * Do).sum(1)) if lens else np.ones(len(cd), dt)
        D = Do / scale[:, None] if lens else Do
        prim, inst = np.asarray(hits["prim"], np.int64), np.asarray(hits["inst"], np.int64)
        hit = prim >= 0
        t = np.asarray(hits["t"], dt)
        cont = np.zeros(len(cd), bool)
        tir = np.zeros(len(cd), bool)
        T = np.zeros((len(cd), 3), dt)
        k = np.flatnonzero(hit)
        if k.size:
            mat = flat.materials[flat.triangles["materialIndex"][prim[k]]]
            basic, rough = mat["type"] == L.MAT_BASIC_REFRACTIVE, mat["type"] == L.MAT_REFRACTIVE
            glass = basic | rough
            if j == 0:
                info["first_glass"][live[k]] = glass
            ior = np.where(basic, mat["refractiveIndexBasic"], mat["refractiveIndexRough"]).astype(dt)
            ior = np.where(glass, ior, dt(1))
            N = g[k, :3]
            facing = -(_real_normal(flat, prim[k], inst[k], dt) * D[k]).sum(1)
            outside = np.where(basic, facing > dt(EPS), facing > 0)  # each material's own compare in shadeHit
            n1n2 = np.where(outside, dt(1) / ior, ior)
            cos1 = -(N * D[k]).sum(1)
            Kt = dt(1) - n1n2 * n1n2 * (dt(1) - cos1 * cos1)
            go = glass & (Kt > dt(EPS)) & (j < K)
            tir[k] = glass & ~(Kt > dt(EPS)) & (j < K)  # (at stage K glass is terminal: the interface is not looked at)
            cont[k] = go
            with np.errstate(invalid="ignore"):
                Tk = n1n2[:, None] * D[k] + N * (n1n2 * cos1 - np.sqrt(np.maximum(Kt, 0)))[:, None]
            T[k] = _unit(np.where(go[:, None], Tk, 1.0))
        end = ~cont
        e = live[end]
        ah[e] = a[end]
        nd[e, :3] = g[end, :3]
        nd[e, 3] = np.where(hit[end], dist[end] + g[end, 3], dt(R.SKY_DEPTH))
        info["prim"][e], info["inst"][e] = np.where(hit[end], prim[end], -1), np.where(hit[end], inst[end], -1)
        info["depth"][e] = j
        info["tir"][e] = tir[end]
        info["dir"][e] = D[end]
        with np.errstate(invalid="ignore"):
            info["point"][e] = np.where(hit[end, None], co[end].astype(dt) + Do[end] * t[end, None], np.nan)
        # the next segment: X with the segment's own origin and un-normalised direction (k_shade's X = o + t d), offset along T
        X = co[cont].astype(dt) + Do[cont] * t[cont, None]
        dist = dist[cont] + t[cont] * scale[cont]
        co = (X + T[cont] * dt(EPS)).astype(np.float32)
        cd = T[cont].astype(np.float32)
        live = live[cont]
    info["segments"] = info["depth"] + 1
    return ah, nd, info
