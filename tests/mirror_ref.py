"""numpy restatement of the guide chain with reflections (include/ptamd.h, "guide reflections"): next to refraction (tests/chain_ref.py) a guide ray
follows MIRRORS -- PBR, metallic, smoothness > 0.94 -- and total internal reflection within the same budget of K interfaces, carries a tint that the
mirrors multiply their base colour onto, and the terminal surface deposits tint (.) its albedo.  Parameterised by dtype like chain_ref.chain, built from
its helpers and denoise_ref's; with reflections=False it IS chain_ref.chain."""
import numpy as np

import chain_ref as CH
import denoise_ref as R
import orclib as O
from ptamd import layout as L

EPS = CH.EPS
MAX_SMOOTHNESS = np.float32(0.94)  # kMaxSmoothness: shading's compare, on the material's own float32


def is_mirror(materials):
    """which records of a material array the chain follows as a MIRROR"""
    return (materials["type"] == L.MAT_PBR) & (materials["metallic"] != 0) & (materials["smoothness"] > MAX_SMOOTHNESS)


def chain(flat, scene, o, d, K, material_textures=None, dtype=np.float64, thin_lens=False, threads=8, reflections=True):
    """One guide sample of the rays (o, d) with max_transmissions = K and guide reflections on.  Returns (albedo_hits (n, 4), normal_depth (n, 4),
    info) as chain_ref.chain does; info = dict(prim, inst, depth, dir, point, segments, first_glass as there; tir: the chain ENDED on glass whose
    interface neither transmits nor lets the reflection through; reflections: the number of reflections followed, mirror or total internal; mirrors:
    those of them off a MIRROR (the multiplies in the tint); met: the chain hit a MIRROR or met a total internal reflection at any stage, followed or
    not; first_mirror: its stage-0 hit is a MIRROR; tint (n, 3))."""
    if not reflections:
        return CH.chain(flat, scene, o, d, K, material_textures, dtype=dtype, thin_lens=thin_lens, threads=threads)
    dt = dtype
    n = len(d)
    ah, nd = np.zeros((n, 4), dt), np.zeros((n, 4), dt)
    info = dict(prim=np.full(n, -1, np.int64), inst=np.full(n, -1, np.int64), depth=np.zeros(n, np.int64), tir=np.zeros(n, bool),
                first_glass=np.zeros(n, bool), first_mirror=np.zeros(n, bool), met=np.zeros(n, bool), reflections=np.zeros(n, np.int64),
                mirrors=np.zeros(n, np.int64),
                dir=np.zeros((n, 3), dt), point=np.full((n, 3), np.nan, dt), tint=np.ones((n, 3), dt))
    live = np.arange(n)
    co, cd = np.asarray(o, np.float32), np.asarray(d, np.float32)
    dist = np.zeros(n, dt)
    tint = np.ones((n, 3), dt)
    count, mirrors = np.zeros(n, np.int64), np.zeros(n, np.int64)
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
        followed, off_mirror = np.zeros(len(cd), bool), np.zeros(len(cd), bool)
        nxt = np.zeros((len(cd), 3), dt)
        k = np.flatnonzero(hit)
        if k.size:
            mat = flat.materials[flat.triangles["materialIndex"][prim[k]]]
            basic, rough = mat["type"] == L.MAT_BASIC_REFRACTIVE, mat["type"] == L.MAT_REFRACTIVE
            glass, mirror = basic | rough, is_mirror(mat)
            if j == 0:
                info["first_glass"][live[k]] = glass
                info["first_mirror"][live[k]] = mirror
            ior = np.where(basic, mat["refractiveIndexBasic"], mat["refractiveIndexRough"]).astype(dt)
            ior = np.where(glass, ior, dt(1))
            N = g[k, :3]
            real = CH._real_normal(flat, prim[k], inst[k], dt)
            facing = -(real * D[k]).sum(1)
            outside = np.where(basic, facing > dt(EPS), facing > 0)  # each material's own compare in shadeHit
            n1n2 = np.where(outside, dt(1) / ior, ior)
            cos1 = -(N * D[k]).sum(1)
            Kt = dt(1) - n1n2 * n1n2 * (dt(1) - cos1 * cos1)
            transmit = glass & (Kt > dt(EPS)) & (j < K)
            total = glass & ~(Kt > dt(EPS)) & (j < K)  # (at stage K every surface is terminal: the interface is not looked at)
            with np.errstate(invalid="ignore"):
                T = n1n2[:, None] * D[k] + N * (n1n2 * cos1 - np.sqrt(np.maximum(Kt, 0)))[:, None]
            Rf = D[k] + N * (dt(2) * cos1)[:, None]
            G = np.where((facing > 0)[:, None], real, -real)
            side = (G * CH._unit(Rf)).sum(1)
            reflect = (total | (mirror & (j < K))) & (side > dt(EPS))
            go = transmit | reflect
            info["met"][live[k]] |= mirror | total
            cont[k] = go
            followed[k] = reflect
            tir[k] = total & ~reflect
            nxt[k] = CH._unit(np.where(transmit[:, None], T, np.where(reflect[:, None], Rf, 1.0)))
            tinted = reflect & mirror
            off_mirror[k] = tinted
            tint[k[tinted]] = tint[k[tinted]] * mat["colour"][tinted, :3].astype(dt)  # one multiply per component, in stage order
        count, mirrors = count + followed, mirrors + off_mirror
        end = ~cont
        e = live[end]
        ah[e, :3] = tint[end] * a[end, :3]
        ah[e, 3] = a[end, 3]
        nd[e, :3] = g[end, :3]
        nd[e, 3] = np.where(hit[end], dist[end] + g[end, 3], dt(R.SKY_DEPTH))
        info["prim"][e], info["inst"][e] = np.where(hit[end], prim[end], -1), np.where(hit[end], inst[end], -1)
        info["depth"][e] = j
        info["tir"][e] = tir[end]
        info["reflections"][e], info["mirrors"][e] = count[end], mirrors[end]
        info["tint"][e] = tint[end]
        info["dir"][e] = D[end]
        with np.errstate(invalid="ignore"):
            info["point"][e] = np.where(hit[end, None], co[end].astype(dt) + Do[end] * t[end, None], np.nan)
        # the next segment: X with the segment's own origin and un-normalised direction (k_shade's X = o + t d), offset along the new direction
        X = co[cont].astype(dt) + Do[cont] * t[cont, None]
        dist = dist[cont] + t[cont] * scale[cont]
        co = (X + nxt[cont] * dt(EPS)).astype(np.float32)
        cd = nxt[cont].astype(np.float32)
        tint, count, mirrors = tint[cont], count[cont], mirrors[cont]
        live = live[cont]
    info["segments"] = info["depth"] + 1
    return ah, nd, info
