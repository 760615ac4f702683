"""Synthetic shade inputs over the material and incidence space of shade (kernel.cl:190-301, neeIsShading shading.cl:356-623): plain numpy, the host
library for the flattening, no GPU import.  Shared by tests/test_shade_grid_cpu.py (oracle against the reference's own kernel, finiteness, conditioning) and
tests/test_gpu_shade_grid.py (k_shade against the oracle).

ONE scene: two meshes -- `axis`, whose every face and vertex normal is exactly +-x, +-y or +-z, and `tilt`, the same mesh turned by an irrational angle
baked into its vertices -- each instanced under four placements.  A mesh is one six-quad room (a cube, normals inwards, EXPLICIT vertex normals) per
material of MATERIALS plus a ceiling light; the rooms coincide, which no shade input can notice: the hit records are made here, not traced.

An entry is a hit record on a triangle of one (mesh, placement) with a chosen material: barycentrics random or at a vertex / an edge midpoint, incidence
from the cosine LADDER against the WORLD-space geometric normal with a random azimuth (every non-zero rung a factor >= 1.5 away from kEPS = 1e-4, from the
0.05 cutoff and from 0: round-off flips no decision of a rung, a wrong constant or comparison flips all of it), t in {1e-3, U(0.1, 1.5), 50}, throughput 1
(a primary ray: bounce 0) or U(0.1, 1) (bounce 1).  Sky misses and emissive hits with and without LASTSPECULAR come with the diffuse family.

Labels per entry (the strata of the tests are the values of each label, at least 64 entries each): family, corner (the material's parameters), incidence
(the rung), placement (mesh/placement); `degenerate` marks the entries whose object-space shading normal is exactly +-x under a sampler seeded with
(1,0,0) -- PBR and rough glass on the x walls of `axis`, under every placement: the reference's tangent frame is NaN there (oracle.cpp, orient).

The family "emissive mis" (emissive_mis_grid) is the input space of the one branch only neeMisShading has (shading.cl:69-90): hits on the light after a
non-specular bounce, over a ladder of incoming densities, a ladder of solid angles and both sides of the light; its entries carry two more labels,
in_pdf and solid_angle.  Every entry of every family carries the incoming density in rays["pdf"] (0 unless a test seeds it: seed_in_pdf)."""
import numpy as np

from ptamd import host as H
from ptamd import layout as L

LADDER = (1.0, 0.9, 0.5, 0.2, 0.06, 0.049, 1e-2, 2e-4, 5e-5, 0.0, -5e-5, -1e-2, -0.5, -1.0)
# The rung 0 is realised as +-ZERO_RUNG: 50 times below kEPS and some twenty times the round-off of a dot product of unit vectors.  An exact 0 has no side
# that round-off keeps: rough glass takes `dot(realNormal, -D) > 0` for the side of the interface the ray is on, every refractive material flips the
# shading normal on `dot(shadingNormal, -D) < 0`, and two correct builds of the same code then refract into opposite half spaces (the strict and the
# -march=native oracle did, on 10 of 165 rough-glass entries of an exactly-zero rung: tests/test_shade_grid_cpu.py, conditioning).
# Rough glass DIVIDES by that cosine (calcWeight, refract.cl:116-134): at 2e-6 its round-off (1e-7) is 5 % of it and the throughput of a smoothness-1
# entry moved by 1 % between the two builds, with one alive / finished flip.  Its zero rung is therefore moved to the nearest value at which the quotient
# is good to the comparison's 2e-3: +-5e-5 (the entries join the two neighbouring rungs' conditions under a label of their own).
ZERO_RUNG, ZERO_RUNG_ROUGH_GLASS = 2e-6, 5e-5
# Rough glass also takes sqrt(1 - NdotV^2) (G_SmithBeckmannCorrelated: tan(acos(NdotV)) in the reference): at exactly normal incidence on a face whose fp32
# normal is not an axis, NdotV rounds to 1 + 1 ulp on one build and not on the other, the root is NaN, the weight 0 and the path ends -- in the reference
# just the same (the oracle equals it bit for bit there).  Its rungs +-1 are moved to +-0.9999, where 1 - NdotV^2 = 2e-4 is good to 5e-4.
NORMAL_RUNG_ROUGH_GLASS = 0.9999
K_MAX_SMOOTHNESS = np.float32(0.94)  # shading.cl:9
BELOW, ABOVE = np.nextafter(K_MAX_SMOOTHNESS, np.float32(0)), np.nextafter(K_MAX_SMOOTHNESS, np.float32(1))
SMOOTHNESS = (("0", 0.0), ("0.3", 0.3), ("0.94-", BELOW), ("0.94+", ABOVE), ("0.97", 0.97), ("1", 1.0))
AIR_IOR = 1.000277  # scene.cl:46
TILT_AXIS, TILT_ANGLE = (1.0, 1.0, 1.0), 2.0 ** 0.5  # radians: irrational, no face of `tilt` near an axis

# name -> (location, rotation axis or None, angle, scale)
PLACEMENTS = {
    "identity": ((0.0, 0.0, 0.0), None, 0.0, (1.0, 1.0, 1.0)),
    "rotated+1.3": ((0.3, 0.1, -0.2), (1, 2, 0), 0.8, (1.3, 1.3, 1.3)),
    "mirrored": ((-0.2, 0.15, 0.1), (1, 2, 0), 0.8, (-1.0, 1.1, 0.9)),
    "quarter turn z": ((0.0, 0.0, 0.0), (0, 0, 1), np.pi / 2, (1.0, 1.0, 1.0)),
}


def _materials():
    """[(family, corner, record)] -- the order is the material index inside either mesh"""
    out = [("diffuse", "plain", L.material_diffuse((0.7, 0.6, 0.5))), ("diffuse", "textured", L.material_diffuse((0, 0, 0), texture_id=0))]
    for name, s in SMOOTHNESS:
        out.append(("pbr dielectric", f"s={name} f0=0.04", L.material_pbr_dielectric((0.2, 0.3, 0.75), s, 0.04)))
    for name, s in (SMOOTHNESS[1], SMOOTHNESS[4]):
        for f0 in (0.0, 1.0):
            out.append(("pbr dielectric", f"s={name} f0={f0:g}", L.material_pbr_dielectric((0.2, 0.3, 0.75), s, f0)))
    for name, s in SMOOTHNESS:
        out.append(("pbr metal", f"s={name}", L.material_pbr_metal((0.955, 0.638, 0.538), s)))
    for name, s in SMOOTHNESS:
        for ior in (1.0, AIR_IOR, 1.5, 2.4):
            out.append(("rough glass", f"s={name} ior={ior:g}", L.material_refractive(s, ior, (1.0, 0.6, 0.6), 5.0)))
    for ior in (0.8, 1.0, AIR_IOR, 1.5, 2.4):
        out.append(("basic glass", f"ior={ior:g}", L.material_basic_refractive(ior, (0.5, 1.0, 0.5), 3.0)))
    out.append(("emissive", "light", L.material_emissive((1.0, 0.92, 0.8), 12.0)))
    return out


MATERIALS = _materials()
FAMILIES = ("diffuse", "pbr dielectric", "pbr metal", "rough glass", "basic glass")  # (sky misses and emissive hits ride with "diffuse")
ENTRIES_PER_CORNER = {"diffuse": 512, "pbr dielectric": 192, "pbr metal": 256, "rough glass": 96, "basic glass": 256}
N_MISS, N_EMISSIVE = 128, 128  # (emissive: each of with / without LASTSPECULAR)


def texture():
    """[1][16][16][4]: random opaque colours, the left half alpha 0 (a bilinear fetch is alpha 0 only where all four texels are)"""
    rng = np.random.default_rng(2)
    t = np.ones((1, 16, 16, 4), np.float32)
    t[0, ..., :3] = rng.uniform(0.1, 0.9, (16, 16, 3))
    t[0, :, :8, 3] = 0.0
    return t


def sky():
    rng = np.random.default_rng(3)
    s = np.ones((1, 8, 16, 4), np.float32)
    s[0, ..., :3] = rng.uniform(0.2, 2.0, (8, 16, 3))
    return s


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _quat(axis, angle):
    if axis is None:
        return (1.0, 0.0, 0.0, 0.0)
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return (float(np.cos(angle / 2)), *(float(c) for c in np.sin(angle / 2) * a))


def _inward_quad(axis, sign, at=1.0, half=1.0):
    """The quad in the plane x_axis = -sign * at whose geometric normal (p1 - p0) x (p2 - p0) is exactly sign * e_axis: corners, that normal"""
    e = np.eye(3)
    b, c = ((axis + 1) % 3, (axis + 2) % 3) if sign > 0 else ((axis + 2) % 3, (axis + 1) % 3)
    p0 = -sign * at * e[axis] - half * e[b] - half * e[c]
    return np.array([p0, p0 + 2 * half * e[b], p0 + 2 * half * e[b] + 2 * half * e[c], p0 + 2 * half * e[c]]), sign * e[axis]


def mesh_arrays(tilted, materials=None, light_material=None):
    """(positions, normals, uv, indices, material index) of one room per material (every one but the last) and the light quad (the last material)"""
    mats = len(MATERIALS) if materials is None else materials
    light = mats - 1 if light_material is None else light_material
    R = _rotation(TILT_AXIS, TILT_ANGLE) if tilted else np.eye(3)
    P, N, UV, I, M = [], [], [], [], []
    uv = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], np.float64) + 0.25  # tiles twice: ADDRESS_REPEAT is exercised
    quads = [(m, *_inward_quad(a, s)) for m in range(mats) if m != light for a in range(3) for s in (1, -1)]
    quads.append((light, *_inward_quad(1, -1, at=0.98, half=0.25)))
    for m, p, n in quads:
        I.append(np.array([[0, 1, 2], [0, 2, 3]]) + 4 * len(P))
        P.append(p @ R.T), N.append(np.tile(n @ R.T, (4, 1))), UV.append(uv), M.extend([m, m])
    return (np.concatenate(P).astype(np.float32), np.concatenate(N).astype(np.float32), np.concatenate(UV).astype(np.float32),
            np.concatenate(I).astype(np.uint32), np.asarray(M, np.uint32))


# The emissive-under-MIS family alone sees one more instance of either mesh: a pure uniform scale that is not 1.  neeMisShading takes the light's area
# in OBJECT space and the distance in WORLD space (shading.cl:75-80); only a scaled placement tells a kernel that "fixes" this apart, and a scale of
# 1/2 moves its solid angle by a factor 4.  The other families keep the scene they were measured on: a ninth and tenth instance would add lights.
EXTRA_PLACEMENTS = {"scaled 0.5": ((0.1, -0.2, 0.3), None, 0.0, (0.5, 0.5, 0.5))}


class Scene:
    """The flattened scene and, per (mesh, placement): the top-level leaf, the float64 matrices, the triangles by material"""

    def __init__(self, extra=False):
        placements = {**PLACEMENTS, **EXTRA_PLACEMENTS} if extra else PLACEMENTS
        recs = [m[2] for m in MATERIALS]
        self.scene = H.Scene()
        meshes = {}
        for name, tilted in (("axis", False), ("tilt", True)):
            p, n, uv, i, m = mesh_arrays(tilted)
            meshes[name] = H.Mesh(p, i, recs, material_index=m, normals=n, tex_coords=uv, builder=H.BVH_BINNED_SAH)
        expect = []
        for mname, mesh in meshes.items():
            for pname, (loc, axis, ang, scale) in placements.items():
                self.scene.add_node(mesh, location=loc, orientation_wxyz=_quat(axis, ang), scale=scale)
                Rm = np.eye(3) if axis is None else _rotation(axis, ang)
                fwd = np.eye(4)
                fwd[:3, :3], fwd[:3, 3] = Rm @ np.diag(scale), loc
                expect.append((mname, pname, fwd))
        self.flat = flat = self.scene.flatten()
        self.tex, self.sky = texture(), sky()
        self.camera = H.camera_data((0.0, 0.0, -3.9), H.look_at_quat((0.0, 0.0, -3.9), (0.0, 0.0, 0.0)), 40.0, 4 / 3)
        raw = [bytes(np.asarray(r, L.MATERIAL).tobytes()) for r in recs]
        self.material_label = np.array([raw.index(bytes(m.tobytes())) for m in flat.materials])  # flat material index -> index into MATERIALS
        axis_normals = {}
        self.where = {}  # (mesh, placement) -> dict(leaf, A (world -> object, 4x4), M (object -> world), tris {MATERIALS index: [global triangle]})
        for leaf in np.flatnonzero(flat.top_nodes["isLeaf"] != 0):
            A = flat.top_nodes["invTransform"][leaf].astype(np.float64).reshape(4, 4).T  # column-major
            tris = self._leaf_triangles(int(flat.top_nodes["a"][leaf]))
            vn = flat.vertices["normal"][flat.triangles["indices"][tris].astype(np.int64).ravel(), :3]
            is_axis = bool(np.all((np.abs(vn) == 1).sum(1) == 1) and np.all((vn == 0).sum(1) == 2))
            match = [k for k, (mn, pn, fwd) in enumerate(expect) if (mn == "axis") == is_axis and np.allclose(A @ fwd, np.eye(4), atol=1e-5)]
            assert len(match) == 1, (leaf, match)
            mn, pn, _ = expect[match[0]]
            by_mat = {}
            for t in tris:
                by_mat.setdefault(int(self.material_label[flat.triangles["materialIndex"][t]]), []).append(int(t))
            self.where[(mn, pn)] = dict(leaf=int(leaf), A=A, M=np.linalg.inv(A), tris={k: np.array(sorted(set(v))) for k, v in by_mat.items()})
            axis_normals[mn] = is_axis
        assert len(self.where) == 2 * len(placements), "every (mesh, placement) found once"
        assert axis_normals == {"axis": True, "tilt": False}, "only `axis` has exact normals"

    def _leaf_triangles(self, root):
        out, stack = [], [root]
        while stack:
            nd = self.flat.sub_nodes[stack.pop()]
            if nd["count"]:
                out += list(range(int(nd["left"]), int(nd["left"]) + int(nd["count"])))
            else:
                stack += [int(nd["left"]), int(nd["left"]) + 1]
        return np.array(out)


_scenes = {}


def scene(extra=False):
    """the grid's scene; extra: with EXTRA_PLACEMENTS (the emissive-under-MIS family's)"""
    if extra not in _scenes:
        _scenes[extra] = Scene(extra)
    return _scenes[extra]


class Grid:
    """Entries of one family: rays (RAY_DATA, outputPixel = the entry's index), hit, t, uv, prim, inst (top-level leaf), labels {name: array of str},
    degenerate (bool), alpha0 (bool: the textured-diffuse entries whose fetch is alpha 0), colour (the hit material's colour)"""


def _perp(n, rng):
    """unit vectors (T, B) completing n to a frame, T turned by a random azimuth"""
    k = np.argmin(np.abs(n), axis=1)
    a = np.zeros_like(n)
    a[np.arange(len(n)), k] = 1.0
    t = np.cross(n, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    phi = rng.uniform(0, 2 * np.pi, (len(n), 1))
    return np.cos(phi) * t + np.sin(phi) * b


def _alpha_is_zero(tex, s, t):
    """the bilinear NORMALIZED | REPEAT fetch of alpha at (s, t) is exactly 0 (float64 restatement of sampleLinearRepeat's addressing)"""
    h, w = tex.shape[1:3]
    u, v = (s - np.floor(s)) * w - 0.5, (t - np.floor(t)) * h - 0.5
    i0, j0 = np.floor(u).astype(int) % w, np.floor(v).astype(int) % h
    i1, j1 = (i0 + 1) % w, (j0 + 1) % h
    a = tex[0, ..., 3]
    return (a[j0, i0] == 0) & (a[j0, i1] == 0) & (a[j1, i0] == 0) & (a[j1, i1] == 0)


def rung_values(family, exact_rungs=False):
    """what each rung of LADDER holds for `family`: [(label, magnitude-signed value, or (+v, -v) for the zero rung)]"""
    out = []
    for r in LADDER:
        if exact_rungs:
            out.append((f"cos={r:g}", r))
        elif r == 0.0:
            z = ZERO_RUNG_ROUGH_GLASS if family == "rough glass" else ZERO_RUNG
            out.append((f"cos=+-{z:g} (the zero rung)", (z, -z)))
        elif abs(r) == 1.0 and family == "rough glass":
            out.append((f"cos={np.sign(r) * NORMAL_RUNG_ROUGH_GLASS:g} (the rung {r:g})", float(np.sign(r)) * NORMAL_RUNG_ROUGH_GLASS))
        else:
            out.append((f"cos={r:g}", r))
    return out


def grid(family, seed=1, exact_rungs=False):
    """The entries of `family` (one of FAMILIES); "diffuse" also carries the sky misses and the emissive hits.
    exact_rungs: every rung holds the value LADDER names -- 0 is 0, +-1 is +-1 for rough glass too.  Such a grid is NOT conditioned (see ZERO_RUNG and
    NORMAL_RUNG_ROUGH_GLASS above): it serves the comparison with the reference's own kernel, which is bit for bit and needs no conditioning."""
    if family == "emissive mis":
        assert not exact_rungs
        return emissive_mis_grid(seed)
    S = scene()
    flat = S.flat
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    corners = [k for k, m in enumerate(MATERIALS) if m[0] == family]
    n_mat = ENTRIES_PER_CORNER[family] * len(corners)
    mat = np.repeat(corners, ENTRIES_PER_CORNER[family])
    flags = np.zeros(n_mat, np.int32)
    if family == "diffuse":
        light = len(MATERIALS) - 1
        mat = np.concatenate([mat, np.full(2 * N_EMISSIVE, light)])
        flags = np.concatenate([flags, np.repeat([L.SHADINGFLAGS_LASTSPECULAR, 0], N_EMISSIVE)]).astype(np.int32)
    n_hit = len(mat)
    n = n_hit + (N_MISS if family == "diffuse" else 0)
    keys = list(S.where)
    place = rng.permutation(np.arange(n_hit) % len(keys))  # balanced over the eight (mesh, placement) pairs
    rung = rng.permutation(np.arange(n_hit) % len(LADDER))
    rungs = rung_values(family, exact_rungs)
    coin = rng.random(n_hit) < 0.5
    c = np.array([(v[0] if coin[i] else v[1]) if isinstance(v, tuple) else v for i, v in enumerate(rungs[r][1] for r in rung)], np.float64)
    # barycentrics: 70 % random, 30 % the three vertices and an edge midpoint
    r1, r2 = np.sqrt(rng.random(n_hit)), rng.random(n_hit)
    u, v = r1 * (1 - r2), r1 * r2
    special = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.5], [0.5, 0.0], [0.0, 0.5]])
    pick = rng.integers(0, len(special), n_hit)
    is_special = rng.random(n_hit) < 0.3
    u, v = np.where(is_special, special[pick, 0], u).astype(np.float32), np.where(is_special, special[pick, 1], v).astype(np.float32)
    tkind = rng.integers(0, 3, n_hit)
    t = np.where(tkind == 0, 1e-3, np.where(tkind == 1, rng.uniform(0.1, 1.5, n_hit), 50.0)).astype(np.float32)
    unit = rng.random(n_hit) < 0.5
    thr = np.where(unit[:, None], 1.0, rng.uniform(0.1, 1.0, (n_hit, 3))).astype(np.float32)

    prim, inst = np.zeros(n_hit, np.int32), np.zeros(n_hit, np.int32)
    X, Nw, shading_n = np.zeros((n_hit, 3)), np.zeros((n_hit, 3)), np.zeros((n_hit, 3), np.float32)
    tc = np.zeros((n_hit, 2))
    for k, key in enumerate(keys):
        w = S.where[key]
        for m in np.unique(mat[place == k]):
            sel = np.flatnonzero((place == k) & (mat == m))
            tri = rng.choice(w["tris"][int(m)], len(sel))
            vi = flat.triangles["indices"][tri].astype(np.int64)
            p = flat.vertices["vertex"][vi, :3].astype(np.float64)
            e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
            obj = p[:, 0] + u[sel, None] * e1 + v[sel, None] * e2
            X[sel] = obj @ w["M"][:3, :3].T + w["M"][:3, 3]
            g = np.cross(e1, e2) @ w["A"][:3, :3]  # (M^-1)^T n: the normal transform (math.cl:22-29)
            Nw[sel] = g / np.linalg.norm(g, axis=1, keepdims=True)
            shading_n[sel] = flat.vertices["normal"][vi[:, 0], :3]
            uvs = flat.vertices["texCoord"][vi].astype(np.float64)
            tc[sel] = uvs[:, 0] + (uvs[:, 1] - uvs[:, 0]) * u[sel, None] + (uvs[:, 2] - uvs[:, 0]) * v[sel, None]
            prim[sel], inst[sel] = tri, w["leaf"]
    D = -(c[:, None] * Nw + np.sqrt(1 - c[:, None] ** 2) * _perp(Nw, rng))
    o = X - t[:, None].astype(np.float64) * D

    g = Grid()
    g.family, g.scene, g.n = family, S, n
    g.rays = np.zeros(n, L.RAY_DATA)
    g.rays["origin"][:n_hit, :3], g.rays["direction"][:n_hit, :3], g.rays["multiplier"][:n_hit, :3] = o, D, thr
    g.rays["flags"][:n_hit] = np.where(unit & (flags == 0) & (mat != len(MATERIALS) - 1), L.SHADINGFLAGS_LASTSPECULAR, flags)  # primary rays carry it
    g.rays["numBounces"][:n_hit] = np.where(unit, 0, 1)  # (a primary ray's throughput is 1 by definition: k_shade does not read it)
    g.hit = np.arange(n) < n_hit
    g.t, g.uv, g.prim, g.inst = (np.zeros(n, np.float32), np.zeros((n, 2), np.float32), np.full(n, -1, np.int32), np.full(n, -1, np.int32))
    g.t[:n_hit], g.uv[:n_hit, 0], g.uv[:n_hit, 1], g.prim[:n_hit], g.inst[:n_hit] = t, u, v, prim, inst
    fam = np.array([MATERIALS[m][0] for m in mat] + ["miss"] * (n - n_hit))
    corner = np.array([MATERIALS[m][1] for m in mat] + ["sky"] * (n - n_hit), dtype=object)
    corner[:n_hit][(fam[:n_hit] == "emissive") & (flags != 0)] = "after a specular bounce"
    corner[:n_hit][(fam[:n_hit] == "emissive") & (flags == 0)] = "after a diffuse bounce"
    g.alpha0 = np.zeros(n, bool)
    g.alpha0[:n_hit] = (np.array([MATERIALS[m][1] for m in mat]) == "textured") & _alpha_is_zero(S.tex, tc[:, 0], tc[:, 1])
    g.labels = dict(family=fam, corner=corner.astype(str),
                    incidence=np.array([rungs[r][0] for r in rung] + ["miss"] * (n - n_hit)),
                    placement=np.array([f"{keys[k][0]}/{keys[k][1]}" for k in place] + ["miss"] * (n - n_hit)))
    seeded_x = np.isin(fam[:n_hit], ("pbr dielectric", "pbr metal", "rough glass"))
    g.degenerate = np.zeros(n, bool)
    g.degenerate[:n_hit] = seeded_x & (np.abs(shading_n[:, 0]) == 1) & (shading_n[:, 1] == 0) & (shading_n[:, 2] == 0)
    g.shading_normal = np.zeros((n, 3), np.float32)  # object space, as shade uses it
    g.shading_normal[:n_hit] = shading_n
    g.colour = np.zeros((n, 3), np.float32)
    g.colour[:n_hit] = np.array([MATERIALS[m][2]["colour"][:3] for m in mat])
    if n > n_hit:  # sky misses: any direction, throughput as above
        d = rng.normal(size=(n - n_hit, 3))
        g.rays["direction"][n_hit:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
        g.rays["origin"][n_hit:, :3] = rng.uniform(-1, 1, (n - n_hit, 3))
        g.rays["multiplier"][n_hit:, :3] = rng.uniform(0.1, 1.0, (n - n_hit, 3))
        g.rays["numBounces"][n_hit:] = 1
    g.rays["outputPixel"] = np.arange(n)
    return g


# ---------------------------------------------------------------- emissive hits under neeMisShading
K_EPS = np.float32(1e-4)  # EPSILON, shading.cl


def d_ggx(n_dot_h, alpha):
    """D_GGX (pbr_brdf.cl:96-105) in float64"""
    a2 = alpha * alpha
    f = n_dot_h * n_dot_h * (a2 - 1) + 1
    return a2 / (np.pi * f * f) if f > 1e-4 else 1.0


# The incoming density (RayData.pdf): INPUTS, handed over as these very floats -- the neighbours of kEPS are exact.  The peak of the sharpest GGX lobe
# that is not treated as a mirror, D_GGX(1, 1 - kMaxSmoothness), is 1 / (pi 0.06^2) = 88.4 (alpha is the roughness itself in this renderer, not its square).
IN_PDF_LADDER = (("0", np.float32(0)), ("kEPS-", np.nextafter(K_EPS, np.float32(0))), ("kEPS+", np.nextafter(K_EPS, np.float32(1))),
                 ("1/pi", np.float32(1 / np.pi)), ("1", np.float32(1)), ("GGX peak of s=0.94", np.float32(d_ggx(1.0, 1 - 0.94))), ("1e7", np.float32(1e7)))
# The solid angle cos * area / t^2 the branch computes, set through t.  Its kEPS neighbours are COMPUTED from an area (Heron, three roots), a normalised
# normal, a dot product and a squared distance, each good to some 1e-6 relative (1e-3 for the cosine at the 2e-4 rung): they sit a factor 1.02 either
# side, twenty times that round-off, where a wrong constant, a wrong comparison or an area off by any scale still flips the whole rung.
SOLID_ANGLE_LADDER = (("1e-6", 1e-6), ("kEPS/1.02", 1e-4 / 1.02), ("kEPS*1.02", 1e-4 * 1.02), ("0.05", 0.05), ("20, clamped to 2 pi", 20.0))
EMISSIVE_MIS_COSINES = (1.0, 0.5, 1e-2, 2e-4, -1e-2, -0.5)  # against the world-space geometric normal: head-on, oblique, grazing; the back side
BACK_SIDE = "negative (back side)"
N_EMISSIVE_MIS, N_EMISSIVE_MIS_CONTROL = 2816, 128


def emissive_mis_grid(seed=1):
    """Hits on the light of either mesh under every placement of PLACEMENTS and EXTRA_PLACEMENTS, LASTSPECULAR clear: N_EMISSIVE_MIS entries at bounce 1,
    throughput U(0.1, 1), over IN_PDF_LADDER x SOLID_ANGLE_LADDER x EMISSIVE_MIS_COSINES x placement (each axis balanced and permuted on its own), and
    N_EMISSIVE_MIS_CONTROL entries at bounce 0 with density 0 and throughput 1 (a primary ray's word is never loaded), front side, solid angle above
    kEPS.  The ray origin is X - t d to fp32 rounding: the branch measures the distance |X - origin| with X = origin + t d.
    g.solid_angle is the solid angle of each entry in float64 from the fp32 inputs (negative on the back side, not clamped)."""
    S = scene(extra=True)
    flat = S.flat
    rng = np.random.default_rng([seed, 977])
    n_main, n = N_EMISSIVE_MIS, N_EMISSIVE_MIS + N_EMISSIVE_MIS_CONTROL
    control = np.arange(n) >= n_main
    light = len(MATERIALS) - 1
    keys = list(S.where)
    place = rng.permutation(np.arange(n) % len(keys))
    pdf_rung = np.where(control, 0, rng.permutation(np.arange(n) % len(IN_PDF_LADDER)))
    front = [k for k, c in enumerate(EMISSIVE_MIS_COSINES) if c > 0]
    cos_rung = np.where(control, rng.choice(front, n), rng.permutation(np.arange(n) % len(EMISSIVE_MIS_COSINES)))
    sa_rung = np.where(control, rng.integers(2, len(SOLID_ANGLE_LADDER), n), rng.permutation(np.arange(n) % len(SOLID_ANGLE_LADDER)))
    c = np.array(EMISSIVE_MIS_COSINES)[cos_rung]
    want_sa = np.array([v for _, v in SOLID_ANGLE_LADDER])[sa_rung]
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    u, v = (r1 * (1 - r2)).astype(np.float32), (r1 * r2).astype(np.float32)
    thr = np.where(control[:, None], 1.0, rng.uniform(0.1, 1.0, (n, 3))).astype(np.float32)

    prim, inst = np.zeros(n, np.int32), np.zeros(n, np.int32)
    X, Nw, area = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    for k, key in enumerate(keys):
        w = S.where[key]
        sel = np.flatnonzero(place == k)
        tri = rng.choice(w["tris"][light], len(sel))
        p = flat.vertices["vertex"][flat.triangles["indices"][tri].astype(np.int64), :3].astype(np.float64)
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        obj = p[:, 0] + u[sel, None] * e1 + v[sel, None] * e2
        X[sel] = obj @ w["M"][:3, :3].T + w["M"][:3, 3]
        gn = np.cross(e1, e2) @ w["A"][:3, :3]
        Nw[sel] = gn / np.linalg.norm(gn, axis=1, keepdims=True)
        area[sel] = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)  # OBJECT space, as the reference takes it
        prim[sel], inst[sel] = tri, w["leaf"]
    D = -(c[:, None] * Nw + np.sqrt(1 - c[:, None] ** 2) * _perp(Nw, rng))
    t = np.sqrt(np.abs(c) * area / want_sa).astype(np.float32)
    o = X - t[:, None].astype(np.float64) * D

    g = Grid()
    g.family, g.scene, g.n = "emissive mis", S, n
    g.rays = np.zeros(n, L.RAY_DATA)
    g.rays["origin"][:, :3], g.rays["direction"][:, :3], g.rays["multiplier"][:, :3] = o, D, thr
    g.rays["numBounces"] = np.where(control, 0, 1)
    g.rays["pdf"] = np.array([val for _, val in IN_PDF_LADDER], np.float32)[pdf_rung]
    g.rays["outputPixel"] = np.arange(n)
    g.hit = np.ones(n, bool)
    g.t, g.uv, g.prim, g.inst = t, np.stack([u, v], 1), prim, inst
    d32 = g.rays["direction"][:, :3].astype(np.float64)
    unit = d32 / np.linalg.norm(d32, axis=1, keepdims=True)
    g.solid_angle = -(Nw * unit).sum(1) * area / (t.astype(np.float64) ** 2 * (d32 * d32).sum(1))
    back = c < 0
    g.labels = dict(family=np.full(n, "emissive"), corner=np.where(control, "bounce 0 (control)", "bounce 1"),
                    incidence=np.array([f"cos={x:g}" for x in c]), placement=np.array([f"{keys[k][0]}/{keys[k][1]}" for k in place]),
                    in_pdf=np.where(control, "0 at bounce 0 (control)", np.array([name for name, _ in IN_PDF_LADDER])[pdf_rung]),
                    solid_angle=np.where(back, BACK_SIDE, np.array([name for name, _ in SOLID_ANGLE_LADDER])[sa_rung]))
    g.alpha0, g.degenerate = np.zeros(n, bool), np.zeros(n, bool)
    g.shading_normal = flat.vertices["normal"][flat.triangles["indices"][prim, 0].astype(np.int64), :3].astype(np.float32)
    g.colour = np.tile(np.asarray(MATERIALS[light][2]["colour"][:3], np.float32), (n, 1))
    return g


def seed_in_pdf(g, seed=5):
    """A copy of `g` whose bounce-1 entries carry an incoming density U(0, 10) (bounce 0 keeps 0: a primary ray's word is never loaded).
    Conditioning: under MIS an emissive hit after a diffuse bounce deposits a weight that goes with its solid angle, hence with the cosine of incidence;
    at the rungs +-5e-5 and the zero rung (+-2e-6) the round-off of that cosine (1e-7) is 0.2 % and 5 % of it -- the strict and the -march=native
    oracle deposited 7.428 and 7.475 on one such entry.  Those emissive entries keep density 0 (they deposit nothing under either integrator); the
    emissive-under-MIS family holds the grazing hits, at cosines whose round-off stays a quarter of the comparison's 2e-3."""
    s = take(g, np.arange(g.n))
    rng = np.random.default_rng([seed, g.n])
    inc = g.labels["incidence"]
    ill = (g.labels["family"] == "emissive") & (np.isin(inc, (f"cos={5e-5:g}", f"cos={-5e-5:g}")) | np.char.endswith(inc, "(the zero rung)"))
    s.rays["pdf"] = np.where((s.rays["numBounces"] != 0) & ~ill, rng.uniform(0.0, 10.0, g.n), 0.0).astype(np.float32)
    return s


def strata(g):
    """[(label, indices)]: per label dimension, the entries of each of its values -- the strata the gates are asserted on"""
    out = []
    for dim in ("family", "corner", "incidence", "placement", "in_pdf", "solid_angle"):
        if dim not in g.labels:
            continue
        for val in sorted(set(g.labels[dim])):
            idx = np.flatnonzero(g.labels[dim] == val)
            if dim != "family" and val == "miss":
                continue
            out.append((f"{dim}: {val}", idx))
    return out


def queue(g):
    """The entries as a queue of N slots (N a multiple of 64) in the reference's records: (N, rays, shading data) for orc_shade / ref_shade"""
    flat = g.scene.flat
    N = (g.n + 63) // 64 * 64
    qr = np.zeros(N, L.RAY_DATA)
    qr[:g.n] = g.rays
    sd = np.zeros(N, L.SHADING_DATA)
    sd["hit"][:g.n] = g.hit
    sd["t"][:g.n], sd["uv"][:g.n], sd["triangleIndex"][:g.n] = g.t, g.uv, np.maximum(g.prim, 0)
    base = flat.top_nodes.ctypes.data + L.TOP_BVH_NODE.fields["invTransform"][1]
    sd["invTransform"][:g.n] = np.where(g.hit, base + g.inst.astype(np.int64) * L.TOP_BVH_NODE.itemsize, 0).astype(np.uint64)
    return N, qr, sd


class Shaded:
    """What one shade pass over a Grid's queue returned, PER ENTRY (the reference enqueues every shaded hit, finished or not, in slot order):
    ray / shadow: RAY_DATA records (zero where the entry was a miss), ray_alive / shadow_alive, radiance (n, 3), streams (LFSR113 mode)"""


def shade(g, which="oracle", rng_mode=None, sample=2, seed=4, fast=False, light_sampling=None, width=64, height=48, integrator=None,
          compare_build=False):
    """orc_shade (which = "oracle"; counter PRNG keyed by (entry = pixel, sample, seed) unless rng_mode says LFSR113; integrator: one of orclib's
    INTEGRATOR_*, neeIsShading by default) or the reference's own shade kernel compiled for the host (which = "ref": LFSR113, stream k for slot k;
    compare_build: its COMPARE_SHADING build, neeMisShading where outputPixel % width < width / 2) over the queue of `g`.  The incoming density is
    rays["pdf"], the one written for the next bounce comes back as Shaded.ray["pdf"]."""
    import ctypes as C
    import orclib as O
    assert which == "ref" or not compare_build
    rng_mode = O.RNG_COUNTER if rng_mode is None else rng_mode
    S = g.scene
    sc = O.BoundScene(S.flat, sky=S.sky, material_textures=S.tex)
    N, qr, sd = queue(g)
    kd = sc.kernel_data(S.camera, width, height)
    kd["numInRays"], kd["maxRays"] = g.n, N
    out_r, out_s = np.zeros(N, L.RAY_DATA), np.zeros(N, L.RAY_DATA)
    acc = np.zeros((max(N, width * height), 4), np.float32)
    streams = O.create_streams(N) if (which == "ref" or rng_mode == O.RNG_LFSR113) else None
    if which == "ref":
        O.ref_kernels(compare_shading=compare_build).ref_shade(C.c_size_t(N), O._p(acc), O._p(out_r), O._p(out_s), O._p(qr), O._p(sd), O._p(kd),
                                                               C.byref(sc.struct), O._p(streams))
    else:
        prm = O.Params(rng_mode, sample, seed, 0, O.INTEGRATOR_IS if integrator is None else integrator,
                       O.LIGHTS_UNIFORM if light_sampling is None else light_sampling)
        O.oracle(fast).orc_shade(C.c_size_t(N), O._p(acc), O._p(out_r), O._p(out_s), O._p(qr), O._p(sd), O._p(kd), C.byref(sc.struct), O._p(streams),
                                 C.byref(prm), None)
    shaded = np.flatnonzero(g.hit)
    assert int(kd["numOutRays"]) == len(shaded)
    r = Shaded()
    r.ray, r.shadow = np.zeros(g.n, L.RAY_DATA), np.zeros(g.n, L.RAY_DATA)
    r.ray[shaded], r.shadow[shaded] = out_r[:len(shaded)], out_s[:len(shaded)]
    r.ray_alive = g.hit & ((r.ray["flags"] & L.SHADINGFLAGS_HASFINISHED) == 0)
    r.shadow_alive = g.hit & ((r.shadow["flags"] & L.SHADINGFLAGS_HASFINISHED) == 0)
    r.radiance = acc[:g.n, :3].copy()
    r.streams = None if streams is None else streams["current"][:g.n].copy()
    return r


RAY_FIELDS = (("origin", 3), ("direction", 3), ("multiplier", 3))


# ---------------------------------------------------------------- the small render
def axis_aligned_room(width=64, height=36):
    """(flat, camera, sky): a room with EXACT axis normals whose x walls are PBR (a dielectric and a metal), whose back wall is rough glass, with a diffuse
    floor and ceiling, a ceiling light and, turned by half a radian about y, an instanced axis-aligned box of PBR -- the scene on which every first
    bounce off an x wall carried NaN before orient() fell back to (0,1,0).  Open towards -z: the sky is seen."""
    mats = [L.material_diffuse((0.73, 0.73, 0.73)), L.material_pbr_dielectric((0.12, 0.45, 0.15), 0.7), L.material_pbr_metal((0.955, 0.638, 0.538), 0.8),
            L.material_refractive(0.9, 1.5, (1.0, 0.6, 0.6), 5.0), L.material_emissive((1.0, 0.92, 0.8), 12.0)]
    wall = {(0, 1): 1, (0, -1): 2, (1, 1): 0, (1, -1): 0, (2, -1): 3}  # (axis, sign of the inward normal) -> material; no wall at z = -1
    P, N, I, M = [], [], [], []
    quads = [(m, *_inward_quad(a, s)) for (a, s), m in wall.items()] + [(4, *_inward_quad(1, -1, at=0.98, half=0.25))]
    for m, p, nrm in quads:
        I.append(np.array([[0, 1, 2], [0, 2, 3]]) + 4 * len(P))
        P.append(p), N.append(np.tile(nrm, (4, 1))), M.extend([m, m])
    room = H.Mesh(np.concatenate(P).astype(np.float32), np.concatenate(I).astype(np.uint32), mats, material_index=np.asarray(M, np.uint32),
                  normals=np.concatenate(N).astype(np.float32), builder=H.BVH_BINNED_SAH)
    P, N, I = [], [], []
    for a in range(3):
        for s in (1, -1):  # outward normals: the inward quad of the opposite side, wound the other way
            p, nrm = _inward_quad(a, s)
            I.append(np.array([[0, 2, 1], [0, 3, 2]]) + 4 * len(P))
            P.append(p), N.append(np.tile(-nrm, (4, 1)))
    box = H.Mesh(np.concatenate(P).astype(np.float32), np.concatenate(I).astype(np.uint32), [L.material_pbr_dielectric((0.2, 0.3, 0.75), 0.96)],
                 normals=np.concatenate(N).astype(np.float32), builder=H.BVH_BINNED_SAH)
    sc = H.Scene()
    sc.add_node(room)
    sc.add_node(box, location=(0.3, -0.698, 0.2), orientation_wxyz=_quat((0, 1, 0), 0.5), scale=(0.3, 0.3, 0.3))
    cam = H.camera_data((0.0, 0.0, -3.9), H.look_at_quat((0.0, 0.0, -3.9), (0.0, 0.0, 0.0)), 40.0, width / height)
    flat = sc.flatten()
    flat._keep = (sc, room, box)
    return flat, cam, sky()


def take(g, idx):
    """the entries `idx` of a grid as a grid of their own (pixels renumbered: the pixel keys the PRNG)"""
    idx = np.asarray(idx)
    s = Grid()
    s.family, s.scene, s.n = g.family, g.scene, len(idx)
    s.rays = g.rays[idx].copy()
    s.rays["outputPixel"] = np.arange(len(idx))
    s.hit, s.t, s.uv, s.prim, s.inst = g.hit[idx], g.t[idx], g.uv[idx], g.prim[idx], g.inst[idx]
    s.alpha0, s.degenerate, s.colour, s.shading_normal = g.alpha0[idx], g.degenerate[idx], g.colour[idx], g.shading_normal[idx]
    s.labels = {k: v[idx] for k, v in g.labels.items()}
    if hasattr(g, "solid_angle"):
        s.solid_angle = g.solid_angle[idx]
    return s
