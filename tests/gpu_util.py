"""Helpers shared by the GPU parity tests (all calls go through the C-ABI via ptamd.device)."""
import re

import numpy as np
import pytest

import orclib as O
from ptamd import device


def make_ctx(D, bundle_or_flat, width, height, camera=None, sky=None, tex=None, **kw):
    flat = getattr(bundle_or_flat, "flat", bundle_or_flat)
    if hasattr(bundle_or_flat, "flat"):
        camera = bundle_or_flat.camera if camera is None else camera
        sky = bundle_or_flat.sky if sky is None else sky
        tex = bundle_or_flat.material_textures if tex is None else tex
    ctx = D.Context(width, height, **kw)
    ctx.upload_scene(flat, sky=sky, material_textures=tex)
    if camera is not None:
        ctx.set_camera(camera)
    return ctx


def oracle_scene(bundle_or_flat, sky=None, tex=None):
    flat = getattr(bundle_or_flat, "flat", bundle_or_flat)
    if hasattr(bundle_or_flat, "flat"):
        sky = bundle_or_flat.sky if sky is None else sky
        tex = bundle_or_flat.material_textures if tex is None else tex
    return O.BoundScene(flat, sky=sky, material_textures=tex)


def random_rays(n, seed, lo, hi):
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def aimed_rays(targets, n, seed, lo, hi):
    """Half of n rays like random_rays(lo, hi), half aimed at the spheres `targets` = [(centre, radius)] from 1.5 to 6 radii away: what finds an instance
    a thousand times smaller than its neighbours, with origins close enough to it that fp32 coordinates resolve its triangles."""
    o, d = random_rays(n, seed, lo, hi)
    rng = np.random.default_rng(seed + 1)
    m = n // 2
    which = rng.integers(0, len(targets), m)
    c = np.asarray([t[0] for t in targets], np.float64)[which]
    r = np.asarray([t[1] for t in targets], np.float64)[which, None]
    away = rng.normal(size=(m, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    oa = c + r * rng.uniform(1.5, 6.0, (m, 1)) * away
    da = c + r * rng.uniform(-0.6, 0.6, (m, 3)) - oa
    da /= np.linalg.norm(da, axis=1, keepdims=True)
    o[:m], d[:m] = oa.astype(np.float32), da.astype(np.float32)
    return o, d


MODES = ["two_level", "baked", "packet", "two_level_packet", "unbaked", "unbaked_packet", "two_level_parked", "unbaked_parked", "team"]


def mode_flags(gpu, mode):
    """two_level: instances are entered like the reference does (meshes that are a single leaf are still copied); unbaked: every
    instance is entered; baked: copied to world space (the default); *packet: pt_intersect runs the packet traversal kernel
    (one wave walks the tree once for 64 rays) -- on the world-space tree, or entering instances as a wave."""
    return {"two_level": gpu.FLAG_TWO_LEVEL_ONLY, "baked": 0, "packet": gpu.FLAG_PACKET_INTERSECT,
            "two_level_packet": gpu.FLAG_TWO_LEVEL_ONLY | gpu.FLAG_PACKET_INTERSECT, "unbaked": gpu.FLAG_NO_BAKED_INSTANCES,
            "unbaked_packet": gpu.FLAG_NO_BAKED_INSTANCES | gpu.FLAG_PACKET_INTERSECT,
            # *parked: the general route into an instance for every instance (rounds 2-4); without it (round 5) the per-ray kernels walk instances that are a
            # translation + uniform scale through entry nodes, the ray taken into the instance's space on the fly
            "two_level_parked": gpu.FLAG_TWO_LEVEL_ONLY | gpu.FLAG_PARKED_INSTANCES, "unbaked_parked": gpu.FLAG_NO_BAKED_INSTANCES | gpu.FLAG_PARKED_INSTANCES,
            # team: four lanes per ray on the world-space tree (pt_team.h: the kernel of launches that do not fill the machine)
            "team": gpu.FLAG_TEAM_INTERSECT}[mode]


def entered(mode):
    return mode.startswith(("two_level", "unbaked"))


def check_kernel_used(ctx, mode, folded=None, general=None):
    assert (ctx.stats()["packet_launches"] > 0) == mode.endswith("packet"), "wrong traversal kernel ran"
    assert (ctx.stats()["team_launches"] > 0) == (mode == "team"), "the team kernel did not run where it should (or ran where it should not)"
    if folded is not None:  # how many instances of the scene the per-ray kernels walk through entry nodes
        assert ctx.stats()["folded_instances"] == folded, (ctx.stats()["folded_instances"], folded)
    if general is not None:  # instances of any transform entered as leaf-kind steps (pt_trace.h, LEVELS 2)
        assert ctx.stats()["general_route"] == (1 if general else 0), (ctx.stats()["general_route"], general)


def zoo_route(kind, mode):
    """(folded_instances, general_route) scenes.transform_zoo(kind) must show in `mode`, by the rules tests/test_convert.py::test_each_instance_route_is_taken_
    where_it_belongs states: copied modes enter nothing; *parked park; entered instances that are all a translation + uniform scale fold (the four blobs, and
    the ground and the light where nothing is copied); one mirrored instance among them (a quarter at most) parks beside the fold; a scene of mirrors, shears
    and non-uniform scales takes the general route."""
    if not entered(mode) or mode.endswith("parked"):
        return 0, 0
    if kind == "general":
        return 0, 1
    return 4 + (2 if mode.startswith("unbaked") else 0), 0


ZOO_LO, ZOO_HI = (-4.0, -1.1, -1.0), (4.0, 3.0, 8.0)  # where scenes.transform_zoo keeps its instances (the eight-fold one reaches beyond)


def zoo_rays(bundle, n, seed, lo=ZOO_LO, hi=ZOO_HI):
    return aimed_rays(bundle.targets, n, seed, lo, hi)


def axis_parallel_rays(flat, n, seed, lo, hi):
    """n rays with one or two exactly-zero direction components (half of them parallel to an axis), origins in [lo, hi], half of them exactly ON a plane of
    a top-level node's box -- one the ray runs in, or one it crosses: where a slab test meets 0 * (1 / 0)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    axis = rng.integers(0, 3, n)
    d[np.arange(n), axis] = 0.0
    second = rng.random(n) < 0.5
    d[np.flatnonzero(second), (axis[second] + 1) % 3] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    planes = [np.unique(np.concatenate([flat.top_nodes[side][:, a] for side in ("min", "max")])) for a in range(3)]
    planes = [p[np.abs(p) < 1e30] for p in planes]  # (not the inverted boxes of unused nodes)
    # Not the plane a flat, TRANSLATED instance lies in (an area light's quad): a ray that starts exactly in a triangle's plane meets it at t = 0 -- no hit, by
    # float64 and by the kernels on a world-space copy.  The reference moves a zero component of the instance-space origin to -FLT_MIN (NO_PARALLEL_RAYS,
    # scene.cl:123-137) and reports a hit there; the kernels apply that nudge to the world-space ray, which is the same thing for an instance that is not
    # translated along that axis (the ground's plane y = 0 stays in) and, for a copy, nothing where it is.  Those rays have a test of their own, which pins
    # exactly that departure: rays_from_the_plane_of, tests/test_gpu_transforms.py::test_rays_that_start_in_the_plane_of_a_translated_copied_quad.
    for leaf, a in flat_translated_leaves(flat):
        planes[a] = planes[a][planes[a] != flat.top_nodes["min"][leaf][a]]
    on = np.flatnonzero(rng.random(n) < 0.5)
    on_axis = (axis[on] + rng.integers(0, 3, len(on))) % 3
    o[on, on_axis] = [rng.choice(planes[a]) for a in on_axis]
    o, d = o.astype(np.float32), d.astype(np.float32)
    assert ((d == 0).sum(1) >= 1).all() and ((d == 0).sum(1) == 2).sum() > 0.3 * n
    return o, d


def flat_translated_leaves(flat):
    """[(top-level leaf, axis)] of the instances that lie IN a plane of their own box (a quad) and are translated along that plane's axis: an area light."""
    out = []
    for leaf in np.flatnonzero(flat.top_nodes["isLeaf"] != 0):
        n = flat.top_nodes[leaf]
        out += [(int(leaf), a) for a in range(3) if n["min"][a] == n["max"][a] and n["invTransform"][12 + a] != 0]
    return out


def rays_from_the_plane_of(flat, leaf, axis, n, seed):
    """n rays whose origins lie EXACTLY in the plane of the flat instance `leaf` (over and around it: 1.5 times its box), a third each leaving the plane
    towards +axis, towards -axis and running in it (that direction component exactly zero); half of each third parallel to a coordinate axis."""
    rng = np.random.default_rng(seed)
    lo, hi = flat.top_nodes["min"][leaf][:3].astype(np.float64), flat.top_nodes["max"][leaf][:3].astype(np.float64)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    o = c + 1.5 * h * rng.uniform(-1, 1, (n, 3))
    o[:, axis] = lo[axis]
    d = rng.normal(size=(n, 3))
    kind = np.arange(n) % 3  # 0: towards +axis, 1: towards -axis, 2: in the plane
    d[:, axis] = np.where(kind == 0, np.abs(d[:, axis]), np.where(kind == 1, -np.abs(d[:, axis]), 0.0))
    parallel = rng.random(n) < 0.5
    other = (axis + 1 + rng.integers(0, 2, n)) % 3
    for k in np.flatnonzero(parallel):
        keep = axis if kind[k] != 2 else other[k]
        d[k, [a for a in range(3) if a != keep]] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = o.astype(np.float32), d.astype(np.float32)
    assert (o[:, axis] == flat.top_nodes["min"][leaf][axis]).all() and (d[kind == 2, axis] == 0).all()
    return o, d, kind


def parse_digest(line):
    """pt_debug_convert's line, 'name value [value]' ... on either side of ' | ' -> {"static": {name: "value [value]"}, "dynamic": {...}} (values are decimal or
    hex numbers)"""
    import re
    out = {}
    for half, part in zip(("static", "dynamic"), line.split(" | ")):
        fields, key = {}, None
        for tok in part.split():
            if re.fullmatch(r"[0-9a-f]+", tok):
                fields[key] = f"{fields[key]} {tok}".strip()
            else:
                key, fields[tok] = tok, ""
        out[half] = fields
    return out


def tri_vertex_ids(flat, prim):
    """Geometric identity of a hit triangle: sorted global vertex indices (SBVH duplicates references)."""
    return np.sort(flat.triangles["indices"][prim], axis=1)


def compare_hits(flat, got, want, t_rtol=2e-4, max_tie_frac=1e-2, edge_flip_frac=0.0, t_outlier_frac=0.0, uv_atol=5e-3, t_atol=1e-6):
    """hit/miss identical; t/u/v within tolerance; (prim, inst) identical except where two primitives are
    hit at the same t within tolerance (shared edges, SBVH-duplicated references): those must agree on t.
    `t_outlier_frac` > 0 (deformed meshes: twisted triangles become slivers, and t of a hit that grazes a sliver is ill-conditioned)
    tolerates that fraction of rays beyond t_rtol, each within 1 %.
    `edge_flip_frac` > 0 (world-space copies of instances: triangle edges are rounded in another space than the
    reference's) tolerates that fraction of hit/miss disagreements, each of which must graze a triangle edge.
    `t_atol`: the absolute error of t scales with the magnitude of the coordinates, not with t (a ray that starts 5e-4 in front of a
    surface 15 units from the origin has t good to a few 1e-6): scenes far larger than the unit cube pass a few ulps of their extent.
    `uv_atol`: barycentrics are compared through the hit point they encode; the direct bound on u and v is loose (they are
    ill-conditioned for small or distant triangles: 5e-3 by default, more for scenes of tiny triangles seen from afar)."""
    gh, wh = got["prim"] >= 0, want["prim"] >= 0
    flips = gh != wh
    edge_flips = 0
    if edge_flip_frac > 0 and flips.any():
        for k in np.flatnonzero(flips):
            h = got if gh[k] else want
            u, v = float(h["u"][k]), float(h["v"][k])
            assert min(abs(u), abs(v), abs(1.0 - u - v)) < 2e-4, f"ray {k}: hit/miss differs away from any edge (u={u}, v={v})"
        edge_flips = int(flips.sum())
        assert flips.mean() <= edge_flip_frac, f"{edge_flips} edge-grazing rays flip"
        flips = np.zeros_like(flips)
    assert flips.mean() <= 1e-4, f"hit/miss differs for {flips.sum()} rays"
    both = gh & wh
    dt = np.abs(got["t"][both] - want["t"][both]) / np.maximum(np.abs(want["t"][both]), 1e-6)
    bad = ~np.isclose(got["t"][both], want["t"][both], rtol=t_rtol, atol=t_atol)
    assert bad.mean() <= t_outlier_frac, f"t differs for {bad.sum()} of {both.sum()} rays, worst {dt.max():.3e}"
    for k in np.flatnonzero(bad):  # a tolerated outlier is within 1 %, or its NEARER hit grazes a triangle edge (the other side missed that
        if dt[k] < 1e-2:           # triangle by round-off and reports what lies behind it)
            continue
        h = got if got["t"][both][k] < want["t"][both][k] else want
        u, v = float(h["u"][both][k]), float(h["v"][both][k])
        assert min(abs(u), abs(v), abs(1.0 - u - v)) < 2e-3, f"t differs by {dt[k]:.2e} away from any edge (u={u}, v={v})"
    same_geom = np.all(tri_vertex_ids(flat, got["prim"][both]) == tri_vertex_ids(flat, want["prim"][both]), axis=1)
    same = same_geom & (got["inst"][both] == want["inst"][both])
    assert (~same).mean() <= max_tie_frac, f"{(~same).sum()} of {both.sum()} rays hit a different primitive"
    # a different primitive is only legitimate as a tie: coincident / edge-sharing triangles hit at the same t
    # (which one is reported depends on the visit order, which is ours -- see pt_trace.h)
    same = same | bad  # (the tolerated t outliers hit what lies behind a gap: another primitive at another distance)
    tie_dt = np.abs(got["t"][both][~same] - want["t"][both][~same]) / np.maximum(want["t"][both][~same], 1e-6)
    assert tie_dt.size == 0 or tie_dt.max() < 2e-5, f"different primitive at a different distance: {tie_dt.max():.2e}"
    # barycentrics: compared through the hit point they encode (object space), v0 + u*e1 + v*e2, because
    # u and v of a grazing hit are ill-conditioned (errors scale with 1/det) while the point is not
    same = same & ~bad
    tri = flat.triangles["indices"][want["prim"][both][same]]
    p0, p1, p2 = (flat.vertices["vertex"][tri[:, k], :3].astype(np.float64) for k in range(3))

    def point(h):
        u, v = h["u"][both][same].astype(np.float64)[:, None], h["v"][both][same].astype(np.float64)[:, None]
        return p0 + u * (p1 - p0) + v * (p2 - p0)
    extent = float(np.abs(flat.vertices["vertex"][:, :3]).max())
    assert np.abs(point(got) - point(want)).max() < 2e-4 * max(extent, 1.0)
    assert np.allclose(got["u"][both][same], want["u"][both][same], atol=uv_atol)
    assert np.allclose(got["v"][both][same], want["v"][both][same], atol=uv_atol)
    return dict(flips=int(flips.sum()), ties=int((~same).sum()), n=int(both.sum()), edge_flips=edge_flips)


def tonemap(accum_rgb, spp, camera):
    """mean -> exposure -> Reinhard, pre-gamma, values in [0,1): the image-parity space of SURVEY 8(d)."""
    ev = np.log2(float(camera["relativeAperture"]) ** 2 / float(camera["shutterTime"]) * 100 / float(camera["ISO"]))
    lum = accum_rgb / spp / (1.2 * 2.0 ** ev)
    return lum / (1 + lum)


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


# ---- parity margins on the record: what every image gate measured, next to the gate (tests/conftest.py writes them out at the end of
# the session: gpurun_out/parity_margins.json on the GPU box, copied to profiles/roundN/ and quoted in DESIGN.md section 2)
MARGINS = {}


def record_margin(name, **values):
    MARGINS[name] = {k: (float(v) if isinstance(v, (int, float, np.floating, np.integer)) else v) for k, v in values.items()}


def image_margins(name, got, want, spp, camera, bias_gate, rmse_gate, **extra):
    """bias of the image mean and tone-mapped RMSE (SURVEY 8(d)'s two statistics) of `got` against the oracle's `want`, recorded and gated"""
    bias = abs(float(got.mean()) - float(want.mean())) / float(want.mean())
    e = rmse(tonemap(got, spp, camera), tonemap(want, spp, camera))
    record_margin(name, bias=bias, bias_gate=bias_gate, tonemapped_rmse=e, rmse_gate=rmse_gate, spp=spp, pixels=int(len(got)), **extra)
    assert bias < bias_gate, (name, bias)
    assert e < rmse_gate, (name, e)
    return bias, e


def fraction_gate(name, close, measured=None, legacy=0.0, slack=0.98):
    """The fraction of entries / pixels that agree with the oracle within a test's tolerances, on the record (parity_margins.json) and gated at what was
    MEASURED, not at a round number (`> 0.85` and `>= 0.97` would have hidden a regression of several percent of a stratum).
    `measured`: {name: fraction} of the test file (the values of the committed profiles/roundN/parity_margins.json); the gate is measured x 0.98 -- the
    kernels and the counter PRNG are deterministic, what moves a fraction between boxes and builds is a handful of fp32 decision flips -- and never
    below the `legacy` gate of rounds 1-5; a name without a measurement is held against `legacy` alone and shows up as such in the record."""
    close = np.asarray(close)
    n = int(close.size)
    frac = float(close.mean()) if n else 1.0
    m = None if measured is None else (measured.get(name) if isinstance(measured, dict) else measured)
    gate = legacy if m is None else max(legacy, m * slack)
    record_margin("fraction: " + name, fraction=frac, n=n, measured=m, gate=gate, legacy_gate=legacy)
    assert frac >= gate, (name, frac, gate)
    return frac


def render_gates(a, ref, st, cnt, spp, cam, pixels, measured, close_frac=0.97, name=""):
    """The gates of a path-by-path render against the oracle's (tests/test_gpu_mis.py, tests/test_gpu_transforms.py): ray counts within 1e-3, the image mean
    within 1e-3, the fraction of pixels within 1e-3 of the oracle's through fraction_gate, tone-mapped RMSE below 5e-3."""
    assert st["rays_generated"] == cnt["raysGenerated"] == pixels * spp
    for k, ck in (("rays_extension", "raysExtension"), ("rays_shadow", "raysShadow"), ("shade_hits", "shadeHits")):
        assert abs(st[k] - cnt[ck]) <= 1e-3 * cnt[ck] + 2, (k, st[k], cnt[ck])
    assert abs(a.mean() - ref.mean()) / ref.mean() < 1e-3
    close = np.isclose(a, ref, rtol=1e-3, atol=1e-3 * ref.max()).all(axis=1)
    fraction_gate(f"{name}: pixels within 1e-3 of the oracle", close, measured, legacy=close_frac)
    assert rmse(tonemap(a, spp, cam), tonemap(ref, spp, cam)) < 5e-3


def assert_hits_of_the_per_ray_kernel(got, want, what=""):
    """What the packet and bundle kernels owe the per-ray kernel: the same triangle and instance and the same t / u / v bits for every ray, except at exact-t
    ties (an SBVH holds a split triangle once per leaf that references it; the traversal order picks the winner): fewer than 1e-3 of the rays, equal in t to 1e-6."""
    same = (got["prim"] == want["prim"]) & (got["inst"] == want["inst"])
    diff = ~same
    assert diff.mean() < 1e-3, (what, int(diff.sum()))
    assert np.allclose(got["t"][diff], want["t"][diff], rtol=1e-6), what
    for k in ("t", "u", "v"):
        assert np.array_equal(got[k][same].view(np.uint32), want[k][same].view(np.uint32)), (what, k)


def status(fn):
    """the status code of a call that must be refused (ptamd.device.PtError), with a message in pt_last_error"""
    with pytest.raises(device.PtError) as e:
        fn()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(e.value), re.S)
    assert m and m.group(2).strip(), "a refusal carries a message in pt_last_error"
    return int(m.group(1))


def read_ppm(path):
    data = open(path, "rb").read()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    w, h = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data[m.end():], np.uint8).reshape(h, w, 3).astype(np.float64)


def mean_abs_laplacian(img):
    return float(np.abs(4 * img[1:-1, 1:-1] - img[:-2, 1:-1] - img[2:, 1:-1] - img[1:-1, :-2] - img[1:-1, 2:]).mean())
