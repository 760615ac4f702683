"""The firefly clamp as tests/firefly_ref.py restates it (include/ptamd.h, "firefly clamp"), without a GPU: the properties any implementation of the
contract has, what the planted cases hold, and the scan over five oracle-rendered rooms that chooses PT_FIREFLY_DEFAULT_RANK / _SCALE."""
import numpy as np
import pytest

import denoise_ref as R
import firefly_ref as F
import firefly_scan as S

BIG = [(n, kw, prm) for (n, kw, prm) in F.CASES if (kw["width"], kw["height"]) not in F.SMALL]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("name,kw,prm", F.CASES, ids=[n for n, _, _ in F.CASES])
def test_what_any_implementation_has(name, kw, prm, dtype):
    """an unclamped pixel keeps its input bits and s == 1; L(d_out) <= Cap up to rounding; every output is finite; a non-finite pixel is (0, 0, 0, 0);
    n_q < rank leaves the pixel alone; the counters count what the plane shows"""
    case = F.make_case(**kw)
    out = F.run_case(case, dtype, **prm)
    plane, finite, clamped = out["plane"], out["finite"], out["clamped"]
    assert plane.dtype == dtype and np.isfinite(plane).all()
    same = finite & ~clamped
    assert np.array_equal(bits(plane[..., :3][same]), bits(out["d"][same])) and np.all(plane[..., 3][same] == 1)
    assert not plane[~finite].any()
    eps = np.finfo(dtype).eps
    assert np.all(R.luminance(plane[..., :3])[clamped] <= out["cap"][clamped] * (1 + 8 * eps))
    assert np.all(plane[..., 3][clamped] < 1) and np.all(plane[..., 3][clamped] > 0)
    rank = prm.get("rank", F.RANK)
    assert not clamped[out["n_q"] < rank].any() and np.all(np.isinf(out["cap"][out["n_q"] < rank]))
    assert out["counts"] == (int((finite & (plane[..., 3] < 1)).sum()), int((~finite).sum()))
    planted = case["planted"]
    assert out["counts"][1] == len(planted.get("nan", [])) + len(planted.get("inf", []))


@pytest.mark.parametrize("name,kw,prm", [c for c in BIG if c[2]], ids=[n for n, _, p in BIG if p])
def test_enough_pixels_clamp_and_few_sit_on_the_cap(name, kw, prm):
    """at (rank 3, scale 2) on every case but the three small ones: at least 8 pixels clamped, at least half unclamped, at most 2 within 1e-4 of their
    cap, and float32 counts what float64 counts give or take those.  Measured: 12 of 256 at 16 x 16, 79 of 3 150 at 70 x 45, 308 of 12 450 at
    150 x 83, float32 and float64 equal on every count, no pixel near its cap."""
    case = F.make_case(**kw)
    r64, r32 = F.run_case(case, np.float64, **prm), F.run_case(case, np.float32, **prm)
    near = F.near(case, r64, **prm)
    print(f"{name}: clamped {r64['counts'][0]} (float32 {r32['counts'][0]}) of {kw['width'] * kw['height']}, near {len(near)}")
    assert r64["counts"][0] >= 8 and r64["counts"][0] <= kw["width"] * kw["height"] // 2
    assert len(near) <= 2
    assert abs(r32["counts"][0] - r64["counts"][0]) <= len(near) and r32["counts"][1] == r64["counts"][1]
    assert np.array_equal(r32["clamped"].ravel()[np.setdiff1d(np.arange(r64["clamped"].size), near)],
                          r64["clamped"].ravel()[np.setdiff1d(np.arange(r64["clamped"].size), near)])


@pytest.mark.parametrize("size", [(16, 16), (70, 45)], ids=["16x16", "70x45"])
def test_the_planted_features(size):
    """the 3-pixel bar passes with s == 1 at rank <= 2 whatever the scale; both adjacent spikes are clamped at rank 2 and neither at rank 1 (each is the
    other's largest neighbour); the corner and the edge spike are clamped at either rank; the zeros stay zeros"""
    case = F.make_case(*size)
    planted = case["planted"]
    idx = lambda name: tuple(np.asarray(planted[name]).T)
    for rank in (1, 2):
        for scale in (1.0, 2.0, 8.0):
            out = F.run_case(case, rank=rank, scale=scale)
            s = out["plane"][..., 3]
            assert np.all(s[idx("bar")] == 1), (rank, scale)
            if scale > 1.0:
                assert np.all(s[idx("pair")] < 1) == (rank == 2) and np.all(s[idx("pair")] == 1) == (rank == 1)
            assert np.all(s[idx("corner")] < 1) and np.all(s[idx("edge")] < 1)
            assert not out["plane"][..., :3][idx("zeros")].any() and np.all(s[idx("zeros")] == 1)
    for rank in (3, 4):  # a bar 3 wide has pixels with five neighbours like them along it: it survives these ranks too, the pair does not
        s = F.run_case(case, rank=rank, scale=2.0)["plane"][..., 3]
        assert np.all(s[idx("bar")] == 1) and np.all(s[idx("pair")] < 1)


def test_too_few_neighbours_leave_the_pixel_alone():
    """1 x 1: no neighbour, 2 x 1: one -- the 1e4 spike in the corner passes at rank 2 and is clamped at rank 1; 5 x 3 has 14 neighbours at most"""
    for (w, h), rank, expect in (((1, 1), 1, 0), ((1, 1), 2, 0), ((2, 1), 2, 0), ((2, 1), 1, 1), ((5, 3), 4, None)):
        case = F.make_case(w, h)
        out = F.run_case(case, rank=rank, scale=2.0)
        assert out["n_q"].max() <= min(w * h - 1, 24)
        if expect is not None:
            assert out["counts"] == (expect, 0), ((w, h), rank)
            assert (out["plane"][0, 0, 3] < 1) == bool(expect)


def test_the_smooth_case_clamps_nothing():
    for (w, h) in ((16, 16), (70, 45)):
        for prm in F.PARAMS + [dict(rank=4, scale=1.5)]:
            assert F.run_case(F.make_smooth_case(w, h), np.float32, **prm)["counts"] == (0, 0)


def test_the_fed_accumulator_is_the_plane():
    """accumulate_case feeds temporal_ref the plane as an accumulator over an albedo of 1: a first frame's colour_count is (d_out, 1), bit for bit"""
    case = F.make_case(70, 45)
    for dtype in (np.float32, np.float64):
        cn = F.accumulate_case(case, dtype, history=False)[0]
        plane = F.run_case(case, dtype)["plane"]
        assert np.array_equal(bits(cn[..., :3]), bits(plane[..., :3])) and np.all(cn[..., 3] == 1)
    assert not np.isfinite(F.accumulate_case(case, np.float64, clamp=False)[0]).all()  # the NaN and the Inf go through without the clamp
    assert np.isfinite(F.accumulate_case(case, np.float64)[0]).all()


# ---------------------------------------------------------------- the scan
@pytest.fixture(scope="module")
def scanned():
    return S.scan()


def test_the_defaults_are_the_scans_choice(scanned):
    """Five rooms x {1, 4} spp x two sample bases x rank 1 .. 4 x scale {1.5, 2, 3, 4, 8}: the defaults are the pair with the smallest worst-case on / off
    ratio among the pairs whose ratio is <= 1.00 on every run, or, if none qualifies, the pair with the smallest worst case.
    Measured: NONE qualifies.  zoo_room at 4 spp, base 1000, is a frame without a firefly, and every pair dims the small light it sees directly: the
    worst ratios run from 1.37 (rank 1, scale 8) to 3.07 (rank 4, scale 1.5); (2, 2) has 2.16.  Without that one run (1, 8), (1, 4), (1, 3), (1, 2),
    (2, 3), (2, 4) and (2, 8) all stay below 1.005.  The choice is (1, 8): worst 1.370, mirror_blob_room 1 spp 0.688 / 0.732, 4 spp 0.909 / 0.893,
    zoo_room 1 spp 0.872 / 0.861, the three Cornell rooms 0.949 .. 1.000."""
    for pair in S.PAIRS:
        print(pair, f"worst {S.worst_ratio(scanned, pair):.3f}", " ".join(f"{run['on'][pair] / run['off']:.3f}" for run in scanned.values()))
    for key, run in scanned.items():
        print(key, f"off {run['off']:.3e}, defaults: ratio {run['on'][(F.RANK, F.SCALE)] / run['off']:.3f}, unfiltered {run['unfiltered'][(F.RANK, F.SCALE)]:.3f}, "
                   f"luminance kept {run['kept'][(F.RANK, F.SCALE)]:.3f}")
    chosen, qualifies = S.choose(scanned)
    print(f"chosen {chosen}, qualifies {qualifies}, worst {S.worst_ratio(scanned, chosen):.3f}")
    assert chosen == (F.RANK, F.SCALE)
    assert not qualifies  # (the day a pair qualifies the docstring above, DESIGN.md section 9 and EXPERIMENTS.md are out of date)


def test_the_clamp_gains_where_paths_are_specular(scanned):
    """what the defaults buy: mirror_blob_room at 1 spp pooled over its bases, r_cpu -- the figure tests/test_gpu_firefly.py's end-to-end gate is
    built on --, and no more than 0.2 % lost on any run of the purely diffuse room"""
    pair = (F.RANK, F.SCALE)
    r_cpu = S.pooled(scanned, "mirror_blob_room", 1, pair)
    print(f"r_cpu = {r_cpu:.4f} (firefly_ref.R_CPU {F.R_CPU})")
    assert abs(r_cpu - F.R_CPU) <= 0.01
    assert r_cpu < 0.8
    for (room, spp, base), run in scanned.items():
        if room == "cornell_box":
            assert run["on"][pair] <= 1.002 * run["off"], (spp, base)
            assert run["kept"][pair] >= 0.98
