"""The yardstick's own test (no GPU): tests/homography_views_cases.py is what tests/test_gpu_homography_views.py measures the view
synthesis kernels with, so its restatements are held here against independent formulations (grid_sample with zeros padding on
the unpadded source, conv2d over a reflect-padded input) and every mutation has to break its bound.  The host side of the
feature is tested here too: the homography sampler is bit-equal to the reference's (side by side where the checkout is
present, and through tests/golden/homography_views.npz everywhere), and the photometric sampler keeps its promises."""
import os
import sys

import numpy as np
import pytest
import torch

import homography_views_cases as vc
from conftest import load_golden

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the sampler against the reference ----------------------------------------------------------------------------------------
def _ours():
    from glue_factory_amd.data.homography_views import compute_homography, sample_homography_corners
    return vc.run_sampler(sample_homography_corners, compute_homography)


def test_sampler_is_bit_equal_to_the_recorded_reference_results():
    ours, gold = _ours(), load_golden("homography_views")
    assert set(ours) == set(gold) and len(gold) == 6 * len(vc.SAMPLER_SETTINGS)
    for k in gold:
        assert ours[k].dtype == gold[k].dtype and np.array_equal(ours[k], gold[k]), k
    # the settings cover what they claim to
    kws = [s[3] for s in vc.SAMPLER_SETTINGS]
    assert {0.0, 0.7, 0.8} <= {k["difficulty"] for k in kws}
    assert any(k["n_angles"] == 0 for k in kws) and any(k["translation"] == 0 for k in kws)
    assert any(s[1] == (37, 29) for s in vc.SAMPLER_SETTINGS) and any(s[1][0] != s[1][1] for s in vc.SAMPLER_SETTINGS)
    # difficulty 0 is the whole frame rescaled to the patch (640 x 480 -> 320 x 240), which is what right_only shows as view 0
    np.testing.assert_allclose(gold["s2_H0"], np.diag([0.5, 0.5, 1.0]), atol=1e-12)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gluefactory")), reason="reference checkout not present (GPU box)")
def test_sampler_is_bit_equal_to_the_reference_side_by_side():
    stubs = os.path.join(ROOT, "oracle", "stubs")
    added = [p for p in (stubs, REF) if p not in sys.path]
    sys.path[:0] = [stubs]
    sys.path.append(REF)
    try:
        from gluefactory.geometry.homography import compute_homography as ref_compute, sample_homography_corners as ref_sample
        from glue_factory_amd.data.homography_views import compute_homography, sample_homography_corners
        theirs, ours = vc.run_sampler(ref_sample, ref_compute), _ours()
        for k in theirs:
            assert np.array_equal(ours[k], theirs[k]), k
        # and beyond the recorded settings: 60 more seeds over sizes and settings, the generator's next draw included
        for seed in range(100, 160):
            r1, r2 = np.random.RandomState(seed), np.random.RandomState(seed)
            shape = [(1024, 768), (37, 29), (640, 480), (333, 500)][seed % 4]
            kw = dict(difficulty=[0.8, 0.7, 0.0, 0.3][(seed // 4) % 4], translation=[1.0, 0.0][(seed // 16) % 2],
                      n_angles=[10, 0][(seed // 32) % 2], max_angle=60, min_convexity=0.05)
            a = sample_homography_corners(shape, (64, 48), rng=r1, **kw)
            b = ref_sample(shape, (64, 48), rng=r2, **kw)
            assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and r1.uniform() == r2.uniform(), seed
    finally:
        for p in added:
            if p in sys.path:
                sys.path.remove(p)


# ---- the warp restatement -------------------------------------------------------------------------------------------------------
def _warp_case(dtype, C, patch, kind="random"):
    return dict(src=vc.sources(dtype, C, kind), sizes=vc.SIZES, view_src=vc.VIEW_SRC, Hinv=vc.view_matrices(patch),
                params=np.tile(vc.IDENT_PARAMS, (6, 1)), patch=patch)


@pytest.mark.parametrize("dtype,C", [(np.uint8, 1), (np.uint8, 3), (np.float32, 3)])
@pytest.mark.parametrize("patch", vc.PATCHES)
def test_warp_restatement_equals_grid_sample(dtype, C, patch):
    case = _warp_case(dtype, C, patch)
    out, bound = vc.warp_ref(**case, finish=False, gray=False)
    pw, ph = patch
    assert out.shape == (6, C, ph, pw) and np.isfinite(bound).all()
    ys, xs = np.mgrid[0:ph, 0:pw].astype(np.float64)
    for v, s in enumerate(vc.VIEW_SRC):
        w, h = vc.SIZES[s]
        img = torch.from_numpy(case["src"][s, :h, :w].astype(np.float64) / (255.0 if dtype == np.uint8 else 1.0))
        M = case["Hinv"][v].astype(np.float64)
        d = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
        sx, sy = (M[0, 0] * xs + M[0, 1] * ys + M[0, 2]) / d, (M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) / d
        grid = torch.from_numpy(np.stack([2 * sx / (w - 1) - 1, 2 * sy / (h - 1) - 1], -1))[None]
        ref = torch.nn.functional.grid_sample(img.permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="zeros",
                                              align_corners=True)[0].numpy()
        np.testing.assert_allclose(out[v], ref, rtol=0, atol=1e-12)
    # the views see the border (zeros) and the inside, and the bound is a rounding bound, not a tolerance
    assert (out == 0).mean() > 0.05 and (out > 0).mean() > 0.3
    assert np.median(bound[out > 0]) < 1e-4 and bound.max() < 2e-2


def test_warp_restatement_reproduces_ramps_and_the_identity():
    case = _warp_case(np.uint8, 3, vc.PATCHES[0], "ramp")
    out, bound = vc.warp_ref(**case, finish=False, gray=False)
    pw, ph = case["patch"]
    ys, xs = np.mgrid[0:ph, 0:pw].astype(np.float64)
    for v, s in enumerate(vc.VIEW_SRC):
        w, h = vc.SIZES[s]
        M = case["Hinv"][v].astype(np.float64)
        d = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
        sx, sy = (M[0, 0] * xs + M[0, 1] * ys + M[0, 2]) / d, (M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) / d
        inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
        assert inside.sum() > 50
        for c in range(3):
            np.testing.assert_allclose(out[v, c][inside], vc.ramp_value(s, c, sx, sy, np.uint8)[inside], rtol=0, atol=1e-12)
    # view 0 is the identity on source 1 (16 x 50): src / 255 inside, zero outside
    w, h = vc.SIZES[vc.VIEW_SRC[0]]
    want = np.zeros((3, ph, pw))
    want[:, :min(h, ph), :min(w, pw)] = np.moveaxis(case["src"][1, :min(h, ph), :min(w, pw)], -1, 0) / 255.0
    assert np.array_equal(out[0], want)


@pytest.mark.parametrize("mutate", vc.WARP_MUTATIONS)
def test_warp_mutations_break_the_bound(mutate):
    case = _warp_case(np.uint8, 3, vc.PATCHES[2])
    case["params"] = vc.photometric_params()
    out, bound = vc.warp_ref(**case, finish=True, gray=True)
    assert vc.violations(out, out, bound)[0] == 0
    bad, ratio = vc.violations(vc.warp_ref(**case, finish=True, gray=True, mutate=mutate)[0], out, bound)
    print(f"{mutate}: {bad} of {out.size} pixels outside their bound, worst ratio {ratio:.3g}")
    assert bad > 0.02 * out.size and ratio > 100


def test_photometric_stages_of_the_restatement():
    case = _warp_case(np.uint8, 3, vc.PATCHES[0])
    case["params"] = vc.photometric_params()
    plain = vc.warp_ref(**dict(case, params=np.tile(vc.IDENT_PARAMS, (6, 1))), finish=False, gray=False)[0]
    out, bound = vc.warp_ref(**case, finish=True, gray=False)
    p = case["params"].astype(np.float64)
    np.testing.assert_allclose(out[1], plain[1] ** p[1, 0], atol=1e-12)                               # gamma alone
    m = plain[2].max(0, keepdims=True)
    k = np.where(m > 0, np.clip(m + p[2, 1], 0, 1) / np.where(m > 0, m, 1), 1)
    np.testing.assert_allclose(out[2], plain[2] * k, atol=1e-12)                                      # value shift alone
    np.testing.assert_allclose(out[4], np.clip(p[4, 2] * plain[4] + p[4, 3], 0, 1), atol=1e-12)       # a v + b alone
    assert np.isfinite(bound).all() and (out[2][:, plain[2].max(0) == 0] == 0).all()                  # black stays black
    g = vc.warp_ref(**case, finish=True, gray=True)[0]
    np.testing.assert_allclose(g[:, 0], np.tensordot(out, vc.GRAY, axes=[[1], [0]]), atol=1e-12)
    # gray is asked for but finish is not: the channels stay (the filter finishes)
    assert vc.warp_ref(**case, finish=False, gray=True)[0].shape[1] == 3


# ---- the filter restatement -----------------------------------------------------------------------------------------------------
FILTER_KINDS = ["id", ("box", 3), ("box", 9), ("line", 25, "h"), ("line", 25, "v"), ("line", 25, "d"), "full"]


def _filter_case(C, ph, pw, seed=0):
    rng = np.random.RandomState(seed)
    off, wgt, n = vc.tap_tables(FILTER_KINDS)
    V = len(FILTER_KINDS)
    params = np.tile(vc.IDENT_PARAMS, (V, 1))
    params[:, 2] = rng.uniform(0.7, 1.0, V)
    params[:, 3] = rng.uniform(-0.4, 0.0, V)
    return dict(x=rng.uniform(0, 1, (V, C, ph, pw)).astype(np.float32), tap_off=off, tap_w=wgt, ntaps=n, params=params)


@pytest.mark.parametrize("C,ph,pw", [(1, 13, 13), (3, 16, 64), (1, 17, 65), (3, 30, 21)])
def test_filter_restatement_equals_conv2d_over_a_reflect_padded_input(C, ph, pw):
    case = _filter_case(C, ph, pw)
    out, bound = vc.filter_ref(**case, gray=False)
    R = vc.RADIUS
    for v in range(len(FILTER_KINDS)):
        kern = np.zeros((2 * R + 1, 2 * R + 1))
        for t in range(case["ntaps"][v]):
            dx, dy = case["tap_off"][v, t]
            kern[dy + R, dx + R] += float(case["tap_w"][v, t])
        x = torch.from_numpy(case["x"][v].astype(np.float64))[:, None]
        ref = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (R, R, R, R), mode="reflect"), torch.from_numpy(kern)[None, None])
        ref = np.clip(float(case["params"][v, 2]) * ref[:, 0].numpy() + float(case["params"][v, 3]), 0, 1)
        np.testing.assert_allclose(out[v], ref, rtol=0, atol=1e-12)
    assert np.array_equal(vc.filter_ref(**dict(case, params=np.tile(vc.IDENT_PARAMS, (7, 1))), gray=False)[0][0], case["x"][0])
    assert bound.max() < 1e-5 and int(case["ntaps"].max()) == vc.MAXTAPS


@pytest.mark.parametrize("mutate", vc.FILTER_MUTATIONS)
def test_filter_mutations_break_the_bound(mutate):
    case = _filter_case(3, 30, 21)
    out, bound = vc.filter_ref(**case, gray=True)
    assert out.shape == (7, 1, 30, 21) and vc.violations(out, out, bound)[0] == 0
    bad, ratio = vc.violations(vc.filter_ref(**case, gray=True, mutate=mutate)[0], out, bound)
    print(f"{mutate}: {bad} of {out.size} pixels outside their bound, worst ratio {ratio:.3g}")
    assert bad > 0.02 * out.size and ratio > 100


# ---- the photometric sampler ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lg", "dark", "identity"])
def test_photometric_presets(name):
    from glue_factory_amd.data import homography_views as hv
    draws = [hv.sample_photometric(name, None, np.random.RandomState(7), gray=True) for _ in range(2)]
    assert np.array_equal(draws[0][0], draws[1][0]) and np.array_equal(draws[0][1][0], draws[1][1][0])   # seeded
    rng = np.random.RandomState(11)
    seen = {"gamma": 0, "vshift": 0, "bc": 0, "blur": 0}
    for _ in range(3000):
        par, (off, wgt) = hv.sample_photometric(name, None, rng, gray=False)
        assert par.dtype == np.float32 and par.shape == (4,) and off.dtype == np.int32 and wgt.dtype == np.float32
        g, s, a, b = par.tolist()
        assert g == 1 or 0.15 <= g <= 0.65 + 1e-6
        assert s == 0 or -100 / 255 - 1e-6 <= s <= -40 / 255 + 1e-6
        assert 0.7 - 1e-6 <= a <= 1 and -0.4 - 1e-6 <= b <= 0
        assert 1 <= len(wgt) <= hv.MAXTAPS and off.shape == (len(wgt), 2) and np.abs(off).max() <= hv.RADIUS
        assert abs(float(wgt.astype(np.float64).sum()) - 1) < 1e-5 and len({tuple(o) for o in off.tolist()}) == len(wgt)
        seen["gamma"] += g != 1
        seen["vshift"] += s != 0
        seen["bc"] += a != 1
        seen["blur"] += len(wgt) > 1
    if name == "identity":
        assert not any(seen.values()) and hv.preset_blurs(name) is False
    else:
        assert all(seen.values()), seen
        assert hv.preset_blurs(name) is True
    if name == "lg":      # 0.95 x the preset's own probabilities, three-sigma bands of 3000 draws
        assert abs(seen["gamma"] / 3000 - 0.095) < 0.02 and abs(seen["bc"] / 3000 - 0.475) < 0.03
        assert abs(seen["blur"] / 3000 - 0.95 * (1 - 0.95 * 0.9 * 0.9)) < 0.03
    with pytest.raises(ValueError):
        hv.sample_photometric("nope", None, rng)


def test_tap_tables_and_table_checks():
    from glue_factory_amd.data import homography_views as hv
    off, wgt = hv.box_taps(9)
    assert len(wgt) == 81 and set(map(tuple, off.tolist())) == {(dx, dy) for dx in range(-4, 5) for dy in range(-4, 5)}
    for angle, want in ((0.0, (1, 0)), (np.pi / 2, (0, 1)), (np.pi / 4, (1, 1))):
        off, wgt = hv.line_taps(25, angle)
        assert len(wgt) == 25 and set(map(tuple, off.tolist())) == {(i * want[0], i * want[1]) for i in range(-12, 13)}
    views = hv.HomographyViews({"photometric": {"name": "lg", "p": 0.95}, "homography": {"patch_shape": [64, 48]}, "seed": 3})
    t = views.tables([(100, 80), (90, 120)])
    again = hv.HomographyViews({"photometric": {"name": "lg", "p": 0.95}, "homography": {"patch_shape": [64, 48]}, "seed": 3})
    t2 = again.tables([(100, 80), (90, 120)])
    assert np.array_equal(t["int"], t2["int"]) and np.array_equal(t["float"], t2["float"])
    assert not np.array_equal(t["float"], again.tables([(100, 80), (90, 120)])["float"])      # the generator moved on
    ok = dict(view_src=np.array([0, 1]), src_sizes=np.array([[5, 5], [4, 6]]), ntaps=np.array([1, 81]),
              tap_off=np.zeros((2, 81, 2), np.int32), n_sources=2, padded=(5, 6))
    hv.check_tables(**ok)
    for bad in (dict(view_src=np.array([0, 2])), dict(view_src=np.array([-1, 0])), dict(ntaps=np.array([0, 1])),
                dict(ntaps=np.array([1, 82])), dict(src_sizes=np.array([[6, 5], [4, 6]])),
                dict(tap_off=np.full((2, 81, 2), 13, np.int32))):
        with pytest.raises(ValueError):
            hv.check_tables(**dict(ok, **bad))


def test_ops_refuse_cpu_tensors():
    from glue_factory_amd import ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.warp_views(torch.zeros(1, 4, 4, 1, dtype=torch.uint8), torch.zeros(1, 2, dtype=torch.int32),
                       torch.zeros(1, dtype=torch.int32), torch.eye(3)[None], torch.zeros(1, 4), (4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.filter_views(torch.zeros(1, 1, 16, 16), torch.zeros(1, 81, 2, dtype=torch.int32), torch.zeros(1, 81),
                         torch.ones(1, dtype=torch.int32), torch.zeros(1, 4))
