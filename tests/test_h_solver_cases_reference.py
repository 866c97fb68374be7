"""The yardstick's own test (no GPU): tests/h_solver_cases.py is what tests/test_gpu_h_solver.py measures the homography
kernels with, so its restatements, scenes and bounds are checked here -- every mutation must break its bound, every
planted scene must be solvable under the stated seed with nothing inside a decision band, the derived threshold band must
cover a numpy fp32 run of the same formulas, and the two evaluation metrics must agree with the reference's own functions
(side by side where the reference checkout is present, and through tests/golden/homography_eval.npz everywhere)."""
import os
import sys

import numpy as np
import pytest
import torch

import h_solver_cases as hc
from conftest import load_golden

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- sampling (the distinctness test and its mutation: tests/test_ransac_cases.py, for both sample sizes) -------------------
def test_small_k_uniformity():
    """Every index of K = 5 is drawn, in every position (a skip mapping that never reaches the last index would not)."""
    s = hc.samples(3, 0, 2000, 5)
    for d in range(4):
        assert set(s[:, d].tolist()) == set(range(5))


# ---- fit -------------------------------------------------------------------------------------------------------------------
def test_fit_reproduces_a_known_homography_and_rejects_degenerate_samples():
    p0 = np.array([[10.0, 20], [200, 30], [220, 210], [15, 180]])
    c = np.concatenate([p0, hc.warp(hc.H_PROJ, p0)], -1)[None]
    fit = hc.fit4(c)
    assert fit["ok"][0] and not fit["band"][0]
    np.testing.assert_allclose(fit["H"][0], hc.H_PROJ, rtol=1e-9, atol=1e-9)
    collinear = c.copy()
    collinear[0, 2, :2] = (c[0, 0, :2] + c[0, 1, :2]) / 2                      # source point 3 on the segment 1-2
    assert not hc.fit4(collinear)["ok"][0]
    flipped = c.copy()
    flipped[0, :, 2] = 700 - flipped[0, :, 2]                                  # mirrored target: every orientation flips
    assert not hc.fit4(flipped)["ok"][0]
    nan = c.copy()
    nan[0, 3, 3] = np.nan
    assert not hc.fit4(nan)["ok"][0]


# ---- scenes and bands --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,K,M,N", hc.PLANTED)
def test_planted_scenes_are_clean_and_the_band_covers_fp32(model, K, M, N):
    for pair in (0, 2):                                   # the pair indices the GPU tests place the scene at
        scene = hc.planted_scene(model, K, M, N, pair)
        ok, res = hc.scene_is_clean(scene, pair, 2 * hc.HYPS + 5)
        assert ok and M != N
        fit, corr = res["fit"], res["corr"]
        # an all-inlier sample that is neither rejected nor near a decision exists: the GPU tests do not rest on luck
        good = scene["planted"][res["idx"]][res["samples"]].all(-1) & fit["ok"] & ~fit["band"]
        assert good.any()
        assert int(res["num"]) == int(scene["planted"].sum()) == (K + 1) // 2
        # outliers are displaced by at least 50 px, or by MEDIUM px exactly
        err, _ = hc.transfer(scene["H"], corr)
        out = ~scene["planted"][res["idx"]]
        assert ((err[out] >= 50) | (np.abs(err[out] - hc.MEDIUM) < 1e-3)).all() and (err[~out] < 1e-3).all()
        # the reference alone: numpy fp32 against fp64 -- no rejection differs, every count inside the band
        f32 = hc.fit4(corr[res["samples"]], np.float32)
        differ = f32["ok"] != fit["ok"]
        assert int(differ.sum()) == 0, f"{int(differ.sum())} rejections differ between fp32 and fp64 on the host"
        dl = hc.delta(fit, scene["range"])
        lo, hi = hc.count_band(fit["H"], corr, dl, coord_range=scene["range"])
        c32 = hc.inlier_mask(f32["H"], corr.astype(np.float32), dtype=np.float32).sum(-1)
        both = fit["ok"]
        assert ((c32 >= lo) & (c32 <= hi))[both].all()
        # ... and the band means something: most hypotheses are pinned to within a few counts
        assert np.median((hi - lo)[both]) <= 2 and np.median(dl[both]) < 0.5


def test_backward_error_mutation_is_caught():
    model, K, M, N = hc.PLANTED[0]
    scene = hc.planted_scene(model, K, M, N, 0)
    res = hc.host_ransac(scene["kpts0"], scene["kpts1"], scene["matches0"], 0, 2 * hc.HYPS + 5, backward=True)
    assert (res["inliers"] != scene["planted"]).any()
    assert res["num"] > int(scene["planted"].sum())           # the medium correspondences came in


def test_dlt_mutations_break_the_corner_bound():
    p0, p1, w = hc.dlt_case("weighted")
    H = hc.dlt(p0, p1, w)
    bound = hc.corner_bound(p0, p1, w)
    print(f"weighted case: bound {bound:.3e} px; weights ignored moves the corners by "
          f"{hc.corner_error(hc.dlt(p0, p1, w, use_weights=False), H):.3e} px")
    assert bound < 1e-2
    assert hc.corner_error(hc.dlt(p0, p1, w, use_weights=False), H) > 10 * bound          # weights ignored
    assert hc.corner_error(hc.dlt(p0, p1, w, transposed=True), H) > 10 * bound            # a transposed H
    assert hc.corner_error(hc.dlt(p0, p1, w, denormalise=False), H) > 10 * bound          # no de-normalisation
    # the restatement is a DLT: exact on exact data, and the weighted answer is closer to the truth than the unweighted
    q0, q1, _ = hc.dlt_case("clean")
    assert hc.corner_error(hc.dlt(q0, q1), hc.H_PROJ) < hc.corner_bound(q0, q1)
    assert hc.corner_error(H, hc.H_PROJ) < hc.corner_error(hc.dlt(p0, p1, w, use_weights=False), hc.H_PROJ)
    assert hc.dlt(p0[:3], p1[:3]) is None


@pytest.mark.parametrize("model,K,M,N", hc.PLANTED)
def test_planted_truth_bound_holds_for_the_restatement(model, K, M, N):
    scene = hc.planted_scene(model, K, M, N, 0)
    res = scene["host"]
    inl = scene["planted"][res["idx"]]
    bound = hc.planted_bound(model, K, M, N)
    reached = hc.corner_error(res["H"], scene["H"])
    print(f"{model} K={K}: restatement reaches {reached:.3e} px, bound {bound:.3e} px")
    assert reached < bound < 0.05
    assert int(inl.sum()) == res["num"]


# ---- the evaluation metrics against the reference ---------------------------------------------------------------------------
def _ours():
    from glue_factory_amd.metrics import homography_corner_error, sym_homography_error
    z = {k: torch.from_numpy(v) for k, v in hc.eval_inputs().items()}
    sym = sym_homography_error(z["kpts0"], z["kpts1"], z["H_gt"])
    corner = homography_corner_error(z["T"], z["H_gt"], z["image_size"])
    one = sym_homography_error(z["kpts0"][1], z["kpts1"][1], z["H_gt"][1])             # one pair, no batch axis
    assert torch.equal(one, sym[1])
    assert torch.equal(homography_corner_error(z["T"][2], z["H_gt"][2], z["image_size"][2]), corner[2])
    return z, sym, corner


def test_metrics_equal_the_recorded_reference_results():
    _, sym, corner = _ours()
    gold = load_golden("homography_eval")
    # the fixture is the reference's fp64 evaluation of the fp32 inputs (see tools/gen_homography_eval_golden.py); ours runs in
    # fp32: a few ulps of the 1000 px coordinate range (2^-24 * 1000 = 6e-5 px per operation)
    torch.testing.assert_close(sym.double(), torch.from_numpy(gold["sym_error"]), rtol=1e-5, atol=3e-4)
    torch.testing.assert_close(corner.double(), torch.from_numpy(gold["corner_error"]), rtol=1e-5, atol=3e-4)
    # the restatement in the cases module says the same in fp64
    z = hc.eval_inputs()
    for i in range(3):
        np.testing.assert_allclose(hc.sym_error(z["kpts0"][i], z["kpts1"][i], z["H_gt"][i]), gold["sym_error"][i], rtol=1e-4, atol=1e-3)
        assert abs(hc.corner_error(z["T"][i], z["H_gt"][i], tuple(z["image_size"][i])) - gold["corner_error"][i]) < 1e-3


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gluefactory")), reason="reference checkout not present (GPU box)")
def test_metrics_equal_the_reference_side_by_side():
    stubs = os.path.join(ROOT, "oracle", "stubs")
    added = [p for p in (stubs, REF) if p not in sys.path]
    sys.path[:0] = [stubs]
    sys.path.append(REF)
    try:
        from gluefactory.geometry.homography import homography_corner_error as ref_corner, sym_homography_error as ref_sym
        z, sym, corner = _ours()
        d = {k: v.double() for k, v in z.items()}        # the reference in fp64: its fp32 pinverse alone is 0.02 px off
        for i in range(3):
            torch.testing.assert_close(sym[i].double(), ref_sym(d["kpts0"][i], d["kpts1"][i], d["H_gt"][i]), rtol=1e-5, atol=3e-4)
            torch.testing.assert_close(corner[i].double(), ref_corner(d["T"][i], d["H_gt"][i], d["image_size"][i]),
                                       rtol=1e-5, atol=3e-4)
            # and in fp32 it stays within its own fp32 error of ours
            torch.testing.assert_close(sym[i], ref_sym(z["kpts0"][i], z["kpts1"][i], z["H_gt"][i]), rtol=0, atol=0.05)
    finally:
        for p in added:
            if p in sys.path:
                sys.path.remove(p)
