"""The yardstick of the point-and-line homography solver tested on its own (tests/hl_solver_cases.py; no GPU): the fp64
restatement recovers every planted scene, a numpy fp64 run of the kernel's own elimination stays inside the derived residual
bound, every listed mutation is caught by the checks tests/test_gpu_hl_solver.py applies to the kernels, the header constants
parse, and the host logic of the estimator and of the metrics works on empty and tiny inputs."""
import numpy as np
import pytest
import torch

import hl_solver_cases as hl

NAMES = list(hl.PLANTED)


# ---- constants and the index mapping -----------------------------------------------------------------------------------------
def test_header_constants_parse():
    c = hl.header_constants()
    assert c["TILE"] >= 64 and c["HYPS"] == 256 and c["JACOBI"] >= 8
    assert 0 < c["EPS_LEN"] <= 4 and 0 < c["EPS_PIVOT"] < 1e-4 and 0 < c["H22_FRAC"] < 1e-2


def test_compaction_and_index_mapping():
    scene = hl.build_scene("proj", 5, 6, 9, 8, 10, 9, seed=3)
    lm = scene["line_matches0"]
    matched = np.nonzero(lm >= 0)[0]
    scene["lines0"][matched[0], 1] = scene["lines0"][matched[0], 0] + np.float32(0.5)          # shorter than EPS_LEN in view 0
    scene["lines1"][lm[matched[1]], 0, 0] = np.nan                                             # non-finite in view 1
    lm[np.nonzero(lm < 0)[0][0]] = 99                                                          # out of range
    ft = hl.features(scene)
    assert ft["Kp"] == 5 and ft["Kl"] == 4 and list(ft["lidx"]) == list(matched[2:])
    assert np.array_equal(ft["idx"], np.nonzero(scene["matches0"] >= 0)[0])
    assert ft["feat"].shape == (9, 8) and list(ft["isline"]) == [False] * 5 + [True] * 4
    k = ft["lidx"][0]
    assert np.array_equal(ft["feat"][5], np.concatenate([scene["lines0"][k].ravel(), scene["lines1"][lm[k]].ravel()]))
    assert np.array_equal(ft["feat"][4, [0, 1, 4, 5]], ft["corr"][4]) and np.array_equal(ft["feat"][4, :2], ft["feat"][4, 2:4])
    smp = hl.samples(hl.SEED, 0, 64, 9)
    feat, isline = hl.take(ft, smp)
    assert np.array_equal(isline, smp >= 5) and np.array_equal(feat[isline], ft["seg"][smp[isline] - 5])
    assert (hl.samples(hl.SEED, 0, 8, 3) == -1).all()


# ---- the fit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_restatement_recovers_the_planted_scene(name):
    scene = hl.planted_scene(name)
    res = scene["host"]
    assert res["success"] and np.array_equal(res["inliers"], scene["planted"])
    assert np.array_equal(res["line_inliers"], scene["line_planted"])
    assert res["num"] == (int(scene["planted"].sum()), int(scene["line_planted"].sum()))
    err, bound = hl.corner_error(res["H"], scene["H"]), hl.planted_bound(name)
    print(f"{name}: corner error of the restatement {err:.3e} px, first-order bound {bound:.3e} px")
    assert err < bound
    assert res["fit"]["band"].sum() <= hl.BAND_CAP * hl.T_FULL
    ok, _ = hl.scene_is_clean(scene, 0, hl.T_FULL)
    assert ok
    # 50 % outliers in both lists, at least 50 px away
    ft = res["ft"]
    pe = hl.point_errors(scene["H"], ft["corr"])[0]
    le = [hl.line_errors(scene["H"], ft["seg"], one_endpoint=True)[0],
          hl.line_errors(scene["H"], np.concatenate([ft["seg"][:, 2:4], ft["seg"][:, :2], ft["seg"][:, 4:]], -1), one_endpoint=True)[0]]
    pin, lin = scene["planted"][ft["idx"]], scene["line_planted"][ft["lidx"]]
    assert (pe[pin] < 1e-3).all() and (pe[~pin] >= 50 - 0.25).all()
    assert (np.maximum(*le)[lin] < 1e-3).all() and (np.minimum(*le)[~lin] >= 50 - 1e-3).all()
    if name != "lines_needed":
        assert pin.sum() == (len(pin) + 1) // 2 and lin.sum() == (len(lin) + 1) // 2
    if lin.any():                  # the endpoints of an inlier segment do not correspond: only the lines do
        moved = np.hypot(*(hl.warp(scene["H"], ft["seg"][lin, :2]) - ft["seg"][lin, 4:6]).T)
        assert np.median(moved) > 2.0


@pytest.mark.parametrize("name", NAMES)
def test_fp64_elimination_stays_inside_the_residual_bound(name):
    """The kernel's algorithm (hl.fit_gj: Gauss-Jordan with full pivoting in numpy fp64, the chosen arithmetic), its nine
    entries rounded to fp32 as the kernel's are, against hl.fit_bound; and against the SVD restatement."""
    res = hl.planted_scene(name)["host"]
    feat, isline, fr = res["feat"], res["isline"], res["fit"]
    gj = hl.fit_gj(feat, isline)
    assert np.array_equal(gj["ok"][~fr["band"]], fr["ok"][~fr["band"]])
    both = gj["ok"] & fr["ok"]
    assert both.sum() > 50
    H32 = gj["H"][both].astype(np.float32).astype(np.float64)
    resid = hl.sample_residual(H32, feat[both], isline[both])
    bound = hl.fit_bound({k: v[both] for k, v in gj.items()}, feat[both], hl.planted_scene(name)["range"])
    print(f"{name}: {int(both.sum())} accepted fits, worst residual / bound {np.max(resid / bound):.3f}, "
          f"median bound {np.median(bound):.2e} px, worst cond {fr['cond'][both].max():.2e}")
    assert (resid <= bound).all()
    # the two ways to the null vector agree to the first term of the bound alone
    diff = np.abs(gj["H"][both] - fr["H"][both]).max((-1, -2)) / np.abs(fr["H"][both]).max((-1, -2))
    assert (diff <= hl.FIT_FACTOR * hl.U64 * fr["cond"][both]).all()


def test_two_points_with_two_lines_is_degenerate():
    """What csrc/hl_fit.h says of such a sample: its null vector is the rank-one c n^T, whatever the data."""
    res = hl.planted_scene("mixed")["host"]
    two = res["isline"].sum(-1) == 2
    assert two.sum() > 100 and not res["fit"]["ok"][two].any() and not res["fit"]["band"][two].any()
    A, _, _ = hl.design(res["feat"][two], res["isline"][two])
    G = np.linalg.svd(A, full_matrices=True)[2][:, -1].reshape(-1, 3, 3)
    s = np.linalg.svd(G, compute_uv=False)
    assert (s[:, 1] <= 1e-6 * s[:, 0]).all()


# ---- the mutations ---------------------------------------------------------------------------------------------------------------
def _gpu_checks(scene, pair, T, hyp_H, hyp_counts):
    """The hypothesis checks of tests/test_gpu_hl_solver.py on (hyp_H, hyp_counts) as a kernel would return them: the
    number of accepted hypotheses whose residual on their own sample exceeds the bound, and whose counts leave the band."""
    ft = hl.features(scene)
    feat, isline = hl.take(ft, hl.samples(hl.SEED, pair, T, ft["Kp"] + ft["Kl"]))
    fr = hl.fit(feat, isline)
    acc = (hyp_counts[:, 0] >= 0) & fr["ok"]
    H = hyp_H.astype(np.float32).astype(np.float64)
    resid = hl.sample_residual(H[acc], feat[acc], isline[acc])
    bound = hl.fit_bound({k: v[acc] for k, v in fr.items()}, feat[acc], scene["range"])
    lo, hi = hl.count_band(H[acc], ft)
    cnt = hyp_counts[acc]
    return int((~(resid <= bound)).sum()), int(((cnt < lo) | (cnt > hi)).any(-1).sum())


def _as_kernel(res):
    ok = res["fit"]["ok"]
    return np.where(ok[:, None, None], res["fit"]["H"], 0.0), res["counts"]


@pytest.mark.parametrize("name", ["mixed", "lines_needed", "lines"])
def test_the_restatement_passes_its_own_checks(name):
    scene = hl.planted_scene(name)
    assert _gpu_checks(scene, 0, hl.T_FULL, *_as_kernel(scene["host"])) == (0, 0)


@pytest.mark.parametrize("mutation", ["swap_views", "kp_off_by_one", "ignore_lines", "raw_normal", "one_endpoint"])
def test_every_mutation_is_caught(mutation):
    """Line rows built from the view-0 line and the view-1 endpoints, and the K_p boundary of the index mapping off by one:
    the residual bound.  A score that ignores lines, an unnormalised line normal, the line rule on one endpoint only: the
    count band.  (Samples of one kind alone still find the planted model under every one of these, so the planted truth alone
    would not see them: the hypothesis checks are what catches them.)"""
    scene = hl.planted_scene("mixed")
    kw = {"fit_mutation": "swap_views"} if mutation == "swap_views" else {mutation: True}
    bad = hl.host_ransac(scene, 0, hl.T_FULL, **kw)
    n_resid, n_count = _gpu_checks(scene, 0, hl.T_FULL, *_as_kernel(bad))
    print(f"{mutation}: {n_resid} residuals over the bound, {n_count} count pairs outside the band")
    if mutation in ("swap_views", "kp_off_by_one"):
        assert n_resid > 10
    else:
        assert n_count > 10


def test_the_lines_needed_scene_needs_its_lines():
    """3 point inliers among 6 point matches: the points alone cannot give the homography (hc.host_ransac on them finds at
    most a model through four matches of which one is an outlier); with the 40 line inliers the restatement recovers it."""
    import h_solver_cases as hc
    scene = hl.planted_scene("lines_needed")
    pts = hc.host_ransac(scene["kpts0"], scene["kpts1"], scene["matches0"], 0, hl.T_FULL, th=hl.TH)
    assert not (pts["success"] and hc.corner_error(pts["H"], scene["H"]) < 1.0)
    assert scene["host"]["num"] == (3, 40)


# ---- host logic of the estimator and the metrics ---------------------------------------------------------------------------------
def test_estimator_on_empty_and_tiny_inputs():
    from glue_factory_amd.base_model import get_model
    from glue_factory_amd.solvers.point_line_homography_ransac import (PointLineHomographyEstimator, PointLineHomographyRansac,
                                                                       _line_inputs, point_line_homography_ransac)
    assert get_model("solvers.point_line_homography_ransac") is PointLineHomographyRansac
    assert get_model("glue_factory_amd.solvers.point_line_homography_ransac") is PointLineHomographyRansac
    assert PointLineHomographyRansac.default_conf["ransac_th"] == 2.0
    est = PointLineHomographyEstimator({"ransac_th": 1.5})
    assert est.conf.ransac_th == 1.5 and est.conf.options.max_iters == 3000
    cases = [{"m_kpts0": torch.rand(3, 2), "m_kpts1": torch.rand(3, 2)},
             {"m_lines0": torch.rand(2, 2, 2), "m_lines1": torch.rand(2, 2, 2)},
             {"m_kpts0": torch.rand(2, 2), "m_kpts1": torch.rand(2, 2), "m_lines0": torch.rand(1, 2, 2), "m_lines1": torch.rand(1, 2, 2)},
             {"m_kpts0": torch.zeros(0, 2), "m_kpts1": torch.zeros(0, 2), "m_lines0": torch.zeros(0, 2, 2), "m_lines1": torch.zeros(0, 2, 2)}]
    for data in cases:
        out = est(data)
        k = data["m_kpts0"].shape[0] if "m_kpts0" in data else 0
        kl = data["m_lines0"].shape[0] if "m_lines0" in data else 0
        assert out["success"] is False and torch.equal(out["M_0to1"], torch.eye(3))
        assert out["inliers"].shape == (k,) and out["line_inliers"].shape == (kl,)
        assert not out["inliers"].any() and not out["line_inliers"].any()
    with pytest.raises(AssertionError):
        est({})
    with pytest.raises(RuntimeError):                       # four features on the CPU: no fallback
        est({"m_kpts0": torch.rand(4, 2), "m_kpts1": torch.rand(4, 2)})
    with pytest.raises(ValueError):
        point_line_homography_ransac(None, None, None, None, None, None)
    a, b = torch.rand(1, 4, 2, 2), torch.rand(1, 5, 2, 2)
    pred = {"lines0": a, "lines1": b, "line_matches0": torch.zeros(1, 4, dtype=torch.long)}
    assert _line_inputs(pred)[0] is a and _line_inputs({"lines0": a, "lines1": b}) == (None, None, None)
    assert _line_inputs({**pred, "orig_lines0": b, "orig_lines1": a})[:2] == (b, a)


def test_line_metrics_on_empty_and_tiny_inputs():
    from glue_factory_amd.metrics import line_inlier_metrics, point_line_homography_metrics  # noqa: F401
    assert line_inlier_metrics({}) == {}
    lm = torch.tensor([[0, -1, 2, 1], [-1, -1, -1, -1]])
    inl = torch.tensor([[True, False, True, False], [False, False, False, False]])
    m = line_inlier_metrics({"line_inliers": inl, "line_matches0": lm})
    assert m["ransac_line_inl"].tolist() == [2.0, 0.0] and m["ransac_line_inl%"].tolist() == pytest.approx([2 / 3, 0.0])
    m = line_inlier_metrics({"line_inliers": torch.zeros(2, 0, dtype=torch.bool), "line_matches0": torch.zeros(2, 0, dtype=torch.long)})
    assert m["ransac_line_inl"].tolist() == [0.0, 0.0] and m["ransac_line_inl%"].tolist() == [0.0, 0.0]
