"""The yardstick's own test (no GPU): tests/e_solver_cases.py is what tests/test_gpu_e_solver.py measures the relative-pose
kernels with, so its restatements, scenes, bounds and recorded measurements are checked here -- every mutation must break
the bound it is meant for, every planted scene must be solvable under the stated seed, the recorded constants must cover a
fresh measurement -- and the pose metrics must agree with the reference's own functions (side by side where the reference
checkout is present, and through tests/golden/relative_pose_eval.npz everywhere).  Also the host view of the C ABI: the
header declares the three entries, lib.py carries them, the ABI number is 20."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import e_solver_cases as ec
from conftest import load_golden

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI, host view ---------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_three_entries_and_abi_20():
    from glue_factory_amd import lib
    code = open(os.path.join(ROOT, "include", "gf_amd.h")).read()
    assert re.search(r"#define\s+GF_AMD_ABI_VERSION\s+20\b", code) and lib.ABI_VERSION == 20
    for name, nargs in (("gf_e_ws_bytes", 3), ("gf_e_ransac", 23), ("gf_e_pose", 14)):
        proto = re.search(r"^int(?:64_t)? " + name + r"\(([^;]*)\);", code, re.M)
        assert proto and proto.group(1).count(",") + 1 == nargs == len(lib.SIGNATURES[name]), name
    assert lib._RESTYPE["gf_e_ws_bytes"] is lib._c.c_int64
    for name in ("GF_E_TILE", "GF_E_HYPS", "GF_E_MAXSOL", "GF_E_EPS_PIVOT", "GF_E_BISECT", "GF_E_JACOBI", "GF_E_JACOBI3"):
        assert re.search(r"#define\s+" + name + r"\s+\S+\s+/\*", code), name
    assert (ec.TILE, ec.HYPS, ec.MAXSOL) == (256, 256, 10)
    src = open(os.path.join(ROOT, "glue-factory_amd", "csrc", "Makefile")).read()
    assert " e_solver.hip " in src
    assert os.path.exists(lib.LIB_PATH) and all(hasattr(lib.load(), n) for n in ("gf_e_ws_bytes", "gf_e_ransac", "gf_e_pose"))


# ---- sampling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 6, 17, ec.TILE + 1])
def test_samples_are_distinct_and_in_range(K):
    s = ec.samples(ec.SEED, 1, 300, K)
    assert s.min() >= 0 and s.max() < K and all(len(set(row)) == 5 for row in s.tolist())
    if K > 5:
        assert len({tuple(r) for r in s.tolist()}) > 1
        for d in range(5):
            assert set(ec.samples(3, 0, 3000, 6)[:, d].tolist()) == set(range(6))
    assert (ec.samples(ec.SEED, 0, 7, 4) == -1).all()


# ---- solver ----------------------------------------------------------------------------------------------------------------
def test_solver_returns_the_true_E_on_noise_free_samples():
    rng = np.random.default_rng(3)
    worst = 0.0
    for i in range(40):
        s = ec.scene(100 + i % 4, 20, 0, 20, 20)
        ray0 = np.concatenate([rng.uniform(-0.5, 0.5, (5, 2)), np.ones((5, 1))], 1) * rng.uniform(2, 10, (5, 1))
        Y = ray0 @ s["R"].T + s["t"]
        pts = np.concatenate([ray0[:, :2] / ray0[:, 2:], Y[:, :2] / Y[:, 2:]], 1)            # exact in fp64
        Es = ec.solve5(pts)
        assert 1 <= len(Es) <= ec.MAXSOL and np.abs(np.linalg.norm(Es, axis=(-2, -1)) - 1).max() < 1e-12
        worst = max(worst, ec.sign_distance(Es, s["E"]).min())
        assert ec.residual(Es, pts).max() < 1e-8
    assert worst < 1e-8
    assert len(ec.solve5(np.repeat(pts[:1], 5, 0))) == 0                                  # one point five times


def test_recorded_measurements_cover_a_fresh_measurement_and_few_samples_are_left_out():
    cs = ec.candidate_samples()
    assert cs["keep"].mean() >= 0.9, "more than 10 % of the samples left out"
    assert np.abs(cs["corr"]).max() <= ec.PT_MAX
    res, dist = 0.0, 0.0
    for s, sols, keep in zip(cs["samples"], cs["sols"], cs["keep"]):
        if not keep:
            continue
        pts = cs["corr"][s].astype(np.float64)
        res = max(res, ec.residual(sols, pts).max())
        rev = ec.solve5(pts[::-1])
        assert len(rev) == len(sols)
        dist = max(dist, max(ec.sign_distance(rev, E).min() for E in sols))
    print("restated residual", res, "restated distance", dist)
    assert res <= ec.RESTATED_RESIDUAL * 1.05 and dist <= ec.RESTATED_DISTANCE * 1.05
    assert res >= ec.RESTATED_RESIDUAL / 4 and dist >= ec.RESTATED_DISTANCE / 4           # recorded, not inflated
    # the bounds separate a right candidate from a wrong one: solutions are at least SEP_MIN apart on kept samples
    assert ec.STORAGE_DISTANCE + ec.SOLVER_FACTOR * ec.RESTATED_DISTANCE < ec.SEP_MIN / 100


# ---- scenes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ec.PLANTED)
def test_planted_scenes_hold_their_conditions(spec):
    s = ec.scene(*spec)
    idx, corr = ec.scene_corr(s)
    planted = s["planted"][idx]
    assert len(corr) == s["K"] == spec[1] + spec[2] and planted.sum() == spec[1]
    assert np.abs(corr).max() <= ec.PT_MAX
    d = ec.sampson_distance(s["E"], corr)
    assert d[~planted].min() >= 10 * float(s["th"]) and d[planted].max() < float(s["th"]) / 100
    assert 600 <= min(s["cam0"][0].min(), s["cam1"][0].min()) and max(s["cam0"][0].max(), s["cam1"][0].max()) <= 1240
    assert not np.allclose(s["cam0"][0], s["cam1"][0]) and not np.allclose(s["cam0"][1], s["cam1"][1])
    assert ec.angle_R(s["R"], np.eye(3)) <= 30.0 + 1e-9 and abs(np.linalg.norm(s["t"]) - 1) < 1e-12
    smp = ec.samples(ec.SEED, 0, ec.PLANTED_T, len(corr))
    assert planted[smp].all(1).any(), "no all-inlier hypothesis among the first T"
    # non-planar: the inliers' 3-D points span space (rank of the homography design matrix would be 8 for a plane)
    c = corr[planted].astype(np.float64)
    x0, x1 = ec._hom(c[:, :2]), ec._hom(c[:, 2:])
    sv = np.linalg.svd((x1[:, :, None] * x0[:, None, :]).reshape(-1, 9), compute_uv=False)
    assert sv[-2] > 1e-3 * sv[0] and sv[-1] < 1e-6 * sv[0]
    assert 0 < ec.refit_bound_deg(s) < 1.0


def test_restated_pipeline_recovers_a_planted_scene_and_mutations_are_caught():
    spec = ec.PLANTED[2]
    s = ec.scene(*spec)
    idx, corr = ec.scene_corr(s)
    planted = s["planted"][idx]
    out = ec.restated(spec)
    assert out["success"] and np.array_equal(out["mask"], planted)
    err = ec.pose_error(out["R"], out["t"], s["R"], s["t"])
    assert err < ec.refit_bound_deg(s)
    th = float(s["th"])
    # E transposed, one Sampson denominator dropped: the inlier mask of the true E changes
    assert np.array_equal(ec.inlier_mask(s["E"], corr, th), planted)
    assert not np.array_equal(ec.inlier_mask(s["E"], corr, th, mutate="transpose"), planted)
    more = np.concatenate([corr, _near(s, th)])
    assert ec.inlier_mask(s["E"], more, th)[len(corr):].all()
    assert not ec.inlier_mask(s["E"], more, th, mutate="one_denominator")[len(corr):].any()
    # the band is narrow: it holds none of the scene's correspondences, so a count is decided exactly
    sure, maybe = ec.count_band(s["E"].astype(np.float32), corr, s["th"])
    assert (sure, maybe) == (planted.sum(), 0)
    # the last tile's ragged rows counted: a tile padded with copies of an inlier leaves the band
    pad = np.concatenate([corr, np.repeat(corr[planted][:1], ec.TILE - len(corr) % ec.TILE, 0)])
    assert ec.inlier_mask(s["E"], pad, th).sum() > sure + maybe
    # cheirality skipped: some scene's first decomposition is not its pose; t not normalised: the norm test sees it
    firsts = [ec.pose_error(*ec.choose_pose(ec.scene(60 + i, 30, 0, 40, 40)["E"], ec.scene_corr(ec.scene(60 + i, 30, 0, 40, 40))[1],
                                            mutate="no_cheirality")[:2], ec.scene(60 + i, 30, 0, 40, 40)["R"],
                            ec.scene(60 + i, 30, 0, 40, 40)["t"]) for i in range(3)]
    assert max(firsts) > 1.0
    assert abs(np.linalg.norm(out["t"]) - 1) < 1e-12 and abs(np.linalg.norm(2 * out["t"]) - 1) > 4 * ec.U32
    # ties to the highest index
    counts = np.array([[3, 7, -1], [7, 2, 7]])
    assert ec.select(counts) == 1 and ec.select(counts, mutate="ties_high") == 5 and ec.select(-np.ones((2, 3))) == -1
    assert set(ec.MUTATIONS) == {"transpose", "one_denominator", "no_cheirality", "ties_high", "ragged_tile", "t_not_normalised"}


def _near(s, th):
    """Correspondences at 1.2 th from their epipolar line in image 1 alone: squared Sampson error ~ 0.72 th^2, an inlier of the
    rule; with one of the two (nearly equal) denominators dropped ~ 1.44 th^2, an outlier."""
    idx, corr = ec.scene_corr(s)
    c = corr[s["planted"][idx]][:8].astype(np.float64)
    x0 = ec._hom(c[:, :2])
    line = x0 @ s["E"].T
    n = line[:, :2] / np.linalg.norm(line[:, :2], axis=1, keepdims=True)
    c[:, 2:] += 1.2 * th * n
    return c


def test_refit_and_decomposition_restate_their_meaning():
    s = ec.scene(*ec.PLANTED[1])
    idx, corr = ec.scene_corr(s)
    planted = s["planted"][idx]
    E = ec.refit(corr, planted)
    assert ec.sign_distance(E, s["E"]) < 1e-5 and abs(np.linalg.norm(E) - 1) < 1e-12
    assert np.allclose(np.linalg.svd(E, compute_uv=False), [2 ** -0.5, 2 ** -0.5, 0], atol=1e-12)
    assert ec.refit(corr, np.arange(len(corr)) < 7) is None
    R, t, counts = ec.choose_pose(s["E"], corr[planted])
    assert sorted(counts) == [0, 0, 0, planted.sum()] and ec.pose_error(R, t, s["R"], s["t"]) < 1e-6
    for Rk, tk in ec.four_poses(s["E"]):
        assert abs(np.linalg.det(Rk) - 1) < 1e-12 and ec.sign_distance(ec.E_of(Rk, tk), s["E"]) < 1e-12


# ---- torch restatements and metrics -------------------------------------------------------------------------------------
def _torch_inputs():
    from glue_factory_amd.geometry import Pose
    z = {k: torch.from_numpy(v) for k, v in ec.eval_inputs().items()}
    return z, Pose.from_Rt(z["R_gt"], z["t_gt"])


def test_geometry_additions():
    from glue_factory_amd.geometry import T_to_E, decompose_essential_matrix, sym_epipolar_distance
    z, T = _torch_inputs()
    E = T_to_E(T)
    for i in range(3):
        R1, R2, t = (x.numpy() for x in decompose_essential_matrix(E[i]))
        Ei = E[i].numpy() / np.linalg.norm(E[i].numpy())
        assert min(ec.angle_R(R1, z["R_gt"][i].numpy()), ec.angle_R(R2, z["R_gt"][i].numpy())) < 1e-5
        assert ec.angle_t(t, z["t_gt"][i].numpy()) < 1e-5 and abs(np.linalg.det(R1) - 1) < 1e-9 and abs(np.linalg.det(R2) - 1) < 1e-9
        assert ec.sign_distance(ec.E_of(R1, t), Ei) < 1e-9
    d2 = sym_epipolar_distance(z["p0"].double(), z["p1"].double(), E, squared=True)
    assert d2.shape == (4, 40) and sym_epipolar_distance(z["p0"][:, :0], z["p1"][:, :0], E).shape == (4, 0)
    e2, den = ec.sampson_terms(E[1].numpy(), np.concatenate([z["p0"][1].numpy(), z["p1"][1].numpy()], 1))
    assert d2[1].numpy().max() > 0


def test_metrics_equal_the_golden_values_of_the_reference():
    from glue_factory_amd.geometry import T_to_E, sym_epipolar_distance
    from glue_factory_amd.metrics import pose_auc, relative_pose_error
    g = load_golden("relative_pose_eval")
    z, T = _torch_inputs()
    t_err, r_err = relative_pose_error(T, z["R"], z["t"])
    np.testing.assert_allclose(t_err.numpy(), g["t_err"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(r_err.numpy(), g["r_err"], rtol=0, atol=1e-6)
    assert g["r_err"][0] == 0 and g["r_err"][2] == 180 and float(r_err[0]) < 1e-6 and float(r_err[2]) == 180.0
    assert (g["t_err"] <= 90).all() and g["t_err"][1] < 15                                # folded at 90 degrees
    one = relative_pose_error(type(T)(T._data[1]), z["R"][1], z["t"][1])
    assert one[0].shape == () and float(one[0]) == float(t_err[1])
    epi = sym_epipolar_distance(z["p0"].double(), z["p1"].double(), T_to_E(T), squared=False)
    np.testing.assert_allclose(epi.numpy(), g["epi"], rtol=1e-9, atol=1e-15)
    assert pose_auc(ec.eval_inputs()["errors_a"], [5, 10, 20]) == g["auc_a"].tolist()
    assert pose_auc(torch.from_numpy(ec.eval_inputs()["errors_b"]), [5, 10, 20]) == g["auc_b"].tolist() == [0.0, 0.0, 0.0]


def test_relative_pose_metrics_on_the_cpu_path():
    """relative_pose_metrics is stock torch: the fixture's pairs as one batch, success 0 -> inf."""
    from glue_factory_amd.geometry import Camera, Pose
    from glue_factory_amd.metrics import relative_pose_metrics
    g = load_golden("relative_pose_eval")
    z, T = _torch_inputs()
    cam = Camera(torch.tensor([[1.0, 1.0, 1.0, 1.0, 0.0, 0.0]]).double().expand(4, 6))        # identity camera
    m0 = torch.arange(40)[None].expand(4, 40).clone()
    m0[0, 5:] = -1
    pred = {"keypoints0": z["p0"].double(), "keypoints1": z["p1"].double(), "matches0": m0,
            "M_0to1": Pose.from_Rt(z["R"], z["t"]), "success": torch.tensor([True, True, False, True]),
            "inliers": m0 > 10}
    data = {"view0": {"camera": cam}, "view1": {"camera": cam}, "T_0to1": T}
    m = relative_pose_metrics(pred, data)
    want = np.maximum(g["t_err"], g["r_err"])
    assert torch.isinf(m["rel_pose_error"][2]) and np.allclose(m["rel_pose_error"].numpy()[[0, 1, 3]], want[[0, 1, 3]], atol=1e-3)
    assert m["num_matches"].tolist() == [5, 40, 40, 40] and m["ransac_inl"].tolist() == [0.0, 29.0, 29.0, 29.0]
    for k, col in (("epi_prec@1e-4", 0), ("epi_prec@5e-4", 1), ("epi_prec@1e-3", 2)):
        np.testing.assert_allclose(m[k].numpy()[1:], g["epi_prec"][1:, col], atol=1e-6)
    assert set(relative_pose_metrics({k: v for k, v in pred.items() if k != "M_0to1"}, data)) == {
        "epi_prec@1e-4", "epi_prec@5e-4", "epi_prec@1e-3", "num_matches"}


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gluefactory")), reason="reference checkout absent")
def test_metrics_side_by_side_with_the_reference():
    sys.path[:0] = [os.path.join(ROOT, "oracle", "stubs")]
    sys.path.append(REF)
    try:
        from gluefactory.geometry import epipolar as ref
        from gluefactory.geometry.wrappers import Pose as RefPose
        from gluefactory.utils.tools import cal_error_auc
    finally:
        sys.path.remove(REF)
        sys.path.pop(0)
    from glue_factory_amd import geometry as ours
    from glue_factory_amd.metrics import pose_auc, relative_pose_error
    if not hasattr(np, "trapz"):
        np.trapz = np.trapezoid
    z, T = _torch_inputs()
    for i in range(4):
        Tr = RefPose.from_Rt(z["R_gt"][i], z["t_gt"][i])
        te, re_ = ref.relative_pose_error(Tr, z["R"][i], z["t"][i])
        to, ro = relative_pose_error(type(T)(T._data[i]), z["R"][i], z["t"][i])
        assert abs(float(te) - float(to)) < 1e-9 and abs(float(re_) - float(ro)) < 1e-6
        assert torch.allclose(ref.T_to_E(Tr), ours.T_to_E(type(T)(T._data[i])))
        for sq in (True, False):
            a = ref.sym_epipolar_distance(z["p0"][i].double(), z["p1"][i].double(), ref.T_to_E(Tr), squared=sq)
            b = ours.sym_epipolar_distance(z["p0"][i].double(), z["p1"][i].double(), ref.T_to_E(Tr), squared=sq)
            assert torch.allclose(a, b, rtol=1e-12, atol=0)
        R1, R2, t = ref.decompose_essential_matrix(ref.T_to_E(Tr))
        S1, S2, s = ours.decompose_essential_matrix(ref.T_to_E(Tr))
        assert min((R1 - S1).abs().max(), (R1 - S2).abs().max()) < 1e-9 and min((t - s).abs().max(), (t + s).abs().max()) < 1e-9
    inp = ec.eval_inputs()
    for key in ("errors_a", "errors_b"):
        assert pose_auc(inp[key], [5, 10, 20]) == [float(v) for v in cal_error_auc(inp[key], [5, 10, 20])]
