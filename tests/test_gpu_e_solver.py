"""Relative-pose solver kernels (csrc/e_solver.hip: gf_e_ransac, gf_e_pose) against the fp64 restatements, planted scenes and
bounds of tests/e_solver_cases.py, and the host code on top of them (glue_factory_amd.solvers.relative_pose_ransac,
metrics.relative_pose_*, the `solver` stage of TwoViewPipeline).  Shapes follow the kernel's constants (GF_E_TILE, GF_E_HYPS,
GF_E_MAXSOL of the header).  Every raw call is made twice into guarded buffers and must give equal bits and leave the guards
alone.

Two identical pairs at DIFFERENT batch positions cannot give equal bits of E: the pair index is an argument of the sampling
hash (ransac_common.h, for either solver), so they draw different samples.  What is asserted instead: the same pair at the same position
gives equal bits whatever else is in the batch and in a second call, and identical pairs at different positions give the
same inlier mask and count on a planted scene."""
import functools

import numpy as np
import pytest
import torch

import e_solver_cases as ec
import solver_harness as sh
from solver_harness import dev as _dev, load as _lib

pytestmark = pytest.mark.gpu


def _ransac_once(p0, p1, m0, th, T, lo_iters, seed):
    B, M = m0.shape
    N = p1.shape[1]
    S = ec.MAXSOL
    spec = {"E": ((B, 3, 3), torch.float32, -7.0), "R": ((B, 3, 3), torch.float32, -7.0), "t": ((B, 3), torch.float32, -7.0),
            "inliers": ((B, M), torch.uint8, 0xAB), "num": ((B,), torch.int32, -77), "success": ((B,), torch.uint8, 0xAB),
            "samples": ((B, T, 5), torch.int32, -77), "cand": ((B, T, S, 3, 3), torch.float32, -7.0),
            "ncand": ((B, T), torch.int32, -77), "counts": ((B, T, S), torch.int32, -77)}
    return sh.run_once("gf_e_ransac", "gf_e_ws_bytes", B, M, T, spec, lambda ws, nbytes, outs: (
        p0.data_ptr(), p1.data_ptr(), m0.data_ptr(), th.data_ptr(), B, M, N, T, lo_iters, seed, ws, nbytes, *outs))


def ransac(p0, p1, m0, th, T, lo_iters=2, seed=ec.SEED):
    """The raw entry on numpy inputs [B,M,2], [B,N,2], [B,M], [B] (normalised): called twice (equal bits), guards checked."""
    a = (_dev(p0, torch.float32), _dev(p1, torch.float32), _dev(m0, torch.int64), _dev(th, torch.float32))
    return sh.run_twice(lambda: _ransac_once(*a, T, lo_iters, seed))


def _stack(scenes):
    return (np.stack([s["p0n"] for s in scenes]), np.stack([s["p1n"] for s in scenes]),
            np.stack([s["matches0"] for s in scenes]), np.array([s["th"] for s in scenes], np.float32))


def _failure(out, b):
    assert not out["success"][b] and out["num"][b] == 0 and not out["inliers"][b].any()
    assert np.array_equal(out["E"][b], np.zeros((3, 3))) and np.array_equal(out["R"][b], np.eye(3))
    assert np.array_equal(out["t"][b], np.zeros(3))


def _is_pose(R, t):
    assert np.isfinite(R).all() and np.isfinite(t).all()
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(R) - 1) < 1e-5
    assert abs(np.linalg.norm(t.astype(np.float64)) - 1) < 4 * ec.U32, "t is not normalised"


def _sized(K, seed):
    """A scene with exactly K matches, half of them outliers, M = K + 7 keypoints."""
    return ec.scene(seed, K - K // 2, K // 2, K + 7, K + 3)


# ---- sampling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, ec.HYPS - 1, ec.HYPS, ec.HYPS + 1])
def test_samples_equal_the_host_function(T):
    Ks = [5, 6, ec.TILE + 1]
    M = ec.TILE + 8
    scenes = [ec.scene(40 + K, K, 0, M, M) for K in Ks]
    out = ransac(*_stack(scenes), T, lo_iters=0)
    for b, K in enumerate(Ks):
        assert np.array_equal(out["samples"][b], ec.samples(ec.SEED, b, T, K)), (b, K)


# ---- candidates -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _candidate_run():
    cs = ec.candidate_samples()
    s = cs["scene"]
    return cs, ransac(*_stack([s]), len(cs["samples"]), lo_iters=0)


def test_candidates_are_unit_norm_and_solve_their_sample():
    cs, out = _candidate_run()
    assert np.abs(cs["corr"]).max() <= ec.PT_MAX
    assert np.array_equal(out["samples"][0], cs["samples"])
    bound = ec.STORAGE_RESIDUAL + ec.SOLVER_FACTOR * ec.RESTATED_RESIDUAL
    worst = 0.0
    for t, s in enumerate(cs["samples"]):
        n = out["ncand"][0, t]
        assert 0 <= n <= ec.MAXSOL and not out["cand"][0, t, n:].any()
        E = out["cand"][0, t, :n].astype(np.float64)
        assert np.abs(np.linalg.norm(E, axis=(-2, -1)) - 1).max(initial=0) <= 4 * ec.U32
        if cs["keep"][t]:
            assert n > 0
            worst = max(worst, ec.residual(E, cs["corr"][s].astype(np.float64)).max())
    print("worst residual of a kernel candidate on a kept sample:", worst, "bound", bound)
    assert worst <= bound


def test_every_restated_solution_is_among_the_candidates_and_so_is_the_true_E():
    cs, out = _candidate_run()
    bound = ec.STORAGE_DISTANCE + ec.SOLVER_FACTOR * ec.RESTATED_DISTANCE
    worst, worst_true = 0.0, 0.0
    for t in np.nonzero(cs["keep"])[0]:
        E = out["cand"][0, t, :out["ncand"][0, t]].astype(np.float64)
        d = max(ec.sign_distance(E, S).min() for S in cs["sols"][t])
        worst = max(worst, d)
        # the true E: as near to a kernel candidate as to a restated one, up to the same bound (triangle inequality)
        worst_true = max(worst_true, ec.sign_distance(E, cs["scene"]["E"]).min() - ec.sign_distance(cs["sols"][t], cs["scene"]["E"]).min())
    print("worst distance of a restated solution to the kernel's candidates:", worst, "of the true E, beyond the restated:",
          worst_true, "bound", bound)
    assert worst <= bound and worst_true <= bound
    near = [ec.sign_distance(out["cand"][0, t, :out["ncand"][0, t]].astype(np.float64), cs["scene"]["E"]).min(initial=9)
            for t in np.nonzero(cs["keep"])[0]]
    assert np.median(near) < 1e-4                  # (fp32 keypoints: the true E up to the conditioning of the sample)


# ---- scoring ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, ec.TILE - 1, ec.TILE, ec.TILE + 1, 2 * ec.TILE + 1])
def test_counts_lie_in_the_fp64_band_of_the_returned_candidate(K):
    T = ec.HYPS // ec.MAXSOL + 1                   # T * MAXSOL = 260: across the 256-candidate workgroup edge
    assert (T - 1) * ec.MAXSOL < ec.HYPS < T * ec.MAXSOL
    s = _sized(K, 50)
    out = ransac(*_stack([s]), T, lo_iters=0)
    _, corr = ec.scene_corr(s)
    assert len(corr) == K
    seen = 0
    for t in range(T):
        n = out["ncand"][0, t]
        assert (out["counts"][0, t, n:] == -1).all()
        for q in range(n):
            sure, maybe = ec.count_band(out["cand"][0, t, q], corr, s["th"])
            assert sure <= out["counts"][0, t, q] <= sure + maybe, (t, q, sure, maybe, out["counts"][0, t, q])
            seen += 1
    assert seen > T                                 # more than one candidate per hypothesis on average
    # selection: the winner is the first maximum of the counts
    win = ec.select(out["counts"][0])
    assert win >= 0 and out["success"][0]
    assert np.array_equal(out["E"][0], out["cand"][0].reshape(-1, 3, 3)[win])
    assert out["num"][0] == out["counts"][0].reshape(-1)[win] == out["inliers"][0].sum()
    assert win != ec.select(out["counts"][0], mutate="ties_high") or (out["counts"][0] == out["num"][0]).sum() == 1


def test_the_same_pair_gives_the_same_bits_whatever_shares_its_batch():
    spec = ec.PLANTED[2]
    a, b = ec.scene(*spec), ec.scene(*ec.PLANTED[1])
    alone = ransac(*_stack([a]), ec.HYPS + 1)
    both = ransac(*_stack([a, b]), ec.HYPS + 1)
    twin = ransac(*_stack([b, a]), ec.HYPS + 1)
    for k in ("E", "R", "t", "inliers", "num", "cand", "counts"):
        assert np.array_equal(alone[k][0], both[k][0]), k
    assert np.array_equal(twin["inliers"][1], both["inliers"][0]) and twin["num"][1] == both["num"][0]


# ---- planted scenes ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted(noise, lo_iters):
    scenes = [ec.scene(*spec, noise=noise) for spec in ec.PLANTED]
    return scenes, ransac(*_stack(scenes), ec.PLANTED_T, lo_iters=lo_iters)


def test_planted_scenes_are_recovered_exactly():
    scenes, lo2 = _planted(0.0, 2)
    _, lo0 = _planted(0.0, 0)
    for b, s in enumerate(scenes):
        for out in (lo0, lo2):
            assert out["success"][b]
            assert np.array_equal(out["inliers"][b], s["planted"]), b
            assert out["num"][b] == s["planted"].sum()
            _is_pose(out["R"][b], out["t"][b])
            assert abs(np.linalg.norm(out["E"][b].astype(np.float64)) - 1) <= 4 * ec.U32
        assert lo2["num"][b] >= lo0["num"][b]
        err, bound = ec.pose_error(lo2["R"][b], lo2["t"][b], s["R"], s["t"]), ec.refit_bound_deg(s)
        print(f"pair {b}: pose error {err:.3e} deg (lo 0: {ec.pose_error(lo0['R'][b], lo0['t'][b], s['R'], s['t']):.3e}), bound {bound:.3e}")
        assert err < bound
        # the model explains its inliers: E against (R, t)
        assert ec.sign_distance(ec.E_of(lo2["R"][b].astype(np.float64), lo2["t"][b].astype(np.float64)), lo2["E"][b]) < 1e-5


def test_noisy_planted_scenes_are_as_good_as_the_restated_pipeline():
    scenes, lo2 = _planted(0.5, 2)
    _, lo0 = _planted(0.5, 0)
    for b, (spec, s) in enumerate(zip(ec.PLANTED, scenes)):
        ref = ec.restated(spec, 0.5, pair=b)
        err = ec.pose_error(lo2["R"][b], lo2["t"][b], s["R"], s["t"])
        ref_err = ec.pose_error(ref["R"], ref["t"], s["R"], s["t"])
        print(f"pair {b}: pose error {err:.4f} deg, restated {ref_err:.4f} deg; inliers {lo2['num'][b]} (lo 0: {lo0['num'][b]}), restated {ref['count']}")
        assert lo2["success"][b] and lo2["num"][b] >= lo0["num"][b]
        assert err <= ref_err + ec.NOISY_MARGIN_DEG


# ---- the pose stage alone -------------------------------------------------------------------------------------------------
# entries of R and t from an exact E given in fp32: E moves by at most 3 U32 in the rounding, R and t by at most 2 sqrt 2 times
# that (tests/e_solver_cases.py: refit_bound_deg), and each returned entry is rounded to fp32 once more.  (An angle is no
# measure here: the arccos of a trace that is off by 3 U32 reads 0.03 degrees.)
R_TOL = (2 * np.sqrt(2.0) * 3 + 1) * ec.U32


def _pose(scenes, Es, flags):
    from glue_factory_amd.solvers.relative_pose_ransac import recover_pose
    p0, p1, m0, _ = _stack(scenes)
    R, t, nf = recover_pose(_dev(p0, torch.float32), _dev(p1, torch.float32), _dev(m0, torch.int64), _dev(flags, torch.bool),
                            _dev(np.stack(Es), torch.float32))
    return R.cpu().numpy(), t.cpu().numpy(), nf.cpu().numpy()


def test_pose_picks_the_decomposition_of_the_restatement():
    scenes = [ec.scene(60 + i, 30 + 40 * i, 0, 120, 110) for i in range(3)]
    flags = np.stack([s["planted"] for s in scenes])
    R, t, nf = _pose(scenes, [s["E"] for s in scenes], flags)
    for b, s in enumerate(scenes):
        idx, corr = ec.scene_corr(s)
        Rr, tr, counts = ec.choose_pose(s["E"].astype(np.float32).astype(np.float64), corr.astype(np.float64))
        _is_pose(R[b], t[b])
        assert nf[b] == max(counts) == s["planted"].sum()
        assert np.abs(R[b] - Rr).max() < R_TOL and np.abs(t[b] - tr).max() < R_TOL
        assert np.abs(R[b] - s["R"]).max() < R_TOL and np.abs(t[b] - s["t"]).max() < R_TOL
        # the mutation: the first decomposition is not the right one for every scene
    firsts = [ec.pose_error(*ec.choose_pose(s["E"], ec.scene_corr(s)[1], mutate="no_cheirality")[:2], s["R"], s["t"]) for s in scenes]
    assert max(firsts) > 1.0


def test_pose_counts_decide_by_one_point():
    """k + 1 points in front of both cameras under (R, t) and k under (R, -t): the same E, the counts differ by one."""
    s = ec.scene(70, 21, 0, 48, 48)
    rng = np.random.default_rng(5)
    idx, corr = ec.scene_corr(s)
    behind = []
    while len(behind) < 20:
        X = np.append(rng.uniform(-0.4, 0.4, 2), 1.0) * rng.uniform(2, 10)
        Y = s["R"] @ X - s["t"]
        if Y[2] > 1.0:
            behind.append(np.concatenate([X[:2] / X[2], Y[:2] / Y[2]]))
    behind = np.array(behind, np.float32)
    p0n, p1n, m0 = s["p0n"].copy(), s["p1n"].copy(), s["matches0"].copy()
    free0, free1 = np.nonzero(m0 < 0)[0][:20], np.setdiff1d(np.arange(48), m0[m0 >= 0])[:20]
    p0n[free0], p1n[free1], m0[free0] = behind[:, :2], behind[:, 2:], free1
    both = dict(s, p0n=p0n, p1n=p1n, matches0=m0)
    for drop, want_t in ((0, 1.0), (2, -1.0)):                     # 21 against 20, then 19 against 20
        flags = m0 >= 0
        flags[idx[:drop]] = False
        R, t, nf = _pose([both], [s["E"]], flags[None])
        assert nf[0] == max(21 - drop, 20)
        assert np.abs(R[0] - s["R"]).max() < R_TOL and np.abs(t[0] - want_t * s["t"]).max() < R_TOL


# ---- degenerate input ---------------------------------------------------------------------------------------------------
def test_fewer_than_five_matches_fail_and_five_do_not_fault():
    M = N = 12
    scenes = [ec.scene(80 + K, K, 0, M, N) for K in (0, 1, 2, 3, 4, 5)]
    scenes.append(dict(scenes[5], matches0=np.full(M, -1, np.int64)))                # all -1
    scenes.append(dict(scenes[5], matches0=np.where(scenes[5]["matches0"] >= 0, N + 3, -1)))   # all outside [0, N)
    out = ransac(*_stack(scenes), ec.HYPS + 1)
    for b in (0, 1, 2, 3, 4, 6, 7):
        _failure(out, b)
        assert (out["samples"][b] == -1).all() and (out["ncand"][b] == 0).all() and (out["counts"][b] == -1).all()
    assert np.array_equal(np.sort(out["samples"][5], -1), np.tile(np.arange(5), (ec.HYPS + 1, 1)))
    if out["success"][5]:
        _is_pose(out["R"][5], out["t"][5])
        assert out["num"][5] == 5
    else:
        _failure(out, 5)


def test_duplicates_pure_rotation_and_coplanar_points():
    """Pure rotation: every E = [t]x R with any t explains the data, so a model may or may not be found.  success is 1
    exactly when some sample gave a candidate (its count does not matter); either way every output is finite and a success
    comes with a rotation matrix, a unit t and the rotation of the scene (t is arbitrary)."""
    base = ec.scene(90, 30, 0, 64, 64)
    dup = dict(base, p0n=np.repeat(base["p0n"][:1], 64, 0), p1n=np.repeat(base["p1n"][:1], 64, 0))
    m0 = base["matches0"].copy()
    half = np.nonzero(m0 >= 0)[0]
    some = dict(base, p0n=base["p0n"].copy(), p1n=base["p1n"].copy())
    some["p0n"][half[1::2]], some["p1n"][m0[half[1::2]]] = some["p0n"][half[0::2]], some["p1n"][m0[half[0::2]]]
    rot = ec.scene(91, 30, 0, 64, 64, mode="rotation")
    plane = ec.scene(92, 30, 0, 64, 64, mode="planar")
    out = ransac(*_stack([dup, some, rot, plane]), ec.HYPS + 1)
    for k in ("E", "R", "t", "cand"):
        assert np.isfinite(out[k]).all(), k
    _failure(out, 0)                                               # one point 30 times: every sample is rejected
    for b in (1, 2, 3):
        assert out["success"][b] == bool((out["ncand"][b] > 0).any())
        if out["success"][b]:
            _is_pose(out["R"][b], out["t"][b])
        else:
            _failure(out, b)
    assert out["success"][1] and out["num"][1] == 30
    print("pure rotation: success", out["success"][2], "inliers", out["num"][2])
    if out["success"][2] and out["num"][2] == 30:
        assert ec.angle_R(out["R"][2].astype(np.float64), rot["R"]) < 0.1
    # coplanar points: the true E is still among the candidates, as near as among the restated ones
    idx, corr = ec.scene_corr(plane)
    assert out["success"][3] and np.array_equal(out["inliers"][3], plane["planted"])
    assert ec.pose_error(out["R"][3], out["t"][3], plane["R"], plane["t"]) < ec.refit_bound_deg(plane)
    bound, hits = ec.STORAGE_DISTANCE + ec.SOLVER_FACTOR * ec.RESTATED_DISTANCE, 0
    for t in range(32):
        sols, cond = ec.solve5(corr[out["samples"][3, t]].astype(np.float64), with_info=True)
        if len(sols) == 0 or cond > ec.COND_MAX or ec.separation(sols) < ec.SEP_MIN:
            continue
        E = out["cand"][3, t, :out["ncand"][3, t]].astype(np.float64)
        assert len(E) and ec.sign_distance(E, plane["E"]).min() <= ec.sign_distance(sols, plane["E"]).min() + bound
        hits += 1
    assert hits >= 16


# ---- rejected calls -------------------------------------------------------------------------------------------------------
def test_rejected_calls_return_their_code_and_write_nothing():
    lib, L = _lib()
    B, M, N, T = 2, 40, 30, 10
    p0, p1 = torch.rand(B, M, 2, device="cuda"), torch.rand(B, N, 2, device="cuda")
    m0 = torch.zeros(B, M, dtype=torch.int64, device="cuda")
    th = torch.full((B,), 1e-3, device="cuda")
    nbytes = int(L.gf_e_ws_bytes(B, M, T))
    ws = torch.full((nbytes + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    f32 = lambda *shape: torch.full(shape, -7.0, device="cuda")
    E, R, t = f32(B, 3, 3), f32(B, 3, 3), f32(B, 3)
    inl = torch.full((B, M), 0xAB, dtype=torch.uint8, device="cuda")
    num = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    suc = torch.full((B,), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    off = (-ws.data_ptr()) % 16
    good = dict(p0=p0.data_ptr(), p1=p1.data_ptr(), m0=m0.data_ptr(), th=th.data_ptr(), B=B, M=M, N=N, T=T, lo=2, seed=1,
                ws=ws.data_ptr() + off, nbytes=nbytes, E=E.data_ptr(), R=R.data_ptr(), t=t.data_ptr(), inl=inl.data_ptr(),
                num=num.data_ptr(), suc=suc.data_ptr())
    shape, align = -2, -3
    bad = [({k: None}, shape) for k in ("p0", "p1", "m0", "th", "ws", "E", "R", "t", "inl", "num", "suc")]
    bad += [({"B": -1}, shape), ({"B": 0}, shape), ({"M": -3}, shape), ({"N": 0}, shape), ({"T": 0}, shape), ({"T": -5}, shape),
            ({"nbytes": nbytes - 1}, shape), ({"nbytes": -1}, shape), ({"lo": -1}, shape), ({"lo": 65}, shape),
            ({"ws": ws.data_ptr() + off + 4}, align)]
    for change, code in bad:
        a = {**good, **change}
        got = L.gf_e_ransac(a["p0"], a["p1"], a["m0"], a["th"], a["B"], a["M"], a["N"], a["T"], a["lo"], a["seed"], a["ws"],
                            a["nbytes"], a["E"], a["R"], a["t"], a["inl"], a["num"], a["suc"], None, None, None, None, st)
        assert got == code, (change, got)
    nf = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    n1 = int(L.gf_e_ws_bytes(B, M, 1))
    for change, code in [({"p0": None}, shape), ({"inl": None}, shape), ({"E": None}, shape), ({"R": None}, shape),
                         ({"t": None}, shape), ({"nf": None}, shape), ({"M": 0}, shape), ({"nbytes": n1 - 1}, shape),
                         ({"ws": ws.data_ptr() + off + 8}, align)]:
        a = {**good, "nf": nf.data_ptr(), "nbytes": n1, **change}
        got = L.gf_e_pose(a["p0"], a["p1"], a["m0"], a["inl"], a["E"], a["B"], a["M"], a["N"], a["ws"], a["nbytes"], a["R"],
                          a["t"], a["nf"], st)
        assert got == code, (change, got)
    assert L.gf_e_ws_bytes(0, M, T) == 0 and L.gf_e_ws_bytes(B, -1, T) == 0 and L.gf_e_ws_bytes(B, M, 0) == 0
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and all(bool((x == -7.0).all()) for x in (E, R, t)) and bool((inl == 0xAB).all())
    assert bool((num == -77).all()) and bool((suc == 0xAB).all()) and bool((nf == -77).all())


# ---- host surface ---------------------------------------------------------------------------------------------------------
def _camera(cams):
    from glue_factory_amd.geometry import Camera
    rows = [np.concatenate([[1024.0, 768.0], f, c]) for f, c in cams]
    return Camera(_dev(np.stack(rows), torch.float32))


def _batch(scenes):
    from glue_factory_amd.geometry import Pose
    kp0, kp1 = np.stack([s["kpts0"] for s in scenes]), np.stack([s["kpts1"] for s in scenes])
    m0 = np.stack([s["matches0"] for s in scenes])
    T = Pose.from_Rt(_dev(np.stack([s["R"] for s in scenes]), torch.float32), _dev(np.stack([s["t"] for s in scenes]), torch.float32))
    cache0 = {"keypoints": _dev(kp0, torch.float32), "matches": _dev(m0, torch.int64),
              "matching_scores": torch.ones(m0.shape, device="cuda")}
    return {"view0": {"camera": _camera([s["cam0"] for s in scenes]), "cache": cache0},
            "view1": {"camera": _camera([s["cam1"] for s in scenes]), "cache": {"keypoints": _dev(kp1, torch.float32)}},
            "T_0to1": T}


def test_one_call_captured_in_a_graph_equals_the_eager_call():
    from glue_factory_amd.solvers.relative_pose_ransac import relative_pose_ransac
    first = [ec.scene(*ec.PLANTED[2]), ec.scene(81, 1, 0, 300, 280)]
    second = [ec.scene(83, 3, 0, 300, 280), ec.scene(*ec.PLANTED[1])]
    cams = lambda scenes: (_camera([s["cam0"] for s in scenes]), _camera([s["cam1"] for s in scenes]))

    def tensors(scenes):
        c0, c1 = cams(scenes)
        return [_dev(np.stack([s["kpts0"] for s in scenes]), torch.float32), _dev(np.stack([s["kpts1"] for s in scenes]), torch.float32),
                _dev(np.stack([s["matches0"] for s in scenes]), torch.int64), c0._data, c1._data]

    from glue_factory_amd.geometry import Camera
    run = lambda a: relative_pose_ransac(a[0], a[1], a[2], Camera(a[3]), Camera(a[4]), max_iters=ec.HYPS + 1, seed=ec.SEED)
    static = tensors(first)
    run(static)                                          # warm-up outside the capture (library load)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        run(static)
        with torch.cuda.graph(graph, stream=side):
            captured = run(static)
    torch.cuda.current_stream().wait_stream(side)
    for scenes in (second, first):
        fresh = tensors(scenes)
        for s, f in zip(static, fresh):
            s.copy_(f)
        for _ in range(2):                               # replayed twice: equal bits
            graph.replay()
            torch.cuda.synchronize()
            eager = run(fresh)
            assert torch.equal(captured["M_0to1"]._data, eager["M_0to1"]._data)
            for k in ("E", "inliers", "num_inliers", "success"):
                assert torch.equal(captured[k], eager[k]), k
    assert captured["success"].tolist() == [True, False]


def test_pipeline_with_the_solver_stage_and_the_metrics():
    from glue_factory_amd.base_model import get_model
    from glue_factory_amd.metrics import relative_pose_metrics
    from glue_factory_amd.pipeline import TwoViewPipeline
    from glue_factory_amd.solvers.relative_pose_ransac import RelativePoseRansac
    assert get_model("solvers.relative_pose_ransac") is RelativePoseRansac
    assert get_model("glue_factory_amd.solvers.relative_pose_ransac") is RelativePoseRansac
    scenes = [ec.scene(*spec) for spec in ec.PLANTED]
    data = _batch(scenes)
    pipe = TwoViewPipeline({"allow_no_extract": True, "solver": {"name": "solvers.relative_pose_ransac",
                                                                 "max_iters": ec.PLANTED_T, "seed": ec.SEED}}).cuda().eval()
    assert type(pipe.solver).__name__ == "RelativePoseRansac"
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pred = pipe(data)
    assert pred["M_0to1"]._data.shape == (3, 12) and pred["M_0to1"]._data.dtype == torch.float32
    assert pred["inliers"].dtype == torch.bool and pred["success"].dtype == torch.bool and bool(pred["success"].all())
    planted = _dev(np.stack([s["planted"] for s in scenes]), torch.bool)
    assert torch.equal(pred["inliers"], planted) and torch.equal(pred["inliers"].sum(1).int(), pred["num_inliers"])
    m = relative_pose_metrics(pred, data)
    assert set(m) == {"rel_pose_error", "ransac_inl", "ransac_inl%", "epi_prec@1e-4", "epi_prec@5e-4", "epi_prec@1e-3", "num_matches"}
    assert all(v.shape == (3,) for v in m.values())
    print("rel_pose_error", m["rel_pose_error"].tolist(), "epi_prec@1e-4", m["epi_prec@1e-4"].tolist())
    for b, s in enumerate(scenes):
        assert float(m["rel_pose_error"][b]) < ec.refit_bound_deg(s)
    assert torch.equal(m["num_matches"], (pred["matches0"] > -1).sum(1)) and torch.equal(m["ransac_inl"], pred["num_inliers"].float())
    assert torch.allclose(m["ransac_inl%"], torch.full((3,), 0.5, device="cuda")) and torch.allclose(m["epi_prec@1e-4"], m["ransac_inl%"])
    empty = dict(pred, matches0=torch.full_like(pred["matches0"], -1))
    empty.update(pipe.solver({**data, **empty}))
    me = relative_pose_metrics(empty, data)
    assert bool(torch.isinf(me["rel_pose_error"]).all()) and bool((me["epi_prec@1e-3"] == 0).all()) and bool((me["ransac_inl%"] == 0).all())
    assert torch.equal(empty["M_0to1"].R.cpu(), torch.eye(3).expand(3, 3, 3)) and not bool(empty["M_0to1"].t.any())
    with pytest.raises(NotImplementedError):
        pipe.solver.loss(pred, data)


def test_estimator_drives_a_loop_written_like_the_reference_and_ends_in_the_auc():
    from glue_factory_amd.geometry import Camera, Pose
    from glue_factory_amd.metrics import pose_auc, relative_pose_error
    from glue_factory_amd.solvers.relative_pose_ransac import RelativePoseEstimator
    with pytest.raises(ValueError):
        RelativePoseEstimator({"options": {"method": "usac_magsac"}})
    est = RelativePoseEstimator({"ransac_th": ec.RANSAC_TH, "max_iters": ec.PLANTED_T, "seed": ec.SEED})
    assert est.conf.options.confidence == 0.99999
    errors = []
    for spec in ec.PLANTED + [(84, 4, 0, 300, 280)]:
        s = ec.scene(*spec)
        data = _batch([s])
        kp0, kp1, m0 = data["view0"]["cache"]["keypoints"][0], data["view1"]["cache"]["keypoints"][0], data["view0"]["cache"]["matches"][0]
        valid = m0 > -1
        out = est({"m_kpts0": kp0[valid], "m_kpts1": kp1[m0[valid]], "camera0": Camera(data["view0"]["camera"]._data[0]),
                   "camera1": Camera(data["view1"]["camera"]._data[0])})
        assert isinstance(out["success"], bool) and isinstance(out["M_0to1"], Pose) and out["inliers"].shape == (int(valid.sum()),)
        if not out["success"]:
            errors.append(float("inf"))
            continue
        t_err, r_err = relative_pose_error(Pose(data["T_0to1"]._data[0]), out["M_0to1"].R, out["M_0to1"].t)
        errors.append(float(max(t_err, r_err)))
        assert np.array_equal(out["inliers"].cpu().numpy(), s["planted"][valid.cpu().numpy()])
    assert errors[-1] == float("inf") and max(errors[:-1]) < 0.3
    assert pose_auc(errors, [5, 10, 20]) == pose_auc(torch.tensor(errors), [5, 10, 20])
    auc = pose_auc(errors, [5, 10, 20])
    print("errors", errors, "AUC@5/10/20", auc)
    assert all(0.70 < a <= 0.75 for a in auc)                     # three of four pairs solved almost exactly
