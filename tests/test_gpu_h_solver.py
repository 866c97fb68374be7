"""Homography solver kernels (csrc/h_solver.hip: gf_h_ransac, gf_h_dlt) against the fp64 restatements, planted scenes and
derived bounds of tests/h_solver_cases.py, and the host code on top of them (glue_factory_amd.solvers, metrics.homography_*,
the `solver` stage of TwoViewPipeline).  Shapes follow the kernel's tile constants (GF_H_TILE, GF_H_HYPS of the header).
Every raw call is made twice into guarded buffers and must give equal bits and leave the guards alone."""
import functools

import numpy as np
import pytest
import torch

import h_solver_cases as hc
import solver_harness as sh
from solver_harness import dev as _dev, load as _lib

pytestmark = pytest.mark.gpu

T_FULL = 2 * hc.HYPS + 5       # several workgroups of hypotheses
K_EDGES = [0, 3, 4, 5, hc.TILE - 1, hc.TILE, hc.TILE + 1]
T_EDGES = [1, hc.HYPS - 1, hc.HYPS, hc.HYPS + 1, T_FULL]


def _ransac_once(kp0, kp1, m0, T, lo_iters, seed, th):
    B, M = m0.shape
    N = kp1.shape[1]
    spec = {"H": ((B, 3, 3), torch.float32, -7.0), "inliers": ((B, M), torch.uint8, 0xAB), "num": ((B,), torch.int32, -77),
            "success": ((B,), torch.uint8, 0xAB), "samples": ((B, T, 4), torch.int32, -77), "counts": ((B, T), torch.int32, -77)}
    return sh.run_once("gf_h_ransac", "gf_h_ws_bytes", B, M, T, spec, lambda ws, nbytes, outs: (
        kp0.data_ptr(), kp1.data_ptr(), m0.data_ptr(), B, M, N, T, th, lo_iters, seed, ws, nbytes, *outs))


def ransac(kp0, kp1, m0, T, lo_iters=2, seed=hc.SEED, th=hc.TH):
    """The raw entry on numpy inputs [B,M,2], [B,N,2], [B,M]: called twice (equal bits), guards checked; numpy outputs."""
    a = (_dev(kp0, torch.float32), _dev(kp1, torch.float32), _dev(m0, torch.int64))
    return sh.run_twice(lambda: _ransac_once(*a, T, lo_iters, seed, th))


def _stack(scenes):
    return (np.stack([s["kpts0"] for s in scenes]), np.stack([s["kpts1"] for s in scenes]),
            np.stack([s["matches0"] for s in scenes]))


def _check_hypotheses(scene, pair, T, out_b):
    """Sampling bit for bit; rejections as on the host outside the decision bands; every count inside its derived band."""
    idx, corr = hc.compact(scene["kpts0"], scene["kpts1"], scene["matches0"])
    K = len(idx)
    smp = hc.samples(hc.SEED, pair, T, K)
    assert np.array_equal(out_b["samples"], smp), "samples differ from the host function"
    if K < 4:
        assert (out_b["counts"] == -1).all() and (out_b["samples"] == -1).all()
        return
    assert smp.min() >= 0 and smp.max() < K and all(len(set(r)) == 4 for r in smp.tolist())
    fit = hc.fit4(corr[smp])
    rej_gpu, rej_host = out_b["counts"] < 0, ~fit["ok"]
    differ = rej_gpu != rej_host
    assert not (differ & ~fit["band"]).any(), "a rejection differs outside the decision bands"
    print(f"pair {pair} K={K} T={T}: {int(rej_host.sum())} rejected on the host, {int(differ.sum())} decided differently in a band")
    assert differ.sum() <= 0.01 * T
    dl = hc.delta(fit, scene["range"])
    lo, hi = hc.count_band(fit["H"], corr, dl, coord_range=scene["range"])
    both = ~rej_gpu & ~rej_host
    cnt = out_b["counts"]
    bad = both & ((cnt < lo) | (cnt > hi))
    assert not bad.any(), f"{int(bad.sum())} counts outside [count(th - delta), count(th + delta)]"
    return fit


def _take(out, b):
    return {k: v[b] for k, v in out.items()}


# ---- sampling, fit and scoring at the tile edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", K_EDGES)
def test_hypotheses_at_the_correspondence_tile_edges(K):
    T = hc.HYPS + 1
    scene = hc.small_scene("proj", K, hc.TILE + 20, hc.TILE + 33, seed=K)
    out = ransac(*_stack([scene]), T)
    _check_hypotheses(scene, 0, T, _take(out, 0))
    assert bool(out["success"][0]) == bool((out["counts"][0] >= 0).any())
    if K < 4:
        assert not out["success"][0] and not out["inliers"].any() and out["num"][0] == 0
        assert np.array_equal(out["H"][0], np.eye(3, dtype=np.float32))
    assert int(out["inliers"][0].sum()) == int(out["num"][0])
    assert not out["inliers"][0][scene["matches0"] < 0].any()


@pytest.mark.parametrize("T", T_EDGES)
def test_hypotheses_at_the_workgroup_edges(T):
    K = hc.TILE + 1
    scene = hc.small_scene("affine", K, K + 20, K + 7, seed=T)
    out = ransac(*_stack([scene]), T)
    fit = _check_hypotheses(scene, 0, T, _take(out, 0))
    # the winner: the highest count, the lowest index (with lo_iters = 0 the result IS that hypothesis)
    out0 = ransac(*_stack([scene]), T, lo_iters=0)
    cnt = out0["counts"][0]
    assert np.array_equal(cnt, out["counts"][0])
    if (cnt >= 0).any():
        best = int(np.argmax(cnt))
        assert out0["success"][0] and int(out0["num"][0]) == int(cnt[best])
        # ... up to the fit's derived fp32 band, measured where the model is used: on its own inliers
        corr = hc.compact(scene["kpts0"], scene["kpts1"], scene["matches0"])[1]
        own = corr[hc.inlier_mask(fit["H"][best], corr), :2]
        # (none when the model's horizon separates its sample from the origin: with h22 = 1 every denominator is negative)
        if len(own):
            moved = np.abs(hc.warp(out0["H"][0], own) - hc.warp(fit["H"][best], own)).max()
            assert moved <= hc.delta(fit, scene["range"])[best], moved
    else:
        assert not out0["success"][0]


# ---- planted truth --------------------------------------------------------------------------------------------------------
def _filler(M, N, kind, seed):
    """A pair of the same shape with no matches ('none') or exactly four planted ones ('four')."""
    rng = np.random.RandomState(seed)
    kp0 = rng.randint(0, 256, size=(M, 2)).astype(np.float32)
    kp1 = rng.randint(0, 600, size=(N, 2)).astype(np.float32)
    m0 = np.full(M, -1, np.int64)
    planted = np.zeros(M, bool)
    if kind == "four":
        slots, partner = [3, M // 2, M - 2, 7], [N - 1, 2, N // 2, 11]
        kp0[slots] = np.array([[10, 20], [200, 30], [220, 210], [15, 180]], np.float32)
        kp1[partner] = hc.warp(hc.H_PROJ, kp0[slots].astype(np.float64)).astype(np.float32)
        m0[slots] = partner
        planted[slots] = True
    return {"kpts0": kp0, "kpts1": kp1, "matches0": m0, "planted": planted, "H": hc.H_PROJ,
            "range": float(max(kp0.max(), kp1.max()))}


def _check_planted(scene, out_b, bound):
    assert out_b["success"]
    assert np.array_equal(out_b["inliers"], scene["planted"]), "the inlier mask is not the planted set"
    assert int(out_b["num"]) == int(scene["planted"].sum())
    err = hc.corner_error(out_b["H"], scene["H"])
    print(f"corner error against the truth {err:.3e} px, bound {bound:.3e} px")
    assert out_b["H"][2, 2] == 1.0 and err < bound


@pytest.mark.parametrize("model,K,M,N", hc.PLANTED)
def test_planted_truth_single_pair(model, K, M, N):
    scene = hc.planted_scene(model, K, M, N, 0)
    out = ransac(*_stack([scene]), T_FULL)
    _check_hypotheses(scene, 0, T_FULL, _take(out, 0))
    _check_planted(scene, _take(out, 0), hc.planted_bound(model, K, M, N))


def test_planted_truth_in_a_batch_with_match_counts_0_4_K():
    model, K, M, N = hc.PLANTED[1]
    scenes = [_filler(M, N, "none", 1), _filler(M, N, "four", 2), hc.planted_scene(model, K, M, N, 2)]
    out = ransac(*_stack(scenes), T_FULL)
    for b in range(3):
        _check_hypotheses(scenes[b], b, T_FULL, _take(out, b))
    assert not out["success"][0] and out["num"][0] == 0 and not out["inliers"][0].any()
    assert np.array_equal(out["H"][0], np.eye(3, dtype=np.float32))
    four = hc.compact(scenes[1]["kpts0"], scenes[1]["kpts1"], scenes[1]["matches0"])[1]
    _check_planted(scenes[1], _take(out, 1), hc.corner_bound(four[:, :2], four[:, 2:]))
    idx, corr = hc.compact(scenes[2]["kpts0"], scenes[2]["kpts1"], scenes[2]["matches0"])
    inl = scenes[2]["planted"][idx]
    _check_planted(scenes[2], _take(out, 2), hc.corner_bound(corr[inl, :2], corr[inl, 2:]))


def test_nan_keypoints_in_unmatched_slots_change_nothing():
    model, K, M, N = hc.PLANTED[2]
    scene = hc.planted_scene(model, K, M, N, 0)
    ref = ransac(*_stack([scene]), hc.HYPS + 1)
    dirty = dict(scene, kpts0=scene["kpts0"].copy(), kpts1=scene["kpts1"].copy())
    dirty["kpts0"][scene["matches0"] < 0] = np.nan
    used = np.zeros(N, bool)
    used[scene["matches0"][scene["matches0"] >= 0]] = True
    dirty["kpts1"][~used] = np.nan
    out = ransac(*_stack([dirty]), hc.HYPS + 1)
    for k in ref:
        assert np.array_equal(ref[k], out[k]), k


# ---- DLT alone ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dlt_batch():
    """clean (40), weighted (40) and four (4) points as three pairs of M = 48 / N = 45 keypoints, scattered."""
    M, N = 48, 45
    rng = np.random.RandomState(5)
    kp0 = rng.uniform(0, 256, size=(3, M, 2)).astype(np.float32)
    kp1 = rng.uniform(0, 600, size=(3, N, 2)).astype(np.float32)
    m0 = np.full((3, M), -1, np.int64)
    wt = rng.uniform(0.1, 1, size=(3, M)).astype(np.float32)
    cases = []
    for b, name in enumerate(("clean", "weighted", "four")):
        p0, p1, w = hc.dlt_case(name)
        k = len(p0)
        slots, partner = np.sort(rng.choice(M, k, replace=False)), rng.permutation(N)[:k]
        kp0[b, slots], kp1[b, partner], m0[b, slots] = p0, p1, partner
        wt[b, slots] = 1.0 if w is None else w
        cases.append((p0, p1, wt[b, slots].copy()))
    return kp0, kp1, m0, wt, cases


@pytest.mark.parametrize("weighted", [False, True])
def test_dlt_equals_the_fp64_restatement(weighted):
    from glue_factory_amd.solvers.dlt import homography_dlt
    kp0, kp1, m0, wt, cases = _dlt_batch()
    args = (_dev(kp0, torch.float32), _dev(kp1, torch.float32), _dev(m0, torch.int64))
    H, ok = homography_dlt(*args, _dev(wt, torch.float32) if weighted else None)
    H2, ok2 = homography_dlt(*args, _dev(wt, torch.float32) if weighted else None)
    assert torch.equal(H, H2) and torch.equal(ok, ok2) and ok.dtype == torch.bool and bool(ok.all())
    H = H.cpu().numpy()
    for b, (p0, p1, w) in enumerate(cases):
        ref = hc.dlt(p0, p1, w if weighted else None)
        bound = hc.corner_bound(p0, p1, w if weighted else None)
        err = hc.corner_error(H[b], ref)
        print(f"pair {b} weighted={weighted}: corner error against the restatement {err:.3e} px, bound {bound:.3e} px")
        assert H[b][2, 2] == 1.0 and err < bound
    if weighted:                                        # the weights change the answer measurably: 'weights ignored' is caught
        p0, p1, w = cases[1]
        assert hc.corner_error(H[1], hc.dlt(p0, p1, None)) > 10 * hc.corner_bound(p0, p1, w)


def test_dlt_with_too_few_matches():
    from glue_factory_amd.solvers.dlt import homography_dlt
    kp0, kp1, m0, _, _ = _dlt_batch()
    m0 = m0.copy()
    m0[0, np.nonzero(m0[0] >= 0)[0][3:]] = -1          # 3 matches
    m0[1] = -1                                         # none
    H, ok = homography_dlt(_dev(kp0, torch.float32), _dev(kp1, torch.float32), _dev(m0, torch.int64))
    assert ok.tolist() == [False, False, True]
    assert torch.equal(H[:2].cpu(), torch.eye(3).expand(2, 3, 3))


# ---- edges ------------------------------------------------------------------------------------------------------------------
def _pair_from(p0, p1):
    k = len(p0)
    return {"kpts0": np.asarray(p0, np.float32), "kpts1": np.asarray(p1, np.float32), "matches0": np.arange(k, dtype=np.int64),
            "range": float(max(np.abs(p0).max(), np.abs(p1).max()))}


def _no_model(out):
    assert not out["success"][0] and out["num"][0] == 0 and not out["inliers"].any()
    assert np.array_equal(out["H"][0], np.eye(3, dtype=np.float32))


def test_all_points_collinear_gives_no_success():
    t = np.arange(20, dtype=np.float64)
    p0 = np.stack([10 + 8 * t, 20 + 4 * t], -1)
    scene = _pair_from(p0, hc.warp(hc.H_AFFINE, p0))
    out = ransac(*_stack([scene]), hc.HYPS + 1)
    assert (out["counts"] == -1).all()
    _no_model(out)


def test_duplicated_correspondences():
    p0 = np.array([[10.0, 20], [200, 30], [220, 210], [15, 180], [100, 90], [60, 150]])
    p0 = np.concatenate([p0, p0])
    scene = _pair_from(p0, hc.warp(hc.H_PROJ, p0))
    scene.update(planted=np.ones(12, bool), H=hc.H_PROJ)
    out = ransac(*_stack([scene]), hc.HYPS + 1)
    assert (out["counts"][0] == -1).any() and (out["counts"][0] == 12).any()     # samples with a repeated point are rejected
    _check_planted(scene, _take(out, 0), hc.corner_bound(scene["kpts0"], scene["kpts1"]))


def test_a_model_with_h22_zero_gives_no_success_and_no_nan():
    """(x, y) -> (256 - 256 / x, 16 y / x): H = [[256, 0, -256], [0, 16, 0], [1, 0, 0]] is the only model consistent with
    these exact correspondences; it keeps every orientation (so the samples pass the area tests) and its h22 is 0.  On the
    host the test |h22| >= GF_H_H22_FRAC ||H||_F rejects every sample, in fp64 and in numpy fp32, down to a fraction of 1e-6."""
    p0 = np.array([[1.0, 0], [16, 0], [1, 16], [16, 16], [4, 8], [8, 2], [2, 12], [8, 14]])
    p1 = np.stack([256 - 256 / p0[:, 0], 16 * p0[:, 1] / p0[:, 0]], -1)
    scene = _pair_from(p0, p1)
    fit = hc.fit4(hc.compact(scene["kpts0"], scene["kpts1"], scene["matches0"])[1][hc.samples(hc.SEED, 0, hc.HYPS, 8)])
    assert not fit["ok"].any()                                                    # the host rejects every sample
    out = ransac(*_stack([scene]), hc.HYPS)
    assert np.isfinite(out["H"]).all()
    _no_model(out)
    from glue_factory_amd.solvers.dlt import homography_dlt
    H, ok = homography_dlt(_dev(p0[None], torch.float32), _dev(p1[None], torch.float32), _dev(scene["matches0"][None], torch.int64))
    assert not bool(ok[0]) and torch.equal(H[0].cpu(), torch.eye(3))


# ---- rejected calls -------------------------------------------------------------------------------------------------------
def test_rejected_calls_return_their_code_and_write_nothing():
    lib, L = _lib()
    B, M, N, T = 2, 40, 30, 10
    kp0, kp1 = torch.rand(B, M, 2, device="cuda"), torch.rand(B, N, 2, device="cuda")
    m0 = torch.zeros(B, M, dtype=torch.int64, device="cuda")
    nbytes = int(L.gf_h_ws_bytes(B, M, T))
    ws = torch.full((nbytes + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    H = torch.full((B, 3, 3), -7.0, device="cuda")
    inl = torch.full((B, M), 0xAB, dtype=torch.uint8, device="cuda")
    num = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    suc = torch.full((B,), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    off = (-ws.data_ptr()) % 16                                  # a 16-byte aligned start inside the buffer
    good = dict(kp0=kp0.data_ptr(), kp1=kp1.data_ptr(), m0=m0.data_ptr(), B=B, M=M, N=N, T=T, th=3.0, lo=2, seed=1,
                ws=ws.data_ptr() + off, nbytes=nbytes, H=H.data_ptr(), inl=inl.data_ptr(), num=num.data_ptr(),
                suc=suc.data_ptr(), smp=None, cnt=None)
    shape, align = -2, -3
    bad = [({"kp0": None}, shape), ({"kp1": None}, shape), ({"m0": None}, shape), ({"ws": None}, shape), ({"H": None}, shape),
           ({"inl": None}, shape), ({"num": None}, shape), ({"suc": None}, shape), ({"B": -1}, shape), ({"B": 0}, shape),
           ({"M": -3}, shape), ({"N": 0}, shape), ({"T": 0}, shape), ({"T": -5}, shape), ({"nbytes": nbytes - 1}, shape),
           ({"nbytes": -1}, shape), ({"th": 0.0}, shape), ({"th": float("nan")}, shape), ({"lo": -1}, shape),
           ({"ws": ws.data_ptr() + off + 4}, align)]
    for change, code in bad:
        a = {**good, **change}
        got = L.gf_h_ransac(a["kp0"], a["kp1"], a["m0"], a["B"], a["M"], a["N"], a["T"], a["th"], a["lo"], a["seed"], a["ws"],
                            a["nbytes"], a["H"], a["inl"], a["num"], a["suc"], a["smp"], a["cnt"], st)
        assert got == code, (change, got)
    wt = None
    for change, code in [({"kp0": None}, shape), ({"H": None}, shape), ({"suc": None}, shape), ({"M": 0}, shape),
                         ({"nbytes": int(L.gf_h_ws_bytes(B, M, 1)) - 1}, shape), ({"ws": ws.data_ptr() + off + 8}, align)]:
        a = {**good, **change}
        got = L.gf_h_dlt(a["kp0"], a["kp1"], a["m0"], wt, a["B"], a["M"], a["N"], a["ws"], a["nbytes"], a["H"], a["suc"], st)
        assert got == code, (change, got)
    assert L.gf_h_ws_bytes(0, M, T) == 0 and L.gf_h_ws_bytes(B, -1, T) == 0 and L.gf_h_ws_bytes(B, M, 0) == 0
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and bool((H == -7.0).all()) and bool((inl == 0xAB).all())
    assert bool((num == -77).all()) and bool((suc == 0xAB).all())
    with pytest.raises(RuntimeError):
        lib.check(shape, "gf_h_ransac")


# ---- captured -------------------------------------------------------------------------------------------------------------
def test_one_call_captured_in_a_graph_equals_the_eager_call():
    from glue_factory_amd.solvers.homography_ransac import homography_ransac
    model, K, M, N = hc.PLANTED[2]
    first = [_filler(M, N, "four", 2), hc.planted_scene(model, K, M, N, 1)]
    second = [hc.planted_scene(model, K, M, N, 0), _filler(M, N, "none", 3)]
    to = lambda scenes: [_dev(a, d) for a, d in zip(_stack(scenes), (torch.float32, torch.float32, torch.int64))]
    static = to(first)
    run = lambda args: homography_ransac(*args, ransac_th=hc.TH, max_iters=hc.HYPS + 1, lo_iters=2, seed=hc.SEED)
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
        fresh = to(scenes)
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(fresh)
        for k in ("M_0to1", "inliers", "num_inliers", "success"):
            assert torch.equal(captured[k], eager[k]), k
    assert captured["success"].tolist() == [True, True]         # (first: four matches, the planted scene)


# ---- plugin surface ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pairs():
    from glue_factory_amd.synthetic import make_pairs, to_device
    d = make_pairs(3, 200, 180, dim=64, size=(640, 480), seed=4, with_gt=False)
    data = {"view0": {"image_size": d["view0"]["image_size"], "cache": {"keypoints": d["keypoints0"], "descriptors": d["descriptors0"]}},
            "view1": {"image_size": d["view1"]["image_size"], "cache": {"keypoints": d["keypoints1"], "descriptors": d["descriptors1"]}},
            "H_0to1": d["H_0to1"]}
    return to_device(data, "cuda")


def test_pipeline_with_the_solver_stage():
    from glue_factory_amd.metrics import homography_corner_error, homography_metrics
    from glue_factory_amd.pipeline import TwoViewPipeline
    data = _pairs()
    base = {"matcher": {"name": "matchers.homography_matcher", "with_reward": False}, "allow_no_extract": True}
    plain = TwoViewPipeline(base).cuda().eval()
    solved = TwoViewPipeline({**base, "solver": {"name": "solvers.homography_ransac", "max_iters": T_FULL, "seed": 3}}).cuda().eval()
    assert type(solved.solver).__name__ == "HomographyRansac" and not hasattr(plain, "solver")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pred = solved(data)
    pred0 = plain(data)
    assert torch.equal(pred["matches0"], pred0["matches0"])
    assert pred["M_0to1"].dtype == torch.float32 and pred["inliers"].dtype == torch.bool and pred["success"].dtype == torch.bool
    assert bool(pred["success"].all())
    err = homography_corner_error(pred["M_0to1"], data["H_0to1"], data["view0"]["image_size"])
    print("corner error of the pipeline's M_0to1 against H_0to1 (px):", err.tolist())
    assert bool((err < 1.0).all())
    assert torch.equal(pred["inliers"].sum(1).int(), pred["num_inliers"]) and not bool((pred["inliers"] & (pred["matches0"] < 0)).any())
    m = homography_metrics(pred, data)
    assert set(m) == {"prec@1px", "prec@3px", "num_matches", "H_error_dlt", "H_error_ransac", "ransac_inl", "ransac_inl%"}
    assert all(v.shape == (3,) for v in m.values())
    assert bool((m["prec@3px"] == 1).all()) and bool((m["prec@1px"] <= 1).all()) and bool((m["prec@1px"] > 0.3).all())
    assert torch.equal(m["num_matches"], (pred["matches0"] > -1).sum(1))
    assert bool((m["H_error_ransac"] < 1.0).all()) and bool((m["H_error_dlt"] < 1.0).all())
    assert torch.equal(m["ransac_inl"], pred["num_inliers"].float())
    assert set(homography_metrics(pred0, data)) == {"prec@1px", "prec@3px", "num_matches", "H_error_dlt"}
    # a pair without matches: precision 0, infinite errors
    empty = dict(pred, matches0=torch.full_like(pred["matches0"], -1))
    empty.update(solved.solver({**data, **empty}))
    me = homography_metrics(empty, data)
    assert bool((me["prec@3px"] == 0).all()) and bool(torch.isinf(me["H_error_dlt"]).all()) and bool(torch.isinf(me["H_error_ransac"]).all())
    assert bool((me["ransac_inl%"] == 0).all())
    # the solver has no loss: the pipeline's loss is what it was
    la, lb = solved.loss(dict(pred), data), plain.loss(dict(pred0), data)
    assert la[0].keys() == lb[0].keys() and la[0]["total"] == lb[0]["total"] and la[1] == lb[1]
    with pytest.raises(NotImplementedError):
        solved.solver.loss(pred, data)


def test_estimator_has_the_reference_shape():
    from glue_factory_amd.base_model import get_model
    from glue_factory_amd.solvers.homography_ransac import HomographyEstimator, HomographyRansac
    assert get_model("solvers.homography_ransac") is HomographyRansac
    assert get_model("glue_factory_amd.solvers.homography_ransac") is HomographyRansac
    model, K, M, N = hc.PLANTED[2]
    scene = hc.planted_scene(model, K, M, N, 0)
    idx, corr = hc.compact(scene["kpts0"], scene["kpts1"], scene["matches0"])
    est = HomographyEstimator({"ransac_th": hc.TH, "options": {"max_iters": T_FULL}, "seed": hc.SEED})
    out = est({"m_kpts0": _dev(corr[:, :2], torch.float32), "m_kpts1": _dev(corr[:, 2:], torch.float32)})
    assert out["success"] is True and out["M_0to1"].shape == (3, 3) and out["inliers"].shape == (K,)
    assert np.array_equal(out["inliers"].cpu().numpy(), scene["planted"][idx])
    assert hc.corner_error(out["M_0to1"].cpu().numpy(), scene["H"]) < hc.planted_bound(model, K, M, N)
    few = est({"m_kpts0": torch.rand(3, 2, device="cuda"), "m_kpts1": torch.rand(3, 2, device="cuda")})
    assert few["success"] is False and torch.equal(few["M_0to1"].cpu(), torch.eye(3)) and not bool(few["inliers"].any())
