"""Point-and-line homography solver kernels (csrc/hl_solver.hip: gf_hl_ransac) against the fp64 restatements, planted scenes and
derived bounds of tests/hl_solver_cases.py, and the host code on top of them (glue_factory_amd.solvers.
point_line_homography_ransac, metrics.point_line_homography_metrics, the `solver` stage of TwoViewPipeline).  Shapes follow the
kernel's tile constants (GF_HL_TILE, GF_HL_HYPS of the header).  Every raw call is made twice into guarded buffers with a
guarded workspace and must give equal bits and leave the guards alone."""
import functools

import numpy as np
import pytest
import torch

import hl_solver_cases as hl
import solver_harness as sh
from solver_harness import dev as _dev, load as _lib

pytestmark = pytest.mark.gpu

T_FULL = hl.T_FULL             # several workgroups of hypotheses
T_EDGES = [1, hl.HYPS - 1, hl.HYPS, hl.HYPS + 1, T_FULL]
# (K_p, K_l): each of 0, 3, 4, TILE - 1, TILE, TILE + 1 in either list, and the mixed totals 3 and 4
K_PAIRS = [(0, 0), (3, 0), (0, 3), (2, 1), (1, 2), (4, 0), (0, 4), (2, 2), (3, 1), (1, 3), (hl.TILE - 1, hl.TILE + 1),
           (hl.TILE, hl.TILE), (hl.TILE + 1, hl.TILE - 1), (hl.TILE, 0), (0, hl.TILE + 1)]
OUT_SPEC = lambda B, M, L, T: {
    "H": ((B, 3, 3), torch.float32, -7.0), "inliers": ((B, M), torch.uint8, 0xAB), "line_inliers": ((B, L), torch.uint8, 0xAB),
    "num": ((B, 2), torch.int32, -77), "success": ((B,), torch.uint8, 0xAB), "samples": ((B, T, 4), torch.int32, -77),
    "hyp_H": ((B, T, 9), torch.float32, -7.0), "counts": ((B, T, 2), torch.int32, -77)}


def run_once(B, M, L, T, spec, args):
    """sh.run_once for the four-argument workspace entry gf_hl_ws_bytes(B, M, L, T)."""
    lib, L_ = _lib()
    nbytes = int(L_.gf_hl_ws_bytes(B, M, L, T))
    assert nbytes > 0 and nbytes % 16 == 0
    ws_buf, ws = sh.guarded((nbytes,), torch.uint8, 0x5A)
    bufs = {k: sh.guarded(*v) for k, v in spec.items()}
    code = L_.gf_hl_ransac(*args(ws.data_ptr(), nbytes, [view.data_ptr() for _, view in bufs.values()]),
                           torch.cuda.current_stream().cuda_stream)
    lib.check(code, "gf_hl_ransac")
    torch.cuda.synchronize()
    sh.intact(ws_buf, 0x5A, "workspace")
    for k, (buf, _) in bufs.items():
        sh.intact(buf, spec[k][2], k)
    return {k: v[1].clone() for k, v in bufs.items()}


def ransac(scenes, T, lo_iters=2, seed=hl.SEED, th=hl.TH):
    """The raw entry on a list of scenes of one shape: called twice (equal bits), guards checked; numpy outputs.  An empty list
    (M == 0 or L == 0) is passed with NULL pointers."""
    st = lambda key, dt: _dev(np.stack([np.asarray(s[key]) for s in scenes]), dt)
    kp0, kp1, m0 = st("kpts0", torch.float32), st("kpts1", torch.float32), st("matches0", torch.int64)
    l0, l1, lm0 = st("lines0", torch.float32), st("lines1", torch.float32), st("line_matches0", torch.int64)
    B, M, N, L, L1 = len(scenes), kp0.shape[1], kp1.shape[1], l0.shape[1], l1.shape[1]
    p = lambda t, n: t.data_ptr() if n > 0 else None

    def once():
        return run_once(B, M, L, T, OUT_SPEC(B, M, L, T), lambda ws, nbytes, o: (
            p(kp0, M), p(kp1, M), p(m0, M), p(l0, L), p(l1, L), p(lm0, L), B, M, N, L, L1, T, th, lo_iters, seed, ws, nbytes,
            o[0], o[1] if M else None, o[2] if L else None, *o[3:]))

    out = sh.run_twice(once)
    assert set(np.unique(out["line_inliers"])) <= ({0, 1} if L else {0xAB})
    out["line_inliers"] = out["line_inliers"] == 1
    if M == 0:
        out["inliers"] = np.zeros((B, 0), bool)
    return out


def _take(out, b):
    return {k: v[b] for k, v in out.items()}


def _check_hypotheses(scene, pair, T, out_b):
    """Sampling bit for bit; rejections as on the host outside the decision bands (inside: at most BAND_CAP of T decided
    differently); every accepted model within the residual bound on its own sample; every pair of counts inside
    [count(th - delta), count(th + delta)] computed in fp64 from the kernel's own hyp_H."""
    ft = hl.features(scene)
    K = ft["Kp"] + ft["Kl"]
    smp = hl.samples(hl.SEED, pair, T, K)
    assert np.array_equal(out_b["samples"], smp), "samples differ from the host function"
    cnt, H = out_b["counts"], out_b["hyp_H"].astype(np.float64).reshape(T, 3, 3)
    if K < 4:
        assert (cnt == -1).all() and (smp == -1).all() and (H == 0).all()
        return None
    assert smp.min() >= 0 and smp.max() < K and all(len(set(r)) == 4 for r in smp.tolist())
    feat, isline = hl.take(ft, smp)
    fit = hl.fit(feat, isline)
    rej_gpu, rej_host = cnt[:, 0] < 0, ~fit["ok"]
    assert np.array_equal(rej_gpu, cnt[:, 1] < 0) and (H[rej_gpu] == 0).all() and (H[~rej_gpu, 2, 2] == 1).all()
    differ = rej_gpu != rej_host
    assert not (differ & ~fit["band"]).any(), "a rejection differs outside the decision bands"
    print(f"pair {pair} K_p={ft['Kp']} K_l={ft['Kl']} T={T}: {int(rej_host.sum())} rejected on the host, {int(fit['band'].sum())} in a band, "
          f"{int(differ.sum())} decided differently")
    assert differ.sum() <= hl.BAND_CAP * T
    both = ~rej_gpu & ~rej_host
    if both.any():
        resid = hl.sample_residual(H[both], feat[both], isline[both])
        bound = hl.fit_bound({k: v[both] for k, v in fit.items()}, feat[both], scene["range"])
        print(f"   {int(both.sum())} accepted: worst residual / bound {np.max(resid / bound):.3f} (worst residual {resid.max():.2e} px)")
        assert (resid <= bound).all(), "a model misses its own sample by more than the derived bound"
        lo, hi = hl.count_band(H[both], ft)
        bad = ((cnt[both] < lo) | (cnt[both] > hi)).any(-1)
        assert not bad.any(), f"{int(bad.sum())} count pairs outside [count(th - delta), count(th + delta)]"
    return fit


def _check_planted(scene, out_b, bound):
    assert out_b["success"]
    assert np.array_equal(out_b["inliers"], scene["planted"]), "the point inlier mask is not the planted set"
    assert np.array_equal(out_b["line_inliers"], scene["line_planted"]), "the line inlier mask is not the planted set"
    assert out_b["num"].tolist() == [int(scene["planted"].sum()), int(scene["line_planted"].sum())]
    err = hl.corner_error(out_b["H"], scene["H"])
    print(f"corner error against the truth {err:.3e} px, bound {bound:.3e} px")
    assert out_b["H"][2, 2] == 1.0 and err < bound


def _no_model(out_b):
    assert not out_b["success"] and out_b["num"].tolist() == [0, 0]
    assert not out_b["inliers"].any() and not out_b["line_inliers"].any()
    assert np.array_equal(out_b["H"], np.eye(3, dtype=np.float32))


# ---- sampling, fit and scoring at the tile edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("Kp,Kl", K_PAIRS)
def test_hypotheses_at_the_feature_tile_edges(Kp, Kl):
    T = hl.HYPS + 1
    M, L = (hl.TILE + 20 if Kp else 0), (hl.TILE + 9 if Kl else 0)
    if Kp == 0 and Kl == 0:
        M = 7                                                         # no match at all, points present: K = 0
    scene = hl.small_scene(Kp, Kl, M, M + 13 if M else 0, L, L + 5 if L else 0)
    out = _take(ransac([scene], T), 0)
    _check_hypotheses(scene, 0, T, out)
    assert bool(out["success"]) == bool((out["counts"][:, 0] >= 0).any())
    if Kp + Kl < 4:
        _no_model(out)
    assert out["num"].tolist() == [int(out["inliers"].sum()), int(out["line_inliers"].sum())]
    assert not out["inliers"][scene["matches0"] < 0].any() and not out["line_inliers"][scene["line_matches0"] < 0].any()


@pytest.mark.parametrize("T", T_EDGES)
def test_hypotheses_at_the_workgroup_edges(T):
    scene = hl.small_scene(40, 40, 51, 47, 45, 52, 0, T)
    out = _take(ransac([scene], T), 0)
    _check_hypotheses(scene, 0, T, out)
    # the winner: the highest total, the lowest index (with lo_iters = 0 the result IS that hypothesis, bit for bit)
    out0 = _take(ransac([scene], T, lo_iters=0), 0)
    cnt = out0["counts"]
    assert np.array_equal(cnt, out["counts"]) and np.array_equal(out0["hyp_H"], out["hyp_H"])
    if (cnt[:, 0] >= 0).any():
        best = int(np.argmax(np.where(cnt[:, 0] >= 0, cnt.sum(-1), -1)))
        assert out0["success"] and out0["num"].tolist() == cnt[best].tolist()
        assert np.array_equal(out0["H"].ravel(), out0["hyp_H"][best])
        assert out0["num"].tolist() == [int(out0["inliers"].sum()), int(out0["line_inliers"].sum())]
    else:
        _no_model(out0)


# ---- planted truth -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["points", "lines", "mixed"])
def test_planted_truth_single_pair(name):
    scene = hl.planted_scene(name)
    out = _take(ransac([scene], T_FULL), 0)
    _check_hypotheses(scene, 0, T_FULL, out)
    _check_planted(scene, out, hl.planted_bound(name))


def test_three_point_inliers_need_the_forty_line_inliers():
    """gf_h_ransac on the scene's points alone (6 matches, 3 of them on the homography) does not recover it; the new solver
    on the points and the lines does."""
    scene = hl.planted_scene("lines_needed")
    kp0, kp1, m0 = (_dev(scene[k][None], d) for k, d in (("kpts0", torch.float32), ("kpts1", torch.float32), ("matches0", torch.int64)))
    M, N, T = kp0.shape[1], kp1.shape[1], T_FULL
    spec = {"H": ((1, 3, 3), torch.float32, -7.0), "inliers": ((1, M), torch.uint8, 0xAB), "num": ((1,), torch.int32, -77),
            "success": ((1,), torch.uint8, 0xAB)}
    pts = sh.run_twice(lambda: sh.run_once("gf_h_ransac", "gf_h_ws_bytes", 1, M, T, spec, lambda ws, nbytes, o: (
        kp0.data_ptr(), kp1.data_ptr(), m0.data_ptr(), 1, M, N, T, hl.TH, 2, hl.SEED, ws, nbytes, *o, None, None)))
    err = hl.corner_error(pts["H"][0], scene["H"]) if pts["success"][0] else float("inf")
    print(f"gf_h_ransac on the points alone: success {bool(pts['success'][0])}, {int(pts['num'][0])} inliers, corner error {err:.3e} px")
    assert not (pts["success"][0] and err < 1.0)
    out = _take(ransac([scene], T_FULL), 0)
    _check_hypotheses(scene, 0, T_FULL, out)
    _check_planted(scene, out, hl.planted_bound("lines_needed"))


def test_planted_truth_in_a_batch_with_unequal_counts():
    _, _, _, M, N, L, L1, _, _ = hl.PLANTED["mixed"]
    scenes = [hl.build_scene("proj", 0, 0, M, N, L, L1, seed=1), hl.four_feature_scene(M, N, L, L1, 1),
              hl.planted_scene("mixed", 2)]
    out = ransac(scenes, T_FULL)
    for b in range(3):
        _check_hypotheses(scenes[b], b, T_FULL, _take(out, b))
    _no_model(_take(out, 0))
    _check_planted(scenes[1], _take(out, 1), hl.corner_bound(*hl.planted_features(scenes[1])))
    _check_planted(scenes[2], _take(out, 2), hl.planted_bound("mixed", 2))


# ---- edge inputs ---------------------------------------------------------------------------------------------------------------
def test_zero_length_and_non_finite_segments_and_bad_indices_are_no_matches():
    scene = hl.planted_scene("mixed")
    ref = ransac([scene], hl.HYPS + 1)
    dirty = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    free0 = np.nonzero(scene["line_matches0"] < 0)[0]
    used1 = np.zeros(len(scene["lines1"]), bool)
    used1[scene["line_matches0"][scene["line_matches0"] >= 0]] = True
    free1 = np.nonzero(~used1)[0]
    assert len(free0) >= 6 and len(free1) >= 6
    for q, (i, j) in enumerate(zip(free0[:6], free1[:6])):
        dirty["line_matches0"][i] = j
        if q == 0:
            dirty["lines0"][i, 1] = dirty["lines0"][i, 0]                               # zero length in view 0
        elif q == 1:
            dirty["lines1"][j, 1] = dirty["lines1"][j, 0] + np.float32(0.5)             # shorter than GF_HL_EPS_LEN in view 1
        elif q == 2:
            dirty["lines0"][i, 0, 1] = np.nan
        elif q == 3:
            dirty["lines1"][j, 1, 0] = np.inf
        elif q == 4:
            dirty["line_matches0"][i] = len(scene["lines1"])                            # one past the end
        else:
            dirty["line_matches0"][i] = -(2 ** 40)
    pfree = np.nonzero(scene["matches0"] < 0)[0]
    dirty["matches0"][pfree[0]], dirty["matches0"][pfree[1]] = len(scene["kpts1"]), 2 ** 40
    dirty["kpts0"][pfree[2:]] = np.nan                                                  # unmatched slots are never read
    out = ransac([dirty], hl.HYPS + 1)
    for k in ref:
        assert np.array_equal(ref[k], out[k]), k
    assert not out["line_inliers"][0][free0].any() and not out["inliers"][0][pfree].any()


def _line_scene(lines0, H):
    """Exactly these view-0 segments, matched one to one to their images under H slid along the line."""
    lines0 = np.asarray(lines0, np.float64)
    img = hl.warp(H, lines0.reshape(-1, 2)).reshape(-1, 2, 2)
    d = img[:, 1] - img[:, 0]
    lines1 = np.stack([img[:, 0] - 0.25 * d, img[:, 1] + 0.5 * d], 1)
    n = len(lines0)
    return {"kpts0": np.zeros((0, 2), np.float32), "kpts1": np.zeros((0, 2), np.float32), "matches0": np.zeros(0, np.int64),
            "lines0": lines0.astype(np.float32), "lines1": lines1.astype(np.float32), "line_matches0": np.arange(n, dtype=np.int64),
            "range": float(max(np.abs(lines0).max(), np.abs(lines1).max()))}


@pytest.mark.parametrize("kind", ["concurrent", "parallel"])
def test_four_concurrent_and_four_parallel_lines_are_rejected(kind):
    """Four lines through one point (their images meet in its image) and four parallel lines under an affine map (their
    images are parallel) leave the homography undetermined: the 8 x 9 system loses rank and a pivot falls under
    GF_HL_EPS_PIVOT.  Dyadic coordinates and the dyadic affine model: the inputs are exact."""
    if kind == "concurrent":
        c = np.array([64.0, 96.0])
        dirs = np.array([[32.0, 8], [8, 32], [-24, 16], [16, -40]])
        lines0 = np.stack([np.stack([c + 0.5 * d, c + 2 * d]) for d in dirs])
    else:
        d = np.array([48.0, 16.0])
        starts = np.array([[8.0, 8], [40, 72], [100, 30], [16, 150]])
        lines0 = np.stack([np.stack([s, s + d * k]) for s, k in zip(starts, (1, 0.5, 1.5, 2))])
    scene = _line_scene(lines0, hl.H_AFFINE)
    feat, isline = hl.take(hl.features(scene), hl.samples(hl.SEED, 0, hl.HYPS, 4))
    fit = hl.fit(feat, isline)
    assert not fit["ok"].any() and not fit["band"].any()               # the host rejects every sample, outside every band
    out = _take(ransac([scene], hl.HYPS), 0)
    assert (out["counts"] == -1).all() and np.isfinite(out["H"]).all() and (out["hyp_H"] == 0).all()
    _no_model(out)


def test_duplicated_features():
    p0 = np.array([[10.0, 20], [200, 30], [220, 210], [15, 180]])
    segs = np.array([[[30.0, 40], [90, 60]], [[150, 100], [120, 180]], [[60, 200], [130, 230]]])
    scene = _line_scene(np.concatenate([segs, segs]), hl.H_PROJ)
    p0 = np.concatenate([p0, p0])
    scene.update(kpts0=p0.astype(np.float32), kpts1=hl.warp(hl.H_PROJ, p0).astype(np.float32), matches0=np.arange(8, dtype=np.int64),
                 planted=np.ones(8, bool), line_planted=np.ones(6, bool), H=hl.H_PROJ)
    scene["range"] = float(max(scene["range"], np.abs(scene["kpts1"]).max()))
    out = _take(ransac([scene], hl.HYPS + 1), 0)
    fit = _check_hypotheses(scene, 0, hl.HYPS + 1, out)
    smp = out["samples"]
    same = lambda a, b: (a < 8 and b < 8 and a % 4 == b % 4) or (a >= 8 and b >= 8 and (a - 8) % 3 == (b - 8) % 3)
    repeated = np.array([any(same(r[i], r[j]) for i in range(4) for j in range(i)) for r in smp.tolist()])
    assert repeated.any() and (out["counts"][repeated] == -1).all()   # a sample with a repeated feature is rejected
    assert (out["counts"].sum(-1) == 14).any() and fit["ok"].any()
    _check_planted(scene, out, hl.corner_bound(*hl.planted_features(scene)))


# ---- rejected calls ------------------------------------------------------------------------------------------------------------
def test_rejected_calls_return_their_code_and_write_nothing():
    lib, L = _lib()
    B, M, N, Ln, L1, T = 2, 40, 30, 20, 25, 10
    f = lambda *s: torch.rand(*s, device="cuda")
    kp0, kp1, l0, l1 = f(B, M, 2), f(B, N, 2), f(B, Ln, 2, 2), f(B, L1, 2, 2)
    m0 = torch.zeros(B, M, dtype=torch.int64, device="cuda")
    lm0 = torch.zeros(B, Ln, dtype=torch.int64, device="cuda")
    nbytes = int(L.gf_hl_ws_bytes(B, M, Ln, T))
    ws = torch.full((nbytes + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    H = torch.full((B, 3, 3), -7.0, device="cuda")
    inl = torch.full((B, M), 0xAB, dtype=torch.uint8, device="cuda")
    linl = torch.full((B, Ln), 0xAB, dtype=torch.uint8, device="cuda")
    num = torch.full((B, 2), -77, dtype=torch.int32, device="cuda")
    suc = torch.full((B,), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    off = (-ws.data_ptr()) % 16
    good = dict(kp0=kp0.data_ptr(), kp1=kp1.data_ptr(), m0=m0.data_ptr(), l0=l0.data_ptr(), l1=l1.data_ptr(), lm0=lm0.data_ptr(),
                B=B, M=M, N=N, L=Ln, L1=L1, T=T, th=2.0, lo=2, seed=1, ws=ws.data_ptr() + off, nbytes=nbytes, H=H.data_ptr(),
                inl=inl.data_ptr(), linl=linl.data_ptr(), num=num.data_ptr(), suc=suc.data_ptr())
    shape, align = -2, -3
    bad = [({k: None}, shape) for k in ("kp0", "kp1", "m0", "l0", "l1", "lm0", "ws", "H", "inl", "linl", "num", "suc")]
    bad += [({"B": -1}, shape), ({"B": 0}, shape), ({"M": -3}, shape), ({"L": -1}, shape), ({"N": 0}, shape), ({"L1": 0}, shape),
            ({"T": 0}, shape), ({"T": -5}, shape), ({"nbytes": nbytes - 1}, shape), ({"nbytes": -1}, shape), ({"th": 0.0}, shape),
            ({"th": float("nan")}, shape), ({"th": 1e19}, shape), ({"lo": -1}, shape), ({"lo": 65}, shape),
            ({"M": 0, "L": 0}, shape),                                   # both lists empty at the C entry
            ({"nbytes": int(L.gf_hl_ws_bytes(B, M, 0, T))}, shape),      # the workspace of a smaller call
            ({"ws": ws.data_ptr() + off + 4}, align), ({"ws": ws.data_ptr() + off + 8}, align)]
    for change, code in bad:
        a = {**good, **change}
        got = L.gf_hl_ransac(a["kp0"], a["kp1"], a["m0"], a["l0"], a["l1"], a["lm0"], a["B"], a["M"], a["N"], a["L"], a["L1"], a["T"],
                             a["th"], a["lo"], a["seed"], a["ws"], a["nbytes"], a["H"], a["inl"], a["linl"], a["num"], a["suc"],
                             None, None, None, st)
        assert got == code, (change, got)
    assert L.gf_hl_ws_bytes(0, M, Ln, T) == 0 and L.gf_hl_ws_bytes(B, -1, Ln, T) == 0 and L.gf_hl_ws_bytes(B, M, -1, T) == 0
    assert L.gf_hl_ws_bytes(B, 0, 0, T) == 0 and L.gf_hl_ws_bytes(B, M, Ln, 0) == 0
    assert L.gf_hl_ws_bytes(B, M, 0, T) > 0 and L.gf_hl_ws_bytes(B, 0, Ln, T) > 0
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and bool((H == -7.0).all()) and bool((inl == 0xAB).all()) and bool((linl == 0xAB).all())
    assert bool((num == -77).all()) and bool((suc == 0xAB).all())
    with pytest.raises(RuntimeError):
        lib.check(shape, "gf_hl_ransac")


def test_both_lists_empty_answer_without_a_launch():
    from glue_factory_amd.solvers.point_line_homography_ransac import point_line_homography_ransac
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    for args in [(z(2, 0, 2), z(2, 0, 2), z(2, 0, dt=torch.long), z(2, 0, 2, 2), z(2, 0, 2, 2), z(2, 0, dt=torch.long)),
                 (z(2, 5, 2), z(2, 0, 2), z(2, 5, dt=torch.long), None, None, None),
                 (None, None, None, z(2, 3, 2, 2), z(2, 0, 2, 2), z(2, 3, dt=torch.long))]:
        out = point_line_homography_ransac(*args)
        m = 0 if args[0] is None else args[0].shape[1]
        l = 0 if args[3] is None else args[3].shape[1]
        assert out["inliers"].shape == (2, m) and out["line_inliers"].shape == (2, l)
        assert not out["success"].any() and not out["inliers"].any() and not out["line_inliers"].any()
        assert out["num_inliers"].tolist() == [0, 0] and out["num_line_inliers"].tolist() == [0, 0]
        assert torch.equal(out["M_0to1"].cpu(), torch.eye(3).expand(2, 3, 3))


# ---- captured --------------------------------------------------------------------------------------------------------------------
def _tensors(scenes):
    st = lambda key, dt: _dev(np.stack([np.asarray(s[key]) for s in scenes]), dt)
    return [st("kpts0", torch.float32), st("kpts1", torch.float32), st("matches0", torch.int64), st("lines0", torch.float32),
            st("lines1", torch.float32), st("line_matches0", torch.int64)]


def test_one_call_captured_in_a_graph_replayed_twice_equals_the_eager_call():
    from glue_factory_amd.solvers.point_line_homography_ransac import point_line_homography_ransac
    _, _, _, M, N, L, L1, _, _ = hl.PLANTED["lines_needed"]
    name = "lines_needed"
    first = [hl.four_feature_scene(M, N, L, L1, 0), hl.planted_scene(name, 1)]
    second = [hl.planted_scene(name, 0), hl.build_scene("proj", 0, 0, M, N, L, L1, seed=2)]
    static = _tensors(first)
    run = lambda args: point_line_homography_ransac(*args, ransac_th=hl.TH, max_iters=hl.HYPS + 1, lo_iters=2, seed=hl.SEED)
    run(static)                                          # warm-up outside the capture (library load)
    # The capture stream comes from the high-priority pool.  torch hands out the streams of a pool in turn and the runtime
    # spreads them over a few hardware queues, so one more draw from the default pool here would move the side stream of every
    # later test in the process onto another queue; tests that need their side stream to run BESIDE the default stream
    # (tests/test_gpu_sinkhorn_safety.py) depend on where it lands.
    side = torch.cuda.Stream(priority=-1)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        run(static)
        with torch.cuda.graph(graph, stream=side):
            captured = run(static)
    torch.cuda.current_stream().wait_stream(side)
    keys = ("M_0to1", "inliers", "line_inliers", "num_inliers", "num_line_inliers", "success")
    for scenes in (second, first):
        fresh = _tensors(scenes)
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(fresh)
        for k in keys:
            assert torch.equal(captured[k], eager[k]), k
    assert captured["success"].tolist() == [True, True]
    assert captured["num_line_inliers"].tolist() == [1, 40] and captured["num_inliers"].tolist() == [3, 3]


# ---- plugin surface --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _line_pairs():
    """Three synthetic.py pairs with points and segments, laid out as cached extractor outputs."""
    from glue_factory_amd.synthetic import make_point_line_pairs, to_device
    w, h = 640, 480
    d = make_point_line_pairs(3, 150, 60, dim=32, size=(w, h), seed=4)
    valid = torch.ones(3, 60, dtype=torch.bool)
    view = lambda i: {"image_size": d[f"view{i}"]["image_size"], "image": torch.zeros(3, 1, h, w),
                      "cache": {"keypoints": d[f"keypoints{i}"], "lines": d[f"lines{i}"], "valid_lines": valid}}
    return to_device({"view0": view(0), "view1": view(1), "H_0to1": d["H_0to1"]}, "cuda")


def test_pipeline_with_the_solver_stage_on_points_and_lines():
    from glue_factory_amd.metrics import homography_corner_error, point_line_homography_metrics
    from glue_factory_amd.pipeline import TwoViewPipeline
    data = _line_pairs()
    base = {"matcher": {"name": "matchers.homography_matcher", "with_reward": False, "use_lines": True}, "allow_no_extract": True}
    solver = {"name": "glue_factory_amd.solvers.point_line_homography_ransac", "max_iters": T_FULL, "seed": 3}
    plain = TwoViewPipeline(base).cuda().eval()
    solved = TwoViewPipeline({**base, "solver": solver}).cuda().eval()
    assert type(solved.solver).__name__ == "PointLineHomographyRansac" and solved.solver.conf.ransac_th == 2.0
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pred = solved(data)
    pred0 = plain(data)
    assert torch.equal(pred["matches0"], pred0["matches0"]) and torch.equal(pred["line_matches0"], pred0["line_matches0"])
    assert pred["M_0to1"].dtype == torch.float32 and pred["inliers"].dtype == torch.bool and pred["line_inliers"].dtype == torch.bool
    assert bool(pred["success"].all())
    err = homography_corner_error(pred["M_0to1"], data["H_0to1"], data["view0"]["image_size"])
    print("corner error of the pipeline's M_0to1 against H_0to1 (px):", err.tolist())
    print("inliers (points, lines):", pred["num_inliers"].tolist(), pred["num_line_inliers"].tolist(),
          "of", (pred["matches0"] > -1).sum(1).tolist(), (pred["line_matches0"] > -1).sum(1).tolist())
    assert bool((err < 1.0).all())
    assert torch.equal(pred["inliers"].sum(1).int(), pred["num_inliers"]) and not bool((pred["inliers"] & (pred["matches0"] < 0)).any())
    assert torch.equal(pred["line_inliers"].sum(1).int(), pred["num_line_inliers"])
    assert not bool((pred["line_inliers"] & (pred["line_matches0"] < 0)).any())
    assert bool((pred["num_line_inliers"] > 10).all()) and bool((pred["num_inliers"] > 30).all())
    m = point_line_homography_metrics(pred, data)
    assert set(m) == {"prec@1px", "prec@3px", "num_matches", "H_error_dlt", "H_error_ransac", "ransac_inl", "ransac_inl%",
                      "ransac_line_inl", "ransac_line_inl%"}
    assert all(v.shape == (3,) for v in m.values())
    assert torch.equal(m["ransac_line_inl"], pred["num_line_inliers"].float()) and bool((m["ransac_line_inl%"] <= 1).all())
    assert bool((m["ransac_line_inl%"] > 0.5).all()) and bool((m["H_error_ransac"] < 1.0).all())
    # a prediction without line keys: points alone, the same keys as the point solver's
    no_lines = {k: v for k, v in {**data, **pred0}.items() if "line" not in k}
    alone = solved.solver(no_lines)
    assert alone["line_inliers"].shape == (3, 0) and bool(alone["success"].all()) and bool((alone["num_line_inliers"] == 0).all())
    err = homography_corner_error(alone["M_0to1"], data["H_0to1"], data["view0"]["image_size"])
    assert bool((err < 1.0).all())
    # orig_lines are preferred over lines where both exist
    junk = {**data, **pred0, "orig_lines0": pred0["lines0"], "orig_lines1": pred0["lines1"],
            "lines0": torch.zeros_like(pred0["lines0"]), "lines1": torch.zeros_like(pred0["lines1"])}
    again = solved.solver(junk)
    for k in ("M_0to1", "inliers", "line_inliers", "success"):
        assert torch.equal(again[k], pred[k]), k
    with pytest.raises(NotImplementedError):
        solved.solver.loss(pred, data)


def test_estimator_loop_ends_in_the_auc_of_the_corner_error():
    from glue_factory_amd.metrics import homography_corner_error, pose_auc
    from glue_factory_amd.solvers.point_line_homography_ransac import PointLineHomographyEstimator
    from glue_factory_amd.pipeline import TwoViewPipeline
    data = _line_pairs()
    base = {"matcher": {"name": "matchers.homography_matcher", "with_reward": False, "use_lines": True}, "allow_no_extract": True}
    pred = TwoViewPipeline(base).cuda().eval()(data)
    est = PointLineHomographyEstimator({"options": {"max_iters": T_FULL}, "seed": 3})
    errors = []
    for variant in ("both", "points", "lines"):
        for b in range(3):
            m0, lm0 = pred["matches0"][b], pred["line_matches0"][b]
            d = {}
            if variant != "lines":
                d.update(m_kpts0=pred["keypoints0"][b][m0 > -1], m_kpts1=pred["keypoints1"][b][m0[m0 > -1]])
            if variant != "points":
                d.update(m_lines0=pred["lines0"][b][lm0 > -1], m_lines1=pred["lines1"][b][lm0[lm0 > -1]])
            out = est(d)
            assert out["success"] is True and out["M_0to1"].shape == (3, 3)
            assert out["inliers"].shape == (d["m_kpts0"].shape[0] if "m_kpts0" in d else 0,)
            assert out["line_inliers"].shape == (d["m_lines0"].shape[0] if "m_lines0" in d else 0,)
            errors.append(float(homography_corner_error(out["M_0to1"], data["H_0to1"][b], data["view0"]["image_size"][b])))
    print("H_error_ransac per (variant, pair):", [round(e, 3) for e in errors])
    few = est({"m_kpts0": torch.rand(2, 2, device="cuda"), "m_kpts1": torch.rand(2, 2, device="cuda"),
               "m_lines0": torch.rand(1, 2, 2, device="cuda"), "m_lines1": torch.rand(1, 2, 2, device="cuda")})
    assert few["success"] is False and torch.equal(few["M_0to1"].cpu(), torch.eye(3))
    errors.append(float("inf"))
    auc = pose_auc(errors, [1, 3, 5])
    print("AUC of H_error_ransac at 1 / 3 / 5 px:", auc)
    assert all(0.0 <= a <= 0.9 for a in auc) and auc[0] <= auc[1] <= auc[2] and auc[2] > 0.5
