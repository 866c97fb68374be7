"""Fused epipolar part of the depth ground truth (csrc/gt_epi.hip: gf_gt_epi_min, gf_gt_depth_reward) behind
gt_matches_from_pose_depth_fused(epi_th=..., with_reward=...) and the depth_matcher plugin: against the reference-generated
vectors of tests/golden/gt_depth.npz and against the dense torch form (gt_matches_from_pose_depth) on the same tensors."""
import functools
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

# (m, n, seed): one and two 256-point tiles with a ragged end in either view (the reward kernel's 64-row tiles too), and a
# single point against five
EDGE_SHAPES = [(300, 257, 7), (513, 300, 11), (1, 5, 3)]
LABELS = ("assignment", "assignment_col0", "matches0", "matches1")


@functools.lru_cache(maxsize=None)
def _golden_scene():
    from test_gt_golden import _depth_data
    z = load_golden("gt_depth")
    return (z,) + tuple(_depth_data(z, "cuda"))


def _points(m, n, seed):
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([127.0, 95.0])
    kp0 = torch.rand(2, m, 2, generator=g) * scale
    kp1 = torch.rand(2, n, 2, generator=g) * scale
    return kp0.cuda(), kp1.cuda()


@functools.lru_cache(maxsize=None)
def _dense(m, n, seed, cc_th, epi_th):
    """The dense torch form on CUDA tensors, computed once per case and shared (never modified)."""
    from glue_factory_amd.gt import gt_matches_from_pose_depth
    data = _golden_scene()[3]
    kp0, kp1 = _points(m, n, seed)
    return gt_matches_from_pose_depth(kp0, kp1, data, pos_th=3.0, neg_th=2.0, epi_th=epi_th, cc_th=cc_th)


def _fused(m, n, seed, cc_th, epi_th, with_reward=False):
    from glue_factory_amd.gt import gt_matches_from_pose_depth_fused
    data = _golden_scene()[3]
    kp0, kp1 = _points(m, n, seed)
    return gt_matches_from_pose_depth_fused(kp0, kp1, data, pos_th=3.0, neg_th=2.0, cc_th=cc_th, epi_th=epi_th,
                                            with_reward=with_reward)


def test_fused_epipolar_gt_matches_reference_vectors():
    """`epi` tag of the golden (epi_th=1, cc_th=4, pos 3, neg 5; 120 x 100 points): labels and reward bit for bit.  The
    extension changes one label per view against the `cc` tag; the nearest epipolar minimum to the 5 px threshold is at
    3.6 / 10.0 px, min |epi - 5| over the 24 000 reward entries is 1.6e-3 px (fp32 error of the dense form: 4e-5 px) and
    min |dist - 9| is 0.10 (dense form on the CPU).  `plain` and `cc`: the reward without flags."""
    from glue_factory_amd.gt import gt_matches_from_pose_depth_fused
    z, kp0, kp1, data = _golden_scene()
    for tag, kw in (("plain", {}), ("cc", {"cc_th": 4.0}), ("epi", {"epi_th": 1.0, "cc_th": 4.0})):
        out = gt_matches_from_pose_depth_fused(kp0, kp1, data, pos_th=3.0, neg_th=5.0, with_reward=True, **kw)
        for k in ("assignment", "matches0", "matches1", "visible0", "visible1", "reward"):
            np.testing.assert_array_equal(out[k].cpu().numpy(), z[f"{tag}.{k}"], err_msg=f"{tag}.{k}")
    assert (z["epi.matches0"] != z["cc.matches0"]).sum() == 1 and (z["epi.matches1"] != z["cc.matches1"]).sum() == 1


@pytest.mark.parametrize("cc_th", [None, 4.0])
@pytest.mark.parametrize("m,n,seed", EDGE_SHAPES)
def test_fused_epipolar_labels_equal_dense_form(m, n, seed, cc_th):
    """neg_th = 2 px, epi_th set: the labels of the fused path equal the dense form's.  Dense form on the CPU: the
    extension flips 9 + 13 labels at 300 x 257 and 16 + 4 at 513 x 300 (8 + 13 and 10 + 4 with cc_th); the closest
    epipolar minimum of a point without depth is 0.05 px from the threshold."""
    dense = _dense(m, n, seed, cc_th, 1.0)
    fused = _fused(m, n, seed, cc_th, 1.0)
    for k in LABELS:
        assert torch.equal(fused[k], dense[k]), k
    assert "reward" not in fused
    if m > 1:
        plain = _fused(m, n, seed, cc_th, None)
        changed = int((plain["matches0"] != fused["matches0"]).sum() + (plain["matches1"] != fused["matches1"]).sum())
        print(f"labels changed by the epipolar extension: {changed}")
        assert changed >= 4
        assert torch.equal(plain["assignment"], fused["assignment"])


def _fp64_epi_and_dist(dense, kp0, kp1, data):
    """fp64 epipolar distance [B,M,N] (unmasked) and fp64 reprojection distance of the dense form's own projections."""
    from glue_factory_amd.geometry import skew_symmetric, sym_epipolar_distance_all
    c0, c1, T = data["view0"]["camera"], data["view1"]["camera"], data["T_0to1"]
    Fm = (c1.calibration_matrix().double().inverse().transpose(-1, -2) @ (skew_symmetric(T.t.double()) @ T.R.double())
          @ c0.calibration_matrix().double().inverse())
    epi = sym_epipolar_distance_all(kp0.double(), kp1.double(), Fm)
    d0 = ((dense["proj_0to1"].double()[:, :, None] - kp1.double()[:, None]) ** 2).sum(-1)
    d1 = ((kp0.double()[:, :, None] - dense["proj_1to0"].double()[:, None]) ** 2).sum(-1)
    return epi, torch.maximum(d0, d1)


@pytest.mark.parametrize("epi_th", [None, 1.0])
@pytest.mark.parametrize("m,n,seed", EDGE_SHAPES)
def test_fused_reward_equals_dense_form(m, n, seed, epi_th):
    """reward [B,M,N] equals the dense form on every entry whose fp64 epipolar distance is farther than 1e-3 px from neg_th
    and whose reprojection distance is farther than 1e-3 from pos_th^2 (an fp32 comparison closer than that to its threshold
    is not decided by either form); at most 0.1 % of the entries may be that close.  Dense form on the CPU: 5 of 154 200
    and 5 of 307 800 are."""
    data = _golden_scene()[3]
    kp0, kp1 = _points(m, n, seed)
    dense = _dense(m, n, seed, None, epi_th)
    fused = _fused(m, n, seed, None, epi_th, with_reward=True)
    assert fused["reward"].shape == (2, m, n) and fused["reward"].dtype == torch.float32
    epi, dist = _fp64_epi_and_dist(dense, kp0, kp1, data)
    near = ((epi - 2.0).abs() < 1e-3) | ((dist - 9.0).abs() < 1e-3)
    differ = fused["reward"] != dense["reward"]
    print(f"reward {m}x{n} epi_th={epi_th}: {int(near.sum())} of {near.numel()} entries near a threshold, "
          f"{int(differ.sum())} differ, {int((differ & ~near).sum())} of them away from the thresholds")
    assert int(near.sum()) <= 1e-3 * near.numel()
    assert not bool((differ & ~near).any())
    for k in LABELS:
        assert torch.equal(fused[k], dense[k]), k


@pytest.mark.parametrize("flags", [False, True])
@pytest.mark.parametrize("m,n", [(2048, 2048), (700, 1025), (1, 1)])
def test_epi_min_kernel_against_fp64(m, n, flags):
    """gf_gt_epi_min alone, both directions, on points uniform in a 1024^2 image (F from the golden's pose and cameras
    rescaled to f = 800, c = 512; flags drawn with probability 0.02): against the fp64 dense minimum on the same fp32
    inputs.  Bound per entry: the larger of 1e-4 relative (the project's fp32 standard) and 4 x the largest error of the
    fp32 dense torch form against fp64 on these inputs -- another order of the same handful of fp32 operations errs by the
    same order.  +inf exactly where the dense form has it."""
    from glue_factory_amd.geometry import Camera, sym_epipolar_distance_all
    from glue_factory_amd.gt import epi_min, fundamental_matrix
    data = _golden_scene()[3]
    cam = Camera(torch.tensor([[1024.0, 1024.0, 800.0, 800.0, 512.0, 512.0]] * 2, device="cuda"))
    Fm = fundamental_matrix(cam, cam, data["T_0to1"]).contiguous()
    g = torch.Generator().manual_seed(1000 * m + n)
    p0 = (torch.rand(2, m, 2, generator=g) * 1024).cuda()
    p1 = (torch.rand(2, n, 2, generator=g) * 1024).cuda()
    f0 = (torch.rand(2, m, generator=g) < 0.02).cuda() if flags else None
    f1 = (torch.rand(2, n, generator=g) < 0.02).cuda() if flags else None
    mask = (f0[:, :, None] & f1[:, None]) if flags else torch.ones(2, m, n, dtype=torch.bool, device="cuda")

    def dense_minima(dtype):
        e = sym_epipolar_distance_all(p0.to(dtype), p1.to(dtype), Fm.to(dtype))
        e = torch.where(mask, e, torch.full_like(e, float("inf")))
        return e.min(-1).values, e.min(-2).values

    ref = dense_minima(torch.float64)
    f32 = dense_minima(torch.float32)
    got = (epi_min(p0, p1, Fm, f0, f1), epi_min(p1, p0, Fm.transpose(-1, -2).contiguous(), f1, f0))
    for name, r, d, o in zip(("0->1", "1->0"), ref, f32, got):
        fin = torch.isfinite(r)
        assert torch.equal(torch.isinf(o) & (o > 0), ~fin), name
        if not bool(fin.any()):
            continue
        dense_err = float((d[fin].double() - r[fin]).abs().max())
        err = (o[fin].double() - r[fin]).abs()
        bound = torch.maximum(1e-4 * r[fin].abs(), torch.full_like(err, 4 * dense_err))
        print(f"epi_min {name} {m}x{n} flags={flags}: max |err| {float(err.max()):.3e} px, fp32 dense form {dense_err:.3e} px, "
              f"max relative {float((err / r[fin].abs().clamp(min=1e-30)).max()):.3e}")
        assert bool((err <= bound).all()), name


def _big_scene(b, n, seed):
    """The golden's depth scene repeated to batch b with n random keypoints per view."""
    from glue_factory_amd.geometry import Camera, Pose
    data = _golden_scene()[3]
    rep = lambda t: t.repeat((b // 2,) + (1,) * (t.dim() - 1))
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([127.0, 95.0])
    kp0 = (torch.rand(b, n, 2, generator=g) * scale).cuda()
    kp1 = (torch.rand(b, n, 2, generator=g) * scale).cuda()
    big = {"view0": {"camera": Camera(rep(data["view0"]["camera"]._data)), "depth": rep(data["view0"]["depth"])},
           "view1": {"camera": Camera(rep(data["view1"]["camera"]._data)), "depth": rep(data["view1"]["depth"])},
           "T_0to1": Pose(rep(data["T_0to1"]._data))}
    return kp0, kp1, big


@pytest.mark.parametrize("with_reward", [False, True])
def test_depth_matcher_memory_with_th_epi(with_reward):
    """B=4, M=N=2048, th_epi=5 through the plugin: the peak allocation above the level before the call stays under one
    fp32 [B,M,N] tensor without the reward (only the bool `assignment` is dense) and under two with it (the reward itself
    is one).  The dense form holds at least five."""
    from glue_factory_amd.base_model import get_model
    b, n = 4, 2048
    kp0, kp1, data = _big_scene(b, n, 5)
    model = get_model("matchers.depth_matcher")({"th_epi": 5.0, "with_reward": with_reward})
    inp = {**data, "keypoints0": kp0, "keypoints1": kp1}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pred = model(inp)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    dense_bytes = b * n * n * 4
    print(f"peak allocation with_reward={with_reward}: {peak / dense_bytes:.3f} x B*M*N*4 bytes")
    assert peak < (2 if with_reward else 1) * dense_bytes
    assert ("reward" in pred) == with_reward and pred["assignment"].shape == (b, n, n)
    assert int((pred["matches0"] == -1).sum()) > 0 and int((pred["matches0"] >= 0).sum()) > 0


def test_depth_matcher_plugin_takes_the_fused_path_with_th_epi(monkeypatch):
    """The configuration of the reference's MegaDepth yamls (th_epi set, reward on) through the plugin on CUDA: the `epi`
    vectors bit for bit, without reaching the dense form."""
    from glue_factory_amd import gt
    from glue_factory_amd.base_model import get_model
    z, kp0, kp1, data = _golden_scene()
    model = get_model("matchers.depth_matcher")({"th_epi": 1.0, "th_consistency": 4.0})

    def dense_form(*a, **k):
        raise AssertionError("the plugin fell back to the dense form")
    monkeypatch.setattr(gt, "gt_matches_from_pose_depth", dense_form)
    monkeypatch.setattr(sys.modules[type(model).__module__], "gt_matches_from_pose_depth", dense_form)
    pred = model({**data, "keypoints0": kp0, "keypoints1": kp1})
    for k in ("matches0", "matches1", "assignment", "reward"):
        np.testing.assert_array_equal(pred[k].cpu().numpy(), z[f"epi.{k}"], err_msg=k)


def test_fundamental_matrix_and_wrappers_replay_in_a_graph():
    """F from cameras + pose (no library inverse, no host read), gf_gt_epi_min both ways and gf_gt_depth_reward captured in
    one graph on one stream, inputs prepared beforehand: the replay reproduces the eager result."""
    from glue_factory_amd.gt import depth_reward, epi_min, fundamental_matrix, gt_matches_from_pose_depth_fused
    _, kp0, kp1, data = _golden_scene()
    pre = gt_matches_from_pose_depth_fused(kp0, kp1, data, pos_th=3.0, neg_th=5.0, cc_th=4.0)
    kp0, kp1 = kp0.float().contiguous(), kp1.float().contiguous()
    p01, p10 = (torch.nan_to_num(pre[k].float(), nan=0.0).contiguous() for k in ("proj_0to1", "proj_1to0"))
    v0, v1 = pre["visible0"].contiguous(), pre["visible1"].contiguous()
    f0, f1 = pre["matches0"] == -2, pre["matches1"] == -2

    def run():
        Fm = fundamental_matrix(data["view0"]["camera"], data["view1"]["camera"], data["T_0to1"]).contiguous()
        return (Fm, epi_min(kp0, kp1, Fm, f0, f1), epi_min(kp1, kp0, Fm.transpose(-1, -2).contiguous(), f1, f0),
                depth_reward(kp0, p01, kp1, p10, v0, v1, Fm, 3.0, 5.0, f0, f1))

    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for t in out:
        t.fill_(-7.0)                      # whatever the capture pass left: the replay has to write every entry
    graph.replay()
    torch.cuda.synchronize()
    for name, a, e in zip(("F", "min0", "min1", "reward"), out, eager):
        assert torch.equal(a, e), name
    np.testing.assert_array_equal(eager[3].cpu().numpy(), _golden_scene()[0]["epi.reward"])
