"""Wireframe extractor on the device: the four gf_wf_* entries through the C ABI against the torch form (computed on the CPU),
the three golden scenes, a captured forced-mode call, and GlueStick driven from images through TwoViewPipeline.

Sizes are the smallest at which the kernels can go wrong: L in {1, 33, 250, 512, 2048} for the cluster kernel (one, several
and the maximum number of points per thread; 2048 is the LDS limit), the chain / isolated / clique / padding / duplicate /
boundary constructions of tests/wireframe_cases.py, N in {1, 65, 1000} x n in {2, 500} for the suppress kernel (one
partial workgroup, several; one partial end-point tile), C in {64, 128, 256} x {fp32, bf16} for the descriptors, P in
{61, 3072} for the associativity (P * P not a multiple of 16; several workgroups per row block).  Every scene's decisions
are away from rounding (asserted on the CPU in tests/test_wireframe_host.py), so ids, counts, means and masks are compared
bit for bit; descriptors at rtol 1e-5 / atol 1e-6, the bound test_sample_descriptors_kernel uses for the same arithmetic."""
import numpy as np
import pytest
import torch

import wireframe_cases as wc
from conftest import load_golden

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-5, atol=1e-6)
GUARD = 64                      # elements in front of and behind every output buffer


class Guarded:
    """An output buffer between two guard zones of a sentinel value."""

    def __init__(self, shape, dtype, sentinel):
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
        self.sentinel = sentinel
        self.t = self.raw[GUARD:GUARD + n].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        raw = self.raw.cpu()
        assert (raw[:GUARD] == self.sentinel).all() and (raw[-GUARD:] == self.sentinel).all(), f"{what}: guard overwritten"
        return self.t.cpu()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ gf_wf_cluster
def _cluster_reference(lines, scores, fill, eps):
    from glue_factory_amd.lines.wireframe import _stage_torch
    b, nl = lines.shape[:2]
    kp = torch.zeros(b, 1, 2)
    points, pscores, _, _, idx, nc, new_lines = _stage_torch(
        lines, scores, kp, torch.ones(b, 1), torch.zeros(b, 1, 64), torch.zeros(b, 64, 2, 2), 8, eps, -1.0, True, fill, kp)
    return points[:, :2 * nl], pscores[:, :2 * nl], idx, nc, new_lines


def _run_cluster(lines, scores, eps, extra_rows=3):
    from glue_factory_amd import lib
    b, nl = lines.shape[:2]
    n = 2 * nl
    p = n + extra_rows
    g = torch.Generator().manual_seed(nl)
    fill = torch.rand(b, n, 2, generator=g) * 100
    idx, nc = Guarded((b, nl, 2), torch.int64, -7), Guarded((b,), torch.int64, -7)
    new_lines = Guarded((b, nl, 2, 2), torch.float32, -7.0)
    points, pscores = Guarded((b, p, 2), torch.float32, -7.0), Guarded((b, p), torch.float32, -7.0)
    dl, ds, df = lines.cuda(), scores.cuda(), fill.cuda()
    code = lib.load().gf_wf_cluster(dl.data_ptr(), ds.data_ptr(), df.data_ptr(), idx.ptr(), nc.ptr(), new_lines.ptr(), points.ptr(),
                                    pscores.ptr(), b, nl, p, float(eps), 1, _stream())
    assert code == 0
    torch.cuda.synchronize()
    got = [g_.check(k) for g_, k in ((points, "points"), (pscores, "scores"), (idx, "idx"), (nc, "nc"), (new_lines, "lines"))]
    assert (got[0][:, n:] == -7).all() and (got[1][:, n:] == -7).all()       # the keypoint rows belong to gf_wf_suppress
    want = _cluster_reference(lines, scores, fill, eps)
    for name, a, w in zip(("points", "scores", "lines_junc_idx", "num_junctions", "lines"), (got[0][:, :n], got[1][:, :n], *got[2:]), want):
        np.testing.assert_array_equal(a.numpy(), w.numpy(), err_msg=name)
    return got[3]


@pytest.mark.parametrize("name", list(wc.CLUSTER_SCENES))
def test_cluster_random_scenes(name):
    spec = wc.CLUSTER_SCENES[name]
    sc = wc.make_scene(**spec)
    nc = _run_cluster(torch.from_numpy(sc["lines"]), torch.from_numpy(sc["line_scores"]), spec.get("eps", 3))
    if spec["n_lines"] > 1:
        assert (nc < 2 * spec["n_lines"]).all() and (nc > 1).all()


@pytest.mark.parametrize("name", list(wc.CONSTRUCTED))
def test_cluster_constructed_sets(name):
    lines = torch.from_numpy(wc.CONSTRUCTED[name]())
    scores = torch.linspace(0.1, 1.0, lines.shape[1])[None]
    nc = int(_run_cluster(lines, scores, 3)[0])
    expect = {"chain": 1, "isolated": 128, "clique": 1, "padded_near_origin": 4, "duplicates": 4, "boundary_pairs": 3}
    assert nc == expect[name]


def test_cluster_rejects_more_lines_than_fit_in_lds():
    from glue_factory_amd import lib
    out = torch.full((8,), -7.0, device="cuda")
    code = lib.load().gf_wf_cluster(out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                    out.data_ptr(), out.data_ptr(), 1, 2049, 5000, 3.0, 1, _stream())
    assert code == -1
    torch.cuda.synchronize()
    assert (out == -7).all()
    from glue_factory_amd.lines.wireframe import _stage_fused
    z = torch.zeros
    with pytest.raises(RuntimeError, match="at most 2048"):
        _stage_fused(z(1, 2049, 2, 2).cuda(), z(1, 2049).cuda(), z(1, 1, 2).cuda(), z(1, 1).cuda(), z(1, 1, 64).cuda(),
                     z(1, 64, 2, 2).cuda(), 8, 3, 3.0, True, z(1, 4098, 2).cuda(), z(1, 1, 2).cuda())


# ------------------------------------------------------------------------------------------------ gf_wf_suppress
@pytest.mark.parametrize("name", list(wc.SUPPRESS_SCENES))
def test_suppress(name):
    from glue_factory_amd import lib
    spec = wc.SUPPRESS_SCENES[name]
    sc = {k: torch.from_numpy(v) for k, v in wc.make_scene(**spec).items()}
    kp, ks, lines = sc["keypoints"], sc["keypoint_scores"], sc["lines"]
    b, nk = ks.shape
    n = 2 * lines.shape[1]
    p, radius = n + nk, float(spec.get("eps", 3))
    fill = torch.rand(b, nk, 2, generator=torch.Generator().manual_seed(1)) * 50
    flag = Guarded((b, nk), torch.uint8, 9)
    points, pscores = Guarded((b, p, 2), torch.float32, -7.0), Guarded((b, p), torch.float32, -7.0)
    dk, dks, dl, df = kp.cuda(), ks.cuda(), lines.cuda(), fill.cuda()
    code = lib.load().gf_wf_suppress(dk.data_ptr(), dks.data_ptr(), dl.data_ptr(), df.data_ptr(), flag.ptr(), points.ptr(),
                                     pscores.ptr(), b, nk, n, p, n, radius, _stream())
    assert code == 0
    torch.cuda.synchronize()
    got_flag, got_p, got_s = flag.check("flag").bool(), points.check("points"), pscores.check("scores")
    want = (torch.norm(kp[:, :, None] - lines.reshape(b, n, 2)[:, None], dim=-1) < radius).any(2)
    np.testing.assert_array_equal(got_flag.numpy(), want.numpy())
    assert (got_p[:, :n] == -7).all() and (got_s[:, :n] == -7).all()          # the junction block belongs to gf_wf_cluster
    np.testing.assert_array_equal(got_p[:, n:].numpy(), torch.where(want[..., None], fill, kp).numpy())
    np.testing.assert_array_equal(got_s[:, n:].numpy(), torch.where(want, torch.zeros_like(ks), ks).numpy())
    if spec.get("plant", True):
        near = min(nk // 4, n)
        assert not want[0, near] and want[0, near + 1] and want[:, :near].all() and not want.all()


# ------------------------------------------------------------------------------------------------ gf_wf_descriptors
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ch", [64, 128, 256])
def test_descriptors(ch, dtype):
    from glue_factory_amd import lib
    from glue_factory_amd.lines.wireframe import sample_descriptors_corner_conv
    b, h, w, s, nj, nk = 2, 6, 7, 8, 13, 10
    p = nj + nk
    g = torch.Generator().manual_seed(ch)
    dense = torch.randn(b, ch, h, w, generator=g).to(dtype)
    points = torch.rand(b, p, 2, generator=g) * torch.tensor([w * s, h * s])
    # on and beyond the border of the map: the zero-padded corners (pixel centres lie at s / 2 + s k)
    edge = torch.tensor([[0, 0], [-3, 10], [3.9, 4], [4, 4.1], [w * s - 4, h * s - 4], [w * s - 0.01, 20], [w * s + 5, 20],
                         [30, h * s + 3.5], [-40, -40], [w * s + 4.5, h * s + 4.5], [2, h * s - 2], [w * s - 4.0, -3.99]])
    points[:, :6], points[:, nj:nj + 6] = edge[:6], edge[6:]
    flag = torch.zeros(b, nk, dtype=torch.bool)
    flag[:, :6], flag[1, 8] = True, True
    kdesc = torch.randn(b, nk, ch, generator=g)
    out = Guarded((b, p, ch), torch.float32, -7.0)
    dm = dense.permute(0, 2, 3, 1).contiguous().cuda()
    dp, dk, dfl = points.cuda(), kdesc.cuda(), flag.cuda()
    code = lib.load().gf_wf_descriptors(dm.data_ptr(), dp.data_ptr(), dk.data_ptr(), dfl.data_ptr(), out.ptr(), b, p, nj, h, w, ch,
                                        s, 1 if dtype == torch.bfloat16 else 0, _stream())
    assert code == 0
    torch.cuda.synchronize()
    got = out.check("descriptors")
    want = sample_descriptors_corner_conv(points, dense.float(), s).mT            # (bf16: the rounded map, in fp32)
    sampled = torch.cat([torch.ones(b, nj, dtype=torch.bool), flag], 1)
    np.testing.assert_allclose(got[sampled].numpy(), want[sampled].numpy(), **TOL)
    np.testing.assert_array_equal(got[:, nj:][~flag].numpy(), kdesc[~flag].numpy())
    assert (got[:, nj + 2].abs().sum(-1) == 0).all()                             # (-40, -40): no corner inside, a zero row
    assert 0 < int((got[sampled].abs().sum(-1) > 0).sum()) < int(sampled.sum())


# ------------------------------------------------------------------------------------------------ gf_wf_associativity
@pytest.mark.parametrize("p,nl", [(61, 24), (3072, 512)])
def test_associativity(p, nl):
    from glue_factory_amd import lib
    from glue_factory_amd.lines.wireframe import associativity_torch
    idx = torch.randint(0, p, (2, nl, 2), generator=torch.Generator().manual_seed(p))
    idx[0, 0], idx[1, 1] = torch.tensor([p - 1, 0]), torch.tensor([5, 5])
    out = Guarded((2, p, p), torch.uint8, 9)
    di = idx.cuda()
    assert lib.load().gf_wf_associativity(di.data_ptr(), out.ptr(), 2, nl, p, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.check("associativity").bool(), associativity_torch(idx, p))


# ------------------------------------------------------------------------------------------------ the whole extractor
@pytest.fixture(scope="module")
def z():
    return load_golden("wireframe")


@pytest.mark.parametrize("name", list(wc.GOLDEN_CONFS))
def test_golden_scenes_on_the_device(z, name):
    torch.manual_seed(3)
    pred = wc.run_golden(z, name, device="cuda", fused=True)
    assert all(v.is_cuda for v in pred.values())
    wc.assert_matches_golden(pred, z, name)


def _deterministic_entries(pred, n):
    """What does not depend on the random fills: decisions, merged lines, and every row that is not a fill."""
    real = pred["keypoint_scores"] != 0
    real[:, :n] = torch.arange(n, device=real.device)[None] < pred["num_junctions"][:, None]
    out = {k: pred[k].clone() for k in ("lines_junc_idx", "num_junctions", "pl_associativity", "lines", "line_scores")}
    out["real"] = real
    for k in ("keypoints", "keypoint_scores", "descriptors"):
        out[k] = torch.where(real.reshape(*real.shape, *([1] * (pred[k].dim() - 2))), pred[k], torch.zeros_like(pred[k]))
    return out


def test_forced_mode_is_captured_and_replayed_on_new_inputs(z):
    """No host synchronisation and no data-dependent shape in forced mode: the call is captured in a graph on one stream, the
    static inputs are overwritten with a second scene, and the replay equals the eager call on that scene."""
    first, second = wc.golden_tensors(z, "forced", "cuda"), wc.golden_tensors(z, "forced_nomerge", "cuda")
    static = {k: v.clone() for k, v in first.items()}
    model = wc.golden_extractor(static, force=True, merge_line_endpoints=True, fused=True)
    image = torch.zeros(2, 1, 128, 160, device="cuda")
    n = 2 * static["lines"].shape[1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model({"image": image})                                  # (library load, allocator warm-up)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = model({"image": image})
    for k in static:
        static[k].copy_(second[k])
    graph.replay()
    torch.cuda.synchronize()
    got = _deterministic_entries(captured, n)
    eager = wc.golden_extractor(second, force=True, merge_line_endpoints=True, fused=True)({"image": image})
    want = _deterministic_entries(eager, n)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert (captured["num_junctions"] < n).all() and not want["real"].all()
    assert not torch.equal(want["lines_junc_idx"].cpu(), torch.from_numpy(z["forced.out.lines_junc_idx"]))


# ------------------------------------------------------------------------------------------------ end to end
def _polyline_view(seed, shift=0.0):
    """18 segments per image that share end points (three polylines), with scores; [2,18,2,2] and [2,18]."""
    rng = np.random.RandomState(seed)
    lines = []
    for _ in range(2):
        segs = []
        for _ in range(3):
            pts = np.stack([np.linspace(14, 130, 7) + rng.uniform(-4, 4, 7), rng.uniform(12, 112, 7)], 1)
            segs += [[pts[i], pts[i + 1]] for i in range(6)]
        lines.append(np.float32(segs))
    lines = torch.from_numpy(np.stack(lines))
    lines[..., 0] += shift
    return lines, torch.from_numpy(rng.uniform(0.5, 3.0, (2, 18)).astype(np.float32))


def test_gluestick_trains_from_images_through_the_pipeline():
    from glue_factory_amd.base_model import get_model
    from glue_factory_amd.synthetic import to_device
    torch.manual_seed(0)
    n_lines = 24
    pipe = get_model("glue_factory_amd.pipeline")({
        "extractor": {"name": "glue_factory_amd.lines.wireframe", "trainable": False,
                      "point_extractor": {"name": "extractors.superpoint_open", "max_num_keypoints": 64, "force_num_keypoints": True,
                                          "dense_outputs": True, "detection_threshold": 0.0, "nms_radius": 3, "trainable": False},
                      "line_extractor": {"name": "lines.given", "max_num_lines": n_lines, "force_num_lines": True, "min_length": 15},
                      "wireframe_params": {"merge_points": True, "merge_line_endpoints": True, "nms_radius": 3}},
        "matcher": {"name": "matchers.gluestick", "GNN_layers": ["self", "cross"] * 2, "inter_supervision": None},
        "ground_truth": {"name": "matchers.homography_matcher", "use_points": True, "use_lines": True, "th_positive": 3,
                         "th_negative": 3},
    }).cuda()
    pipe.eval()
    pipe.matcher.train()
    assert pipe.extractor.batchable_views
    g = torch.Generator().manual_seed(0)
    img = torch.rand(2, 3, 128, 160, generator=g)
    size = torch.tensor([[160.0, 128.0]]).repeat(2, 1)
    (l0, s0), (l1, _) = _polyline_view(1), _polyline_view(1, shift=8.0)
    data = to_device({"view0": {"image": img, "image_size": size, "lines": l0, "line_scores": s0},
                      "view1": {"image": img.roll(8, -1), "image_size": size, "lines": l1, "line_scores": s0.clone()},
                      "H_0to1": torch.tensor([[1.0, 0, 8], [0, 1, 0], [0, 0, 1]])[None].repeat(2, 1, 1)}, "cuda")
    pred = pipe(data)
    for i in "01":
        valid, idx = pred["valid_lines" + i], pred["lines_junc_idx" + i]
        assert pred["keypoints" + i].shape == (2, 2 * n_lines + 64, 2) and pred["descriptors" + i].shape == (2, 2 * n_lines + 64, 256)
        assert pred["pl_associativity" + i].shape == (2, 112, 112) and pred["num_junctions" + i].shape == (2,)
        for b in range(2):
            real = idx[b][valid[b]]
            assert valid[b].sum() >= 12 and real.unique().numel() < 2 * int(valid[b].sum())      # a junction merges two lines
        assert (pred["num_junctions" + i] < 2 * n_lines).all()
    losses, _ = pipe.loss(pred, data)
    assert all(torch.isfinite(v).all() for v in losses.values())
    losses["total"].mean().backward()
    missing = [k for k, p_ in pipe.matcher.named_parameters() if p_.requires_grad and (p_.grad is None or not torch.isfinite(p_.grad).all())]
    assert not missing, missing
