"""Fused close-point counts of the line ground truth (csrc/gt_lines.hip: gf_line_close_counts) behind
gt._close_point_counts_fused, gt_line_matches_from_homography / _from_pose_depth and the two ground-truth matcher plugins.
The yardstick throughout is gt._close_point_counts (the torch form) on the same CUDA tensors; equality is exact integer
equality, no tolerance and no entry left out."""
import functools
import sys

import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

B = 3
# (A, C, P): one segment against one line; ragged ends of the 256-segment / 32-line tiles on either side of 64; two line
# tiles + part of a third with more than 128 segments; full tiles only; lines longer than the 64-point chunk (5 chunks)
EDGE_SHAPES = [(1, 1, 2), (63, 65, 7), (130, 67, 50), (64, 256, 50), (5, 3, 300)]
KEEPS = ("none", "random", "all_false")


def _random_segments(b, n, g):
    """[b,n,4] segments with both end points uniform in a 1024^2 image, redrawn until every one is at least 15 px long."""
    seg = torch.rand(b, n, 4, generator=g) * 1024
    while True:
        short = (seg[..., 2:] - seg[..., :2]).norm(dim=-1) < 15
        if not bool(short.any()):
            return seg
        seg[short] = torch.rand(int(short.sum()), 4, generator=g) * 1024


def _samples(seg, npts, lo, hi):
    """npts points on every segment between the fractions lo and hi of its length: [b,n,4] -> [b,n,npts,2]."""
    t = torch.linspace(lo, hi, npts)[:, None]
    return seg[..., None, :2] + t * (seg[..., None, 2:] - seg[..., None, :2])


@functools.lru_cache(maxsize=None)
def _case(a, c, p):
    """Segments [B,a,4] and point sets [B,c,p,2]: the even lines are samples of segment (line index mod a) between 25 % and
    75 % of its length, jittered inside a disc of 2 px (so every one of them passes against its own segment: the nearest
    end is 0.25 * 15 - 2 = 1.75 px away for the shortest segment, far more than fp16 rounding there), the odd lines are
    samples of unrelated segments; plus the random 70 % keep flags."""
    g = torch.Generator().manual_seed(10000 * a + 100 * c + p)
    seg = _random_segments(B, a, g)
    own = _samples(seg[:, torch.arange(c) % a], p, 0.25, 0.75)
    r, phi = 2 * torch.rand(B, c, p, generator=g).sqrt(), 6.2831853 * torch.rand(B, c, p, generator=g)
    own = own + torch.stack([r * phi.cos(), r * phi.sin()], -1)
    other = _samples(_random_segments(B, c, g), p, 0.0, 1.0)
    pts = torch.where((torch.arange(c) % 2 == 0)[None, :, None, None], own, other)
    keep = torch.rand(B, c, p, generator=g) < 0.7
    return seg.cuda().contiguous(), pts.cuda().contiguous(), keep.cuda().contiguous()


def _keep(mode, keep):
    return {"none": None, "random": keep, "all_false": torch.zeros_like(keep)}[mode]


@functools.lru_cache(maxsize=None)
def _yardstick(a, c, p, mode):
    """The torch form on the CUDA tensors of the case: computed once, shared, never modified."""
    from glue_factory_amd.gt import _close_point_counts
    seg, pts, keep = _case(a, c, p)
    return _close_point_counts(seg, pts, 5, _keep(mode, keep))


def _check(got, ref, transposed, what=""):
    assert got.dtype == torch.int32 and got.is_contiguous(), what
    ref = ref.transpose(1, 2) if transposed else ref
    assert got.shape == ref.shape, what
    assert torch.equal(got.long(), ref), f"{what}: {int((got.long() != ref).sum())} of {ref.numel()} counts differ"


@pytest.mark.parametrize("mode", KEEPS)
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("a,c,p", EDGE_SHAPES)
def test_counts_equal_torch_form_at_tile_edges(a, c, p, transposed, mode):
    from glue_factory_amd.gt import _close_point_counts_fused
    seg, pts, keep = _case(a, c, p)
    ref = _yardstick(a, c, p, mode)
    got = _close_point_counts_fused(seg, pts, 5, _keep(mode, keep), transposed=transposed)
    print(f"A={a} C={c} P={p} keep={mode}: total {int(ref.sum())}, counts equal to P: {int((ref == p).sum())}")
    _check(got, ref, transposed)
    if mode == "none":                                # not vacuous: whole lines lie on their own segment
        assert int(ref.sum()) > 0 and int((ref == p).sum()) >= B * ((c + 1) // 2)
    elif mode == "random":
        full = _yardstick(a, c, p, "none")
        assert 0 < int(ref.sum()) < int(full.sum()) or p * c < 8
    else:
        assert int(ref.sum()) == 0


def _special_batch():
    """One batch.  Segments: 0 zero length (NaN direction); 1 horizontal, 64 px, ending in (264, 300); 2 ending in the
    origin, direction (-0.6, -0.8), 50 px; 3 generic.  Lines of 8 points: 0 non-finite and huge coordinates; 1 the
    boundaries of segment 1's test (dist_th = 5); 2 points 1e-6 px around the origin (fp16-subnormal products)."""
    nan, inf = float("nan"), float("inf")
    seg = torch.tensor([[[100.0, 100.0, 100.0, 100.0], [200.0, 300.0, 264.0, 300.0], [30.0, 40.0, 0.0, 0.0],
                         [10.5, 20.25, 500.75, 700.5]]])
    line0 = [[inf, 5.0], [5.0, -inf], [nan, nan], [1e30, 1e30], [-1e30, 3.0], [nan, 300.0], [inf, inf], [264.0, inf]]
    line1 = [[264.0, 300.0],             # along == 0, perp == 0: counts
             [264.0, 304.0],             # along == 0, |perp| = 4: counts
             [200.0, 300.0],             # |along| == len: counts
             [199.5, 300.0],             # |along| = 64.5 > len
             [264.5, 300.0],             # along = 0.5 > 0
             [230.0, 305.0],             # |perp| == dist_th: the comparison is strict
             [230.0, 295.00390625],      # |perp| = 4.99609375, the fp16 value below 5: counts
             [230.0, 295.0]]             # perp == -dist_th
    e = 1e-6
    line2 = [[e, e], [-e, -e], [e, -e], [-e, e], [0.0, 0.0], [e, 0.0], [0.0, -e], [nan, 0.0]]
    pts = torch.tensor([line0, line1, line2])[None]
    return seg.cuda(), pts.cuda()


@pytest.mark.parametrize("transposed", [False, True])
def test_special_values(transposed):
    """Zero-length segment, inf / nan / 1e30 points, fp16-subnormal products and the three boundaries of the test."""
    from glue_factory_amd.gt import _close_point_counts, _close_point_counts_fused
    seg, pts = _special_batch()
    ref = _close_point_counts(seg, pts, 5)
    print("torch form, count[segment, line]:", ref[0].tolist())
    got = _close_point_counts_fused(seg, pts, 5, transposed=transposed)
    _check(got, ref, transposed)
    # what the case is built to exercise, read off the torch form itself
    assert ref[0, 0].tolist() == [0, 0, 0]            # NaN direction: nothing counts
    assert ref[0, :, 0].tolist() == [0, 0, 0, 0]      # non-finite points count for nobody
    assert int(ref[0, 1, 1]) == 4                     # the four marked points of line 1
    # segment 2 ends in the origin: along = -(0.6 x + 0.8 y) in fp16 subnormals.  (e,e) and (e,0) and the origin itself
    # pass, (-e,-e), (0,-e) have along > 0; (e,-e): along = +2e-7 > 0, (-e,e): along = -2e-7 passes.  Flushing the
    # subnormals to zero would let all seven finite points pass.
    assert int(ref[0, 2, 2]) == 4


@pytest.mark.parametrize("dist_th", [4.298, 4.3, 5])
def test_threshold_rounding(dist_th):
    """|perp| against a threshold that is not an fp16 number: 4.298 rounds DOWN to 4.296875, so a point at exactly that
    offset separates "the scalar is rounded to fp16 first" (does not count) from "compared in fp32" (counts).  One point
    per line, so the counts show every point's verdict.  4.3 rounds up to 4.30078125 and 5 is exact: both rules agree."""
    from glue_factory_amd.gt import _close_point_counts, _close_point_counts_fused
    offs = [4.29296875, 4.296875, 4.30078125, -4.29296875, -4.296875, -4.30078125]
    seg = torch.tensor([[[100.0, 200.0, 300.0, 200.0]]]).cuda()
    pts = torch.tensor([[[[200.0, 200.0 + o]] for o in offs]]).cuda()              # [1,6,1,2]
    ref = _close_point_counts(seg, pts, dist_th)
    print(f"dist_th={dist_th}: torch form {ref[0, 0].tolist()} at offsets {offs}")
    for transposed in (False, True):
        _check(_close_point_counts_fused(seg, pts, dist_th, transposed=transposed), ref, transposed)
    assert ref[0, 0, 0] == 1 and ref[0, 0, 3] == 1
    if dist_th == 5:
        assert ref[0, 0].tolist() == [1] * 6
    else:
        assert ref[0, 0, 2] == 0 and ref[0, 0, 5] == 0


# ------------------------------------------------------------------------------------------------ whole functions
def _homography_args(device="cuda"):
    z = load_golden("gt_lines")
    t = lambda k: torch.from_numpy(z[k]).to(device)
    h, w = (int(v) for v in z["hw"])
    return (t("lines0"), t("lines1"), t("valid0"), t("valid1"), (2, 1, h, w), (2, 1, h, w), t("H"))


def _depth_args():
    from test_gt_golden import _line_depth_data
    return _line_depth_data(load_golden("gt_lines_depth"), "cuda")


def _count_kernel_calls(monkeypatch):
    from glue_factory_amd import gt
    calls = []
    inner = gt._close_point_counts_fused

    def spy(*a, **k):
        calls.append(k.get("transposed", False))
        return inner(*a, **k)
    monkeypatch.setattr(gt, "_close_point_counts_fused", spy)
    return calls


def _same(got, ref):
    for name, g, r in zip(("assignment", "matches0", "matches1"), got, ref):
        assert g.dtype == r.dtype and torch.equal(g, r), name


def test_line_gt_from_homography_fused_equals_torch_form(monkeypatch):
    from glue_factory_amd.gt import gt_line_matches_from_homography
    calls = _count_kernel_calls(monkeypatch)
    args = _homography_args()
    kw = dict(npts=50, dist_th=5, overlap_th=0.2, min_visibility_th=0.5)
    ref = gt_line_matches_from_homography(*args, **kw, fused=False)
    assert calls == []
    _same(gt_line_matches_from_homography(*args, **kw, fused=True), ref)
    _same(gt_line_matches_from_homography(*args, **kw), ref)                       # the default on a HIP device
    assert calls == [False, True] * 2
    assert int(ref[0].sum()) > 10 and int((ref[1] == -2).sum()) > 0 and int((ref[1] == -1).sum()) > 0


def test_line_gt_from_pose_depth_fused_equals_torch_form(monkeypatch):
    from glue_factory_amd.gt import gt_line_matches_from_pose_depth
    calls = _count_kernel_calls(monkeypatch)
    args = _depth_args()
    for kw in ({}, {"npts": 30, "dist_th": 3, "overlap_th": 0.4, "min_visibility_th": 0.3}):
        ref = gt_line_matches_from_pose_depth(*args, **kw, fused=False)
        _same(gt_line_matches_from_pose_depth(*args, **kw, fused=True), ref)
        _same(gt_line_matches_from_pose_depth(*args, **kw), ref)
        assert int(ref[0].sum()) > 5 and int((ref[1] == -2).sum()) > 0
    assert calls == [False, True] * 4


def test_matcher_plugins_count_with_the_kernel_and_label_the_same(monkeypatch):
    """homography_matcher and depth_matcher with use_lines: the same dicts as with the functions forced to fused=False."""
    from glue_factory_amd import gt
    from glue_factory_amd.base_model import get_model
    l0, l1, v0, v1, shape, _, H = _homography_args()
    img = torch.zeros(shape, device="cuda")
    hdata = {"H_0to1": H, "lines0": l0, "lines1": l1, "valid_lines0": v0, "valid_lines1": v1, "view0": {"image": img},
             "view1": {"image": img}}
    d0, d1, dv0, dv1, ddata = _depth_args()
    ddata = {**ddata, "lines0": d0, "lines1": d1, "valid_lines0": dv0, "valid_lines1": dv1}
    hm = get_model("matchers.homography_matcher")({"use_points": False, "use_lines": True})
    dm = get_model("matchers.depth_matcher")({"use_points": False, "use_lines": True})
    calls = _count_kernel_calls(monkeypatch)
    fused = (hm(hdata), dm(ddata))
    assert calls == [False, True] * 2
    with monkeypatch.context() as mp:
        mp.setattr(gt, "gt_line_matches_from_homography", functools.partial(gt.gt_line_matches_from_homography, fused=False))
        mp.setattr(sys.modules[type(dm).__module__], "gt_line_matches_from_pose_depth",
                   functools.partial(gt.gt_line_matches_from_pose_depth, fused=False))
        torch_form = (hm(hdata), dm(ddata))
    assert calls == [False, True] * 2                 # the forced runs did not reach the kernel
    for f, t in zip(fused, torch_form):
        assert set(f) == set(t) and "line_matches0" in f
        for k in f:
            assert f[k].dtype == t[k].dtype and torch.equal(f[k], t[k]), k
    assert int(fused[0]["line_assignment"].sum()) > 10 and int(fused[1]["line_assignment"].sum()) > 5


@pytest.mark.parametrize("side", [0, 1])
def test_empty_view_takes_the_torch_form(side, monkeypatch):
    from glue_factory_amd.gt import gt_line_matches_from_homography
    calls = _count_kernel_calls(monkeypatch)
    l0, l1, v0, v1, *rest = _homography_args()
    if side == 0:
        l0, v0 = l0[:, :0], v0[:, :0]
    else:
        l1, v1 = l1[:, :0], v1[:, :0]
    pos, m0, m1 = gt_line_matches_from_homography(l0, l1, v0, v1, *rest)
    assert calls == []
    assert pos.shape == (2, l0.shape[1], l1.shape[1]) and pos.dtype == torch.bool and pos.is_cuda


# ------------------------------------------------------------------------------------------------ memory, capture
def test_fused_counts_allocate_little():
    """B=4, A=C=512, P=50: the peak allocation above the level before the call is at most 4 x the bytes of the int32 output
    (output + the [B,A]-sized prologue tensors, with the allocator's rounding; the torch form's `rel` alone is 100 x)."""
    from glue_factory_amd.gt import _close_point_counts_fused
    b, n, p = 4, 512, 50
    g = torch.Generator().manual_seed(5)
    seg = _random_segments(b, n, g).cuda()
    pts = _samples(_random_segments(b, n, g), p, 0.0, 1.0).cuda().contiguous()
    keep = (torch.rand(b, n, p, generator=g) < 0.7).cuda()
    _close_point_counts_fused(seg[:1, :8].contiguous(), pts[:1, :8].contiguous(), 5)         # library loaded, kernel resident
    for kp, transposed in ((None, False), (keep, True)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = _close_point_counts_fused(seg, pts, 5, kp, transposed=transposed)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        out_bytes = out.numel() * out.element_size()
        print(f"peak rise {rise} bytes = {rise / out_bytes:.3f} x the output ({out_bytes} bytes)")
        assert out_bytes == b * n * n * 4 and rise <= 4 * out_bytes
        assert int(out.sum()) > 0


def test_both_count_calls_replay_in_one_graph():
    """The two calls of one step (the second transposed) captured in one graph on one stream, replayed twice on fresh input
    values: equal to the eager kernel calls and to the torch form on those values."""
    from glue_factory_amd.gt import _close_point_counts, _close_point_counts_fused
    b, n0, n1, p = 2, 130, 67, 50

    def draw(seed):
        g = torch.Generator().manual_seed(seed)
        l0, l1 = _random_segments(b, n0, g), _random_segments(b, n1, g)
        # each view's samples near the other view's segments, so that the counts are not all zero
        p1_in0 = _samples(l0[:, torch.arange(n1) % n0], p, 0.1, 0.9) + torch.rand(b, n1, p, 2, generator=g)
        p0_in1 = _samples(l1[:, torch.arange(n0) % n1], p, 0.1, 0.9) + torch.rand(b, n0, p, 2, generator=g)
        keep = torch.rand(b, n0, p, generator=g) < 0.7
        return [t.cuda().contiguous() for t in (l0, l1, p0_in1, p1_in0, keep)]

    def run(l0, l1, p0_in1, p1_in0, keep0):
        return (_close_point_counts_fused(l0, p1_in0, 5),
                _close_point_counts_fused(l1, p0_in1, 5, keep0, transposed=True))

    static = draw(1)
    run(*static)                                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(*static)
    for seed in (2, 3):
        fresh = draw(seed)
        for s, f in zip(static, fresh):
            s.copy_(f)
        for t in out:
            t.fill_(-7)                               # the replay has to write every entry
        graph.replay()
        torch.cuda.synchronize()
        eager = run(*fresh)
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]), seed
        l0, l1, p0_in1, p1_in0, keep0 = fresh
        _check(out[0], _close_point_counts(l0, p1_in0, 5), False, f"seed {seed} c0")
        _check(out[1], _close_point_counts(l1, p0_in1, 5, keep0), True, f"seed {seed} c1t")
        assert int(out[0].sum()) > 0 and int(out[1].sum()) > 0
