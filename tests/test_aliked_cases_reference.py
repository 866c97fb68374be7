"""The restatements and bounds of tests/aliked_cases.py, held on the CPU: the fp32 run of every restatement (and the
extractor's stock formulation, where it has one) lies within the fp64 run's bound, and every named mutation leaves it.
test_gpu_aliked.py holds the kernels of csrc/aliked.hip to the same fp64 values and bounds.

The deform_conv2d restatements (extractors/aliked.py: deform_cols; tests/aliked_stubs: deform_conv2d) are checked three
ways -- F.conv2d at zero offsets, shifted convolutions at integer offsets, a direct fp64 loop at fractional offsets that
include the (-1, 0) and (H-1, H) bands.  The published torchvision operator itself is not available to these tests."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import aliked_cases as ac
from glue_factory_amd.extractors.aliked import ALIKED, deform_cols


def _standin_deform_conv2d():
    path = ac.reference_paths("")[0]
    sys.path.insert(0, path)
    try:
        saved = sys.modules.pop("torchvision", None)
        import torchvision.ops as tvo
        fn = tvo.deform_conv2d
    finally:
        sys.path.remove(path)
        for k in [k for k in sys.modules if k == "torchvision" or k.startswith("torchvision.")]:
            del sys.modules[k]
        if saved is not None:
            sys.modules["torchvision"] = saved
    return fn


def dcn_case(h, w, seed, c=3, batch=2):
    """Offsets: zero, integer, fractional, beyond the clamp (as the caller's clamp leaves them) and in each border band."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, c, h, w, generator=g)
    lim = max(h, w) / 4.0
    off = (4 * torch.randn(batch, 18, h, w, generator=g)).clamp(-lim, lim)
    off[:, :, 0, 0] = 0
    off[:, :, 1, 1] = torch.randint(-2, 3, (batch, 18), generator=g).float()
    off[0, :, 0, 1] = -0.5          # tap rows above the map: py in (-1, 0) for ky = 1
    off[0, :, h - 1, 1] = 0.5       # py in (H-1, H) for ky = 1, beyond H for ky = 2
    off[0, 0::2, 2, 0] = 0.25
    off[0, 1::2, 2, 0] = -0.75      # px in (-1, 0) for kx = 1
    off[0, 1::2, 2, w - 1] = 0.75   # px in (W-1, W) for kx = 1
    return x, off


@pytest.mark.parametrize("h,w", [(8, 8), (4, 3)])
def test_deform_cols_restatements(h, w):
    x, off = dcn_case(h, w, 5)
    ref, bound = ac.deform_cols64(x, off)
    assert ac.within(deform_cols(x, off), ref, bound)
    assert ac.within(deform_cols(x.double(), off.double()), ref, bound * 1e-6 + 1e-12)
    for m in ac.MUTATIONS["deform_cols"]:
        assert not ac.within(ac.deform_cols64(x, off, mutation=m)[0], ref, bound), m
    # the stand-in used by the reference sweep computes the same convolution
    wgt = torch.randn(5, x.shape[1], 3, 3, generator=torch.Generator().manual_seed(6)).double()
    out = _standin_deform_conv2d()(x.double(), off.double(), wgt, padding=(1, 1))
    want = (wgt.reshape(5, -1) @ ref).view(x.shape[0], 5, h, w)
    torch.testing.assert_close(out, want, rtol=1e-9, atol=1e-9)


def test_deform_cols_equals_plain_and_shifted_convolutions():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 4, 7, 6, generator=g).double()
    wgt = torch.randn(5, 4, 3, 3, generator=g).double()
    zero = torch.zeros(2, 18, 7, 6, dtype=torch.float64)
    fn = _standin_deform_conv2d()
    for dy, dx in ((0, 0), (1, -2), (-1, 1)):
        off = zero.clone()
        off[:, 0::2], off[:, 1::2] = dy, dx
        big = F.pad(x, (4, 4, 4, 4))          # integer sample points: a plain convolution over the shifted, zero-padded window
        want = F.conv2d(big[..., 3 + dy:3 + dy + 9, 3 + dx:3 + dx + 8], wgt)
        got = (wgt.reshape(5, -1) @ deform_cols(x, off)).view(2, 5, 7, 6)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(fn(x, off, wgt, padding=(1, 1)), want, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("dim", [64, 128])
def test_aggregate_restatement(dim):
    t = ac.aggregate_inputs(dim, 64, 96, seed=dim)
    feat, s8, bf, bs = ac.aggregate64(t)
    f32, s32, _, _ = ac.aggregate64(t, dt=torch.float32)
    assert ac.within(f32, feat, bf) and ac.within(s32, s8, bs)
    assert float(feat[0, :, 0, 0].abs().max()) == 0.0              # the planted all-zero pixel stays 0 (eps clamp)
    # the extractor's stock formulation, fp32
    x1, g2, g3, g4 = t["x1"], t["g2"], t["g3"], t["g4"]
    a = F.selu(F.conv2d(x1, t["w1"][:, :, None, None]))
    cat = torch.cat([a] + [F.interpolate(g, scale_factor=s, mode="bilinear", align_corners=True)
                           for g, s in ((g2, 2), (g3, 8), (g4, 32))], 1)
    assert ac.within(F.normalize(cat, p=2, dim=1), feat, bf)
    assert ac.within(F.selu(F.conv2d(cat, t["w8"][:, :, None, None])), s8, bs)
    for m in ac.MUTATIONS["aggregate"]:
        fm, sm, _, _ = ac.aggregate64(t, mutation=m)
        assert not ac.within(fm, feat, bf), m


def dkd_case(r, seed=3, h=16, w=23, batch=2):
    """Score map and selected pixels: every pixel at distance r from a border or corner, planted flat and one-hot windows."""
    g = torch.Generator().manual_seed(seed)
    score = torch.rand(batch, h, w, generator=g)
    flat_c, hot_c = (r + 3, r + 3), (h - r - 4, w - r - 4)
    score[0, flat_c[0] - r:flat_c[0] + r + 1, flat_c[1] - r:flat_c[1] + r + 1] = 0.5
    score[0, hot_c[0] - r:hot_c[0] + r + 1, hot_c[1] - r:hot_c[1] + r + 1] = 0.0
    score[0, hot_c[0], hot_c[1]] = 1.0
    pts = [flat_c, hot_c, (r, r), (r, w - 1 - r), (h - 1 - r, r), (h - 1 - r, w - 1 - r), (r, w // 2), (h - 1 - r, w // 2),
           (h // 2, r), (h // 2, w - 1 - r), (0, 0), (h - 1, w - 1), (h // 2, w // 2)]
    idx = torch.tensor([[y * w + x for y, x in pts]] * batch)
    return score, idx


@pytest.mark.parametrize("r", [2, 3])
def test_dkd_restatement_and_closed_forms(r):
    score, idx = dkd_case(r)
    ref = ac.dkd64(score, idx, r)
    f32 = ac.dkd64(score, idx, r, dt=torch.float32)
    model = ALIKED({"model_name": "aliked-t16", "pretrained": False, "nms_radius": r})
    stock = dict(zip(("kxy", "kscore", "disp"), model._refine_stock(score[:, None], idx)))
    for k, (v, bound) in ref.items():
        assert ac.within(f32[k][0], v, bound), k
        assert ac.within(stock[k], v, bound), k
    h, w = score.shape[1:]
    # flat window: residual exactly 0, dispersity = mean |grid / r|^2 = 2 (r + 1) / (3 r); bilinear score = the pixel
    kxy, disp, ksc = ref["kxy"][0][0], ref["disp"][0][0], ref["kscore"][0][0]
    assert abs(float((kxy[0, 0] + 1) / 2 * (w - 1)) - (r + 3)) < 1e-12 and abs(float((kxy[0, 1] + 1) / 2 * (h - 1)) - (r + 3)) < 1e-12
    assert abs(float(disp[0]) - 2 * (r + 1) / (3 * r)) < 1e-12 and abs(float(ksc[0]) - 0.5) < 1e-12
    # one-hot window: every other weight is exp(-10); the residual stays 0 by symmetry
    e = torch.exp(torch.tensor(-10.0, dtype=torch.float64))
    n = (2 * r + 1) ** 2
    want = float(e * n * 2 * (r + 1) / (3 * r) / (1 + (n - 1) * e))
    assert abs(float(disp[1]) - want) < 1e-12 and abs(float(ksc[1]) - 1.0) < 1e-9
    for m in ac.MUTATIONS["dkd_refine"]:
        mut = ac.dkd64(score, idx, r, mutation=m)
        assert not all(ac.within(mut[k][0], v, bound) for k, (v, bound) in ref.items()), m


@pytest.mark.parametrize("dim,M,K", [(64, 16, 3), (128, 32, 3), (128, 16, 1)])
def test_sddh_restatement(dim, M, K):
    feat, pos, wts = ac.sddh_inputs(dim, M, K, 40, seed=dim + M + K)
    ref, bound, offs = ac.sddh64(feat, pos, wts, K, M)
    assert ac.within(ac.sddh64(feat, pos, wts, K, M, dt=torch.float32)[0], ref, bound)
    torch.testing.assert_close(ref.norm(dim=-1), torch.ones(ref.shape[:2], dtype=torch.float64))
    lim = max(feat.shape[1:3]) / 4.0
    assert bool((offs.abs() == lim).any()) and bool((offs.abs() < lim).any())         # some offsets clamp ...
    assert float(bound.max()) < 0.05                                                   # ... and the bound still means something
    muts = [m for m in ac.MUTATIONS["sddh"] if K > 1 or m != "patch_clamp_w_minus_k"]
    for m in muts:
        assert not ac.within(ac.sddh64(feat, pos, wts, K, M, mutation=m)[0], ref, bound), m


def test_sddh_restatement_is_the_stock_formulation():
    """The extractor's stock description (the reference's formulation) computes what sddh64 restates."""
    model = ac.build_model({"model_name": "aliked-t16", "max_num_keypoints": 32, **ac.TOPK}).double()
    feat, pos, _ = ac.sddh_inputs(64, 16, 3, 40, seed=1)
    h, w = feat.shape[1:3]
    kxy = pos.double() / torch.tensor([w - 1.0, h - 1.0], dtype=torch.float64) * 2 - 1
    p = (kxy / 2 + 0.5) * torch.tensor([w - 1, h - 1])
    keep = ((p - p.round()).abs() > 1e-9).all(-1).all(0)        # (the round trip moves exact integers: the truncation would differ)
    with torch.no_grad():
        got = model._describe_stock(feat.double().permute(0, 3, 1, 2), kxy[:, keep])
    wts = {k: v.double() for k, v in model._sddh_weights().items()}
    ref, _, _ = ac.sddh64(feat, p[:, keep], wts, 3, 16)
    torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-9)


def test_pretrained_needs_a_local_weights_file(tmp_path, monkeypatch):
    def no_network(*a, **k):
        raise AssertionError("torch.hub was called")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_network)
    with pytest.raises(ValueError, match="weights"):
        ALIKED({"model_name": "aliked-t16"})
    with pytest.raises(FileNotFoundError):
        ALIKED({"model_name": "aliked-t16", "weights": str(tmp_path / "missing.pth")})
    src = ALIKED({"model_name": "aliked-t16", "pretrained": False})
    torch.save(src.state_dict(), tmp_path / "aliked-t16.pth")
    dst = ALIKED({"model_name": "aliked-t16", "weights": str(tmp_path / "aliked-t16.pth")})
    assert all(torch.equal(a, b) for a, b in zip(src.state_dict().values(), dst.state_dict().values()))
    with pytest.raises(NotImplementedError):
        dst.loss({}, {})


def test_threshold_mode_refuses_a_batch_with_different_counts():
    from glue_factory_amd.base_model import BatchedExtractionUnsupported
    conf, data = ac.sweep_case("threshold")
    model = ac.build_model({**conf, "max_num_keypoints": -1})          # (no n_limit cut: the counts are the images' own)
    img = torch.cat([data["image"], 0.5 * data["image"].flip(-1)])
    with torch.no_grad(), pytest.raises(BatchedExtractionUnsupported):
        model({"image": img})
