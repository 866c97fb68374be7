"""The view synthesis kernels (csrc/hviews.hip) through the C ABI of include/gf_amd.h, the ops wrappers and the
data.homography_views stage on the GPU.  References, inputs, bounds: tests/homography_views_cases.py (held by
tests/test_homography_views_reference.py).  Every raw call is made twice into guarded buffers: equal bits, guards intact."""
import numpy as np
import pytest
import torch

import homography_views_cases as vc
from solver_harness import dev, guarded, intact, load

pytestmark = pytest.mark.gpu

GF_ERR_SHAPE, GF_ERR_DTYPE = -2, -4
U8, F32 = 2, 0
FILL = -7.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _twice(call, shape):
    """call(out pointer) -> error code, into a guarded buffer, twice: equal bits; -> numpy."""
    lib, _ = load()
    outs = []
    for _ in range(2):
        buf, view = guarded(shape, torch.float32, FILL)
        lib.check(call(view.data_ptr()), "view synthesis")
        torch.cuda.synchronize()
        intact(buf, FILL, "out")
        outs.append(view.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two calls differ"
    return outs[0].cpu().numpy()


def warp(src, sizes, view_src, Hinv, params, patch, finish, gray):
    _, L = load()
    S, Hm, Wm, C = src.shape
    V, (pw, ph) = len(view_src), patch
    cout = 1 if (finish and gray) else C
    d = [dev(src, torch.uint8 if src.dtype == np.uint8 else torch.float32), dev(sizes, torch.int32), dev(view_src, torch.int32),
         dev(Hinv.reshape(V, 9), torch.float32), dev(params, torch.float32)]
    code = U8 if src.dtype == np.uint8 else F32
    return _twice(lambda out: L.gf_hv_warp(d[0].data_ptr(), code, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                           d[4].data_ptr(), out, S, Hm, Wm, C, V, cout, ph, pw, int(finish), int(gray), _stream()),
                  (V, cout, ph, pw))


def filt(x, tap_off, tap_w, ntaps, params, gray):
    _, L = load()
    V, C, ph, pw = x.shape
    cout = 1 if gray else C
    d = [dev(x, torch.float32), dev(tap_off, torch.int32), dev(tap_w, torch.float32), dev(ntaps, torch.int32),
         dev(params, torch.float32)]
    return _twice(lambda out: L.gf_hv_filter(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                             out, V, C, cout, ph, pw, int(gray), _stream()), (V, cout, ph, pw))


def _within(got, ref, bound, what):
    bad, ratio = vc.violations(got, ref, bound)
    print(f"{what}: worst error / bound {ratio:.3f}, {int((~np.isfinite(bound)).sum())} pixels without a bound")
    assert np.isfinite(got).all(), what
    assert bad == 0, f"{what}: {bad} pixels outside their bound (worst ratio {ratio:.3g})"


def _case(dtype, C, patch, kind="random", params=None):
    return dict(src=vc.sources(dtype, C, kind), sizes=vc.SIZES, view_src=vc.VIEW_SRC, Hinv=vc.view_matrices(patch),
                params=np.tile(vc.IDENT_PARAMS, (6, 1)) if params is None else params, patch=patch)


# ---- warp -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("patch", vc.PATCHES)
def test_warp_against_the_restatement(dtype, C, patch):
    """Random sources in a padded buffer whose padding holds 255 / NaN, six views out of order, every photometric stage on for
    some view; finish and gray on and off."""
    case = _case(dtype, C, patch, params=vc.photometric_params())
    for finish, gray in ((False, False), (True, False), (True, True), (False, True)):
        ref, bound = vc.warp_ref(**case, finish=finish, gray=gray)
        assert np.isfinite(bound).all()
        _within(warp(**case, finish=finish, gray=gray), ref, bound, f"warp {dtype.__name__} C={C} {patch} finish={finish} gray={gray}")


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_warp_reproduces_ramps_in_closed_form(dtype):
    case = _case(dtype, 3, vc.PATCHES[2], "ramp")
    got = warp(**case, finish=False, gray=False)
    ref, bound = vc.warp_ref(**case, finish=False, gray=False)
    pw, ph = case["patch"]
    ys, xs = np.mgrid[0:ph, 0:pw].astype(np.float64)
    checked = 0
    for v, s in enumerate(vc.VIEW_SRC):
        w, h = vc.SIZES[s]
        M = case["Hinv"][v].astype(np.float64)
        d = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
        sx, sy = (M[0, 0] * xs + M[0, 1] * ys + M[0, 2]) / d, (M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) / d
        inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
        for c in range(3):
            closed = vc.ramp_value(s, c, sx, sy, dtype)
            assert (np.abs(got[v, c] - closed)[inside] <= bound[v, c][inside]).all()
        checked += int(inside.sum())
    assert checked > 1000
    _within(got, ref, bound, f"ramp {dtype.__name__}")


@pytest.mark.parametrize("C", [1, 3])
def test_identity_is_bit_equal_and_zero_outside(C):
    src = vc.sources(np.uint8, C)
    pw, ph = 40, 56                                         # larger than source 0 (37 x 29) both ways
    got = warp(src, vc.SIZES, np.array([0, 1], np.int32), np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)),
               np.tile(vc.IDENT_PARAMS, (2, 1)), (pw, ph), True, False)
    for v in range(2):
        w, h = vc.SIZES[v]
        want = np.zeros((C, ph, pw), np.float32)
        want[:, :h, :w] = np.moveaxis(src[v, :h, :w].astype(np.float32) / np.float32(255.0), -1, 0)
        assert np.array_equal(got[v].view(np.int32), want.view(np.int32))


def test_a_horizon_across_the_patch_leaves_every_output_finite():
    patch = vc.PATCHES[0]
    for dtype in (np.uint8, np.float32):
        src = vc.sources(dtype, 3)
        Hinv = np.stack([vc.horizon_matrix(patch), np.full((3, 3), np.nan, np.float32), np.zeros((3, 3), np.float32)])
        view_src = np.array([0, 1, 0], np.int32)
        params = vc.photometric_params()[3:6]
        got = warp(src, vc.SIZES, view_src, Hinv, params, patch, True, True)
        assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
        ref, bound = vc.warp_ref(src, vc.SIZES, view_src, Hinv, params, patch, True, True)
        assert (~np.isfinite(bound[0])).any() and np.isfinite(bound[0]).sum() > 100     # the horizon is there, and so is the rest
        _within(got, ref, bound, f"horizon {dtype.__name__}")
        # NaN and all-zero matrices: no pixel is sampled; what is left is the post stage of 0
        for v in (1, 2):
            assert np.abs(got[v] - np.clip(params[v, 3], 0, 1)).max() <= 8 * vc.U


def test_gamma_at_zero_and_value_shift_on_black_pixels():
    """The top-left 3 x 3 of every random source is 0: under the identity those pixels stay exactly 0 through powf and the shift."""
    for C in (1, 3):
        src = vc.sources(np.uint8, C)
        params = np.array([[0.3, -0.25, 1, 0], [0.15, -100 / 255, 1, 0]], np.float32)
        got = warp(src, vc.SIZES, np.array([0, 1], np.int32), np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)), params, (16, 16),
                   True, False)
        assert (got[:, :, :3, :3] == 0).all() and np.isfinite(got).all() and got.max() > 0.2
        ref, bound = vc.warp_ref(src, vc.SIZES, np.array([0, 1]), np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)), params, (16, 16),
                                 True, False)
        _within(got, ref, bound, f"gamma and shift C={C}")


# ---- filter ---------------------------------------------------------------------------------------------------------------------
KINDS = ["id", ("box", 3), ("box", 9), ("line", 25, "h"), ("line", 25, "v"), ("line", 25, "d"), "full"]


def _filter_case(C, ph, pw, seed=0, identity_post=False):
    rng = np.random.RandomState(seed)
    off, wgt, n = vc.tap_tables(KINDS)
    V = len(KINDS)
    params = np.tile(vc.IDENT_PARAMS, (V, 1))
    if not identity_post:
        params[:, 2] = rng.uniform(0.7, 1.0, V)
        params[:, 3] = rng.uniform(-0.4, 0.0, V)
    return dict(x=rng.uniform(0, 1, (V, C, ph, pw)).astype(np.float32), tap_off=off, tap_w=wgt, ntaps=n, params=params)


@pytest.mark.parametrize("C,ph,pw,gray", [(1, 16, 64, False), (1, 17, 65, False), (3, 13, 13, True), (3, 33, 130, False),
                                          (3, 30, 21, True)])
def test_filter_against_the_restatement(C, ph, pw, gray):
    """One tile, a tile plus one, the smallest extent (13), several tiles; box 3 / 9, 25-tap lines, 81 taps; gray epilogue."""
    case = _filter_case(C, ph, pw)
    got = filt(**case, gray=gray)
    ref, bound = vc.filter_ref(**case, gray=gray)
    _within(got, ref, bound, f"filter C={C} {ph}x{pw} gray={gray}")
    for y, x in ((0, 0), (0, pw - 1), (ph - 1, 0), (ph - 1, pw - 1)):                 # the four corners, explicitly
        assert (np.abs(got[..., y, x] - ref[..., y, x]) <= bound[..., y, x]).all()
    assert int(case["ntaps"].max()) == vc.MAXTAPS


def test_identity_tap_passes_bits_through():
    case = _filter_case(3, 20, 70, identity_post=True)
    got = filt(**case, gray=False)
    assert np.array_equal(got[0].view(np.int32), case["x"][0].view(np.int32))


# ---- rejected calls -------------------------------------------------------------------------------------------------------------
def test_rejected_calls():
    _, L = load()
    src, sz, vs = dev(vc.sources(np.uint8, 3), torch.uint8), dev(vc.SIZES, torch.int32), dev(vc.VIEW_SRC, torch.int32)
    hm, pr = dev(vc.view_matrices((40, 24)).reshape(6, 9), torch.float32), dev(vc.photometric_params(), torch.float32)
    buf, out = guarded((6, 3, 24, 40), torch.float32, FILL)
    P = lambda t: t.data_ptr()

    def w(src_p=P(src), code=U8, sz_p=P(sz), vs_p=P(vs), hm_p=P(hm), pr_p=P(pr), out_p=P(out), S=2, Hm=vc.HMAX, Wm=vc.WMAX, C=3,
          V=6, cout=3, ph=24, pw=40, finish=0, gray=0):
        return L.gf_hv_warp(src_p, code, sz_p, vs_p, hm_p, pr_p, out_p, S, Hm, Wm, C, V, cout, ph, pw, finish, gray, _stream())

    assert w() == 0
    for kw in (dict(src_p=None), dict(sz_p=None), dict(vs_p=None), dict(hm_p=None), dict(pr_p=None), dict(out_p=None),
               dict(S=0), dict(Hm=0), dict(Wm=-1), dict(V=0), dict(ph=0), dict(pw=-3), dict(C=2), dict(C=4),
               dict(cout=1), dict(finish=1, gray=1, cout=3), dict(finish=0, gray=1, cout=1), dict(C=1, cout=3, gray=1, finish=1)):
        assert w(**kw) == GF_ERR_SHAPE, kw
    assert w(code=1) == GF_ERR_DTYPE and w(code=7) == GF_ERR_DTYPE

    x = torch.rand(6, 3, 24, 40, device="cuda")
    off, wgt, n = (dev(a, t) for a, t in zip(vc.tap_tables(["id"] * 6), (torch.int32, torch.float32, torch.int32)))

    def f(x_p=P(x), off_p=P(off), wgt_p=P(wgt), n_p=P(n), pr_p=P(pr), out_p=P(out), V=6, C=3, cout=3, ph=24, pw=40, gray=0):
        return L.gf_hv_filter(x_p, off_p, wgt_p, n_p, pr_p, out_p, V, C, cout, ph, pw, gray, _stream())

    assert f() == 0
    for kw in (dict(x_p=None), dict(off_p=None), dict(wgt_p=None), dict(n_p=None), dict(pr_p=None), dict(out_p=None),
               dict(out_p=P(x)), dict(V=0), dict(ph=12), dict(pw=12), dict(ph=0), dict(C=2), dict(cout=1), dict(gray=1, cout=3),
               dict(C=1, gray=1, cout=3)):
        assert f(**kw) == GF_ERR_SHAPE, kw
    torch.cuda.synchronize()
    intact(buf, FILL, "out")

    # the wrappers raise on what they can see without a device read
    from glue_factory_amd import ops
    with pytest.raises(RuntimeError):
        ops.warp_views(src, sz, vs.long(), hm, pr, (40, 24))
    with pytest.raises(RuntimeError):
        ops.filter_views(x, off, wgt, n, pr[:, :3].contiguous())
    with pytest.raises(RuntimeError, match="bad shape"):
        ops.filter_views(x[:, :, :12].contiguous(), off, wgt, n, pr)


def test_table_values_out_of_range_are_clamped():
    """Device tables are not read on the host (include/gf_amd.h): a view_src / ntaps / offset outside its range behaves as the
    clamped value does, and nothing outside the buffers is touched (the guards of _twice)."""
    case = _case(np.uint8, 1, vc.PATCHES[1])
    ref = warp(**case, finish=True, gray=False)
    got = warp(**dict(case, view_src=np.where(vc.VIEW_SRC == 1, 9, -4).astype(np.int32)), finish=True, gray=False)
    assert np.array_equal(got, ref)
    fc = _filter_case(1, 20, 30)
    ref = filt(**fc, gray=False)
    wild = dict(fc, ntaps=np.where(fc["ntaps"] == vc.MAXTAPS, 500, fc["ntaps"]).astype(np.int32))
    wild["ntaps"][0] = -3                                               # the identity view: clamps to its one tap
    assert np.array_equal(filt(**wild, gray=False), ref)
    far = dict(fc, tap_off=np.where(np.abs(fc["tap_off"]) == vc.RADIUS, fc["tap_off"] * 1000, fc["tap_off"]).astype(np.int32))
    assert np.array_equal(filt(**far, gray=False), ref)


# ---- the stage ------------------------------------------------------------------------------------------------------------------
def _views(**conf):
    from glue_factory_amd.data.homography_views import HomographyViews
    base = {"homography": {"patch_shape": [64, 48]}, "photometric": {"name": "lg", "p": 0.95}, "seed": 5}
    base.update(conf)
    return HomographyViews(base)


def _ramp_images():
    """Two ramp sources 10 + c + x + y in one padded uint8 stack [2, 120, 100, 3] (sizes 100 x 80 and 90 x 120)."""
    sizes = [(100, 80), (90, 120)]
    img = np.full((2, 120, 100, 3), 255, np.uint8)
    for s, (w, h) in enumerate(sizes):
        ys, xs = np.mgrid[0:h, 0:w]
        img[s, :h, :w] = np.stack([10 + c + xs + ys for c in range(3)], -1)
    return torch.from_numpy(img).cuda(), sizes


def test_homography_views_batch_and_ramps():
    images, sizes = _ramp_images()
    ys, xs = np.mgrid[0:48, 0:64].astype(np.float64)
    for triplet, right_only, gray in ((False, False, False), (True, True, True)):
        conf = dict(triplet=triplet, right_only=right_only, grayscale=gray, photometric={"name": "identity", "p": 1.0})
        views = _views(**conf)
        assert not views.two_launches
        host = views.tables(sizes, padded=(100, 120))
        batch = views.run(views.upload(host), images)
        again = _views(**conf)(images, sizes)
        n = 3 if triplet else 2
        assert set(batch) == {f"view{k}" for k in range(n)} | {"original_image_size"} | (
            {"H_0to1", "H_0to2", "H_1to2"} if triplet else {"H_0to1"})
        assert batch["original_image_size"].tolist() == [list(s) for s in sizes]
        # the whole stack against the restatement on the tables that were uploaded
        ints, floats = views._segments(2, 2)
        ti, tf = views._carve(host["int"], ints), views._carve(host["float"], floats)
        assert ti["view_src"].tolist() == [0, 1] * n and (ti["ntaps"] == 1).all()
        ref, bound = vc.warp_ref(images.cpu().numpy(), ti["src_sizes"], ti["view_src"], tf["Hinv"].reshape(-1, 3, 3), tf["params"],
                                 (64, 48), True, gray)
        stack = torch.cat([batch[f"view{k}"]["image"] for k in range(n)]).cpu().numpy()
        _within(stack, ref, bound, f"stage triplet={triplet} gray={gray}")
        for k in range(n):
            view = batch[f"view{k}"]
            assert set(view) == {"image", "H_", "coords", "image_size"}
            assert view["image"].shape == (2, 1 if gray else 3, 48, 64) and view["image"].dtype == torch.float32
            assert view["H_"].shape == (2, 3, 3) and view["coords"].shape == (2, 4, 2) and view["image_size"].tolist() == [[64, 48]] * 2
            assert all(t.is_cuda and t.dtype == torch.float32 for t in view.values())
            assert torch.equal(view["image"], again[f"view{k}"]["image"]) and torch.equal(view["H_"], again[f"view{k}"]["H_"])
            # on ramp sources view_k(p) is the ramp at H_k^-1 p.  H_ is the fp32 rounding of the fp64 H whose fp64 inverse,
            # rounded to fp32, the kernel uses: M = inv(H_) differs from that table entrywise by at most
            # u |M| + u |M| |H| |M| to first order (doubled for the rest); carried through the perspective division it moves
            # the source point by (Ex, Ey), and the ramp has slope 1 / 255 along both axes
            H = view["H_"].double().cpu().numpy()
            got = view["image"].double().cpu().numpy()
            for b in range(2):
                M = np.linalg.inv(H[b])
                dM = 2 * vc.U * (np.abs(M) + np.abs(M) @ np.abs(H[b]) @ np.abs(M))
                d = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
                sx, sy = (M[0, 0] * xs + M[0, 1] * ys + M[0, 2]) / d, (M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) / d
                dd = dM[2, 0] * xs + dM[2, 1] * ys + dM[2, 2]
                Ex = (dM[0, 0] * xs + dM[0, 1] * ys + dM[0, 2] + np.abs(sx) * dd) / np.abs(d)
                Ey = (dM[1, 0] * xs + dM[1, 1] * ys + dM[1, 2] + np.abs(sy) * dd) / np.abs(d)
                w, h = sizes[b]
                inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
                assert inside.mean() > 0.9
                want = np.stack([(10 + c + sx + sy) / 255.0 for c in range(3)])
                want = (vc.GRAY[:, None, None] * want).sum(0, keepdims=True) if gray else want
                tol = (Ex + Ey) / 255.0 + bound[k * 2 + b]
                assert (np.abs(got[b] - want) <= tol)[:, inside].all(), (k, b, np.abs(got[b] - want)[:, inside].max())
        if right_only:                                                   # view 0: the whole image rescaled to the patch
            for b, (w, h) in enumerate(sizes):
                np.testing.assert_allclose(batch["view0"]["H_"][b].cpu().numpy(), np.diag([64 / w, 48 / h, 1.0]), atol=1e-6)
        if triplet:
            # H_0to1, H_0to2, H_1to2 are each solved (fp64) from the fp32 corners and rounded to fp32: entrywise u |H|.  The
            # product of two rounded matrices against the third: 2 u |H12| |H01| + u |H02|, times 8 for the normalisation by
            # the product's own h22 and the conditioning of the three 8 x 8 solves
            H01, H02, H12 = (batch[k].double() for k in ("H_0to1", "H_0to2", "H_1to2"))
            prod = H12 @ H01
            mag = (H12.abs() @ H01.abs()) / prod[:, 2:, 2:].abs()
            prod = prod / prod[:, 2:, 2:]
            excess = ((prod - H02).abs() / (8 * vc.U * (2 * mag + H02.abs()))).max().item()
            print(f"triplet consistency: worst |H12 H01 - H02| / bound = {excess:.3f}")
            assert excess <= 1


def test_seeded_reproducibility_with_the_lg_preset():
    images, sizes = _ramp_images()
    a, b = _views()(images, sizes), _views()(images, sizes)
    for k in ("view0", "view1"):
        assert torch.equal(a[k]["image"], b[k]["image"]) and torch.isfinite(a[k]["image"]).all()
    assert torch.equal(a["H_0to1"], b["H_0to1"])
    views = _views()
    first, second = views(images, sizes), views(images, sizes)
    assert not torch.equal(first["H_0to1"], second["H_0to1"])            # the generator moves on between batches


def test_captured_run_replays_on_rewritten_tables():
    images, sizes = _ramp_images()
    views = _views(grayscale=True)
    dev_tables = views.upload(views.tables(sizes, padded=(100, 120)))
    out = torch.empty(4, 1, 48, 64, device="cuda")
    scratch = torch.empty(4, 3, 48, 64, device="cuda")
    views.run(dev_tables, images, out=out, scratch=scratch)              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # (torch's own capture stream: no new stream for the suite)
        batch = views.run(dev_tables, images, out=out, scratch=scratch)
    before = out.clone()
    fresh = views.tables(sizes, padded=(100, 120))
    views.upload(fresh, into=dev_tables)                                 # in place: same addresses
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
    other = _views(grayscale=True)
    eager = other.run(other.upload(fresh), images)
    assert torch.equal(replayed, torch.cat([eager["view0"]["image"], eager["view1"]["image"]]))
    assert not torch.equal(replayed, before)
    assert batch["view1"]["image"].data_ptr() == out[2:].data_ptr() and torch.equal(batch["H_0to1"], eager["H_0to1"])


def test_two_view_pipeline_train_step():
    """One 640 x 480 pair from a textured 1024 x 768 source through SuperPoint-open -> homography ground truth -> LightGlue."""
    from glue_factory_amd.pipeline import TwoViewPipeline
    torch.manual_seed(0)
    pipe = TwoViewPipeline({
        "extractor": {"name": "extractors.superpoint_open", "max_num_keypoints": 512, "force_num_keypoints": True,
                      "detection_threshold": 0.0, "nms_radius": 3, "trainable": False},
        "ground_truth": {"name": "matchers.homography_matcher", "th_positive": 3, "th_negative": 3},
        "matcher": {"name": "matchers.lightglue", "filter_threshold": 0.1, "n_layers": 2},
    }).cuda()
    pipe.eval()
    pipe.matcher.train()
    image = torch.from_numpy(vc.textured_image(1024, 768))[None].cuda()
    views = _views(homography={"patch_shape": [640, 480], "difficulty": 0.7}, photometric={"name": "lg", "p": 0.95},
                   grayscale=True, seed=1)
    data = views(image)
    assert data["view0"]["image"].shape == (1, 1, 480, 640)
    pred = pipe(data)
    losses, _ = pipe.loss(pred, data)
    losses["total"].mean().backward()
    positives = int((pred["gt_matches0"] >= 0).sum())
    print(f"positive ground-truth matches: {positives} of 512 (recorded: {vc.TRAIN_STEP_POSITIVES})")
    assert torch.isfinite(losses["total"]).all()
    assert positives > 0
    assert all(torch.isfinite(p.grad).all() for p in pipe.matcher.parameters() if p.grad is not None)
