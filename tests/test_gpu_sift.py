"""csrc/sift.hip on the device: every entry through the C ABI against the fp64 restatement of tests/sift_cases.py, fed the
stock path's tensors for the previous stage, called twice for equal bits, with guard bands around every output; then the
module: fused against stock, a captured forced-count call, the integer shift and one TwoViewPipeline train step."""
import ctypes
import os

import numpy as np
import pytest
import torch

import homography_views_cases as vc
import sift_cases as sc
from conftest import GOLDEN
from solver_harness import dev, guarded, intact, load

pytestmark = pytest.mark.gpu

NAMES = ["plain", "odd", "early", "coarse"]
_cache = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _case(name):
    """(restatement, stock fp32 pyramid on the CPU, stock candidate rows) of a case image."""
    if name not in _cache:
        from glue_factory_amd.extractors import sift as S
        img = sc.case_images()[NAMES.index(name)]
        gauss, dog = S.build_pyramid(torch.from_numpy(img).float()[None], -1, 4)
        m = S.SIFT({"nms_radius": None, "max_num_keypoints": None, "rootsift": False})
        meta, vals = m._detect_stock(dog)
        ok = meta[0, :, 0] >= 0
        _cache[name] = (sc.ref_keypoints(img), img, gauss, dog, meta[0][ok], vals[0][ok])
    return _cache[name]


# ------------------------------------------------------------------------------------------------ gf_sift_blur
def _blur(src, h, w, mode, sigma, want_dog, want_copy):
    """src [B,hs,ws] on the device -> dict of outputs; called twice, guards checked."""
    lib, L = load()
    b, hs, ws = src.shape
    outs = []
    for _ in range(2):
        dbuf, dst = guarded((b, h, w), torch.float32, -7.0)
        gbuf, dogt = guarded((b, h, w), torch.float32, -7.0)
        cbuf, cpy = guarded((b, h, w), torch.float32, -7.0)
        code = L.gf_sift_blur(src.data_ptr(), dst.data_ptr(), dogt.data_ptr() if want_dog else None, cpy.data_ptr() if want_copy else None,
                              b, hs, ws, h, w, hs * ws, h * w, h * w, mode, float(sigma), _stream())
        lib.check(code, "gf_sift_blur")
        torch.cuda.synchronize()
        for buf, what in ((dbuf, "dst"), (gbuf, "dog"), (cbuf, "src_copy")):
            intact(buf, -7.0, what)
        if not want_dog:
            assert bool((dogt == -7.0).all())
        if not want_copy:
            assert bool((cpy == -7.0).all())
        outs.append((dst.clone(), dogt.clone(), cpy.clone()))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    return [t.cpu().double().numpy() for t in outs[0]]


def _blur_bound(sigma, upsample=False):
    r = int(np.ceil(4 * sigma))
    return (2 * (r + 2) + (4 if upsample else 0)) * sc.U * sc.VMAX


@pytest.mark.parametrize("name", NAMES[:3] + ["tile", "tile+1"])
def test_blur_three_variants(name):
    from glue_factory_amd.extractors import sift as S
    if name in NAMES:
        img = sc.case_images()[NAMES.index(name)]
    else:
        img = sc.make_image(32, 64 if name == "tile" else 65, 7, margin=8.0)[0]
    img32 = np.stack([img, img[::-1].copy()]).astype(np.float32)
    h, w = img.shape
    # base level: through the 2 x upsampling
    s0 = S.base_sigma(-1)
    dst, _, _ = _blur(dev(img32, torch.float32), 2 * h, 2 * w, 1, s0, False, False)
    for b in range(2):
        ref = sc.ref_blur(sc.ref_upsample2(img32[b].astype(np.float64)), s0)
        assert np.abs(dst[b] - ref).max() <= _blur_bound(s0, True)
    # plain levels with the DoG write, every increment (radii 5 .. 13)
    level = dst.astype(np.float32)
    for i in range(1, 6):
        si = S.increment_sigma(i)
        dst, dog, _ = _blur(dev(level, torch.float32), 2 * h, 2 * w, 0, si, True, False)
        for b in range(2):
            ref = sc.ref_blur(level[b].astype(np.float64), si)
            assert np.abs(dst[b] - ref).max() <= _blur_bound(si)
            assert np.abs(dog[b] - (ref - level[b])).max() <= _blur_bound(si) + sc.U * sc.VMAX
        if i == 3:
            third = dst.astype(np.float32)
        level = dst.astype(np.float32)
    # octave base: every second pixel of level 3
    s1 = S.increment_sigma(1)
    dst, dog, cpy = _blur(dev(third, torch.float32), h, w, 2, s1, True, True)
    for b in range(2):
        sub = third[b, ::2, ::2].astype(np.float64)
        assert sub.shape == (h, w) and np.array_equal(cpy[b], sub)
        ref = sc.ref_blur(sub, s1)
        assert np.abs(dst[b] - ref).max() <= _blur_bound(s1)
        assert np.abs(dog[b] - (ref - sub)).max() <= _blur_bound(s1) + sc.U * sc.VMAX
    # the same from a source of the image's own size: odd sides for "odd" (61 x 97 -> 31 x 49), "early" and "tile+1"
    hh, ww = (h + 1) // 2, (w + 1) // 2
    dst, dog, cpy = _blur(dev(img32, torch.float32), hh, ww, 2, s1, True, True)
    for b in range(2):
        sub = img32[b, ::2, ::2].astype(np.float64)
        assert sub.shape == (hh, ww) and np.array_equal(cpy[b], sub)
        ref = sc.ref_blur(sub, s1)
        assert np.abs(dst[b] - ref).max() <= _blur_bound(s1)
        assert np.abs(dog[b] - (ref - sub)).max() <= _blur_bound(s1) + sc.U * sc.VMAX


def test_blur_rejects_radius_17_and_bad_shapes():
    lib, L = load()
    x = torch.zeros((1, 16, 16), device="cuda")
    y = torch.zeros((1, 32, 32), device="cuda")
    call = lambda src, dst, dog, hs, ws, h, w, mode, sigma: L.gf_sift_blur(src.data_ptr(), dst.data_ptr(), dog, None, 1, hs, ws, h, w, hs * ws, h * w,   # noqa: E731
                                                                            h * w, mode, sigma, _stream())
    assert call(x, x.clone(), None, 16, 16, 16, 16, 0, 4.0) == 0             # radius 16
    assert call(x, x.clone(), None, 16, 16, 16, 16, 0, 4.2) == -1            # radius 17: GF_ERR_UNSUPPORTED
    assert call(x, y, None, 16, 16, 32, 32, 0, 1.0) == -2                    # mode 0 needs equal sizes
    assert call(x, y, y.data_ptr(), 16, 16, 32, 32, 1, 1.0) == -2            # no DoG level for the base
    assert call(y, x, None, 32, 32, 15, 16, 2, 1.0) == -2
    assert call(x, x.clone(), None, 16, 16, 16, 16, 3, 1.0) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ gf_sift_extrema
def _extrema(dog, cap):
    """dog: list of [1,5,h,w] CPU tensors -> (count, meta [cap,4], vals [cap,4]); called twice."""
    lib, L = load()
    res = []
    for _ in range(2):
        cbuf, count = guarded((1,), torch.int32, 0)
        mbuf, meta = guarded((1, max(cap, 1), 4), torch.int32, -9)
        vbuf, vals = guarded((1, max(cap, 1), 4), torch.float32, -9.0)
        for o, d in enumerate(dog):
            d = d.cuda().contiguous()
            h, w = d.shape[-2:]
            n = int(L.gf_sift_extrema_ws_ints(1, h, w))
            wbuf, ws = guarded((n,), torch.int32, -5)
            lib.check(L.gf_sift_extrema(d.data_ptr(), 1, h, w, o, sc.THR, sc.EDGE, ws.data_ptr(), count.data_ptr(), meta.data_ptr(),
                                        vals.data_ptr(), cap, _stream()), "gf_sift_extrema")
            torch.cuda.synchronize()
            intact(wbuf, -5, "workspace")
        intact(mbuf, -9, "meta")
        intact(vbuf, -9.0, "vals")
        res.append((int(count[0]), meta[0].cpu().clone(), vals[0].cpu().clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2].view(torch.int32), res[1][2].view(torch.int32))
    return res[0]


@pytest.mark.parametrize("name", NAMES)
def test_extrema_against_the_restatement(name):
    (gauss_r, dog_r, cands), _, gauss, dog, meta_s, vals_s = _case(name)
    count, meta, vals = _extrema(dog, 256)
    assert 3 <= count <= 256
    rows = [tuple(int(v) for v in r) for r in meta[:count]]
    by_cell = {(c["octave"],) + tuple(int(v) for v in c["cell"]): c for c in sc.accepted(cands)}
    undecided = {(c["octave"],) + tuple(int(v) for v in c.get("cell", c["cell0"])) for c in cands if not sc.decisive(c)}
    undecided |= {(c["octave"],) + tuple(int(v) for v in c["cell0"]) for c in cands if not sc.decisive(c)}
    for cell, c in by_cell.items():
        assert not sc.decisive(c) or cell in rows, cell                      # every decisive candidate is present
    stayed = []
    for i, cell in enumerate(rows):
        assert cell in by_cell or cell in undecided, cell                    # nothing the restatement rejects decisively
        c = by_cell.get(cell)
        if c is not None and sc.decisive(c):
            assert np.all(np.abs(vals[i, :3].double().numpy() - c["offset"]) <= c["offset_band"] + 4 * sc.U)
            assert abs(float(vals[i, 3]) - c["dhat"]) <= 3 * sc.e_dog(c["octave"])
            if tuple(c["cell"]) == tuple(c["cell0"]):
                stayed.append(cell)
    if name == "coarse":                                                     # the count is carried over every octave
        assert len({r[0] for r in rows}) >= 3 and sum(r[0] >= 2 for r in rows) >= 3
    assert stayed == sorted(stayed) and len(stayed) >= 2                     # ascending (octave, layer, y, x)
    assert (meta[count:] == -9).all()
    # the stock path's list from the same DoG tensors: same rows in the same order
    assert rows == [tuple(int(v) for v in r) for r in meta_s]
    # a cap below the total: the count keeps counting, the list holds the first `cap` rows
    cap = count - 2
    count2, meta2, vals2 = _extrema(dog, cap)
    assert count2 == count > cap and torch.equal(meta2, meta[:cap]) and torch.equal(vals2, vals[:cap])


def test_extrema_applies_the_prefilter():
    """sift_cases.prefilter_stack(): a cell under 0.8 thr whose fitted value passes the contrast test; the restatement
    accepts it only without the prefilter, and the kernel's list is the restatement's with it."""
    D, cell = sc.prefilter_stack()
    acc = lambda cands: [(0,) + tuple(int(v) for v in c["cell"]) for c in cands if c["accepted"]]   # noqa: E731
    with_pf, without = acc(sc.ref_detect(D)), acc(sc.ref_detect(D, prefilter=0.0))
    assert (0,) + cell in without and (0,) + cell not in with_pf
    count, meta, _ = _extrema([torch.from_numpy(D).float()[None]], 16)
    assert [tuple(int(v) for v in r) for r in meta[:count]] == with_pf and count == len(with_pf) >= 1


def test_extrema_constant_image_and_bad_arguments():
    lib, L = load()
    dog = [torch.zeros((1, 5, 20, 31)), torch.full((1, 5, 9, 10), 0.3)]
    count, meta, _ = _extrema(dog, 8)
    assert count == 0 and (meta == -9).all()
    d = dog[0].cuda()
    ws = torch.zeros(64, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.gf_sift_extrema(d.data_ptr(), 1, 2, 31, 0, sc.THR, sc.EDGE, ws.data_ptr(), cnt.data_ptr(), None, None, 0, _stream()) == -2
    assert L.gf_sift_extrema(d.data_ptr(), 1, 20, 31, 8, sc.THR, sc.EDGE, ws.data_ptr(), cnt.data_ptr(), None, None, 0, _stream()) == -2
    assert L.gf_sift_extrema(d.data_ptr(), 1, 20, 31, 0, sc.THR, sc.EDGE, ws.data_ptr(), cnt.data_ptr(), None, None, 4, _stream()) == -2
    assert L.gf_sift_extrema_ws_ints(1, 20, 31) == (3 * 18 * 29 + 255) // 256
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ gf_sift_orient / describe
def _geometry(gauss):
    dg = [g.cuda().contiguous() for g in gauss]
    ptrs = (ctypes.c_void_p * len(dg))(*[g.data_ptr() for g in dg])
    hw = (ctypes.c_int * (2 * len(dg)))(*[v for g in dg for v in g.shape[-2:]])
    return dg, ptrs, hw


def _keypoints(name):
    """Stock candidates of a case image plus keypoints whose windows cross the border, as per-keypoint arrays."""
    (gauss_r, _, cands), _, gauss, _, meta, vals = _case(name)
    octv, layer, yi, xi = [meta[:, k].clone() for k in range(4)]
    s_o = layer.float() + vals[:, 2]
    sigma = 1.6 * torch.exp2(s_o / 3)
    lvl = torch.round(s_o).long().clamp(0, 5)
    xo, yo = xi.float() + vals[:, 0], yi.float() + vals[:, 1]
    h1, w1 = gauss[1].shape[-2:]
    extra = [(1, 2, 2, 2, 2.9), (1, 1, w1 - 2, h1 - 3, 2.2), (0, 3, 4, gauss[0].shape[-2] - 3, 3.4), (len(gauss) - 1, 2, 3, 3, 2.0)]
    for o, l, x, y, s in extra:
        octv, lvl, xi, yi = [torch.cat([t, torch.tensor([v])]) for t, v in ((octv, o), (lvl, l), (xi, x), (yi, y))]
        sigma, xo, yo = [torch.cat([t, torch.tensor([v], dtype=torch.float32)]) for t, v in ((sigma, s), (xo, x + 0.3), (yo, y - 0.2))]
    if len(octv) % 4 == 0:                                                   # not a multiple of the waves per workgroup
        octv, lvl, xi, yi, sigma, xo, yo = [torch.cat([t, t[:1]]) for t in (octv, lvl, xi, yi, sigma, xo, yo)]
    return gauss, octv, lvl, xi, yi, sigma, xo, yo


@pytest.mark.parametrize("name", NAMES)
def test_orient_and_describe_against_the_restatement(name):
    lib, L = load()
    gauss, octv, lvl, xi, yi, sigma, xo, yo = _keypoints(name)
    n = len(octv)
    assert n % 4 != 0
    dg, ptrs, hw = _geometry(gauss)
    i32 = lambda t: t.to(torch.int32).cuda().contiguous()   # noqa: E731
    d_oct, d_lvl, d_xi, d_yi, d_sig = i32(octv), i32(lvl), i32(xi), i32(yi), sigma.cuda()
    res = []
    for _ in range(2):
        obuf, ori = guarded((1, n, 2), torch.float32, -7.0)
        vbuf, valid = guarded((1, n, 2), torch.int32, -7)
        lib.check(L.gf_sift_orient(ptrs, hw, len(dg), d_oct.data_ptr(), d_lvl.data_ptr(), d_xi.data_ptr(), d_yi.data_ptr(), d_sig.data_ptr(),
                                   ori.data_ptr(), valid.data_ptr(), 1, n, _stream()), "gf_sift_orient")
        torch.cuda.synchronize()
        intact(obuf, -7.0, "ori")
        intact(vbuf, -7, "valid")
        res.append((ori[0].cpu().clone(), valid[0].cpu().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    ori, valid = res[0]
    assert set(valid.unique().tolist()) <= {0, 1}
    compared = second = border = 0
    refs = []
    for i in range(n):
        Lv = gauss[int(octv[i])][0, int(lvl[i])].double().numpy()
        oris, bound, margin, hist = sc.ref_orient(Lv, int(xi[i]), int(yi[i]), float(sigma[i]), e_level=sc.E_STAGE)
        refs.append(oris)
        if margin is not None and margin <= 1.0:
            continue                                                         # the second peak is within the band of 0.8 max
        assert int(valid[i].sum()) == len(oris), (i, oris, ori[i], valid[i])  # a second peak exactly where the margin says so
        second += len(oris) == 2
        border += i >= n - 5
        for k, th in enumerate(oris):
            kb = int(np.round(th * 36 / (2 * np.pi))) % 36
            d = abs(float(ori[i, k]) - th)
            assert min(d, 2 * np.pi - d) <= sc.ori_bound(hist, kb, bound), (i, k)
            compared += 1
    assert compared >= 4 and second >= 1 and border >= 1
    # descriptors at the first orientation of every keypoint that has one, plus skipped keypoints (octave -1)
    has = torch.tensor([len(r) > 0 for r in refs])
    th0 = torch.tensor([r[0] if r else 0.0 for r in refs], dtype=torch.float32)
    d_oct2 = i32(torch.where(has, octv, torch.full_like(octv, -1)))
    d_xo, d_yo, d_th = xo.cuda(), yo.cuda(), th0.cuda()
    for rootsift in (0, 1):
        res = []
        for _ in range(2):
            dbuf, desc = guarded((1, n, 128), torch.float32, -7.0)
            lib.check(L.gf_sift_describe(ptrs, hw, len(dg), d_oct2.data_ptr(), d_lvl.data_ptr(), d_xo.data_ptr(), d_yo.data_ptr(),
                                         d_sig.data_ptr(), d_th.data_ptr(), desc.data_ptr(), 1, n, rootsift, _stream()), "gf_sift_describe")
            torch.cuda.synchronize()
            intact(dbuf, -7.0, "desc")
            res.append(desc[0].cpu().clone())
        assert torch.equal(res[0], res[1])
        for i in range(n):
            if not has[i]:
                assert (res[0][i] == 0).all()
                continue
            Lv = gauss[int(octv[i])][0, int(lvl[i])].double().numpy()
            ref, bound = sc.ref_describe(Lv, float(xo[i]), float(yo[i]), float(sigma[i]), float(th0[i]), rootsift=bool(rootsift),
                                         e_level=sc.E_STAGE)
            if rootsift:      # d sqrt(x) = dx / (2 sqrt(x)) with x >= 1e-6 after the L1 step
                bound = bound / (2 * np.sqrt(np.maximum(ref * ref, 1e-6))) * 2 + 8 * sc.U
            assert np.all(np.abs(res[0][i].double().numpy() - ref) <= bound), (i, rootsift)
            assert abs(float(res[0][i].norm()) - 1) < 1e-5


def test_describe_clips_and_zero_keypoints():
    lib, L = load()
    Lv, xo, yo, sigma, ori = sc.edge_level()
    g = torch.from_numpy(Lv).float()[None, None].expand(1, 6, -1, -1).contiguous()
    dg, ptrs, hw = _geometry([g])
    f = lambda v, dt=torch.float32: torch.tensor([v], dtype=dt, device="cuda")   # noqa: E731
    desc = torch.empty((1, 1, 128), device="cuda")
    args = [f(0, torch.int32), f(2, torch.int32), f(xo), f(yo), f(sigma), f(ori)]           # (kept alive over the call)
    lib.check(L.gf_sift_describe(ptrs, hw, 1, *[a.data_ptr() for a in args], desc.data_ptr(), 1, 1, 0, _stream()), "gf_sift_describe")
    ref, bound = sc.ref_describe(g[0, 2].double().numpy(), float(np.float32(xo)), float(np.float32(yo)), sigma, float(np.float32(ori)),
                                 e_level=sc.E_STAGE)
    unclipped = sc.ref_describe(g[0, 2].double().numpy(), xo, yo, sigma, ori, clip=False)[0]
    assert np.abs(unclipped - ref).max() > 10 * bound
    assert np.all(np.abs(desc[0, 0].cpu().double().numpy() - ref) <= bound)
    assert L.gf_sift_orient(ptrs, hw, 1, None, None, None, None, None, None, None, 1, 0, _stream()) == 0
    assert L.gf_sift_describe(ptrs, hw, 1, None, None, None, None, None, None, None, 1, 0, 0, _stream()) == 0
    assert L.gf_sift_orient(ptrs, hw, 9, None, None, None, None, None, None, None, 1, 0, _stream()) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ gf_sift_dedupe
def test_dedupe_against_the_reference_golden():
    from glue_factory_amd.extractors import sift as S
    lib, L = load()
    z = np.load(os.path.join(GOLDEN, "sift_post.npz"))
    for i, (pts, scales, angles, scores, (h, w)) in enumerate(sc.post_lists()):
        n = len(pts)
        pix = np.round(pts - 0.5).astype(np.int32)
        ix, iy = dev(pix[:, 0], torch.int32), dev(pix[:, 1], torch.int32)
        d_sc, d_an, d_ok = dev(scores, torch.float32), dev(angles, torch.float32), torch.ones(n, dtype=torch.int32, device="cuda")
        res = []
        for _ in range(2):
            kbuf, keep = guarded((1, n), torch.int32, -7)
            sbuf_g, sbuf = guarded((1, h, w), torch.float32, -7.0)
            bbuf, buf = guarded((1, h, w), torch.int64, -7)
            lib.check(L.gf_sift_dedupe(ix.data_ptr(), iy.data_ptr(), d_sc.data_ptr(), d_an.data_ptr(), d_ok.data_ptr(), buf.data_ptr(), sbuf.data_ptr(),
                                       keep.data_ptr(), 1, n, h, w, _stream()), "gf_sift_dedupe")
            torch.cuda.synchronize()
            for b_, fill, what in ((kbuf, -7, "keep"), (sbuf_g, -7.0, "sbuf"), (bbuf, -7, "buf")):
                intact(b_, fill, what)
            res.append((keep[0].cpu().clone(), sbuf[0].cpu().clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert np.array_equal(np.nonzero(res[0][0].numpy())[0], z[f"keep_{i}_r0"])
        for radius in (0, 3):            # the module's fused post-processing: kernel + max-pool
            t = lambda a: torch.from_numpy(a).cuda()[None]   # noqa: E731
            keep = S.dedupe_keep(t(pts), t(scores), t(angles), torch.ones((1, n), dtype=torch.bool, device="cuda"), h, w, radius, fused=True)
            assert np.array_equal(keep[0].nonzero()[:, 0].cpu().numpy(), z[f"keep_{i}_r{radius}"])


# ------------------------------------------------------------------------------------------------ the module
def _pair_up(a, c, b):
    """Rows of image b of two outputs: real rows, partner index and the share without a partner (either direction)."""
    ra, rc = a["scales"][b] > 0, c["scales"][b] > 0
    ka, kc = a["keypoints"][b][ra].double(), c["keypoints"][b][rc].double()
    d = torch.cdist(ka, kc)
    same = (a["scales"][b][ra][:, None].double() / c["scales"][b][rc][None].double()).log2().abs() < 0.02      # same octave and layer
    near_ori = (a["oris"][b][ra][:, None] - c["oris"][b][rc][None]).abs()
    near_ori = torch.minimum(near_ori, 2 * np.pi - near_ori) < 0.35
    ok = (d <= 0.01) & same & near_ori
    lost = int((~ok.any(1)).sum()) + int((~ok.any(0)).sum())
    pairs = [(int(i), int(ok[i].float().argmax())) for i in range(len(ka)) if ok[i].any()]
    return ra, rc, pairs, lost, len(ka) + len(kc)


def test_module_fused_against_stock_on_the_device():
    from glue_factory_amd.extractors.sift import SIFT
    imgs, sizes = sc.e2e_batch()
    data = {"image": imgs.float().cuda(), "image_size": sizes.cuda()}
    conf = {"max_num_keypoints": 128, "force_num_keypoints": True, "nms_radius": None}
    fused = SIFT(conf)
    out_f = fused(data)
    assert not bool(fused.overflow.any())
    stock = SIFT(conf)
    stock._use_fused = lambda image: False
    out_s = stock(data)
    compared = 0
    for b in range(3):
        cands = [c for c in sc.ref_keypoints(imgs[b, 0].numpy())[2] if c["accepted"] and sc.decisive(c)]
        ra, rc, pairs, lost, total = _pair_up(out_f, out_s, b)
        print(f"image {b}: {int(ra.sum())} fused, {int(rc.sum())} stock rows, {lost} without a partner")
        assert int(ra.sum()) >= 10 and lost <= 0.05 * total
        assert bool((out_f["keypoints"][b][ra] + 0.5 < sizes[b].cuda()).all())
        for i, j in pairs:
            fa = {k: out_f[k][b][ra][i].cpu() for k in out_f}
            st = {k: out_s[k][b][rc][j].cpu() for k in out_s}
            c = min(cands, key=lambda c: np.hypot(c["xy"][0] - float(fa["keypoints"][0]), c["xy"][1] - float(fa["keypoints"][1])))
            if np.hypot(c["xy"][0] - float(fa["keypoints"][0]), c["xy"][1] - float(fa["keypoints"][1])) > 0.05:
                continue                                                     # not a decisive candidate of the restatement
            # both paths err by at most the band against fp64: twice the band between them; scale = 1.6 2^(s/3) step
            off_band = float(np.max(c["offset_band"]))
            th = min(c["oris"], key=lambda t: min(abs(t - float(fa["oris"])), 2 * np.pi - abs(t - float(fa["oris"]))))
            ori_band = sc.ori_bound(c["hist"], int(np.round(th * 36 / (2 * np.pi))) % 36, c["ori_bin_bound"])
            scale_tol = 2 * off_band * np.log(2) / 3
            assert abs(float(fa["scales"] / st["scales"]) - 1) <= scale_tol + 4 * sc.U
            d_ori = abs(float(fa["oris"] - st["oris"]))
            d_ori = min(d_ori, 2 * np.pi - d_ori)
            assert d_ori <= 2 * ori_band
            # descriptor, first order: a tent per coordinate (slope 1 in cell / bin units) on entries <= 1: position
            # 2 off_band / (3 sigma) cells, orientation 2 ori_band (8 / 2 pi bins + 2 cells of rotation at the window's rim),
            # scale 2.5 cells x its relative change; the renormalisations at most double it; + this stage's own rounding
            tol = 2 * (2 * off_band / (3 * c["sigma"]) + 2 * ori_band * (8 / (2 * np.pi) + 2) + 2.5 * scale_tol) + 1e-4
            assert float((fa["descriptors"] - st["descriptors"]).abs().max()) <= tol
            compared += 1
    assert compared >= 20
    # with the reference's post-processing on top (per-pixel dedupe, max-pool NMS of radius 3): the same keypoints survive
    conf = dict(conf, nms_radius=3)
    stock = SIFT(conf)
    stock._use_fused = lambda image: False
    out_f, out_s = SIFT(conf)(data), stock(data)
    for b in range(3):
        ra, rc, pairs, lost, total = _pair_up(out_f, out_s, b)
        print(f"image {b}, nms_radius 3: {int(ra.sum())} fused, {int(rc.sum())} stock rows, {lost} without a partner")
        assert 10 <= int(ra.sum()) < total and lost <= 0.05 * total


def test_captured_forced_call_replays_on_a_rewritten_buffer():
    from glue_factory_amd.extractors.sift import SIFT
    imgs, sizes = sc.e2e_batch()
    first, second = imgs.float().cuda(), imgs.float().flip(0).contiguous().cuda()
    model = SIFT({"max_num_keypoints": 96, "force_num_keypoints": True, "nms_radius": 3})
    static = first.clone()
    sz = sizes.cuda()
    # warm-up on the current stream (padding table, library handles); no stream of its own: later test files pick streams
    # from torch's round-robin pool and one of them (test_gpu_sinkhorn_safety.py) is sensitive to the position it finds
    model({"image": static, "image_size": sz})
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model({"image": static, "image_size": sz})
    static.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.clone() for k, v in out.items()}
    eager = model({"image": second, "image_size": sz})
    for k in eager:
        assert torch.equal(replayed[k], eager[k]), k
    assert not torch.equal(replayed["keypoints"], model({"image": first, "image_size": sz})["keypoints"])
    assert int((replayed["scales"] > 0).sum()) >= 30 and not bool(model.overflow.any())


def test_integer_shift_recovers_every_keypoint():
    """The two images are shifted copies on a constant background and 16 px is a whole number of cells in every octave, so
    every pixel of the shifted pyramid is computed by the same sequence of fp32 operations on the same values: the fused
    path takes the same decisions at the shifted positions, decisive or not.  Recovered share: sift_cases.SHIFT_RECOVERED_FP64
    (1.0, what the fp64 stock path reaches on the CPU)."""
    from glue_factory_amd.extractors.sift import SIFT
    pair, _ = sc.shift_pair()
    model = SIFT({"max_num_keypoints": None, "nms_radius": None})
    a, b = (model({"image": torch.from_numpy(p).float()[None, None].cuda()}) for p in pair)
    a, b = ({k: v.cpu() for k, v in o.items()} for o in (a, b))
    rec, n = sc.shift_recovered(a, b, pair[0].shape, 2e-4, 1e-5)
    print(f"shift: {rec} of {n} keypoints recovered")
    assert n >= 10 and rec / n >= sc.SHIFT_RECOVERED_FP64


def test_overflow_raises_in_eager_mode_and_is_flagged_in_forced_mode():
    from glue_factory_amd.extractors.sift import SIFT
    img = sc.e2e_batch()[0][:1].float().cuda()
    with pytest.raises(RuntimeError, match="candidate_cap"):
        SIFT({"candidate_cap": 4, "nms_radius": None})({"image": img})
    forced = SIFT({"candidate_cap": 4, "nms_radius": None, "max_num_keypoints": 16, "force_num_keypoints": True})
    out = forced({"image": img})
    assert bool(forced.overflow.all()) and 1 <= int((out["scales"] > 0).sum()) <= 8


def test_forced_mode_rejects_more_keypoints_than_the_top_k_kernel_takes():
    from glue_factory_amd.extractors.sift import SIFT
    img = sc.e2e_batch()[0][:1].float().cuda()
    with pytest.raises(ValueError, match="4096"):
        SIFT({"max_num_keypoints": 5000, "force_num_keypoints": True})({"image": img})
    assert SIFT({"max_num_keypoints": 4096, "force_num_keypoints": True})({"image": img})["keypoints"].shape == (1, 4096, 2)


def test_two_view_pipeline_train_step():
    """One pair from HomographyViews through this extractor -> homography ground truth -> LightGlue (input_dim 128,
    add_scale_ori), the configuration of sift+lightglue_homography.yaml with fewer keypoints."""
    from glue_factory_amd.data.homography_views import HomographyViews
    from glue_factory_amd.pipeline import TwoViewPipeline
    torch.manual_seed(0)
    pipe = TwoViewPipeline({
        "extractor": {"name": "extractors.sift", "backend": "pycolmap_cuda", "max_num_keypoints": 256, "force_num_keypoints": True,
                      "nms_radius": 3, "trainable": False},
        "ground_truth": {"name": "matchers.homography_matcher", "th_positive": 3, "th_negative": 3},
        "matcher": {"name": "matchers.lightglue", "filter_threshold": 0.1, "n_layers": 2, "input_dim": 128, "add_scale_ori": True},
    }).cuda()
    pipe.eval()
    pipe.matcher.train()
    image = torch.from_numpy(vc.textured_image(512, 384))[None].cuda()
    views = HomographyViews({"homography": {"patch_shape": [320, 240], "difficulty": 0.5}, "photometric": {"name": "lg", "p": 0.95},
                             "grayscale": True, "seed": 1})
    data = views(image)
    pred = pipe(data)
    losses, _ = pipe.loss(pred, data)
    losses["total"].mean().backward()
    positives = int((pred["gt_matches0"] >= 0).sum())
    print(f"positive ground-truth matches: {positives} of 256")
    assert pred["descriptors0"].shape == (1, 256, 128) and "scales0" in pred and "oris0" in pred
    assert torch.isfinite(losses["total"]).all() and positives > 0
    grads = [p.grad for p in pipe.matcher.parameters() if p.grad is not None]
    assert len(grads) >= 10 and all(torch.isfinite(g).all() for g in grads)
