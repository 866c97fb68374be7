"""Shared cases of the ALIKED tests: seeded weight / input builders, the comparison rule of the end-to-end tests, fp64
restatements of the four kernels of csrc/aliked.hip with per-value bounds from an fp32 rounding model, and the named
mutations those bounds must catch (test_aliked_cases_reference.py holds all of this on the CPU; test_gpu_aliked.py
holds the kernels to it).

Rounding model.  Every kernel output is a short chain of fp32 operations on inputs that are exact in fp64.  With
u = 2^-24, a sum of n products computed in any order and with any fusing errs by at most gamma_n * sum |a_i b_i|,
gamma_n = n u / (1 - n u); a following elementwise function with derivative bound L multiplies the incoming error by L
and adds its own (a few u relative; exp / SELU on the device are allowed 4 ulp).  The restatements therefore return,
next to each fp64 value, the MAGNITUDE sum |terms| it was built from, and ``bound = ROUNDINGS * u * magnitude + tiny``
where ROUNDINGS counts the fp32 operations on the longest path (stated per kernel below, with a factor 4 of slack for
the elementwise functions).  Nothing here is fitted to what a kernel returns."""
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SELU_A, SELU_S = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946


def reference_paths(ref):
    """sys.path entries that let the unmodified reference ALIKED module import: stand-ins first, the checkout last."""
    return [os.path.join(ROOT, "tests", "aliked_stubs"), os.path.join(ROOT, "oracle", "stubs"), ref]


# ------------------------------------------------------------------------------------------------ models and inputs
def build_model(conf, device="cpu"):
    """Our ALIKED with seeded weights: random BatchNorm statistics and affine terms, the last score-head convolution
    x 30 (scores spread over most of (0, 1)), desc_head.offset_conv scaled so that some offsets hit the clamp and some
    samples leave the map."""
    from glue_factory_amd.extractors.aliked import ALIKED
    g = torch.Generator().manual_seed(sum(map(ord, conf["model_name"])) + 11)
    torch.manual_seed(int(torch.randint(0, 2 ** 31, (1,), generator=g)))
    model = ALIKED({**conf, "pretrained": False})
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
            m.weight.data.copy_(0.7 + 0.6 * torch.rand(m.num_features, generator=g))
            m.bias.data.copy_(0.2 * torch.randn(m.num_features, generator=g))
    model.score_head[6].weight.data.mul_(30.0)
    model.desc_head.offset_conv[0].weight.data.mul_(6.0)
    model.desc_head.offset_conv[2].weight.data.mul_(12.0)
    model.desc_head.offset_conv[2].bias.data.mul_(20.0)
    return model.eval().to(device)


def image(shape, seed):
    """Smooth-ish random image: noise plus a few low-frequency waves, in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    b, c, h, w = shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    img = 0.5 * torch.rand(shape, generator=g)
    for _ in range(4):
        f = 0.05 + 0.4 * torch.rand(b, c, 2, generator=g)
        img = img + 0.125 * (1 + torch.sin(f[..., 0, None, None] * ys + f[..., 1, None, None] * xs))
    return img.clamp(0, 1)


TOPK = {"detection_threshold": -1.0, "force_num_keypoints": True}
SWEEP = {
    "t16": ({"model_name": "aliked-t16", "max_num_keypoints": 64, **TOPK}, (2, 3, 64, 96), None),
    "n16_padded": ({"model_name": "aliked-n16", "max_num_keypoints": 128, **TOPK}, (2, 3, 72, 100), None),
    "n32": ({"model_name": "aliked-n32", "max_num_keypoints": 64, **TOPK}, (1, 3, 64, 64), None),
    # (the first image is smaller than the tensor; the last one fills it: see the module text of extractors/aliked.py)
    "image_size": ({"model_name": "aliked-t16", "max_num_keypoints": 64, **TOPK}, (2, 3, 64, 96), [[80, 50], [96, 64]]),
    "threshold": ({"model_name": "aliked-n16", "max_num_keypoints": 128, "detection_threshold": 0.6}, (1, 3, 64, 96), None),
    "radius3": ({"model_name": "aliked-t16", "max_num_keypoints": 64, "nms_radius": 3, **TOPK}, (2, 3, 72, 100), None),
}
GOLDEN_CASES = ("t16", "n16_padded")


def sweep_case(name):
    conf, shape, sizes = SWEEP[name]
    data = {"image": image(shape, 1000 + sorted(SWEEP).index(name))}
    if sizes is not None:
        data["image_size"] = torch.tensor(sizes)
    return dict(conf), data


def nms_scores_of(score_map, conf, data):
    """[B, H, W] NMS scores (0 where suppressed or in the border) of a recorded score map, as the selection sees them."""
    from glue_factory_amd.extractors.superpoint_open import batched_nms
    s = torch.as_tensor(score_map)
    b, _, h, w = s.shape
    r = conf.get("nms_radius", 2)
    nms = batched_nms(s, r)[:, 0].clone()
    nms[:, :r] = 0
    nms[:, :, :r] = 0
    for i in range(b):
        wi, hi = (int(v) for v in data["image_size"][i]) if data.get("image_size") is not None else (w, h)
        nms[i, hi - r:] = 0
        nms[i, :, wi - r:] = 0
    return nms.numpy()


def compare_predictions(pred, ref, nms, conf, tol=1e-4, skip_near_integer=False):
    """The end-to-end rule.  Keypoints are paired by position (mutual nearest neighbour closer than 0.01 px); a keypoint
    of one side without a partner must sit within the NMS radius of a maximum whose NMS score is within 1e-5 of the
    deciding score (the k-th largest in top-k mode, the threshold otherwise); >= 97 % of the reference's keypoints are
    common; positions, scores, dispersity and descriptors of the common ones and the score map agree at `tol`.
    `skip_near_integer`: descriptors only where both pixel coordinates are farther than 1e-3 from an integer (the
    truncation decides the patch).  Returns the largest per-image fraction of common keypoints that rule leaves out."""
    r = conf.get("nms_radius", 2)
    topk = conf.get("detection_threshold", 0.2) <= 0
    np.testing.assert_allclose(pred["score_map"], ref["score_map"], rtol=tol, atol=tol)
    worst = 0.0
    for b in range(ref["keypoints"].shape[0]):
        ko, kr = pred["keypoints"][b].astype(np.float64), ref["keypoints"][b].astype(np.float64)
        d = np.abs(ko[:, None] - kr[None]).max(-1)
        jo, jr = d.argmin(1), d.argmin(0)
        io = np.array([i for i in range(len(ko)) if jr[jo[i]] == i and d[i, jo[i]] < 1e-2], dtype=np.int64)
        ir = jo[io]
        if topk:
            edge = float(np.sort(nms[b].ravel())[::-1][conf["max_num_keypoints"] - 1])
        else:
            edge = conf["detection_threshold"]
        maxima = np.argwhere(np.abs(nms[b] - edge) < 1e-5)[:, ::-1]            # (x, y) of maxima on the deciding edge
        for k in list(np.delete(ko, io, 0)) + list(np.delete(kr, ir, 0)):
            assert len(maxima) and np.abs(maxima - k[None]).max(-1).min() <= r + 1e-3, (b, k, edge)
        assert len(io) >= 0.97 * len(kr), (len(io), len(kr))
        np.testing.assert_allclose(ko[io], kr[ir], rtol=tol, atol=tol)
        for key in ("keypoint_scores", "score_dispersity"):
            np.testing.assert_allclose(pred[key][b][io], ref[key][b][ir], rtol=tol, atol=tol)
        frac = np.abs(kr[ir] - np.round(kr[ir]))
        near = (frac < 1e-3).any(-1)
        worst = max(worst, float(near.mean()) if len(near) else 0.0)
        keep = ~near if skip_near_integer else np.ones_like(near)
        np.testing.assert_allclose(pred["descriptors"][b][io][keep], ref["descriptors"][b][ir][keep], rtol=tol, atol=tol)
    return worst


# ------------------------------------------------------------------------------------------------ kernel restatements (fp64)
def rnd(n):
    """Roundings charged to a length-n fp32 dot product in units of u: the probabilistic bound lambda sqrt(n) with lambda = 4
    (Higham & Mary 2019; the worst case n is never approached by sums of mixed sign), plus 4 for the operations around it."""
    return 4.0 * float(n) ** 0.5 + 4.0


def selu64(x):
    return SELU_S * torch.where(x > 0, x, SELU_A * torch.expm1(x))


SELU_LIP = SELU_S * SELU_A        # largest slope of SELU (at 0-)
MUTATIONS = {
    "deform_cols": ("dcn_dy_dx_swapped", "dcn_border_corners_kept"),
    "aggregate": ("align_corners_false", "eps_clamp_missing"),
    "dkd_refine": ("dispersity_wrong_window",),
    "sddh": ("offset_halves_swapped", "offsets_interleaved", "patch_clamp_w_minus_k"),
}


def deform_cols64(x, off, pad=1, mutation=None):
    """Direct fp64 loop over taps and pixels.  -> (cols [B, C*9, H*W], bound)."""
    x, off = x.double(), off.double()
    b, c, h, w = x.shape
    cols = torch.zeros(b, c, 9, h, w, dtype=torch.float64)
    mag = torch.zeros(b, 1, 9, h, w, dtype=torch.float64)
    for bi in range(b):
        for k in range(9):
            for y in range(h):
                for xq in range(w):
                    o0, o1 = float(off[bi, 2 * k, y, xq]), float(off[bi, 2 * k + 1, y, xq])
                    if mutation == "dcn_dy_dx_swapped":
                        o0, o1 = o1, o0
                    py, px = y - pad + k // 3 + o0, xq - pad + k % 3 + o1
                    if py <= -1 or py >= h or px <= -1 or px >= w:
                        continue
                    y0, x0 = int(np.floor(py)), int(np.floor(px))
                    ly, lx = py - y0, px - x0
                    for yy, xx, wt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx),
                                       (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
                        if mutation == "dcn_border_corners_kept":
                            yy, xx = min(max(yy, 0), h - 1), min(max(xx, 0), w - 1)
                        if 0 <= yy < h and 0 <= xx < w:
                            cols[bi, :, k, y, xq] += wt * x[bi, :, yy, xx]
                            mag[bi, 0, k, y, xq] = max(mag[bi, 0, k, y, xq], (1 + abs(py) + abs(px)))
    # fp32: p = integer + offset rounds once (u |p|), which moves every weight by as much; 4 products and 3 sums
    smax = x.abs().amax(dim=(2, 3)).view(b, c, 1, 1, 1)
    bound = 16 * U * mag * smax + 1e-30
    return cols.reshape(b, c * 9, h * w), bound.reshape(b, c * 9, h * w)


def aggregate_inputs(dim, hp, wp, seed, batch=2):
    g = torch.Generator().manual_seed(seed)
    c1, d4 = dim // 8, dim // 4
    t = {"x1": torch.randn(batch, c1, hp, wp, generator=g),
         "g2": selu64(torch.randn(batch, d4, hp // 2, wp // 2, generator=g).double()).float(),
         "g3": selu64(torch.randn(batch, d4, hp // 8, wp // 8, generator=g).double()).float(),
         "g4": selu64(torch.randn(batch, d4, hp // 32, wp // 32, generator=g).double()).float(),
         "w1": 0.4 * torch.randn(d4, c1, generator=g), "w8": 0.2 * torch.randn(8, dim, generator=g)}
    for k in ("x1", "g2", "g3", "g4"):      # one all-zero pixel: the eps clamp of the normalisation decides it
        t[k][0, :, 0, 0] = 0
    return t


def aggregate64(t, mutation=None, dt=torch.float64):
    """-> (feat [B,dim,Hp,Wp] normalised, s8 [B,8,Hp,Wp], bound_feat, bound_s8), all at padded size.  (`dt`: the same
    formulation in another precision -- the CPU tests hold the fp32 run of every restatement to its fp64 run's bound.)"""
    x1, w1, w8 = t["x1"].to(dt), t["w1"].to(dt), t["w8"].to(dt)
    b, c1, hp, wp = x1.shape
    d4 = w1.shape[0]
    dim = 4 * d4
    z = torch.einsum("jc,bchw->bjhw", w1, x1)
    parts = [selu64(z)]
    errs = [SELU_LIP * rnd(c1) * U * torch.einsum("jc,bchw->bjhw", w1.abs(), x1.abs()) + 8 * U * (parts[0].abs() + 1)]
    for k in ("g2", "g3", "g4"):
        gk = t[k].to(dt)
        parts.append(F.interpolate(gk, size=(hp, wp), mode="bilinear", align_corners=mutation != "align_corners_false"))
        # src = scale * dst carries 2 u src <= 2 u in; the weight moves by as much, the value by that times a corner difference
        errs.append((U * (8 + 4 * max(gk.shape[-2:])) * 2 * gk.abs().amax(dim=(2, 3), keepdim=True)).expand(b, d4, hp, wp))
    x, e = torch.cat(parts, 1), torch.cat(errs, 1)
    norm = x.pow(2).sum(1, keepdim=True).sqrt()
    n = norm if mutation == "eps_clamp_missing" else norm.clamp(min=1e-12)
    feat = x / n
    nn_ = norm.clamp(min=1e-12)
    bound_feat = e / nn_ + x.abs() / nn_ ** 2 * (e.pow(2).sum(1, keepdim=True).sqrt() + rnd(dim) * U * nn_) + 4 * U * x.abs() / nn_ + 1e-30
    z8 = torch.einsum("jc,bchw->bjhw", w8, x)
    s8 = selu64(z8)
    ez = torch.einsum("jc,bchw->bjhw", w8.abs(), e) + rnd(dim) * U * torch.einsum("jc,bchw->bjhw", w8.abs(), x.abs())
    return feat, s8, bound_feat, SELU_LIP * ez + 8 * U * (s8.abs() + 1)


def _bilinear64(m, ix, iy):
    """Zero-padded bilinear read of m [H,W,(C)] at pixel coordinates ix, iy [n] (fp64)."""
    h, w = m.shape[:2]
    x0, y0 = torch.floor(ix), torch.floor(iy)
    out = 0
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = (x0 + dx).long(), (y0 + dy).long()
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            wt = (1 - (ix - x0 - dx).abs()) * (1 - (iy - y0 - dy).abs()) * ok
            v = m[yy.clamp(0, h - 1), xx.clamp(0, w - 1)]
            out = out + (wt.unsqueeze(-1) * v if v.dim() > wt.dim() else wt * v)
    return out


def dkd64(score, idx, r, temperature=0.1, mutation=None, dt=torch.float64):
    """score [B,H,W], idx [B,N] -> dict of (value, bound) for kxy (normalised), kscore, disp."""
    s = score.to(dt)
    b, h, w = s.shape
    ks = 2 * r + 1
    n = ks * ks
    pad = F.pad(s, (r, r, r, r))
    out = {k: [] for k in ("kxy", "kscore", "disp")}
    d = torch.arange(ks)
    gx = (d - r).view(1, ks).expand(ks, ks).reshape(-1).to(dt)
    gy = (d - r).view(ks, 1).expand(ks, ks).reshape(-1).to(dt)
    for bi in range(b):
        x0, y0 = idx[bi] % w, idx[bi] // w
        win = pad[bi][(y0[:, None, None] + d.view(1, ks, 1)), (x0[:, None, None] + d.view(1, 1, ks))].reshape(-1, n)
        e = ((win - win.max(1, keepdim=True).values) / temperature).exp()
        tot = e.sum(1)
        rx, ry = (e * gx).sum(1) / tot, (e * gy).sum(1) / tot
        dist2 = ((gx[None] - rx[:, None]) / r) ** 2 + ((gy[None] - ry[:, None]) / r) ** 2
        den = torch.roll(tot, 1) if mutation == "dispersity_wrong_window" else tot
        out["disp"].append((e * dist2).sum(1) / den)
        kx, ky = (x0 + rx) / (w - 1) * 2 - 1, (y0 + ry) / (h - 1) * 2 - 1
        out["kxy"].append(torch.stack([kx, ky], -1))
        out["kscore"].append(_bilinear64(s[bi], (kx + 1) / 2 * (w - 1), (ky + 1) / 2 * (h - 1)))
    # e_i: the argument (s - max) / T <= 1 / T in magnitude carries 3 u of itself, exp 4 ulp; sums of n terms
    rel = (3.0 / temperature + 4 + rnd(n)) * U
    e_r = 2 * rel * r                                           # residual, pixels
    e_p = e_r + 8 * U * max(h, w)                               # + the round trip through [-1, 1]
    smax = float(s.abs().max())
    res = {"kxy": (torch.stack(out["kxy"]), torch.full((b, idx.shape[1], 2), 2 * e_p / (min(h, w) - 1) + 4 * U)),
           "disp": (torch.stack(out["disp"]), torch.full(idx.shape, 8 * 2 * rel + 8 * e_r / r + 8 * U)),
           "kscore": (torch.stack(out["kscore"]), torch.full(idx.shape, 4 * smax * e_p + 8 * U * smax))}
    return res


def sddh_inputs(dim, M, K, n, seed, batch=2, h=12, w=17):
    """Feature map, keypoints in pixels (random ones after the planted ones: 0, integers, every border clamp of the patch
    rule, the far corner) and the head's weights in the kernel's layouts, scaled so that offsets clamp and leave the map."""
    g = torch.Generator().manual_seed(seed)
    feat = F.normalize(torch.randn(batch, h, w, dim, generator=g), dim=-1)
    planted = torch.tensor([[0.0, 0.0], [w - 1.0, h - 1.0], [3.0, 4.0], [1.0, 0.5], [0.5, 1.0], [w - 2.0, 2.0], [w - 3.0, h - 3.0],
                            [2.25, h - 2.0], [w - 1.5, h - 1.25], [1.999999, 2.000001], [w - 4.0, h - 4.0], [w - 3.5, 5.0]])
    pos = torch.rand(batch, n, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0])
    m = min(n, len(planted))
    pos[:, :m] = planted[:m]
    O, KK = 2 * M, K * K * dim
    wts = {"w1": 6.0 / KK ** 0.5 * torch.randn(O, KK, generator=g) * 3, "b1": 0.3 * torch.randn(O, generator=g),
           "w2": 6.0 / O ** 0.5 * torch.randn(O, O, generator=g), "b2": torch.randn(O, generator=g),
           "sf": torch.randn(dim, dim, generator=g) / dim ** 0.5 * 3, "agg": torch.rand(M, dim, dim, generator=g) - 0.3}
    return feat, pos, wts


def sddh64(feat, pos, wts, K, M, mutation=None, dt=torch.float64):
    """-> (descriptors [B,N,dim], bound, offsets [B,N,2M]).  `wts` in the kernel's layouts (see ALIKED._sddh_weights).

    Four dense stages deep, a worst-case bound (sum of magnitudes at every stage) exceeds the descriptors themselves, so
    this one kernel is held to the INDEPENDENT-ERROR model instead: the operands of these cases are zero-mean by
    construction, a length-n fp32 fma chain then leaves a standard error of at most 2 u sum |a_i b_i| (its partial sums
    grow like sqrt(k)), a linear stage carries incoming standard errors in quadrature, a Lipschitz stage multiplies them, a
    sample moves by (position error) x (the largest difference of neighbouring pixels of its channel); bound = 6 sigma."""
    f = feat.to(dt)
    b, h, w, dim = f.shape
    n = pos.shape[1]
    w1, b1, w2, b2, sf, agg = (wts[k].to(dt) for k in ("w1", "b1", "w2", "b2", "sf", "agg"))
    O, KK = 2 * M, K * K * dim
    lim = max(h, w) / 4.0
    fz = F.pad(f, (0, 0, 1, 1, 1, 1))                           # zero frame: samples fade to 0 outside the map
    grad = torch.maximum((fz[:, 1:] - fz[:, :-1]).abs().amax(dim=(1, 2)), (fz[:, :, 1:] - fz[:, :, :-1]).abs().amax(dim=(1, 2)))
    descs, bounds, offs = [], [], []

    def quad(sig, wabs):
        return (sig.pow(2) @ wabs.pow(2).t()).sqrt()

    for bi in range(b):
        p = pos[bi].to(dt)
        pl = torch.trunc(p)
        if K > 1:
            corner = torch.trunc(pl - K / 2 + 1)
            up = 0 if mutation == "patch_clamp_w_minus_k" else 1
            cx = corner[:, 0].clamp(0, w - up - K).long()
            cy = corner[:, 1].clamp(0, h - up - K).long()
        else:
            cx, cy = pl[:, 0].long(), pl[:, 1].long()
        d = torch.arange(K)
        patch = f[bi][(cy[:, None, None] + d.view(1, K, 1)), (cx[:, None, None] + d.view(1, 1, K))].reshape(n, KK)
        h1 = selu64(patch @ w1.t() + b1)
        s1 = SELU_LIP * 2 * U * (patch.abs() @ w1.abs().t() + b1.abs()) + 2 * U * (h1.abs() + 1)
        o = (h1 @ w2.t() + b2).clamp(-lim, lim)
        so = (quad(s1, w2.abs()).pow(2) + (2 * U * (h1.abs() @ w2.abs().t() + b2.abs())).pow(2)).sqrt()
        offs.append(o)
        if mutation == "offset_halves_swapped":
            ox, oy, ex, ey = o[:, M:], o[:, :M], so[:, M:], so[:, :M]
        elif mutation == "offsets_interleaved":
            ox, oy, ex, ey = o[:, 0::2], o[:, 1::2], so[:, 0::2], so[:, 1::2]
        else:
            ox, oy, ex, ey = o[:, :M], o[:, M:], so[:, :M], so[:, M:]
        sx, sy = p[:, :1] + ox, p[:, 1:] + oy                   # [n, M]
        X = _bilinear64(f[bi], sx.reshape(-1), sy.reshape(-1)).view(n, M, dim)
        sX = (ex + ey + 8 * U * max(h, w)).unsqueeze(-1) * grad[bi].view(1, 1, dim) + 4 * U * X.abs()
        Fm = selu64(X @ sf.t())
        sF = SELU_LIP * (quad(sX.reshape(-1, dim), sf.abs()).view(n, M, dim).pow(2)
                         + (2 * U * (X.abs() @ sf.abs().t())).pow(2)).sqrt() + 2 * U * (Fm.abs() + 1)
        dsc = torch.einsum("npc,pdc->nd", Fm, agg)
        sd = (torch.einsum("npc,pdc->nd", sF.pow(2), agg.pow(2)) + (2 * U * torch.einsum("npc,pdc->nd", Fm.abs(), agg.abs())).pow(2)).sqrt()
        nrm = dsc.pow(2).sum(1, keepdim=True).sqrt().clamp(min=1e-12)
        descs.append(dsc / nrm)
        bounds.append(6 * (sd / nrm + dsc.abs() / nrm ** 2 * sd.pow(2).sum(1, keepdim=True).sqrt()) + 8 * U + 1e-30)
    return torch.stack(descs), torch.stack(bounds).double(), torch.stack(offs)


def within(value, ref, bound):
    """Every element of `value` within its bound of the fp64 value (NaN never is)."""
    return bool(((torch.as_tensor(value).double() - ref).abs() <= bound).all())
