"""Wrappers of the four ALIKED entry points of libgf_amd.so (csrc/aliked.hip; contracts in include/gf_amd.h).

No-grad, stream-ordered and capturable: a wrapper allocates its outputs through torch's allocator and enqueues one kernel;
it never reads a value back.  A missing library or a rejected call raises (lib.check): there is no eager fallback here.
(The wrappers live beside the extractor, not in glue_factory_amd.ops: that package is pinned to its nine kernel-family
modules by tests/test_capi_and_host.py.)"""
import torch

from .. import lib as _lib


def _f32(t):
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def deform_cols(x, offset, pad=1):
    """x [B,C,H,W], offset [B,18,H,W] (clamped) -> column matrix [B, C*9, H*W] of the 3 x 3 deformable convolution."""
    x, offset = _f32(x), _f32(offset)
    b, c, h, w = x.shape
    assert offset.shape == (b, 18, h, w)
    cols = torch.empty((b, c * 9, h * w), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().gf_ak_deform_cols(x.data_ptr(), offset.data_ptr(), cols.data_ptr(), b, c, h, w, pad, _stream()),
               "gf_ak_deform_cols")
    return cols


def aggregate(x1, g2, g3, g4, w1, w8, top, left, h, w):
    """-> (normalised feature map [B,h,w,dim] channels-last for the crop, 8-channel score-head map [B,8,Hp,Wp])."""
    x1, g2, g3, g4 = _f32(x1), _f32(g2), _f32(g3), _f32(g4)
    b, c1, hp, wp = x1.shape
    d4 = g2.shape[1]
    assert g2.shape == (b, d4, hp // 2, wp // 2) and g3.shape == (b, d4, hp // 8, wp // 8) and g4.shape == (b, d4, hp // 32, wp // 32)
    w1 = _f32(w1).reshape(d4, c1)
    w8 = _f32(w8).reshape(8, 4 * d4)
    feat = torch.empty((b, h, w, 4 * d4), dtype=torch.float32, device=x1.device)
    s8 = torch.empty((b, 8, hp, wp), dtype=torch.float32, device=x1.device)
    _lib.check(_lib.load().gf_ak_aggregate(x1.data_ptr(), g2.data_ptr(), g3.data_ptr(), g4.data_ptr(), w1.data_ptr(), w8.data_ptr(),
                                           feat.data_ptr(), s8.data_ptr(), b, c1, 4 * d4, hp, wp, top, left, h, w, _stream()),
               "gf_ak_aggregate")
    return feat, s8


def dkd_refine(score, ind, radius, temperature=0.1):
    """score [B,1,H,W] or [B,H,W], ind [B,N] int64 flat pixels -> (normalised xy [B,N,2], score [B,N], dispersity [B,N])."""
    score = _f32(score)
    b, h, w = score.shape[0], score.shape[-2], score.shape[-1]
    ind = ind.contiguous()
    assert ind.dtype == torch.int64 and ind.shape[0] == b
    n = ind.shape[1]
    kxy = torch.empty((b, n, 2), dtype=torch.float32, device=score.device)
    ksc = torch.empty((b, n), dtype=torch.float32, device=score.device)
    disp = torch.empty((b, n), dtype=torch.float32, device=score.device)
    _lib.check(_lib.load().gf_ak_dkd_refine(score.data_ptr(), ind.data_ptr(), kxy.data_ptr(), ksc.data_ptr(), disp.data_ptr(),
                                            b, n, h, w, int(radius), float(temperature), _stream()), "gf_ak_dkd_refine")
    return kxy, ksc, disp


def sddh(feat, pos, weights, K, M):
    """feat [B,H,W,dim] channels-last, pos [B,N,2] keypoints in pixels of the map, weights as ALIKED._sddh_weights()
    -> descriptors [B,N,dim]."""
    feat, pos = _f32(feat), _f32(pos)
    b, h, w, dim = feat.shape
    n = pos.shape[1]
    out = torch.empty((b, n, dim), dtype=torch.float32, device=feat.device)
    wt = {k: _f32(v) for k, v in weights.items()}
    assert wt["w1"].shape == (2 * M, K * K * dim) and wt["agg"].shape == (M, dim, dim)
    _lib.check(_lib.load().gf_ak_sddh(feat.data_ptr(), pos.data_ptr(), wt["w1"].data_ptr(), wt["b1"].data_ptr(), wt["w2"].data_ptr(),
                                      wt["b2"].data_ptr(), wt["sf"].data_ptr(), wt["agg"].data_ptr(), out.data_ptr(),
                                      b, n, h, w, dim, M, K, _stream()), "gf_ak_sddh")
    return out
