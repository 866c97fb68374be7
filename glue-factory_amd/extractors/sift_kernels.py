"""Wrappers of the SIFT entry points of libgf_amd.so (csrc/sift.hip; contracts in include/gf_amd.h).

No-grad, stream-ordered and capturable: a wrapper allocates its outputs through torch's allocator and enqueues kernels; it
never reads a value back.  A missing library or a rejected call raises (lib.check): there is no eager fallback here."""
import ctypes

import torch

from .. import lib as _lib
from .sift import N_LEVELS, base_sigma, increment_sigma, octave_shapes


def _f32(t):
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _i32(t):
    return t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def blur(src, dst, sigma, mode=0, dog=None, src_copy=None):
    """One gf_sift_blur call on [B,h,w] VIEWS whose rows are dense (stride(1) == w, stride(2) == 1)."""
    for t in (src, dst, dog, src_copy):
        assert t is None or (t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2])
    b, hs, ws = src.shape
    _, h, w = dst.shape
    assert src_copy is None or (src_copy.shape == dst.shape and src_copy.stride(0) == dst.stride(0))
    _lib.check(_lib.load().gf_sift_blur(src.data_ptr(), dst.data_ptr(), dog.data_ptr() if dog is not None else None,
                                        src_copy.data_ptr() if src_copy is not None else None, b, hs, ws, h, w, src.stride(0),
                                        dst.stride(0), dog.stride(0) if dog is not None else 0, mode, float(sigma), _stream()),
               "gf_sift_blur")
    return dst


def pyramid(img, first_octave, num_octaves):
    """img [B,H,W] fp32 -> (gauss, dog): per octave [B,6,h,w] and [B,5,h,w]; 6 launches per octave, nothing else."""
    img = _f32(img)
    b, h, w = img.shape
    gauss, dog = [], []
    for o, (oh, ow) in enumerate(octave_shapes(h, w, first_octave, num_octaves)):
        g = torch.empty((b, N_LEVELS, oh, ow), dtype=torch.float32, device=img.device)
        d = torch.empty((b, N_LEVELS - 1, oh, ow), dtype=torch.float32, device=img.device)
        if o == 0:
            blur(img, g[:, 0], base_sigma(first_octave), mode=1 if first_octave == -1 else 0)
            blur(g[:, 0], g[:, 1], increment_sigma(1), dog=d[:, 0])
        else:
            blur(gauss[-1][:, N_LEVELS - 3], g[:, 1], increment_sigma(1), mode=2, dog=d[:, 0], src_copy=g[:, 0])
        for i in range(2, N_LEVELS):
            blur(g[:, i - 1], g[:, i], increment_sigma(i), dog=d[:, i - 1])
        gauss.append(g)
        dog.append(d)
    return gauss, dog


def extrema(dog, thr, edge_r, cap):
    """dog: list of [B,5,h,w] -> (meta [B,cap,4] int32 (octave, layer, y, x), vals [B,cap,4], count [B] int32)."""
    L = _lib.load()
    b = dog[0].shape[0]
    dev = dog[0].device
    count = torch.zeros((b,), dtype=torch.int32, device=dev)
    meta = torch.zeros((b, cap, 4), dtype=torch.int32, device=dev)
    vals = torch.zeros((b, cap, 4), dtype=torch.float32, device=dev)
    for o, d in enumerate(dog):
        d = _f32(d)
        h, w = d.shape[-2:]
        ws = torch.empty((max(int(L.gf_sift_extrema_ws_ints(b, h, w)), 1),), dtype=torch.int32, device=dev)
        _lib.check(L.gf_sift_extrema(d.data_ptr(), b, h, w, o, float(thr), float(edge_r), ws.data_ptr(), count.data_ptr(),
                                     meta.data_ptr(), vals.data_ptr(), cap, _stream()), "gf_sift_extrema")
    return meta, vals, count


def _geometry(gauss):
    gauss = [_f32(g) for g in gauss]
    ptrs = (ctypes.c_void_p * len(gauss))(*[g.data_ptr() for g in gauss])
    hw = (ctypes.c_int * (2 * len(gauss)))(*[v for g in gauss for v in g.shape[-2:]])
    return gauss, ptrs, hw


def orient(gauss, octv, lvl, xi, yi, sigma):
    """Per keypoint [B,N] -> (ori [B,N,2], valid [B,N,2] bool)."""
    gauss, ptrs, hw = _geometry(gauss)
    b, n = octv.shape
    ori = torch.empty((b, n, 2), dtype=torch.float32, device=sigma.device)
    valid = torch.empty((b, n, 2), dtype=torch.int32, device=sigma.device)
    octv, lvl, xi, yi, sigma = _i32(octv), _i32(lvl), _i32(xi), _i32(yi), _f32(sigma)
    _lib.check(_lib.load().gf_sift_orient(ptrs, hw, len(gauss), octv.data_ptr(), lvl.data_ptr(), xi.data_ptr(), yi.data_ptr(),
                                          sigma.data_ptr(), ori.data_ptr(), valid.data_ptr(), b, n, _stream()), "gf_sift_orient")
    return ori, valid != 0


def describe(gauss, octv, lvl, xo, yo, sigma, ori, rootsift):
    """Per keypoint [B,N] -> descriptors [B,N,128] (zeros where octv < 0)."""
    gauss, ptrs, hw = _geometry(gauss)
    b, n = octv.shape
    desc = torch.empty((b, n, 128), dtype=torch.float32, device=sigma.device)
    octv, lvl, xo, yo, sigma, ori = _i32(octv), _i32(lvl), _f32(xo), _f32(yo), _f32(sigma), _f32(ori)
    _lib.check(_lib.load().gf_sift_describe(ptrs, hw, len(gauss), octv.data_ptr(), lvl.data_ptr(), xo.data_ptr(), yo.data_ptr(),
                                            sigma.data_ptr(), ori.data_ptr(), desc.data_ptr(), b, n, int(bool(rootsift)), _stream()),
               "gf_sift_describe")
    return desc


def dedupe(ix, iy, scores, angles, valid, h, w):
    """-> (keep [B,N] bool, score buffer [B,h,w] of the kept entries)."""
    b, n = scores.shape
    dev = scores.device
    buf = torch.empty((b, h, w), dtype=torch.int64, device=dev)
    sbuf = torch.empty((b, h, w), dtype=torch.float32, device=dev)
    keep = torch.empty((b, n), dtype=torch.int32, device=dev)
    ix, iy, scores, angles, valid = _i32(ix), _i32(iy), _f32(scores), _f32(angles), _i32(valid)
    _lib.check(_lib.load().gf_sift_dedupe(ix.data_ptr(), iy.data_ptr(), scores.data_ptr(), angles.data_ptr(), valid.data_ptr(),
                                          buf.data_ptr(), sbuf.data_ptr(), keep.data_ptr(), b, n, h, w, _stream()), "gf_sift_dedupe")
    return keep != 0, sbuf


def topk(scores, k):
    """Indices [B,k] of the k largest of scores [B,n] (negative = empty slot), descending, ties by position."""
    scores = _f32(scores)
    b, n = scores.shape
    payload = torch.arange(n, dtype=torch.int32, device=scores.device).repeat(b, 1)
    out_s = torch.empty((b, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((b, k), dtype=torch.int64, device=scores.device)
    _lib.check(_lib.load().gf_topk_candidates(scores.data_ptr(), payload.data_ptr(), out_s.data_ptr(), out_i.data_ptr(), b, n, k,
                                              _stream()), "gf_topk_candidates")
    return out_i
