"""Homography view synthesis (csrc/hviews.hip): gf_hv_warp and gf_hv_filter behind thin wrappers, re-exported as
``ops.warp_views`` and ``ops.filter_views``.

Data-preparation ops, not autograd ops: HIP tensors in, an fp32 view stack out, nothing read back to the host, so both can be
captured in a graph.  The table layouts and the arithmetic are stated in include/gf_amd.h and csrc/hviews.hip."""
import torch

from .. import lib as _lib
from ..ops._base import _chk, _stream

NPARAM, MAXTAPS, RADIUS = 4, 81, 12          # GF_HV_NPARAM, GF_HV_MAXTAPS, GF_HV_RADIUS of include/gf_amd.h
_U8, _F32 = 2, 0                             # GF_DTYPE_U8, GF_DTYPE_F32


def _table(t, dtype, shape, name):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t


@torch.no_grad()
def warp_views(src, src_sizes, view_src, Hinv, params, patch_shape, finish=True, gray=False, out=None):
    """src [S,Hmax,Wmax,C] uint8 or fp32 (NHWC, C in {1,3}), src_sizes [S,2] int32 (w, h), view_src [V] int32, Hinv [V,3,3] or
    [V,9] fp32 (patch pixel -> source pixel), params [V,4] fp32 (gamma, value shift, a, b), patch_shape (pw, ph)
    -> out [V,Cout,ph,pw] fp32 (Cout = 1 with finish and gray, else C).  One launch."""
    _chk(src, src_sizes, view_src, Hinv, params, out)
    if src.dim() != 4 or not src.is_contiguous() or src.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError("warp_views: src must be a contiguous [S,Hmax,Wmax,C] uint8 or float32 tensor")
    s, hmax, wmax, c = src.shape
    v = view_src.shape[0]
    pw, ph = int(patch_shape[0]), int(patch_shape[1])
    _table(src_sizes, torch.int32, (s, 2), "src_sizes")
    _table(view_src, torch.int32, (v,), "view_src")
    if Hinv.dim() == 3 and Hinv.is_contiguous():
        Hinv = Hinv.view(v, 9)
    _table(Hinv, torch.float32, (v, 9), "Hinv")
    _table(params, torch.float32, (v, NPARAM), "params")
    cout = 1 if (finish and gray) else c
    if out is None:
        out = torch.empty((v, cout, max(ph, 0), max(pw, 0)), dtype=torch.float32, device=src.device)
    else:
        _table(out, torch.float32, (v, cout, ph, pw), "out")
    _lib.check(_lib.load().gf_hv_warp(src.data_ptr(), _U8 if src.dtype == torch.uint8 else _F32, src_sizes.data_ptr(),
                                      view_src.data_ptr(), Hinv.data_ptr(), params.data_ptr(), out.data_ptr(), s, hmax, wmax, c,
                                      v, cout, ph, pw, int(bool(finish)), int(bool(gray)), _stream()), "gf_hv_warp")
    return out


@torch.no_grad()
def filter_views(x, tap_off, tap_w, ntaps, params, gray=False, out=None):
    """x [V,C,ph,pw] fp32, tap_off [V,81,2] int32 (dx, dy), tap_w [V,81] fp32, ntaps [V] int32, params [V,4] fp32
    -> out [V,Cout,ph,pw] fp32: the per-view correlation (reflect-101 border), clamp(a v + b, 0, 1) and, with gray, the
    luma reduction of a 3-channel view.  One launch; not in place."""
    _chk(x, tap_off, tap_w, ntaps, params, out)
    if x.dim() != 4 or not x.is_contiguous() or x.dtype != torch.float32:
        raise RuntimeError("filter_views: x must be a contiguous [V,C,ph,pw] float32 tensor")
    v, c, ph, pw = x.shape
    _table(tap_off, torch.int32, (v, MAXTAPS, 2), "tap_off")
    _table(tap_w, torch.float32, (v, MAXTAPS), "tap_w")
    _table(ntaps, torch.int32, (v,), "ntaps")
    _table(params, torch.float32, (v, NPARAM), "params")
    cout = 1 if gray else c
    if out is None:
        out = torch.empty((v, cout, ph, pw), dtype=torch.float32, device=x.device)
    else:
        _table(out, torch.float32, (v, cout, ph, pw), "out")
    _lib.check(_lib.load().gf_hv_filter(x.data_ptr(), tap_off.data_ptr(), tap_w.data_ptr(), ntaps.data_ptr(), params.data_ptr(),
                                        out.data_ptr(), v, c, cout, ph, pw, int(bool(gray)), _stream()), "gf_hv_filter")
    return out
