"""Per-step compute-dtype copies of the fp32 master parameters and the weights derived from them
(csrc/smallops.hip, csrc/fold.hip)."""
import struct
import weakref

import torch

from .. import lib as _lib
from ._base import BF16, F32, _p, _stream


# ---- per-step low-precision copies of the fp32 master parameters -------------------------------
# Every linear casts its weight / bias to the compute dtype; done one by one that is two tiny kernels per
# layer per step.  precast() converts a whole parameter list with one multi-tensor copy into a flat buffer
# and _lp() serves the views made by the precast() of the CURRENT forward.
_LP_CACHE = {}        # id(param) -> (param._version, dtype, view)
_LP_PTR = {}          # (data_ptr, numel) of a parameter -> the same record (serves reshaped views of it)
_LP_T = {}            # data_ptr of a compute-dtype weight -> (its transposed copy [K,N], weakref(param), dtype)
_LP_FLAT = {}         # (key, dtype) -> (flat buffer, [views], [params])


def precast(params, dtype, key="default", derived=None):
    """One launch per forward: every fp32 master parameter -> the compute dtype (flat buffer, served by _lp()), and the
    transposed copy W^T of every matrix (served by _wt_t(): the weight of the input-gradient GEMM dx = dy W), by
    gf_multi_cast_transpose.  Always re-done: a fused / capturable optimiser step, ``param.data = ...`` or a replayed
    hipGraph change the values without bumping the version counter (measured: stale bf16 weights in an eval forward
    after fused Adam steps), so skipping it "when nothing moved" is not safe.

    derived: [(name, [(src_param, perm | None, rscale | None, scale[, cperm]), ...]), ...] -- prepared weights built from row blocks
    of parameters (rows gathered by the int32 vector `perm` -- columns by `cperm` --, scaled per row by the fp32 vector `rscale` and by the float
    `scale`, in fp32 before the single rounding), written by the SAME launch: matrices in the compute dtype with their
    transposed copy, vectors (biases) in fp32.  derived_weight(key, name) hands them to the linears."""
    params = [p_ for p_ in params if p_.is_cuda and p_.dtype == torch.float32]
    if not params or dtype not in (torch.bfloat16, torch.float32):
        return
    derived = derived or []
    assert not derived or dtype != torch.float32, "derived weights are a compute-dtype (cast) feature"
    # (name, "fold", W0, b0, Wo, bo, c0, cperm): the FOLDED weight [W0[:, :c0] | W0[:, c0:] Wo[:, cperm]] and bias
    # b0 + W0[:, c0:] bo of a linear that consumes cat[x, Wo ctx + bo] (csrc/fold.hip; served by folded_linear())
    folds = [d_ for d_ in derived if len(d_) > 2 and d_[1] == "fold"]
    derived = [d_ for d_ in derived if not (len(d_) > 2 and d_[1] == "fold")]
    dkey = (tuple((name, tuple(id(b_[0]) for b_ in blocks)) for name, blocks in derived)
            + tuple((f[0], "fold", id(f[2]), id(f[4]), f[6]) for f in folds))
    slot = _LP_FLAT.get((key, dtype))
    ptrs = tuple(p_.data_ptr() for p_ in params)          # (`p.data = ...` / module.to() move the storage under the same object)
    if (slot is None or len(slot["params"]) != len(params) or any(a is not b for a, b in zip(slot["params"], params))
            or slot["dkey"] != dkey or slot["ptrs"] != ptrs):
        cast = dtype != torch.float32
        dev = params[0].device
        al = lambda n_: (n_ + 7) // 8 * 8                      # noqa: E731  (16-byte aligned views)
        sizes = [al(p_.numel()) for p_ in params]
        dmat = [(name, blocks) for name, blocks in derived if blocks[0][0].dim() >= 2]
        dvec = [(name, blocks) for name, blocks in derived if blocks[0][0].dim() < 2]
        dsize = lambda blocks: sum(b_[0].numel() for b_ in blocks)   # noqa: E731
        fgeo = []                                               # (R, ldw0, K, N, c0) of every folded linear
        for f in folds:
            w0, wo, c0 = f[2], f[4], int(f[6])
            R, K = w0.shape[0], wo.shape[0]
            ldw0, N = w0.numel() // R, wo.numel() // K
            assert w0.is_contiguous() and wo.is_contiguous() and ldw0 == c0 + K, "fold: W0 must be [R, c0 + K], Wo [K, N]"
            fgeo.append((R, ldw0, K, N, c0))
        fsize = sum(al(R * (c0 + N)) for R, _, _, N, c0 in fgeo)
        flat = torch.empty((sum(sizes) if cast else 0) + sum(al(dsize(bl)) for _, bl in dmat) + fsize, dtype=dtype, device=dev)
        mats = [p_ for p_ in params if p_.dim() >= 2]
        flat_t = torch.empty(sum(al(p_.numel()) for p_ in mats) + sum(al(dsize(bl)) for _, bl in dmat) + fsize, dtype=dtype, device=dev)
        fold32 = torch.empty(sum(al(R * N) + al(R) for R, _, _, N, _ in fgeo), dtype=torch.float32, device=dev)
        flat32 = torch.empty(sum(al(dsize(bl)) for _, bl in dvec), dtype=torch.float32, device=dev)
        views, tviews, rec, off, toff, tile0 = [], {}, b"", 0, 0, 0

        def entry(src, dst, dst_t, rows, cols, perm=None, rscale=None, scale=1.0, ldt=None, flags=0, cperm=None, lds=0, ldd=0):
            nonlocal rec, tile0
            tx = (cols + 31) // 32
            rec += struct.pack("<QQQiiiiQQfiiiQii", src, dst, dst_t, rows, cols, tile0, tx, 0 if perm is None else perm.data_ptr(),
                               0 if rscale is None else rscale.data_ptr(), float(scale), rows if ldt is None else ldt, flags, ldd,
                               0 if cperm is None else cperm.data_ptr(), lds, 0)
            tile0 += tx * ((rows + 31) // 32)

        for p_, sz in zip(params, sizes):
            v = flat[off:off + p_.numel()].view(p_.shape) if cast else p_
            off += sz if cast else 0
            views.append(v)
            rows = p_.shape[0] if p_.dim() >= 2 else 1
            cols = p_.numel() // rows
            vt = None
            if p_.dim() >= 2:
                vt = flat_t[toff:toff + p_.numel()].view(cols, rows)
                toff += al(p_.numel())
                tviews[id(p_)] = vt
            elif not cast:
                continue                                       # fp32 vector: nothing to do
            entry(p_.data_ptr(), v.data_ptr() if cast else 0, 0 if vt is None else vt.data_ptr(), rows, cols)
        dslot, off32, keep = {}, 0, []
        for name, blocks in derived:
            mat = blocks[0][0].dim() >= 2
            cols = blocks[0][0].numel() // blocks[0][0].shape[0]      # (a Conv1d(k=1) weight [O, I, 1] is the matrix [O, I])
            rows_all = sum(b_[0].shape[0] for b_ in blocks)
            if mat:
                v = flat[off:off + rows_all * cols].view(rows_all, cols)
                vt = flat_t[toff:toff + rows_all * cols].view(cols, rows_all)
                off += al(rows_all * cols)
                toff += al(rows_all * cols)
                handle = torch.empty((rows_all, cols), dtype=torch.float32, device=dev)    # never written: _lp() maps it to v
            else:
                v = flat32[off32:off32 + rows_all]
                off32 += al(rows_all)
                vt, handle = None, v
            r0, meta = 0, []
            for blk in blocks:
                src, perm, rscale, scale = blk[:4]
                cperm = blk[4] if len(blk) > 4 else None              # optional column gather (SuperGlue's merge weight)
                assert src.is_contiguous() and src.dtype == torch.float32 and src.numel() == src.shape[0] * cols
                rows = src.shape[0]
                perm = None if perm is None else perm.to(device=dev, dtype=torch.int32).contiguous()
                cperm = None if cperm is None else cperm.to(device=dev, dtype=torch.int32).contiguous()
                rscale = None if rscale is None else rscale.to(device=dev, dtype=torch.float32).contiguous()
                keep += [perm, rscale, cperm]
                esz = v.element_size()
                entry(src.data_ptr(), v.data_ptr() + r0 * cols * esz, 0 if vt is None else vt.data_ptr() + r0 * vt.element_size(),
                      rows, cols, perm, rscale, scale, rows_all, 0 if mat else 1, cperm)
                meta.append((r0, rows, perm, rscale, float(scale), tuple(src.shape), cperm))
                r0 += rows
            dslot[name] = {"view": v, "view_t": vt, "handle": handle, "meta": meta, "cols": cols}
        # folded linears: fp32 products by gf_fold_linear_fwd (its own table, launched first), stacked / cast / transposed by
        # two column-block entries of the cast table
        frec, ftile0, foff = b"", 0, 0
        for f, (R, ldw0, K, N, c0) in zip(folds, fgeo):
            name, _, w0, b0, wo, bo, _, cperm = f
            cperm = None if cperm is None else cperm.to(device=dev, dtype=torch.int32).contiguous()
            keep.append(cperm)
            wc = fold32[foff:foff + R * N].view(R, N)
            foff += al(R * N)
            bc = fold32[foff:foff + R] if (b0 is not None or bo is not None) else None
            foff += al(R)
            wid = c0 + N
            v = flat[off:off + R * wid].view(R, wid)
            vt = flat_t[toff:toff + R * wid].view(wid, R)
            off += al(R * wid)
            toff += al(R * wid)
            esz_ = v.element_size()
            entry(w0.data_ptr(), v.data_ptr(), vt.data_ptr(), R, c0, ldt=R, lds=ldw0, ldd=wid)
            entry(wc.data_ptr(), v.data_ptr() + c0 * esz_, vt.data_ptr() + c0 * R * esz_, R, N, ldt=R, ldd=wid)
            ftx = (N + 63) // 64
            frec += struct.pack("<QQQQQQQiiiiiiii", w0.data_ptr(), wo.data_ptr(), 0 if b0 is None else b0.data_ptr(),
                                0 if bo is None else bo.data_ptr(), 0 if cperm is None else cperm.data_ptr(), wc.data_ptr(),
                                0 if bc is None else bc.data_ptr(), R, K, N, ldw0, c0, ftile0, ftx, 0)
            ftile0 += (ftx + 1) * ((R + 63) // 64)           # (+ 1: the bias tile column of every row block)
            handle = torch.empty((R, wid), dtype=torch.float32, device=dev)      # never written: _lp() maps it to v
            dslot[name] = {"view": v, "view_t": vt, "handle": handle, "bias": bc, "fold": (R, ldw0, K, N, c0), "cperm": cperm}
        esz = _lib.load().gf_cast_entry_bytes()
        assert len(rec) % esz == 0 and esz == 88
        table = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(dev) if rec else None
        ftable = None
        if frec:
            assert len(frec) == len(folds) * _lib.load().gf_fold_entry_bytes()
            ftable = torch.frombuffer(bytearray(frec), dtype=torch.uint8).to(dev)
        slot = {"flat": flat, "flat_t": flat_t, "flat32": flat32, "views": views, "tviews": tviews, "params": params, "table": table,
                "n": len(rec) // esz, "tiles": tile0, "dkey": dkey, "derived": dslot, "keep": keep, "ptrs": ptrs,
                "fold32": fold32, "ftable": ftable, "fn": len(folds), "ftiles": ftile0}
        _LP_FLAT[(key, dtype)] = slot
    if slot["ftable"] is not None:
        _lib.check(_lib.load().gf_fold_linear_fwd(_p(slot["ftable"]), slot["fn"], slot["ftiles"], _stream()), "gf_fold_linear_fwd")
    if slot["table"] is not None:
        _lib.check(_lib.load().gf_multi_cast_transpose(_p(slot["table"]), slot["n"], slot["tiles"], BF16 if dtype == torch.bfloat16 else F32, _stream()),
                   "gf_multi_cast_transpose")
    for p_, v in zip(params, slot["views"]):
        if v is not p_:
            _LP_CACHE[id(p_)] = (p_._version, dtype, v, weakref.ref(p_))
            _LP_PTR[(p_.data_ptr(), p_.numel())] = (p_._version, dtype, v, weakref.ref(p_))   # views (conv weight.squeeze(-1))
        vt = slot["tviews"].get(id(p_))
        if vt is not None:
            _LP_T[v.data_ptr()] = (vt, weakref.ref(p_), dtype)
    for d in slot["derived"].values():
        h, v = d["handle"], d["view"]
        if d["view_t"] is not None:             # matrices: the fp32 handle stands for the compute-dtype view
            _LP_PTR[(h.data_ptr(), h.numel())] = (h._version, dtype, v, weakref.ref(h))
            _LP_T[v.data_ptr()] = (d["view_t"], weakref.ref(h), dtype)


class _DerivedWeight(torch.autograd.Function):
    """The autograd face of a derived weight (precast(derived=...)): forward hands out the prepared tensor -- for a matrix
    an fp32 HANDLE that _lp() / _wt_t() resolve to the compute-dtype copy and its transpose written by this forward's
    precast launch, for a vector the fp32 values themselves --, backward sends the gradient of each row block back to its
    source parameter (gf_weight_grad_map: un-gather, scales)."""

    @staticmethod
    def forward(ctx, d, *srcs):
        ctx.d = d
        return d["handle"].view(d["handle"].shape)          # a fresh alias: the cached tensor keeps no autograd state

    @staticmethod
    def backward(ctx, g):
        d = ctx.d
        g = g.float().contiguous()
        outs = []
        for i, (r0, rows, perm, rscale, scale, shape, cperm) in enumerate(d["meta"]):
            if not ctx.needs_input_grad[1 + i]:
                outs.append(None)
                continue
            gi = g[r0:r0 + rows]
            if perm is None and rscale is None and scale == 1.0 and cperm is None:
                outs.append(gi.reshape(shape))
                continue
            out = torch.empty(shape, dtype=torch.float32, device=g.device)
            _lib.check(_lib.load().gf_weight_grad_map(_p(gi), _p(out), None if perm is None else _p(perm),
                                                      None if cperm is None else _p(cperm),
                                                      None if rscale is None else _p(rscale), scale, rows, d["cols"], _stream()),
                       "gf_weight_grad_map")
            outs.append(out)
        return (None, *outs)


def derived_weight(key, dtype, name, *srcs):
    """The prepared weight `name` of this forward's precast(key=..., derived=...) launch, differentiable w.r.t. the source
    parameters of its row blocks (passed again here, in block order, so autograd sees them), or None when this forward
    did not precast it (fp32 parity mode: the caller builds the weight with torch ops)."""
    slot = _LP_FLAT.get((key, dtype))
    d = None if slot is None else slot["derived"].get(name)
    if d is None:
        return None
    return _DerivedWeight.apply(d, *srcs)


class _FoldedLinear(torch.autograd.Function):
    """The autograd face of a folded linear (precast(derived=[(name, "fold", ...)]), csrc/fold.hip): forward hands out the
    fp32 HANDLE of the stacked weight [W0a | W0b Wo] (resolved by _lp() / _wt_t() to the compute-dtype copy and its transpose
    this forward's precast launch wrote) and the folded bias b0 + W0b bo (fp32 values); backward turns their gradients into
    those of W0, b0, Wo, bo with ONE launch (gf_fold_linear_bwd)."""

    @staticmethod
    def forward(ctx, d, w0, b0, wo, bo):
        ctx.d = d
        ctx.save_for_backward(w0, wo, bo)
        ctx.has = (b0 is not None, bo is not None)
        bias = d["bias"]
        return d["handle"].view(d["handle"].shape), (None if bias is None else bias.view(bias.shape))

    @staticmethod
    def backward(ctx, gw, gb):
        w0, wo, bo = ctx.saved_tensors
        R, ldw0, K, N, c0 = ctx.d["fold"]
        if gw is None:
            gw = torch.zeros((R, c0 + N), dtype=torch.float32, device=w0.device)
        gw = gw.float().contiguous()
        gb = None if gb is None else gb.float().contiguous()
        dw0, dwo = torch.empty_like(w0), torch.empty_like(wo)
        dbo = torch.empty_like(bo) if ctx.has[1] else None
        cperm = ctx.d["cperm"]
        _lib.check(_lib.load().gf_fold_linear_bwd(_p(gw), _p(gb), _p(w0), _p(wo), _p(bo) if ctx.has[1] else None,
                                                  None if cperm is None else _p(cperm), _p(dw0), _p(dwo), _p(dbo),
                                                  R, K, N, ldw0, c0, _stream()), "gf_fold_linear_bwd")
        if dbo is not None and gb is None:
            dbo = None
        return None, dw0, (gb if ctx.has[0] else None), dwo, dbo


def folded_linear(key, dtype, name, w0, b0, wo, bo):
    """(weight handle, bias) of the folded linear `name` of this forward's precast(key=..., derived=...) launch --
    y = linear_cat(x, ctx, weight, bias) then equals W0 cat[x, Wo ctx + bo] + b0 -- differentiable w.r.t. the four
    parameters, or None when this forward did not prepare it (fp32 parity mode: the caller runs the two linears)."""
    from . import FOLD_ENABLED      # the package attribute, read at call time: tools/probe/ab_matcher.py rebinds it
    slot = _LP_FLAT.get((key, dtype)) if FOLD_ENABLED else None
    d = None if slot is None else slot["derived"].get(name)
    if d is None or "fold" not in d:
        return None
    return _FoldedLinear.apply(d, w0, b0, wo, bo)


def invalidate_precast():
    """Forget the per-parameter cache entries (the flat buffers stay): needed when parameters change without a
    version bump, e.g. after a captured optimiser step is replayed from a hipGraph."""
    _LP_CACHE.clear()
    _LP_PTR.clear()
    _LP_T.clear()


def _lp(t, dtype):
    """t in `dtype`: the precast copy when it is current, else a fresh cast."""
    if t is None or t.dtype == dtype:
        return t
    hit = _LP_CACHE.get(id(t))
    if hit is not None and hit[3]() is t and hit[0] == t._version and hit[1] == dtype:
        return hit[2]
    if t.is_contiguous():          # a reshaped view of a precast parameter (e.g. a Conv1d weight without its kernel axis)
        hit = _LP_PTR.get((t.data_ptr(), t.numel()))
        if hit is not None and hit[3]() is not None and hit[0] == t._version and hit[1] == dtype:
            return hit[2].view(t.shape)
    return t.to(dtype)


def _wt_t(wt, k0=None, k1=None):
    """Columns [k0, k1) of the [N,K] compute-dtype weight, transposed and contiguous ([k1-k0, N]: the "weight" of the
    input-gradient GEMM dx = dy W).  Served from this forward's precast() when there is one (no kernel), else copied."""
    hit = _LP_T.get(wt.data_ptr())
    n = wt.shape[0]
    kk = wt.numel() // n
    if hit is not None and hit[1]() is not None and hit[2] == wt.dtype and hit[0].shape == (kk, n):
        wt_t = hit[0]
        return wt_t if k0 is None else wt_t[k0:k1]
    w2 = wt.reshape(n, kk)
    return (w2 if k0 is None else w2[:, k0:k1]).t().contiguous()
