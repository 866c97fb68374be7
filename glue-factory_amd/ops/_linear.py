"""Linear layers (csrc/gemm_*.hip, linear_dw.hip, rowdot.hip, elementwise.hip): GEMM dispatch, GradChain, the linear /
row-dot / LayerNorm+GELU nodes."""
import torch

from .. import lib as _lib
from ._base import _chk, _dt, _p, _stream
from ._params import _lp, _wt_t


# ------------------------------------------------------------------------------ linear layer
# ---- GEMMs of the linear layers: the hand-written weight-streaming kernel gf_gemm (csrc/gemm_ws.hip) is the path of
# every forward and input-gradient GEMM it supports (N % 32 == 0, K a power of two in [32, 512] -- [32, 256] in fp32 --
# or a sum of such pieces, which are accumulated through the fused residual input).  Anything else (3- or 5-channel
# encoder inputs, 1-channel heads) is a tiny library call.
_GEMM_KMAX = {torch.bfloat16: 512, torch.float32: 256}


def _k_pieces(k, dtype):
    """Split K into power-of-two pieces gf_gemm takes (largest first); None if impossible."""
    kmax = _GEMM_KMAX.get(dtype)
    if kmax is None or k < 32:
        return None
    out, rest = [], k
    while rest:
        piece = min(kmax, 1 << (rest.bit_length() - 1))
        if piece < 32:
            return None
        out.append(piece)
        rest -= piece
    return out


def _row_ok(t, dtype):
    al = 8 if dtype == torch.bfloat16 else 4
    return t.stride(1) == 1 and t.stride(0) % al == 0 and t.data_ptr() % 16 == 0


def gemm(x2, wt, bias=None, res2=None, out=None, x2b=None, cs=None, rot_n=0, res3=None):
    """y [M,N] = [x2 | x2b] wt^T (+ bias) (+ res2) (+ res3), optional rotary epilogue; x2 / x2b / wt / res2 / res3 2-D with unit
    inner stride, all in the compute dtype (bias: any float dtype).  ``out`` may alias ``res2``.  Returns y.
    res3: a second residual, fused on the streamed kernel's shapes (gf_gemm_res2), added beforehand otherwise."""
    M, K0 = x2.shape
    N = wt.shape[0]
    dtype = x2.dtype
    K1 = 0 if x2b is None else x2b.shape[1]
    if res3 is not None:
        if res2 is None:
            res2, res3 = res3, None
        else:
            if res3.dim() != 2:
                res3 = res3.reshape(M, N)
            fused = (dtype == torch.bfloat16 and cs is None and x2.is_cuda and wt.dtype == dtype and (K0 + K1) in (256, 512)
                     and (K1 == 0 or K1 == K0) and N % 256 == 0 and M % 64 == 0 and res2.dtype == dtype and res3.dtype == dtype
                     and all(_row_ok(t_, dtype) for t_ in (x2, wt, res2, res3) + ((x2b,) if x2b is not None else ())
                             + ((out,) if out is not None else ())))
            if fused:
                y = torch.empty((M, N), dtype=dtype, device=x2.device) if out is None else out
                b32 = None if bias is None else bias.detach().float().contiguous()
                rc = _lib.load().gf_gemm_res2(_p(x2), _p(x2b), _p(wt), _p(b32), _p(res2), _p(res3), _p(y), M, N, K0, K1,
                                              x2.stride(0), 0 if x2b is None else x2b.stride(0), wt.stride(0), res2.stride(0),
                                              res3.stride(0), y.stride(0), _dt(x2), _stream())
                if rc == 0:
                    return y
                if rc != -1:
                    _lib.check(rc, "gf_gemm_res2")
            res2, res3 = res2 + res3, None
    ok = (x2.is_cuda and dtype in _GEMM_KMAX and wt.dtype == dtype and N % 32 == 0 and _row_ok(x2, dtype)
          and _row_ok(wt, dtype) and (x2b is None or (x2b.dtype == dtype and _row_ok(x2b, dtype)))
          and (res2 is None or (res2.dtype == dtype and _row_ok(res2, dtype)))
          and (out is None or _row_ok(out, dtype)))
    plan = None
    if ok:
        if x2b is not None and K1 == K0 and _k_pieces(K0 + K1, dtype) == [K0 + K1]:
            plan = "two"
        else:
            p0 = _k_pieces(K0, dtype)
            p1 = _k_pieces(K1, dtype) if x2b is not None else []
            if p0 is not None and p1 is not None:
                plan = "pieces"
    if plan is None:                                  # library fallback for the odd shapes: counted and reported once per shape
        _note_library_gemm(M, N, K0 + K1, dtype)
        xx = x2 if x2b is None else torch.cat([x2, x2b], 1)
        y = torch.nn.functional.linear(xx, wt, None if bias is None else _lp(bias, dtype))
        if res2 is not None:
            y = y + res2
        if cs is not None:
            raise RuntimeError("rotary epilogue needs the gf_gemm path")
        if out is not None:
            out.copy_(y)
            return out
        return y
    L = _lib.load()
    y = torch.empty((M, N), dtype=dtype, device=x2.device) if out is None else out
    b32 = None if bias is None else bias.detach().float().contiguous()
    st = _stream()
    dt = _dt(x2)
    if plan == "two":
        _lib.check(L.gf_gemm(_p(x2), _p(x2b), _p(wt), _p(b32), _p(res2), _p(y), _p(cs), rot_n, M, N, K0, K1,
                             x2.stride(0), x2b.stride(0), wt.stride(0), 0 if res2 is None else res2.stride(0),
                             y.stride(0), dt, st), "gf_gemm")
        return y
    # K pieces: the first call carries bias / residual, the others accumulate into y through the residual input;
    # a rotary epilogue rides on the last one
    pieces = [(x2, k0, n) for k0, n in _offsets(_k_pieces(K0, dtype))]
    if x2b is not None:
        pieces += [(x2b, k0, n) for k0, n in _offsets(_k_pieces(K1, dtype))]
    wofs = 0
    for i, (src, k0, n) in enumerate(pieces):
        first, last = i == 0, i == len(pieces) - 1
        xs = src[:, k0:k0 + n]
        ws = wt[:, wofs:wofs + n]
        r = res2 if first else y
        _lib.check(L.gf_gemm(_p(xs), None, _p(ws), _p(b32) if first else None, _p(r), _p(y),
                             _p(cs) if last else None, rot_n if last else 0, M, N, n, 0,
                             xs.stride(0), 0, ws.stride(0), 0 if r is None else r.stride(0), y.stride(0), dt, st),
                   "gf_gemm")
        wofs += n
    return y


LIBRARY_GEMMS = {}       # (M, N, K, dtype) -> number of products that left the hand-written path (ops.gemm's fallback)


def _note_library_gemm(M, N, K, dtype):
    """A product outside gf_gemm's plans (N % 32, K not a sum of powers of two >= 32, misaligned rows, fp32 K > 256 pieces ...)
    runs on the vendor library.  Correct, but not the path the rooflines describe: say so once per shape instead of silently."""
    key = (int(M), int(N), int(K), str(dtype))
    n = LIBRARY_GEMMS.get(key, 0)
    LIBRARY_GEMMS[key] = n + 1
    if n == 0:
        import warnings
        warnings.warn(f"glue_factory_amd.ops.gemm: [{M} x {K}] x [{N} x {K}]^T in {dtype} is outside gf_gemm's plans and runs on the "
                      "vendor library (ops.LIBRARY_GEMMS counts these calls)", RuntimeWarning, stacklevel=3)


def gemm_takes(k, n, dtype):
    """True when a [*, k] x [n, k]^T product runs as ONE gf_gemm launch (needed for its rotary epilogue)."""
    return n % 32 == 0 and _k_pieces(k, dtype) == [k]


def _offsets(sizes):
    out, o = [], 0
    for n in sizes:
        out.append((o, n))
        o += n
    return out


def _linear_fwd(x2, wt, bias, res2=None, out=None, cs=None, rot_n=0):
    """y [M,N] = x2 [M,K] wt[N,K]^T + bias (+ res2).  bias: the fp32 master."""
    return gemm(x2, wt, bias, res2, out, cs=cs, rot_n=rot_n)


class GradChain:
    """Sums the gradient contributions of ONE tensor that feeds several linears of a block (residual, FFN input,
    projection) inside the GEMM epilogues instead of leaving them to autograd's accumulation (one 3-pass add kernel
    per extra consumer): every consumer but the designated last one parks its contribution here and returns no
    gradient; the last one's input-gradient GEMM adds the parked sum in its residual epilogue and returns the total.
    The last consumer must be the one whose backward runs last -- true by data dependence for the transformer blocks
    (the projection's gradient needs the attention backward, which needs the FFN's) and checked by the counter."""
    __slots__ = ("acc", "got", "expected", "closed", "extra")

    def __init__(self, consumers):
        self.acc, self.got, self.expected, self.closed = None, 0, consumers - 1, False
        # a second parked tensor that has not been added to `acc` yet: it rides as the SECOND residual of the next link's
        # GEMM (gf_gemm_res2) -- the place where a loss head's gradient meets the block's residual gradient
        self.extra = None

    def pop_extra(self):
        e, self.extra = self.extra, None
        return e

    def park(self, g, counted=True):
        """counted=False: an OPTIONAL contribution (the per-layer loss heads of LightGlue, which exist only when the
        fused loss is evaluated and whose backward always runs before the blocks': they were created later)."""
        if self.closed:
            raise RuntimeError("GradChain: a contribution arrived after the last consumer closed the chain (it would be lost)")
        self.acc = g
        if counted:
            self.got += 1

    def take(self):
        if self.got != self.expected:
            raise RuntimeError(f"GradChain: {self.got} of {self.expected} contributions arrived before the last consumer")
        acc, self.acc, self.got, self.closed = self.acc, None, 0, True
        extra = self.pop_extra()
        if extra is not None:           # no link in between took it along: one explicit add after all
            acc = extra if acc is None else acc + extra
        return acc


def _flat2(t, n):
    t2 = t.reshape(-1, n)
    return t2 if t2.is_contiguous() else t2.contiguous()


def _dw(dy2, x2, nout, k, with_bias, x2b=None, k1=0):
    """fp32 (dW [nout, k], db [nout] or None) of y = x W^T + b from dy2 [M, nout] and x = x2 [M, k] or, with ``x2b``, the
    virtual concatenation [x2 (k1 columns) | x2b] in one launch (gf_linear_dw2: the caller checks its shape limits).
    The only place that allocates for, and calls, the weight-gradient kernels."""
    L = _lib.load()
    m = x2.shape[0]
    ws = torch.empty(int(L.gf_linear_dw_ws_bytes(m, nout, k)), dtype=torch.uint8, device=x2.device)
    dw32 = torch.empty((nout, k), dtype=torch.float32, device=x2.device)
    db32 = torch.empty((nout,), dtype=torch.float32, device=x2.device) if with_bias else None
    if x2b is None:
        _lib.check(L.gf_linear_dw(_p(dy2), _p(x2), _p(dw32), _p(db32), _p(ws), m, nout, k, _dt(x2), _stream()),
                   "gf_linear_dw")
    else:
        _lib.check(L.gf_linear_dw2(_p(dy2), _p(x2), _p(x2b), k1, _p(dw32), _p(db32), _p(ws), m, nout, k, _dt(x2),
                                   _stream()), "gf_linear_dw2")
    return dw32, db32


class _Linear(torch.autograd.Function):
    """y = x W^T + b (+ res) (+ rotary epilogue): forward and input-gradient GEMM on gf_gemm (library GEMM only for
    shapes outside its plans), weight / bias gradient (a tiny-output, 1e5-deep reduction) on gf_linear_dw, which
    returns fp32 gradients for the fp32 master parameters directly.  ``res`` is a fused residual (gradient = dy)."""

    @staticmethod
    def forward(ctx, x, w, b, res=None, cs=None, rot_n=0, chain=None, chain_last=False, res_chain=None, out=None):
        ctx.chain, ctx.chain_last, ctx.res_chain = chain, chain_last, res_chain
        wt = _lp(w, x.dtype)
        k = x.shape[-1]
        x2 = x.reshape(-1, k)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        res2 = None
        if res is not None:
            res2 = res.reshape(-1, wt.shape[0])
            if not res2.is_contiguous():
                res2 = res2.contiguous()
        out2 = None if out is None else out.view(-1, wt.shape[0])       # caller-owned destination (contiguous rows)
        y = _linear_fwd(x2, wt, b, res2, out=out2, cs=cs, rot_n=rot_n).view(*x.shape[:-1], wt.shape[0])
        ctx.save_for_backward(x, wt)
        ctx.wdtype = w.dtype
        ctx.has_bias = b is not None
        ctx.bdtype = None if b is None else b.dtype
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wt = ctx.saved_tensors
        nout, k = wt.shape
        dy2 = dy.reshape(-1, nout)
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dx = dw = db = None
        dres = dy if ctx.has_res and ctx.needs_input_grad[3] else None
        if dres is not None and ctx.res_chain is not None:       # first link of the residual tensor's chain
            d2 = _flat2(dres, nout)
            rc = ctx.res_chain
            if rc.acc is not None:      # optional contributions got here first (the previous output's loss heads): they wait
                if rc.extra is not None:                     # in `extra` for the next link's two-residual GEMM
                    d2 = d2 + rc.pop_extra()
                rc.extra = rc.acc
            rc.park(d2)
            dres = None
        if ctx.needs_input_grad[0]:
            ch = ctx.chain
            if ch is None:
                dx = gemm(dy2, _wt_t(wt)).view(x.shape)
            elif ctx.chain_last is True:
                dx = gemm(dy2, _wt_t(wt), res2=ch.take()).view(x.shape)
            else:                                       # chain_last == "extra": an optional, uncounted contribution
                ch.park(gemm(dy2, _wt_t(wt), res2=ch.acc, res3=ch.pop_extra()), counted=ctx.chain_last != "extra")
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            x2 = x.reshape(-1, k)
            if not x2.is_contiguous():
                x2 = x2.contiguous()
            dw32, db32 = _dw(dy2, x2, nout, k, ctx.has_bias)
            dw = dw32.to(ctx.wdtype)
            db = None if db32 is None else db32.to(ctx.bdtype)
        return dx, dw, db, dres, None, None, None, None, None, None


def linear(x, w, b=None, res=None, rotary_cs=None, rot_n=0, chain=None, chain_last=False, res_chain=None, out=None):
    """w, b: fp32 master parameters (or differentiable functions of them); x (and the optional fused residual
    ``res``, same shape as the output) in the compute dtype.  ``rotary_cs`` [.., 64] fp32 interleaved (cos, sin):
    the output channels [0, rot_n) leave the GEMM already rotated (the buffer then belongs to
    self_attention_rotary(pre_rotated=True), whose backward hands the UN-rotated gradient back to this node).
    ``chain`` / ``res_chain``: GradChain of x / of res (see there); only used when that tensor requires grad.
    ``out``: optional destination with the output's shape (e.g. a slice of a per-layer buffer): written, and returned."""
    _chk(x)
    if rotary_cs is not None:
        rotary_cs = rotary_cs.reshape(-1, rotary_cs.shape[-1])
        assert rotary_cs.shape[-1] == 64 and rotary_cs.dtype == torch.float32 and rotary_cs.is_contiguous()
    if not x.requires_grad:
        chain = None
    if res is None or not res.requires_grad:
        res_chain = None
    return _Linear.apply(x, w, b, res, rotary_cs, rot_n, chain, chain_last, res_chain, out)


class _LinearCat(torch.autograd.Function):
    """y = [x1 | x2] W^T + b without building the concatenation: two accumulating GEMMs forward, two
    input-gradient GEMMs and two gf_linear_dw calls backward (the FFN input cat[x, message] of
    lightglue.py:163 / :219-220)."""

    @staticmethod
    def forward(ctx, x1, x2, w, b, chain1=None):
        ctx.chain1 = chain1
        k1 = x1.shape[-1]
        wt = _lp(w, x1.dtype)
        a2 = x1.reshape(-1, k1)
        c2 = x2.reshape(-1, x2.shape[-1])
        a2 = a2 if a2.is_contiguous() else a2.contiguous()
        c2 = c2 if c2.is_contiguous() else c2.contiguous()
        y = gemm(a2, wt, b, x2b=c2).view(*x1.shape[:-1], wt.shape[0])
        ctx.save_for_backward(x1, x2, wt)
        ctx.wdtype = w.dtype
        ctx.bdtype = None if b is None else b.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, x2, wt = ctx.saved_tensors
        nout, k = wt.shape
        k1 = x1.shape[-1]
        dy2 = dy.reshape(-1, nout)
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dx1 = None
        if ctx.needs_input_grad[0]:
            ch = ctx.chain1
            if ch is None:
                dx1 = gemm(dy2, _wt_t(wt, 0, k1)).view(x1.shape)
            else:                                   # a middle link: the parked residual gradient rides in the epilogue
                ch.park(gemm(dy2, _wt_t(wt, 0, k1), res2=ch.acc, res3=ch.pop_extra()))
        dx2 = gemm(dy2, _wt_t(wt, k1, wt.shape[1])).view(x2.shape) if ctx.needs_input_grad[1] else None
        dw = db = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            a = x1.reshape(-1, k1)
            c = x2.reshape(-1, k - k1)
            a = a if a.is_contiguous() else a.contiguous()
            c = c if c.is_contiguous() else c.contiguous()
            if a.dtype == torch.bfloat16 and nout % 128 == 0 and k1 % 128 == 0 and (k - k1) % 128 == 0:
                # ONE launch over the virtual concatenation (gf_linear_dw2): dY streamed once, dw comes out whole
                dw32, db32 = _dw(dy2, a, nout, k, ctx.bdtype is not None, x2b=c, k1=k1)
                dw = dw32.to(ctx.wdtype)
            else:
                dwa, db32 = _dw(dy2, a, nout, k1, ctx.bdtype is not None)
                dwb, _ = _dw(dy2, c, nout, k - k1, False)
                dw = torch.cat([dwa, dwb], 1).to(ctx.wdtype)
            db = None if db32 is None else db32.to(ctx.bdtype)
        return dx1, dx2, dw, db, None


def linear_cat(x1, x2, w, b=None, chain1=None):
    _chk(x1, x2)
    return _LinearCat.apply(x1, x2, w, b, chain1 if x1.requires_grad else None)


class _RowDot(torch.autograd.Function):
    """z = x w^T + b for a single output channel (w [1,C], b [1]); returns fp32 [..]."""

    @staticmethod
    def forward(ctx, x, w, b, chain=None, counted=True):
        ctx.chain, ctx.counted = chain, counted
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        M = x2.shape[0]
        w32 = w.reshape(-1).float().contiguous()
        z = torch.empty(M, dtype=torch.float32, device=x.device)
        # the bias stays on the device (no .item() sync): the kernel reads the parameter itself
        b32 = None if b is None else b.detach().reshape(-1).float()
        _lib.check(_lib.load().gf_rowdot_fwd(_p(x2), _p(w32), 0.0, _p(b32), _p(z), M, C, _dt(x2), _stream()), "gf_rowdot_fwd")
        ctx.save_for_backward(x2, w32)
        ctx.meta = (x.shape, w.shape, w.dtype, None if b is None else b.dtype)
        return z.view(x.shape[:-1])

    @staticmethod
    def backward(ctx, dz):
        x2, w32 = ctx.saved_tensors
        xshape, wshape, wdt, bdt = ctx.meta
        M, C = x2.shape
        L = _lib.load()
        dz = dz.reshape(-1).float().contiguous()
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        ch = ctx.chain if dx is not None else None
        base = None if ch is None else ch.acc           # the chain's running sum rides in this kernel (dx = base + dz w)
        if ch is not None and ch.extra is not None:
            e = ch.pop_extra()
            base = e if base is None else base + e
        part = torch.empty((L.gf_rowdot_nblk(M), C + 1), dtype=torch.float32, device=x2.device)
        _lib.check(L.gf_rowdot_bwd(_p(x2), _p(dz), _p(w32), _p(dx), _p(base), _p(part), M, C, _dt(x2), _stream()),
                   "gf_rowdot_bwd")
        s = part.sum(0)
        dw = s[:C].reshape(wshape).to(wdt)
        db = None if bdt is None else s[C:].to(bdt)
        if ch is not None:
            ch.park(dx, counted=ctx.counted)
            dx = None
        return (None if dx is None else dx.view(xshape)), dw, db, None, None


class _RowDot2(torch.autograd.Function):
    """(z0, z1) = (x w0^T + b0, x.detach() w1^T + b1) for two single-output heads on the same rows with ONE read of x
    (gf_rowdot2_*): a LightGlue layer's matchability (differentiable w.r.t. x: the rank-1 term joins x's gradient chain) and
    token-confidence logits (the reference feeds that head desc.detach(), lightglue.py:81-94)."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1, chain=None, counted=True):
        ctx.chain, ctx.counted = chain, counted
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        M = x2.shape[0]
        w0f, w1f = w0.reshape(-1).float().contiguous(), w1.reshape(-1).float().contiguous()
        z0 = torch.empty(M, dtype=torch.float32, device=x.device)
        z1 = torch.empty(M, dtype=torch.float32, device=x.device)
        b0f = None if b0 is None else b0.detach().reshape(-1).float()
        b1f = None if b1 is None else b1.detach().reshape(-1).float()
        _lib.check(_lib.load().gf_rowdot2_fwd(_p(x2), _p(w0f), _p(w1f), _p(b0f), _p(b1f), _p(z0), _p(z1), M, C, _dt(x2),
                                              _stream()), "gf_rowdot2_fwd")
        ctx.save_for_backward(x2, w0f)
        ctx.meta = (x.shape, w0.shape, w0.dtype, None if b0 is None else b0.dtype, w1.shape, w1.dtype,
                    None if b1 is None else b1.dtype)
        return z0.view(x.shape[:-1]), z1.view(x.shape[:-1])

    @staticmethod
    def backward(ctx, dz0, dz1):
        x2, w0f = ctx.saved_tensors
        xshape, w0shape, w0dt, b0dt, w1shape, w1dt, b1dt = ctx.meta
        M, C = x2.shape
        L = _lib.load()
        dz0 = torch.zeros(M, dtype=torch.float32, device=x2.device) if dz0 is None else dz0.reshape(-1).float().contiguous()
        dz1 = torch.zeros(M, dtype=torch.float32, device=x2.device) if dz1 is None else dz1.reshape(-1).float().contiguous()
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        ch = ctx.chain if dx is not None else None
        base = None if ch is None else ch.acc
        if ch is not None and ch.extra is not None:
            e = ch.pop_extra()
            base = e if base is None else base + e
        part = torch.empty((L.gf_rowdot_nblk(M), 2, C + 1), dtype=torch.float32, device=x2.device)
        _lib.check(L.gf_rowdot2_bwd(_p(x2), _p(dz0), _p(dz1), _p(w0f), _p(dx), _p(base), _p(part), M, C, _dt(x2), _stream()),
                   "gf_rowdot2_bwd")
        s = part.sum(0)                                        # [2, C + 1]: ONE reduction for both heads
        dw0 = s[0, :C].reshape(w0shape).to(w0dt)
        db0 = None if b0dt is None else s[0, C:].to(b0dt)
        dw1 = s[1, :C].reshape(w1shape).to(w1dt)
        db1 = None if b1dt is None else s[1, C:].to(b1dt)
        if ch is not None:
            ch.park(dx, counted=ctx.counted)
            dx = None
        return (None if dx is None else dx.view(xshape)), dw0, db0, dw1, db1, None, None


def rowdot2(x, w0, b0, w1, b1, chain=None, counted=True):
    """See _RowDot2.  ``chain``: GradChain of x (the input gradient of head 0 is parked there)."""
    _chk(x)
    if not x.requires_grad:
        chain = None
    return _RowDot2.apply(x, w0, b0, w1, b1, chain, counted)


def rowdot(x, w, b=None, chain=None, counted=True):
    """``chain``: GradChain of x -- the input gradient is parked there (added to the chain's running sum inside the
    kernel) instead of being returned."""
    _chk(x)
    if not x.requires_grad:
        chain = None
    return _RowDot.apply(x, w, b, chain, counted)


# ------------------------------------------------------------------------------ LN + GELU
class _LnGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        _chk(x, gamma, beta)
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        R = x2.shape[0]
        g32, b32 = gamma.float().contiguous(), beta.float().contiguous()
        y = torch.empty_like(x2)
        mean = torch.empty(R, dtype=torch.float32, device=x.device)
        rstd = torch.empty(R, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().gf_ln_gelu_fwd(_p(x2), _p(g32), _p(b32), _p(y), _p(mean), _p(rstd),
                                              R, C, float(eps), _dt(x2), _stream()), "gf_ln_gelu_fwd")
        ctx.save_for_backward(x2, g32, b32, mean, rstd)
        ctx.shape = x.shape
        ctx.pdtypes = (gamma.dtype, beta.dtype)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, g32, b32, mean, rstd = ctx.saved_tensors
        R, C = x2.shape
        dy2 = dy.reshape(R, C)
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        L = _lib.load()
        nblk = L.gf_ln_gelu_nblk(R)
        dx = torch.empty_like(x2)
        part = torch.empty((2, nblk, C), dtype=torch.float32, device=x2.device)        # per-block dgamma | dbeta partials
        _lib.check(L.gf_ln_gelu_bwd(_p(x2), _p(g32), _p(b32), _p(mean), _p(rstd), _p(dy2), _p(dx),
                                    _p(part[0]), _p(part[1]), R, C, _dt(x2), _stream()), "gf_ln_gelu_bwd")
        sums = colsum(part)                                                             # one deterministic reduction
        return (dx.view(ctx.shape), sums[0].to(ctx.pdtypes[0]), sums[1].to(ctx.pdtypes[1]), None)


def colsum(x):
    """out[g, c] = sum_r x[g, r, c] for contiguous fp32 x [G, R, C] (deterministic two-stage reduction)."""
    _chk(x)
    G, R, C = x.shape
    L = _lib.load()
    ws = torch.empty(L.gf_colsum_ws_floats(G, C), dtype=torch.float32, device=x.device)
    out = torch.empty((G, C), dtype=torch.float32, device=x.device)
    _lib.check(L.gf_colsum_f32(_p(x), _p(ws), _p(out), G, R, C, _stream()), "gf_colsum_f32")
    return out


class _SmallLinear(torch.autograd.Function):
    """theta = x W^T for a tall fp32 x [M, K] with K <= 8 input columns (the Fourier positional encoding's Wr,
    lightglue.py:52-65): the forward is the stock product (tiny), the weight gradient a dedicated reduction
    (gf_small_dw) instead of a skinny library GEMM over M = 131072 rows."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        O, K = w.shape
        if not x.is_cuda or K > 8 or x.dtype != torch.float32 or w.dtype != torch.float32:
            return torch.nn.functional.linear(x, w)
        x2 = x.reshape(-1, K).contiguous()
        y = torch.empty((x2.shape[0], O), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().gf_small_fwd(_p(x2), _p(w.contiguous()), _p(y), x2.shape[0], O, K, _stream()), "gf_small_fwd")
        return y.view(*x.shape[:-1], O)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        O, K = w.shape
        g2, x2 = g.reshape(-1, O).float().contiguous(), x.reshape(-1, K).float().contiguous()
        dx = g @ w if ctx.needs_input_grad[0] else None       # (keypoints / scores carry no gradient on the train path)
        L = _lib.load()
        if not g2.is_cuda or K > 8 or O * K > 256:
            _note_library_gemm(g2.shape[0], O, K, "fp32 (small_linear weight gradient)")
            return dx, (g2.t() @ x2).to(w.dtype)
        ws = torch.empty(L.gf_small_dw_ws_floats(O, K), dtype=torch.float32, device=g2.device)
        dw = torch.empty((O, K), dtype=torch.float32, device=g2.device)
        _lib.check(L.gf_small_dw(_p(g2), _p(x2), _p(ws), _p(dw), g2.shape[0], O, K, _stream()), "gf_small_dw")
        return dx, dw.to(w.dtype)


def small_linear(x, w):
    return _SmallLinear.apply(x, w)


def ln_gelu(x, gamma, beta, eps=1e-5):
    return _LnGelu.apply(x, gamma, beta, eps)
