"""Assignment head, per-layer loss and nearest-neighbour matching (csrc/assignment.hip, head_bwd.hip, lg_loss.hip, bgemm.hip,
nn_match.hip)."""
import torch

from .. import lib as _lib
from ._base import _chk, _dt, _p, _stream
from ._nll import _known_sparse


# ------------------------------------------------------------------------------ assignment head
def _mat3(t):
    assert t.dim() == 3
    return t if t.is_contiguous() else t.contiguous()


def rows_lse(a, b, colbias=None):
    """lse[b,i] = log sum_j exp(a_i . b_j + colbias_j); no autograd (see dual_lse)."""
    _chk(a, b, colbias)
    a, b = _mat3(a), _mat3(b)
    B, M, D = a.shape
    N = b.shape[1]
    out = torch.empty((B, M), dtype=torch.float32, device=a.device)
    cb = None if colbias is None else colbias.float().contiguous()
    _lib.check(_lib.load().gf_rows_lse(_p(a), _p(b), _p(cb), _p(out), B, M, N, D, _dt(a), _stream()),
               "gf_rows_lse")
    return out


@torch.no_grad()
def rows_argmax(a, b, colbias=None, alpha=1.0):
    """max_j / argmax_j of alpha * a_i . b_j + colbias_j  ->  ([B,M] float, [B,M] int64)."""
    _chk(a, b, colbias)
    a, b = _mat3(a), _mat3(b)
    B, M, D = a.shape
    N = b.shape[1]
    vmax = torch.empty((B, M), dtype=torch.float32, device=a.device)
    arg = torch.empty((B, M), dtype=torch.int64, device=a.device)
    cb = None if colbias is None else colbias.float().contiguous()
    _lib.check(_lib.load().gf_rows_argmax(_p(a), _p(b), _p(cb), float(alpha), _p(vmax), _p(arg),
                                          B, M, N, D, _dt(a), _stream()), "gf_rows_argmax")
    return vmax, arg


def bgemm(a, b, out=None, alpha=1.0):
    """out[bt] = alpha * a[bt] @ b[bt] for 3-d a [B,M,K], b [B,K,N] with ARBITRARY strides (transposed views cost
    nothing); fp32 operands on the exact-fp32 MFMA.  No autograd (callers own their backward)."""
    _chk(a, b)
    assert a.dim() == 3 and b.dim() == 3 and a.shape[0] == b.shape[0] and a.shape[2] == b.shape[1] and a.dtype == b.dtype
    B, M, K = a.shape
    N = b.shape[2]
    if out is None:
        out = torch.empty((B, M, N), dtype=a.dtype, device=a.device)
    st = lambda t: _lib.strides(t.stride(0), t.stride(1), t.stride(2))  # noqa: E731
    _lib.check(_lib.load().gf_bgemm(_p(a), _p(b), _p(out), B, M, N, K, st(a), st(b), st(out), float(alpha), _dt(a),
                                    _stream()), "gf_bgemm")
    return out


def _head_bwd(a, b, r, c, gr, gc, da, db):
    """da = dS b, db = dS^T a for dS = P_row * gr + P_col * gc (module docstring of _DualLSE), written into the given
    buffers.  bf16 / D = 256: the fused gf_head_bwd (no dS tensor); otherwise dS is written once and two batched
    products (gf_bgemm) follow."""
    B, M, D = a.shape
    N = b.shape[1]
    if a.dtype == torch.bfloat16 and D == 256 and da.is_contiguous() and db.is_contiguous():
        _lib.check(_lib.load().gf_head_bwd(_p(a), _p(b), _p(r), _p(c), _p(gr), _p(gc), _p(da), _p(db), B, M, N, D,
                                           _dt(a), _stream()), "gf_head_bwd")
        return
    dS = torch.empty((B, M, N), dtype=a.dtype, device=a.device)
    _lib.check(_lib.load().gf_dual_softmax_bwd(_p(a), _p(b), _p(r), _p(c), _p(gr), _p(gc), None, 0,
                                               0.0, _p(dS), B, M, N, D, _dt(a), _stream()), "gf_dual_softmax_bwd")
    bgemm(dS, b, out=da)                       # exact-fp32 MFMA in the fp32 parity mode: no library product on the path
    bgemm(dS.transpose(1, 2), a, out=db)


class _DualLSE(torch.autograd.Function):
    """(r, c) = (LSE_j S_ij, LSE_i S_ij) for S = a b^T, never materialising S.
    Backward: dS = P_row * gr + P_col * gc (written once in the compute dtype), then two GEMMs."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _mat3(a), _mat3(b)
        r = rows_lse(a, b)
        c = rows_lse(b, a)
        ctx.save_for_backward(a, b, r, c)
        return r, c

    @staticmethod
    def backward(ctx, gr, gc):
        a, b, r, c = ctx.saved_tensors
        B, M, D = a.shape
        N = b.shape[1]
        gr = torch.zeros_like(r) if gr is None else gr.float().contiguous()
        gc = torch.zeros_like(c) if gc is None else gc.float().contiguous()
        da, db = torch.empty_like(a), torch.empty_like(b)
        _head_bwd(a, b, r, c, gr, gc, da, db)
        return da, db


def dual_lse(a, b):
    return _DualLSE.apply(a, b)


class _DualLSEStacked(torch.autograd.Function):
    """dual_lse on a batch-stacked md [2B,N,D] (image 0 = first half): the gradient comes back as ONE
    stacked tensor (the two GEMMs write into its halves), so autograd needs no slice/zero-fill/add."""

    @staticmethod
    def forward(ctx, md):
        B = md.shape[0] // 2
        a, b = md[:B], md[B:]
        r = rows_lse(a, b)
        c = rows_lse(b, a)
        ctx.save_for_backward(md, r, c)
        return r, c

    @staticmethod
    def backward(ctx, gr, gc):
        md, r, c = ctx.saved_tensors
        B2, N, D = md.shape
        B = B2 // 2
        a, b = md[:B], md[B:]
        gr = torch.zeros_like(r) if gr is None else gr.float().contiguous()
        gc = torch.zeros_like(c) if gc is None else gc.float().contiguous()
        d = torch.empty_like(md)
        _head_bwd(a, b, r, c, gr, gc, d[:B], d[B:])
        return d


def dual_lse_stacked(md):
    return _DualLSEStacked.apply(md)


class _LGLayerLoss(torch.autograd.Function):
    """Partial sums acc [B,4] of one layer's deep-supervision loss (gf_lg_loss_fwd) from the batch-stacked
    head inputs md [2B,N,D], z [2B,N] (matchability logits), t [2B,N] (token-confidence logits or None).
    One node in the autograd graph: its backward writes d(md) (dense double-softmax part + sparse positives),
    dz and dt directly."""

    @staticmethod
    def forward(ctx, md, z, t, rc, pos, neg0, neg1, fin0, fin1):
        _chk(md, z, t)
        lib = _lib.load()
        md = _mat3(md)
        B2, N, D = md.shape
        B = B2 // 2
        a, b = md[:B], md[B:]
        z = z.float().contiguous()
        if rc is None:
            c = rows_lse(b, a)
            r = None
        else:
            r, c = (x.detach().float().contiguous() for x in rc)
        pb, pi, pj = (x.contiguous() for x in pos)
        P = pb.shape[0]
        neg0, neg1 = neg0.float().contiguous(), neg1.float().contiguous()
        acc = torch.empty((B, 4), dtype=torch.float32, device=md.device)
        tgt = None
        if t is not None or r is None:      # three passes: c, then (r, row arg-max), then column arg-max
            st = torch.empty((5, B, N), dtype=torch.float32, device=md.device)
            ar = torch.empty((2, B, N), dtype=torch.int64, device=md.device)
            v0, v1, a0, a1 = st[0], st[1], ar[0], ar[1]
            want_r = r is None
            if want_r:
                r = st[2]
            _lib.check(lib.gf_rows_lse_argmax(_p(a), _p(b), _p(z[B:]), _p(c), 2.0, _p(r) if want_r else None,
                                              _p(v0), _p(a0), B, N, N, D, _dt(md), _stream()), "gf_rows_lse_argmax")
            if t is not None:
                _lib.check(lib.gf_rows_lse_argmax(_p(b), _p(a), _p(z[:B]), _p(r), 2.0, None, _p(v1), _p(a1),
                                                  B, N, N, D, _dt(md), _stream()), "gf_rows_lse_argmax")
        if t is not None:
            t = t.float().contiguous()
            tgt = torch.empty((B2, N), dtype=torch.float32, device=md.device)
            fin0, fin1 = fin0.contiguous(), fin1.contiguous()
            extra = (_p(t[:B]), _p(t[B:]), _p(v0), _p(a0), _p(v1), _p(a1), _p(fin0), _p(fin1), _p(tgt[:B]), _p(tgt[B:]))
        else:
            extra = (None,) * 10
        _lib.check(lib.gf_lg_loss_fwd(_p(a), _p(b), _p(z[:B]), _p(z[B:]), _p(r), _p(c), _p(pb), _p(pi), _p(pj), P,
                                      _p(neg0), _p(neg1), *extra, _p(acc), B, N, N, D, _dt(md), _stream()),
                   "gf_lg_loss_fwd")
        ctx.save_for_backward(md, z, t, r, c, tgt, pb, pi, pj, neg0, neg1)
        return acc

    @staticmethod
    def backward(ctx, gacc):
        md, z, t, r, c, tgt, pb, pi, pj, neg0, neg1 = ctx.saved_tensors
        lib = _lib.load()
        B2, N, D = md.shape
        B = B2 // 2
        P = pb.shape[0]
        a, b = md[:B], md[B:]
        gacc = gacc.float().contiguous()
        dz = torch.empty_like(z)
        dt = None if t is None else torch.empty_like(t)
        grc = torch.empty((2, B, N), dtype=torch.float32, device=md.device)
        tp = (None,) * 4 if t is None else (_p(t[:B]), _p(t[B:]), _p(tgt[:B]), _p(tgt[B:]))
        dtp = (None, None) if t is None else (_p(dt[:B]), _p(dt[B:]))
        _lib.check(lib.gf_lg_loss_bwd_tokens(_p(z[:B]), _p(z[B:]), _p(neg0), _p(neg1), *tp, _p(pb), _p(pi), _p(pj), P,
                                             _p(gacc), _p(dz[:B]), _p(dz[B:]), *dtp, _p(grc[0]), _p(grc[1]),
                                             B, N, N, _stream()), "gf_lg_loss_bwd_tokens")
        d = torch.empty_like(md)
        _head_bwd(a, b, r, c, grc[0], grc[1], d[:B], d[B:])
        _lib.check(lib.gf_lg_loss_bwd_rows(_p(a), _p(b), _p(pb), _p(pi), _p(pj), P, _p(gacc), _p(d[:B]), _p(d[B:]),
                                           B, N, N, D, _dt(md), _stream()), "gf_lg_loss_bwd_rows")
        return d, dz, dt, None, None, None, None, None, None


def lg_layer_loss(md, z, t, rc, pos, neg0, neg1, fin0, fin1):
    """acc [B,4] = (sum_pos A_ij, sum of weighted dustbin terms, sum bce image 0, sum bce image 1)."""
    return _LGLayerLoss.apply(md, z, t, rc, pos, neg0, neg1, fin0, fin1)


class _AssignWrite(torch.autograd.Function):
    """out[b,i,j] = alpha a_i.b_j + rowbias_i + colbias_j, plus dustbin column/row/corner."""

    @staticmethod
    def forward(ctx, a, b, rowbias, colbias, bin_col, bin_row, alpha, corner, expsum=None):
        # corner: python float, or a 0-d / [B] tensor (differentiable, e.g. SuperGlue's bin_score)
        # expsum: optional [B] fp32 buffer, filled with sum_{i<M, j<=N} exp(out) (not differentiable)
        _chk(a, b, rowbias, colbias, bin_col, bin_row)
        corner_t = corner if torch.is_tensor(corner) else None
        corner = 0.0 if corner_t is not None else corner
        a, b = _mat3(a), _mat3(b)
        B, M, D = a.shape
        N = b.shape[1]
        rb, cb, bc, br = (t.float().contiguous() for t in (rowbias, colbias, bin_col, bin_row))
        out = torch.empty((B, M + 1, N + 1), dtype=torch.float32, device=a.device)
        _lib.check(_lib.load().gf_assign_write(_p(a), _p(b), _p(rb), _p(cb), _p(bc), _p(br),
                                               float(alpha), float(corner), _p(out), _p(expsum), B, M, N, D,
                                               _dt(a), _stream()), "gf_assign_write")
        if corner_t is not None:
            out[:, -1, -1] = corner_t.detach().float()
        ctx.corner_shape = None if corner_t is None else corner_t.shape
        ctx.save_for_backward(a, b)
        ctx.alpha = alpha
        ctx.dts = (rowbias.dtype, colbias.dtype, bin_col.dtype, bin_row.dtype)
        return out

    @staticmethod
    def backward(ctx, G):
        # Dense upstream gradient: only reached when somebody differentiates through the
        # materialised matrix (never in the training step, whose loss heads are sparse).
        a, b = ctx.saved_tensors
        sp = _known_sparse(G)
        if sp is not None:
            # the upstream node was the NLL of the matrix itself (GlueStick's point head): G holds one positive per row at
            # most plus the dustbin row / column, so the two products are a row gather and a row scatter -- O((M + N) D)
            # instead of two [M, N] x [N, D] products, a cast pass and two reductions over the dense gradient
            idx, vpos, n0, n1 = sp
            d = ctx.dts
            wv = (ctx.alpha * vpos)[..., None]
            da = db = grow = gcol = None
            if ctx.needs_input_grad[0]:
                da = (wv * b.gather(1, idx[..., None].expand(-1, -1, b.shape[2])).float()).to(a.dtype)
            if ctx.needs_input_grad[1]:
                db = torch.zeros(b.shape, dtype=torch.float32, device=b.device).scatter_add_(
                    1, idx[..., None].expand(-1, -1, a.shape[2]), wv * a.float()).to(b.dtype)
            if ctx.needs_input_grad[2]:
                grow = vpos.to(d[0])
            if ctx.needs_input_grad[3]:
                gcol = torch.zeros((b.shape[0], b.shape[1]), dtype=torch.float32, device=b.device).scatter_add_(1, idx, vpos).to(d[1])
            gcorner = None
            if ctx.corner_shape is not None:
                gcorner = G[:, -1, -1].sum() if len(ctx.corner_shape) == 0 else G[:, -1, -1].reshape(ctx.corner_shape)
            return (da, db, grow, gcol, n0.to(d[2]), n1.to(d[3]), None, gcorner, None)
        core = G[:, :-1, :-1]
        g = core.to(a.dtype, memory_format=torch.contiguous_format)      # ONE pass over the dense gradient; alpha rides in the products
        da = bgemm(g, b, alpha=ctx.alpha) if ctx.needs_input_grad[0] else None
        db = bgemm(g.transpose(1, 2), a, alpha=ctx.alpha) if ctx.needs_input_grad[1] else None
        d = ctx.dts
        gcorner = None
        if ctx.corner_shape is not None:
            gcorner = G[:, -1, -1].sum() if len(ctx.corner_shape) == 0 else G[:, -1, -1].reshape(ctx.corner_shape)
        grow = core.sum(2).to(d[0]) if ctx.needs_input_grad[2] else None     # (SuperGlue's couplings have no row / column bias)
        gcol = core.sum(1).to(d[1]) if ctx.needs_input_grad[3] else None
        return (da, db, grow, gcol, G[:, :-1, -1].to(d[2]), G[:, -1, :-1].to(d[3]), None, gcorner, None)


def assign_write(a, b, rowbias, colbias, bin_col, bin_row, alpha=2.0, corner=0.0, with_expsum=False):
    """-> out [B,M+1,N+1]; with_expsum: (out, expsum [B]) where expsum = exp(out)[:, :-1].sum((1, 2)), detached."""
    if not with_expsum:
        return _AssignWrite.apply(a, b, rowbias, colbias, bin_col, bin_row, alpha, corner)
    expsum = torch.empty((a.shape[0],), dtype=torch.float32, device=a.device)
    return _AssignWrite.apply(a, b, rowbias, colbias, bin_col, bin_row, alpha, corner, expsum), expsum


@torch.no_grad()
def filter_matches(max0, arg0, arg1, th):
    """Mutual-NN filter from the row/column arg-max vectors -> (m0, m1, s0, s1)."""
    _chk(max0, arg0, arg1)
    B, M = arg0.shape
    N = arg1.shape[1]
    max0, arg0, arg1 = max0.float().contiguous(), arg0.contiguous(), arg1.contiguous()
    m0 = torch.empty((B, M), dtype=torch.int64, device=arg0.device)
    m1 = torch.empty((B, N), dtype=torch.int64, device=arg0.device)
    s0 = torch.empty((B, M), dtype=torch.float32, device=arg0.device)
    s1 = torch.empty((B, N), dtype=torch.float32, device=arg0.device)
    _lib.check(_lib.load().gf_filter_matches(_p(max0), _p(arg0), _p(arg1), float(th), _p(m0), _p(m1),
                                             _p(s0), _p(s1), B, M, N, _stream()), "gf_filter_matches")
    return m0, m1, s0, s1


# ------------------------------------------------------------------------------ nearest-neighbour matcher (csrc/nn_match.hip)
@torch.no_grad()
def rows_top2(a, b):
    """(best, arg, second) of every row of a b^T without the [B,M,N] tensor -> ([B,M] float, [B,M] int64, [B,M] float).
    `second` is the second element of the row as a multiset (a duplicated maximum gives second == best); the lowest index
    wins a tie."""
    _chk(a, b)
    a, b = _mat3(a), _mat3(b)
    assert a.dtype == b.dtype and a.shape[0] == b.shape[0] and a.shape[2] == b.shape[2]
    B, M, D = a.shape
    N = b.shape[1]
    best = torch.empty((B, M), dtype=torch.float32, device=a.device)
    arg = torch.empty((B, M), dtype=torch.int64, device=a.device)
    second = torch.empty((B, M), dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().gf_rows_top2(_p(a), _p(b), _p(best), _p(arg), _p(second), B, M, N, D, _dt(a), _stream()),
               "gf_rows_top2")
    return best, arg, second


@torch.no_grad()
def nn_filter(top0, top1, ratio_thresh=None, distance_thresh=None, mutual=True):
    """find_nn's ratio / distance thresholds and mutual_check on the rows_top2 triples of both directions
    -> (m0, m1, s0, s1); a falsy threshold is "not set", as in the reference."""
    best0, arg0, sec0 = (t.contiguous() for t in top0)
    best1, arg1, sec1 = (t.contiguous() for t in top1)
    _chk(best0, arg0, sec0, best1, arg1, sec1)
    B, M = arg0.shape
    N = arg1.shape[1]
    dev = arg0.device
    m0 = torch.empty((B, M), dtype=torch.int64, device=dev)
    m1 = torch.empty((B, N), dtype=torch.int64, device=dev)
    s0 = torch.empty((B, M), dtype=torch.float32, device=dev)
    s1 = torch.empty((B, N), dtype=torch.float32, device=dev)
    r2 = float(ratio_thresh) ** 2 if ratio_thresh else -1.0
    d2 = float(distance_thresh) ** 2 if distance_thresh else -1.0
    _lib.check(_lib.load().gf_nn_filter(_p(best0), _p(arg0), _p(sec0), _p(best1), _p(arg1), _p(sec1), r2, d2,
                                        int(bool(mutual)), _p(m0), _p(m1), _p(s0), _p(s1), B, M, N, _stream()),
               "gf_nn_filter")
    return m0, m1, s0, s1


class _Similarity(torch.autograd.Function):
    """sim = a b^T [B,M,N] in the operands' dtype; backward da = dsim b, db = dsim^T a (all three through gf_bgemm)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _mat3(a), _mat3(b)
        ctx.save_for_backward(a, b)
        return bgemm(a, b.transpose(1, 2))

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.to(a.dtype, memory_format=torch.contiguous_format)
        da = bgemm(g, b) if ctx.needs_input_grad[0] else None
        db = bgemm(g.transpose(1, 2), a) if ctx.needs_input_grad[1] else None
        return da, db


def similarity(a, b):
    return _Similarity.apply(a, b)


class _NPairLoss(torch.autograd.Function):
    """(nll [B], num [B]) of the N-pair loss on a dense similarity with the positives (pb, pi, pj) (pj < 0 = padding):
    nll = -sum_pos (2 score - lse_row - lse_col) / (2 num), num = max(#positives, 1), score = T (2 - sqrt(max(2 (1 - sim),
    1e-6))).  The backward writes dsim dense in one pass and reduces dT on the device."""

    @staticmethod
    def forward(ctx, sim, temperature, pb, pi, pj):
        _chk(sim, temperature, pb, pi, pj)
        s = sim.detach().float().contiguous()
        t = temperature.detach().float().reshape(1)
        pb, pi, pj = (x.long().contiguous() for x in (pb, pi, pj))
        B, M, N = s.shape
        P = pb.shape[0]
        dev = s.device
        lse_row = torch.empty((B, M), dtype=torch.float32, device=dev)
        lse_col = torch.empty((B, N), dtype=torch.float32, device=dev)
        acc = torch.empty((2, B), dtype=torch.float32, device=dev)
        cnt_row = torch.empty((B, M), dtype=torch.float32, device=dev)
        cnt_col = torch.empty((B, N), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().gf_npair_fwd(_p(s), _p(t), _p(pb), _p(pi), _p(pj), P, _p(lse_row), _p(lse_col), _p(acc[0]),
                                            _p(acc[1]), _p(cnt_row), _p(cnt_col), B, M, N, _stream()), "gf_npair_fwd")
        num = acc[1].clamp(min=1.0)
        ctx.save_for_backward(s, t, lse_row, lse_col, cnt_row, cnt_col, num, pb, pi, pj)
        ctx.meta = (sim.dtype, temperature.dtype, temperature.shape)
        ctx.mark_non_differentiable(num)
        return -acc[0] / (2.0 * num), num

    @staticmethod
    def backward(ctx, g, _gnum):
        s, t, lse_row, lse_col, cnt_row, cnt_col, num, pb, pi, pj = ctx.saved_tensors
        B, M, N = s.shape
        coef = (g.float() / (2.0 * num)).contiguous()
        dsim = torch.empty_like(s)
        dT = torch.empty((1,), dtype=torch.float32, device=s.device)
        _lib.check(_lib.load().gf_npair_bwd(_p(s), _p(t), _p(lse_row), _p(lse_col), _p(cnt_row), _p(cnt_col), _p(coef),
                                            _p(pb), _p(pi), _p(pj), pb.shape[0], _p(dsim), _p(dT), B, M, N, _stream()),
                   "gf_npair_bwd")
        sdt, tdt, tshape = ctx.meta
        return dsim.to(sdt), dT.reshape(tshape).to(tdt), None, None, None


def n_pair_loss(sim, temperature, pos):
    """-> (nll [B], num [B]) for sim [B,M,N], a scalar temperature tensor and pos = (b, i, j) index vectors (j < 0 is
    padding).  A (b, i, j) listed k times is a positive of weight k, in the loss, in num and in both gradients."""
    return _NPairLoss.apply(sim, temperature, *pos)
