"""GlueStick line message passing and line head (csrc/line_layer.hip, line_head.hip)."""
import torch

from .. import lib as _lib
from ._base import _chk, _dt, _p, _stream
from ._assignment import bgemm


# ------------------------------------------------------------------------------ GlueStick line message passing
@torch.no_grad()
def _line_graph_sorted(idx, n):
    """line_graph by a stable sort (any size): endpoints grouped by junction in their original order + segment starts."""
    B = idx.shape[0]
    order = torch.argsort(idx, dim=1, stable=True)
    sorted_idx = idx.gather(1, order).contiguous()
    seg = torch.searchsorted(sorted_idx, torch.arange(n + 1, device=idx.device).expand(B, -1).contiguous())
    return order.to(torch.int32).contiguous(), seg.to(torch.int32).contiguous()


@torch.no_grad()
def line_graph(idx, n):
    """idx [B,E] int64 junction of every line endpoint -> (order [B,E] int32: endpoints grouped by junction, stable;
    seg [B,n+1] int32: segment starts).  Built once per forward: all line layers (and the backward) share it."""
    _chk(idx)
    idx = idx.contiguous()
    B, E = idx.shape
    # a junction index outside [0, n) would corrupt LDS in the kernels below; the torch gather they replace raises too
    # (device-side assert: no host synchronisation)
    torch._assert_async(((idx >= 0) & (idx < n)).all())
    if E > 4096 or n > 8192:
        # gf_line_csr keeps one image's junction graph in LDS (4096 endpoints, 8192 junctions): larger graphs -- far beyond the
        # 250-512 lines of the shipped configurations -- are built by a stable sort instead (same order / segment arrays)
        return _line_graph_sorted(idx, n)
    order = torch.empty((B, E), dtype=torch.int32, device=idx.device)
    seg = torch.empty((B, n + 1), dtype=torch.int32, device=idx.device)
    _lib.check(_lib.load().gf_line_csr(_p(idx), _p(order), _p(seg), B, E, n, _stream()), "gf_line_csr")
    return order, seg


def _segsum(s0, s1, order, seg, base, B, E, N, D, mode):
    out = torch.empty((B, N, D), dtype=s0.dtype, device=s0.device)
    _lib.check(_lib.load().gf_line_segsum(_p(s0), s0.stride(1), _p(s1), 0 if s1 is None else s1.stride(1), _p(order),
                                          _p(seg), _p(base), _p(out), B, E, N, D, mode, _dt(s0), _stream()),
               "gf_line_segsum")
    return out


class _LineGather(torch.autograd.Function):
    """msg [B,E,3D] = [x[idx[e]] | x[idx[e^1]] | enc[e]] (gluestick.py:609-621); backward: deterministic segment sums."""

    @staticmethod
    def forward(ctx, x, enc, idx, order, seg, chain=None):
        _chk(x, enc, idx)
        x, enc, idx = x.contiguous(), enc.contiguous(), idx.contiguous()
        B, N, D = x.shape
        E = idx.shape[1]
        msg = torch.empty((B, E, 3 * D), dtype=x.dtype, device=x.device)
        _lib.check(_lib.load().gf_line_gather(_p(x), _p(idx), _p(enc), _p(msg), B, E, N, D, _dt(x), _stream()),
                   "gf_line_gather")
        ctx.save_for_backward(order, seg)
        ctx.dims = (B, E, N, D)
        ctx.chain = chain
        return msg

    @staticmethod
    def backward(ctx, dmsg):
        order, seg = ctx.saved_tensors
        B, E, N, D = ctx.dims
        if not dmsg.is_contiguous():
            dmsg = dmsg.contiguous()
        # chain: the residual gradient of the same x (parked by _LineAggregate.backward) is the base of the segment sum
        base = ctx.chain.take() if ctx.chain is not None else None
        dx = _segsum(dmsg[:, :, :D], dmsg[:, :, D:2 * D], order, seg, base, B, E, N, D, 0)
        return dx, dmsg[:, :, 2 * D:], None, None, None, None


class _LineAggregate(torch.autograd.Function):
    """x + (mean | sum) over the endpoints on each junction of upd [B,E,D] (gluestick.py:660-700)."""

    @staticmethod
    def forward(ctx, x, upd, idx, order, seg, mean, chain=None):
        _chk(x, upd, idx)
        x, upd = x.contiguous(), upd.contiguous()
        B, N, D = x.shape
        E = upd.shape[1]
        out = _segsum(upd, None, order, seg, x, B, E, N, D, 1 if mean else 0)
        ctx.save_for_backward(idx.contiguous(), seg)
        ctx.dims = (B, E, N, D, mean)
        ctx.chain = chain
        return out

    @staticmethod
    def backward(ctx, g):
        idx, seg = ctx.saved_tensors
        B, E, N, D, mean = ctx.dims
        if not g.is_contiguous():
            g = g.contiguous()
        dupd = torch.empty((B, E, D), dtype=g.dtype, device=g.device)
        _lib.check(_lib.load().gf_line_expand(_p(g), _p(idx), _p(seg), _p(dupd), B, E, N, D, 1 if mean else 0, _dt(g),
                                              _stream()), "gf_line_expand")
        if ctx.chain is not None:                  # x's residual gradient rides in the gather's segment sum (see GradChain)
            ctx.chain.park(g)
            g = None
        return g, dupd, None, None, None, None, None


def line_gather(x, enc, idx, order, seg, chain=None):
    """chain: ops.GradChain(2) shared with the line_aggregate of the same x (a LineLayer reads its descriptors twice: the
    endpoint gather and the residual of the aggregation): the two gradients meet in the gather's segment-sum kernel."""
    return _LineGather.apply(x, enc, idx, order, seg, chain if x.requires_grad else None)


def line_aggregate(x, upd, idx, order, seg, mean=True, chain=None):
    return _LineAggregate.apply(x, upd, idx, order, seg, mean, chain if x.requires_grad else None)


# ------------------------------------------------------------------------------ GlueStick line head (dense scores)
class _RowsGather(torch.autograd.Function):
    """out[b,e,:] = x[b, idx[b,e], :]; backward: deterministic segment sum over the junction graph (order, seg)."""

    @staticmethod
    def forward(ctx, x, idx, order, seg):
        _chk(x, idx)
        x = x.contiguous()
        B, N, D = x.shape
        E = idx.shape[1]
        out = torch.empty((B, E, D), dtype=x.dtype, device=x.device)
        _lib.check(_lib.load().gf_rows_gather(_p(x), _p(idx), _p(out), B, E, N, D, _dt(x), _stream()), "gf_rows_gather")
        ctx.save_for_backward(order, seg)
        ctx.n = N
        return out

    @staticmethod
    def backward(ctx, g):
        order, seg = ctx.saved_tensors
        g = g.contiguous()
        B, E, D = g.shape
        return _segsum(g, None, order, seg, None, B, E, ctx.n, D, 0), None, None, None


def rows_gather(x, idx, order, seg):
    return _RowsGather.apply(x, idx.contiguous(), order, seg)


class _LinePairScores(torch.autograd.Function):
    """raw[a,c] = scale/2 * max(S[2a,2c] + S[2a+1,2c+1], S[2a,2c+1] + S[2a+1,2c]) with S = g0 g1^T the endpoint
    scores (gluestick.py:345-354), fp32.  S is kept for the backward (16 MB per pair at 512 lines); the gradient
    reaches g0 / g1 through two gf_bgemm products."""

    @staticmethod
    def forward(ctx, g0, g1, scale):
        g0, g1 = g0.float().contiguous(), g1.float().contiguous()
        B, E0, D = g0.shape
        E1 = g1.shape[1]
        S = bgemm(g0, g1.transpose(1, 2), alpha=scale)
        raw = torch.empty((B, E0 // 2, E1 // 2), dtype=torch.float32, device=g0.device)
        _lib.check(_lib.load().gf_line_pair_scores(_p(S), None, _p(raw), B, E0 // 2, E1 // 2, 0, _stream()),
                   "gf_line_pair_scores")
        ctx.save_for_backward(g0, g1, S)
        ctx.scale = scale
        return raw

    @staticmethod
    def backward(ctx, draw):
        g0, g1, S = ctx.saved_tensors
        B, E0, _ = g0.shape
        E1 = g1.shape[1]
        dS = torch.empty_like(S)
        draw = draw.contiguous()
        _lib.check(_lib.load().gf_line_pair_scores(_p(S), _p(draw), _p(dS), B, E0 // 2, E1 // 2, 1, _stream()),
                   "gf_line_pair_scores")
        return bgemm(dS, g1, alpha=ctx.scale), bgemm(dS.transpose(1, 2), g0, alpha=ctx.scale), None


def line_pair_scores(g0, g1, scale):
    return _LinePairScores.apply(g0, g1, scale)


def _dense_rowcol(z, M, N, mode):
    B = z.shape[0]
    rows = torch.empty((B, M), dtype=torch.float32, device=z.device)
    cols = torch.empty((B, N), dtype=torch.float32, device=z.device)
    _lib.check(_lib.load().gf_dense_rowcol(_p(z), z.stride(0), z.stride(1), _p(rows), _p(cols), B, M, N, mode, _stream()),
               "gf_dense_rowcol")
    return rows, cols


class _DenseLogDoubleSoftmax(torch.autograd.Function):
    """gluestick.py:772-783 on a dense fp32 [B,M,N] score matrix with a learnable bin score beta:
    out[:, :M, :N] = raw - (r_i + c_j) / 2, out[:, :M, N] = beta - r_i, out[:, M, :N] = beta - c_j, out[:, M, N] = 0 with
    r_i = log(sum_j exp raw_ij + exp beta), c_j likewise over rows.  The [B,M,N] passes are HIP kernels
    (csrc/line_head.hip); the [B,M] / [B,N] vector algebra stays in torch."""

    @staticmethod
    def forward(ctx, raw, beta):
        _chk(raw)
        raw = raw.float().contiguous()
        B, M, N = raw.shape
        beta = beta.float().reshape(())
        r0, c0 = _dense_rowcol(raw, M, N, 0)
        r, c = torch.logaddexp(r0, beta), torch.logaddexp(c0, beta)
        out = torch.empty((B, M + 1, N + 1), dtype=torch.float32, device=raw.device)
        rb, cb, br, bc = (-0.5 * r).contiguous(), (-0.5 * c).contiguous(), (beta - r).contiguous(), (beta - c).contiguous()
        _lib.check(_lib.load().gf_dense_assign(_p(raw), _p(rb), _p(cb), _p(br), _p(bc), 0.0, _p(out),
                                               B, M, N, _stream()), "gf_dense_assign")
        ctx.save_for_backward(raw, r, c, beta)
        return out

    @staticmethod
    def backward(ctx, G):
        raw, r, c, beta = ctx.saved_tensors
        B, M, N = raw.shape
        G = G.float().contiguous()
        gs_r, gs_c = _dense_rowcol(G, M, N, 1)                    # sums of the core block of G ([B,M+1,N+1] view strides)
        A = 0.5 * gs_r + G[:, :M, N]                              # gradient arriving at -r_i
        Bv = 0.5 * gs_c + G[:, M, :N]                             # ... at -c_j
        draw = torch.empty_like(raw)
        A, Bv = A.contiguous(), Bv.contiguous()      # (named: a temporary's storage could be reused before the launch reads it)
        _lib.check(_lib.load().gf_dense_assign_bwd(_p(raw), _p(r), _p(c), _p(A), _p(Bv), _p(G),
                                                   _p(draw), B, M, N, _stream()), "gf_dense_assign_bwd")
        dbeta = (G[:, :M, N] - A * torch.exp(beta - r)).sum() + (G[:, M, :N] - Bv * torch.exp(beta - c)).sum()
        return draw, dbeta


def dense_log_double_softmax(raw, beta):
    return _DenseLogDoubleSoftmax.apply(raw, beta)
