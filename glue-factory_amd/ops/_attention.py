"""Attention family (csrc/attention*.hip): generic, rotary self, bidirectional cross and fused-qkv attention."""
import weakref

import torch

from .. import lib as _lib
from ._base import _chk, _dt, _p, _s3, _stream


# ------------------------------------------------------------------------------ attention
ATTN_SPLIT = 4       # GF_ATTN_SPLIT (include/gf_amd.h): P / dS as hi + lo bf16 pairs = fp32-equivalent second products


def attn_fwd_raw(q, k, v, scale, out=None, lse=None, split=False, o32=None):
    """split (bf16 only): fp32-equivalent second products; o32: [B, Nq, H, D] fp32 contiguous buffer that receives the
    un-rounded output next to `out` (attn_bwd_raw(split=True) takes it as its `o`)."""
    _chk(q, k, v)
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    o = torch.empty((B, Nq, H, D), dtype=q.dtype, device=q.device) if out is None else out
    if lse is None:
        lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    split = bool(split) and q.dtype == torch.bfloat16
    assert o32 is None or (o32.dtype == torch.float32 and o32.is_contiguous() and tuple(o32.shape) == (B, Nq, H, D))
    _lib.check(_lib.load().gf_attn_fwd_ex(_p(q), _p(k), _p(v), _p(o), _p(lse), B, H, Nq, Nk, D,
                                          _s3(q), _s3(k), _s3(v), _s3(o), float(scale), _dt(q), ATTN_SPLIT if split else 0,
                                          _p(o32) if split else None, _stream()), "gf_attn_fwd_ex")
    return o, lse


def attn_bwd_raw(q, k, v, o, do, lse, dq, dk, dv, scale, acc_dq=False, acc_dk=False, split=False):
    """split (bf16 only): `o` must be the fp32 copy attn_fwd_raw(split=True, o32=...) wrote."""
    B, Nq, H, D = q.shape
    split = bool(split) and q.dtype == torch.bfloat16
    assert not split or o.dtype == torch.float32
    Nk = k.shape[1]
    if do.stride(3) != 1:
        do = do.contiguous()
    delta = lse.new_empty((2,) + tuple(lse.shape))      # scratch: the two per-row vectors the dQ kernel hands to dK/dV
    _lib.check(_lib.load().gf_attn_bwd_acc(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(delta),
                                       _p(dq), _p(dk), _p(dv), B, H, Nq, Nk, D,
                                       _s3(q), _s3(k), _s3(v), _s3(o), _s3(do), _s3(dq), _s3(dk),
                                       _s3(dv), float(scale), _dt(q),
                                       int(acc_dq) | 2 * int(acc_dk) | (ATTN_SPLIT if split else 0), _stream()),
               "gf_attn_bwd_acc")


class _Attention(torch.autograd.Function):
    """o = softmax(scale q k^T) v on [B,N,H,D] views (generic entry, used by SuperGlue/GlueStick)."""

    @staticmethod
    def forward(ctx, q, k, v, scale, split=False):
        split = bool(split) and q.dtype == torch.bfloat16
        o32 = torch.empty(q.shape, dtype=torch.float32, device=q.device) if split else None
        o, lse = attn_fwd_raw(q, k, v, scale, split=split, o32=o32)
        ctx.save_for_backward(q, k, v, o32 if split else o, lse)
        ctx.scale, ctx.split = scale, split
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dq, dk, dv = (t.contiguous() for t in (dq, dk, dv))
        attn_bwd_raw(q, k, v, o, do, lse, dq, dk, dv, ctx.scale, split=ctx.split)
        return dq, dk, dv, None, None


def attention(q, k, v, scale=None, split=False):
    """split: fp32-equivalent second products on bf16 operands (GF_ATTN_SPLIT; no effect on fp32 tensors)."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    return _Attention.apply(q, k, v, scale, split)


class _SelfAttentionRotary(torch.autograd.Function):
    """Rotary(q,k) + self attention on the fused projection qkv [B,N,3,H,D].

    qkv is the private output buffer of the Wqkv GEMM: it is rotated IN PLACE (nobody else
    reads it) and kept for the backward.  theta [B,N,D/2] are the pair angles (differentiable,
    they carry the gradient to posenc.Wr); cs [B,N,D] = interleaved (cos, sin) of theta."""

    @staticmethod
    def forward(ctx, qkv, theta, cs, pre_rotated=False, scale=None, theta_sum=None):
        _chk(qkv, cs)
        ctx.theta_sum = theta_sum
        B, N, three, H, D = qkv.shape
        assert three == 3 and qkv.is_contiguous() and cs.is_contiguous() and cs.dtype == torch.float32
        L = _lib.load()
        if not pre_rotated:      # else: q and k left the Wqkv GEMM already rotated (gf_gemm's rotary epilogue)
            _lib.check(L.gf_rotary_qk(_p(qkv), _p(cs), B, N, H, D, 0, _dt(qkv), _stream()), "gf_rotary_qk")
        ctx.scale = D ** -0.5 if scale is None else scale
        o, lse = attn_fwd_raw(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], ctx.scale)
        ctx.save_for_backward(qkv, cs, o, lse)
        ctx.theta_dtype = theta.dtype
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, cs, o, lse = ctx.saved_tensors
        B, N, _, H, D = qkv.shape
        dqkv = torch.empty_like(qkv)
        attn_bwd_raw(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], o, do, lse,
                     dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2], ctx.scale)
        dtheta = torch.empty((B, N, D // 2), dtype=torch.float32, device=qkv.device)
        ts = ctx.theta_sum
        base = None if ts is None else ts.acc
        _lib.check(_lib.load().gf_rotary_qk_bwd(_p(dqkv), _p(qkv), _p(cs), _p(dtheta), _p(base), B, N, H, D,
                                                _dt(qkv), _stream()), "gf_rotary_qk_bwd")
        if ts is not None:          # the layers share theta: only the LAST backward returns the (complete) sum
            dtheta = ts.add(dtheta)
            if dtheta is None:
                return dqkv, None, None, None, None, None
        return dqkv, dtheta.to(ctx.theta_dtype), None, None, None, None


class SharedGradSum:
    """Gradient of ONE tensor consumed by `consumers` nodes of the same kind (the rotary angles of LightGlue's L self
    blocks): every node's backward kernel adds the running sum of the nodes that ran before it (`acc`, passed as the
    kernel's base operand) and only the last one hands the total to autograd -- L - 1 elementwise adds fewer.  A backward
    pass that does not visit all consumers (torch.autograd.grad on an intermediate layer, a loss on layer k < L - 1 only)
    would silently drop the visited consumers' share: `check()` raises in that case; TrainStep calls `check_all()` after its
    backward (callers that drive autograd themselves on a partial graph can do the same)."""
    __slots__ = ("acc", "got", "expected", "__weakref__")
    live = None           # the sums armed by the last forward (weak): TrainStep checks them after its backward

    def __init__(self, consumers):
        self.acc, self.got, self.expected = None, 0, int(consumers)
        if SharedGradSum.live is None:
            SharedGradSum.live = weakref.WeakSet()
        SharedGradSum.live.add(self)

    def add(self, g):
        self.got += 1
        if self.got < self.expected:
            self.acc = g
            return None
        self.acc, self.got = None, 0
        return g

    def check(self):
        if 0 < self.got < self.expected:
            got = self.got
            self.acc, self.got = None, 0
            raise RuntimeError(f"SharedGradSum: the backward visited {got} of {self.expected} consumers of a shared tensor -- "
                               "its gradient is incomplete (differentiate through all layers, or build the model without the shared sum)")

    @classmethod
    def check_all(cls):
        for s_ in list(cls.live or ()):
            s_.check()


LN2 = 0.6931471805599453
# "Pre-multiplied operands": a caller that folds head_dim^-1/2 * log2(e) into the projection that PRODUCES q (one rounding,
# in the GEMM's fp32 epilogue) passes scale = LN2, i.e. softmax(ln2 * q'.k) = 2^(q'.k) / sum: the kernels then take the
# scores straight from the matrix pipe as exp2 arguments (no multiply per score; csrc/attn_common.h host_split_scale).
def attn_premul(head_dim):
    """The factor to fold into q (self attention) -- or its square root into both operands (cross attention, where the
    same tensor is query in one direction and key in the other) -- when calling the attention ops with scale=LN2."""
    return head_dim ** -0.5 * 1.4426950408889634


def self_attention_rotary(qkv, theta, cs, pre_rotated=False, scale=None, theta_sum=None):
    """theta_sum: a SharedGradSum over all layers that share `theta` (None: every call returns its own angle gradient)."""
    if theta_sum is not None and not (torch.is_grad_enabled() and theta.requires_grad):
        theta_sum = None
    return _SelfAttentionRotary.apply(qkv, theta, cs, pre_rotated, scale, theta_sum)


class _CrossAttention(torch.autograd.Function):
    """Bidirectional cross attention with shared qk projection.

    p0, p1: [B,N_i,2,H,D] fused (to_qk, to_v) projections of image 0 / 1.
    m0 = softmax(qk0 qk1^T / sqrt(D)) v1,  m1 = softmax(qk1 qk0^T / sqrt(D)) v0."""

    @staticmethod
    def forward(ctx, p0, p1, scale=None):
        D = p0.shape[-1]
        sc = ctx.scale = D ** -0.5 if scale is None else scale
        m0, lse0 = attn_fwd_raw(p0[:, :, 0], p1[:, :, 0], p1[:, :, 1], sc)
        m1, lse1 = attn_fwd_raw(p1[:, :, 0], p0[:, :, 0], p0[:, :, 1], sc)
        ctx.save_for_backward(p0, p1, m0, m1, lse0, lse1)
        return m0, m1

    @staticmethod
    def backward(ctx, dm0, dm1):
        p0, p1, m0, m1, lse0, lse1 = ctx.saved_tensors
        D = p0.shape[-1]
        d0, d1 = torch.empty_like(p0), torch.empty_like(p1)
        # direction 0->1: q = qk0, k = qk1, v = v1: writes d qk0 (as query) and d qk1 (as key)
        attn_bwd_raw(p0[:, :, 0], p1[:, :, 0], p1[:, :, 1], m0, dm0, lse0,
                     d0[:, :, 0], d1[:, :, 0], d1[:, :, 1], ctx.scale)
        # direction 1->0: q = qk1, k = qk0, v = v0: ADDS d qk1 (as query) and d qk0 (as key) in the kernels' epilogues
        attn_bwd_raw(p1[:, :, 0], p0[:, :, 0], p0[:, :, 1], m1, dm1, lse1,
                     d1[:, :, 0], d0[:, :, 0], d0[:, :, 1], ctx.scale, acc_dq=True, acc_dk=True)
        return d0, d1, None


class _CrossAttentionStacked(torch.autograd.Function):
    """Same as _CrossAttention for equal keypoint counts, on the batch-stacked projection
    p [2B,N,2,H,D] (image 0 in the first half); returns the stacked messages [2B,N,H,D] so
    the following to_out GEMM runs once over both images without a concat."""

    @staticmethod
    def forward(ctx, p, scale=None):
        B2, N, _, H, D = p.shape
        B = B2 // 2
        sc = ctx.scale = D ** -0.5 if scale is None else scale
        m = torch.empty((B2, N, H, D), dtype=p.dtype, device=p.device)
        lse = torch.empty((B2, H, N), dtype=torch.float32, device=p.device)
        p0, p1 = p[:B], p[B:]
        attn_fwd_raw(p0[:, :, 0], p1[:, :, 0], p1[:, :, 1], sc, out=m[:B], lse=lse[:B])
        attn_fwd_raw(p1[:, :, 0], p0[:, :, 0], p0[:, :, 1], sc, out=m[B:], lse=lse[B:])
        ctx.save_for_backward(p, m, lse)
        return m

    @staticmethod
    def backward(ctx, dm):
        from . import XBWD_ENABLED      # the package attribute, read at call time: bench.py and the probes rebind it
        p, m, lse = ctx.saved_tensors
        B2, N, _, H, D = p.shape
        B = B2 // 2
        if not dm.is_contiguous():
            dm = dm.contiguous()
        d = torch.empty_like(p)
        if XBWD_ENABLED and p.dtype == torch.bfloat16 and D == 64 and H <= 4 and N % 64 == 0:
            # both directions from ONE score tile per image side (csrc/attention_xbwd.hip): 10 MFMA products instead of 14
            stat = torch.empty((2, B2, H, N), dtype=torch.float32, device=p.device)
            _lib.check(_lib.load().gf_attn_cross_bwd(_p(p[:, :, 0]), _p(p[:, :, 1]), _p(m), _p(dm), _p(lse), _p(stat),
                                                     _p(d[:, :, 0]), _p(d[:, :, 1]), B2, B, H, N, D,
                                                     _s3(p[:, :, 0]), _s3(p[:, :, 1]), _s3(m), _s3(dm), _s3(d[:, :, 0]),
                                                     _s3(d[:, :, 1]), float(ctx.scale), _dt(p), _stream()), "gf_attn_cross_bwd")
            return d, None
        p0, p1, d0, d1 = p[:B], p[B:], d[:B], d[B:]
        attn_bwd_raw(p0[:, :, 0], p1[:, :, 0], p1[:, :, 1], m[:B], dm[:B], lse[:B],
                     d0[:, :, 0], d1[:, :, 0], d1[:, :, 1], ctx.scale)
        # the second direction adds its query / key gradients to the first one's in the kernels' epilogues
        attn_bwd_raw(p1[:, :, 0], p0[:, :, 0], p0[:, :, 1], m[B:], dm[B:], lse[B:],
                     d1[:, :, 0], d0[:, :, 0], d0[:, :, 1], ctx.scale, acc_dq=True, acc_dk=True)
        return d, None


def cross_attention(p0, p1, scale=None):
    return _CrossAttention.apply(p0, p1, scale)


def cross_attention_stacked(p, scale=None):
    return _CrossAttentionStacked.apply(p, scale)


# ------------------------------------------------------------------------------ generic fused-qkv attention
class _AttentionQKV(torch.autograd.Function):
    """Attention on a fused projection qkv [B',N,3,H,D] (no rotary; SuperGlue / GlueStick GNN).

    cross=False: every image attends to itself.  cross=True: B' = 2B stacked images, image b
    attends to the keys/values of image (b + B) mod 2B.  Every q/k/v slot is consumed by exactly
    one call, so the backward writes dq/dk/dv straight into one dqkv buffer."""

    @staticmethod
    def forward(ctx, qkv, cross, scale=None, split=False):
        B2, N, _, H, D = qkv.shape
        sc = ctx.scale = D ** -0.5 if scale is None else scale       # LN2: the caller folded head_dim^-1/2 log2(e) into q
        split = bool(split) and qkv.dtype == torch.bfloat16
        o = torch.empty((B2, N, H, D), dtype=qkv.dtype, device=qkv.device)
        o32 = torch.empty((B2, N, H, D), dtype=torch.float32, device=qkv.device) if split else None   # kept for the backward's delta
        lse = torch.empty((B2, H, N), dtype=torch.float32, device=qkv.device)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        if not cross:
            attn_fwd_raw(q, k, v, sc, out=o, lse=lse, split=split, o32=o32)
        else:
            B = B2 // 2
            attn_fwd_raw(q[:B], k[B:], v[B:], sc, out=o[:B], lse=lse[:B], split=split, o32=None if o32 is None else o32[:B])
            attn_fwd_raw(q[B:], k[:B], v[:B], sc, out=o[B:], lse=lse[B:], split=split, o32=None if o32 is None else o32[B:])
        ctx.save_for_backward(qkv, o32 if split else o, lse)
        ctx.cross, ctx.split = cross, split
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        B2, N, _, H, D = qkv.shape
        if not do.is_contiguous():
            do = do.contiguous()
        d = torch.empty_like(qkv)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        dq, dk, dv = d[:, :, 0], d[:, :, 1], d[:, :, 2]
        sp = ctx.split
        if not ctx.cross:
            attn_bwd_raw(q, k, v, o, do, lse, dq, dk, dv, ctx.scale, split=sp)
        else:
            B = B2 // 2
            attn_bwd_raw(q[:B], k[B:], v[B:], o[:B], do[:B], lse[:B], dq[:B], dk[B:], dv[B:], ctx.scale, split=sp)
            attn_bwd_raw(q[B:], k[:B], v[:B], o[B:], do[B:], lse[B:], dq[B:], dk[:B], dv[:B], ctx.scale, split=sp)
        return d, None, None, None


def attention_qkv(qkv, cross=False, scale=None, split=False):
    """split: fp32-equivalent second products on bf16 operands (GF_ATTN_SPLIT) -- the reference's fp32-pinned attention of
    GlueStick under mixed precision (gluestick.py:524-529)."""
    return _AttentionQKV.apply(qkv, cross, scale, split)
