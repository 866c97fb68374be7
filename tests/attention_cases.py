"""CPU side of tests/test_gpu_attention_edges.py: inputs, float64 references, the error metric and the mutations for the bf16
attention kernels (csrc/attention_fwd3.hip, attention_bwd3.hip, attention_dkv.hip, attention_xbwd.hip, attention_generic.hip).
Pure torch on the CPU, nothing of the library: the conditions on the inputs are checked wherever torch runs
(tests/test_attention_cases_reference.py).

All tensors are [B, N, H, D] float64 holding bf16-representable values (`bf`), `lse` is [B, H, Nq].

`reference`       fp64 attention forward and backward in closed form.
`rounding_model`  the same with the kernels' rounding points and nothing else: the yardstick for the tolerance
                  `bound = max(3 * row_error(model, reference), 4e-3)` per tensor -- not the code under test.
`row_error`       max over rows of |a_row - r_row| / (|r_row| + rms of the row norms).
`mutations`       the reference with one key or one query row dropped / counted twice, or one row's lse off by ln 2: the
                  errors the GPU tests have to be able to see (at least 5 bounds away in one of o, dq, dk, dv)."""
import math

import torch

LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
FLOOR = 4e-3             # one bf16 rounding of an output row: 2^-9 relative per element, 2^-8 worst case
FACTOR = 3.0             # the model leaves out fast_exp2 / fast_log2, the fp32 summation order and the fp32 lse: each < one bf16 rounding
DETECT = 5.0             # a mutation has to move one tensor by this many bounds
B, H = 2, 2

# (Nq, Nk) at D = 64 on the LDS-DMA kernels: what each shape is there for is said in test_gpu_attention_edges.py
SHAPES_D64 = [(64, 64), (128, 192), (256, 320), (65, 65), (63, 127), (129, 193), (191, 257), (128, 65), (65, 128)]
BASIC = ["rand", "last_key", "last_query"]
HARD = ["late_spike", "ramp_steep", "huge_logits", "first_key_dominates"]
HARD_N = 192
SHAPES_GENERIC = [(65, 65), (257, 129)]          # D = 32 and 128: 256-row query blocks, 128-key blocks
SHAPES_ACC = [(65, 129), (128, 128)]
SHAPES_PAD = [(65, 65), (129, 193)]
CROSS_N, CROSS_H, CROSS_B2 = [64, 128, 192, 256], [1, 3, 4], [2, 4]
CROSS_TWO_LAUNCH = [(65, 4), (128, 5)]           # (N, H) the fused cross backward does not take


def bf(x):
    """fp64 -> nearest bf16 value, as fp64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def premul(D):
    """head_dim^-1/2 * log2(e): folded into q by callers that pass scale = ln 2 (ops.attn_premul)."""
    return D ** -0.5 * LOG2E


# ------------------------------------------------------------------------------------------------------------------ inputs
def _seed(case, Nq, Nk, D):
    return 7919 * (BASIC + HARD).index(case) + 131 * Nq + 17 * Nk + D


def make_case(case, Nq, Nk, D=64, pre=False, b=B, h=H):
    """(q, k, v, do, scale).  pre: q carries premul(D) (rounded to bf16 once, as the projection's epilogue does) and scale = ln 2."""
    g = torch.Generator().manual_seed(_seed(case, Nq, Nk, D))
    q, k, v, do = (torch.randn(b, n, h, D, generator=g, dtype=torch.float64) for n in (Nq, Nk, Nk, Nq))
    pos = torch.arange(Nk, dtype=torch.float64)[None, :, None, None]
    if case in BASIC:
        # asymmetric content as in test_attention_fwd_bwd: a transposed operand or output does not go unnoticed
        k = k * (1 + torch.arange(D, dtype=torch.float64) / D)
        v = v + pos / Nk
    if case == "last_key":
        u = torch.randn(b, 1, h, D, generator=g, dtype=torch.float64)
        u = u / u.norm(dim=-1, keepdim=True)
        amp = math.sqrt(math.log(Nk) + 2) * D ** 0.25           # logit of the marked queries on the last key: ln(Nk) + 2 + noise
        k[:, Nk - 1:] = u * amp
        q[:, ::3] = 0.5 * q[:, ::3] + u * amp
    elif case == "last_query":
        q[:, -1] *= 0.05                                          # flat attention: the row reaches every key
        do[:, -1] *= 32.0
    elif case == "late_spike":                                    # the cases of test_attention_bf16_forward_reference_cases at 3 tiles
        k[:, 170] *= 12.0
        k[:, 75] *= 5.0
    elif case == "ramp_steep":
        k = k * (1 + 12.0 * pos / Nk)
    elif case == "huge_logits":
        q = q * 6.0
        k = k * 6.0
    elif case == "first_key_dominates":
        k[:, 0] = q[:, 7] * 40.0
    scale = D ** -0.5
    if pre:
        q, scale = q * premul(D), LN2
    return bf(q), bf(k), bf(v), bf(do), scale


def cross_case(case, N, h, b2, pre=False, D=64):
    """(p [2B, N, 2, H, D] = (qk, v) per image, dm [2B, N, H, D], scale) for LightGlue's bidirectional cross attention: image i
    attends to image (i + B) mod 2B with q = its own qk, k = the other's qk.  The `last_key` / `last_query` constructions sit
    on token N - 1 of every image.  pre: BOTH operands carry sqrt(premul) (the same tensor is query one way and key the other)."""
    g = torch.Generator().manual_seed(_seed(case, N, N, D) + 1000 * h + b2)
    Bh = b2 // 2
    qk, v, dm = (torch.randn(b2, N, h, D, generator=g, dtype=torch.float64) for _ in range(3))
    qk = qk * (1 + torch.arange(D, dtype=torch.float64) / D) * 0.8
    v = v + torch.arange(N, dtype=torch.float64)[None, :, None, None] / N
    if case == "last_key":
        u = torch.randn(Bh, 1, h, D, generator=g, dtype=torch.float64)
        u = (u / u.norm(dim=-1, keepdim=True)).repeat(2, 1, 1, 1)                   # one direction per pair, shared by both images
        amp = math.sqrt(math.log(N) + 2) * D ** 0.25
        qk[:, :-1:3] = 0.5 * qk[:, :-1:3] + u * amp
        qk[:, N - 1:] = u * amp
        dm[:, -1] *= 4.0                     # token N - 1 is also the last QUERY of the other direction: keep that row visible in dv
    elif case == "last_query":
        qk[:, -1] *= 0.05
        dm[:, -1] *= 32.0
    else:
        assert case == "rand"
    scale = D ** -0.5
    if pre:
        qk, scale = qk * math.sqrt(premul(D)), LN2
    return bf(torch.stack((qk, v), 2)), bf(dm), scale


# -------------------------------------------------------------------------------------------------------------- references
def _scores(q, k, scale):
    return torch.einsum("bqhd,bkhd->bhqk", q, k) * scale


def _backward(q, k, v, do, scale, p, p_v, ds_round, delta, qw=None):
    """dq, dk, dv from P [B,H,Nq,Nk]: p_v is what enters the dV product, ds_round what dS passes through in front of the dQ / dK
    products, qw [Nq] a weight per query row in the dK / dV sums (mutations)."""
    dp = torch.einsum("bqhd,bkhd->bhqk", do, v)
    ds = ds_round(p * (dp - delta[..., None]))
    dq = torch.einsum("bhqk,bkhd->bqhd", ds, k) * scale
    if qw is not None:
        ds, p_v = ds * qw[:, None], p_v * qw[:, None]
    dk = torch.einsum("bhqk,bqhd->bkhd", ds, q) * scale
    dv = torch.einsum("bhqk,bqhd->bkhd", p_v, do)
    return dq, dk, dv


def reference(q, k, v, do, scale, keys=None, qw=None, lse_shift=None):
    """fp64 attention: dict o, lse, dq, dk, dv.  The optional arguments make the mutations: `keys` [Nk] bool keeps a subset of
    the keys (the others get no mass and zero gradients), `qw` [Nq] weighs the query rows in dk / dv, `lse_shift` [Nq] is added
    to the lse the BACKWARD recomputes P from (o and delta stay)."""
    s = _scores(q, k, scale)
    if keys is not None:
        s = s.masked_fill(~keys, -math.inf)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum("bhqk,bkhd->bqhd", p, v)
    delta = torch.einsum("bqhd,bqhd->bhq", o, do)
    if lse_shift is not None:
        p = torch.exp(s - (lse + lse_shift)[..., None])
    dq, dk, dv = _backward(q, k, v, do, scale, p, p, lambda x: x, delta, qw)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _hi_lo(x):
    hi = bf(x)
    return hi + bf(x - hi)


def rounding_model(q, k, v, do, scale, split, round_grads=True):
    """The reference with the bf16 kernels' rounding points: P in front of the PV and dV products and dS in front of the dQ and
    dK products rounded to bf16 (split: kept as a hi + lo bf16 pair), delta = sum(o dO) from the bf16 o (split: from the
    unrounded o), lse kept in fp32, the four outputs rounded to bf16 (round_grads=False: the gradients as they stand in the
    accumulators, for a caller that models the accumulate flags)."""
    rnd = _hi_lo if split else bf
    s = _scores(q, k, scale)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    pr = rnd(p)
    o = torch.einsum("bhqk,bkhd->bqhd", pr, v)
    delta = torch.einsum("bqhd,bqhd->bhq", o if split else bf(o), do)
    dq, dk, dv = _backward(q, k, v, do, scale, p, pr, rnd, delta)
    if round_grads:
        dq, dk, dv = bf(dq), bf(dk), bf(dv)
    return dict(o=bf(o), lse=lse.float().double(), dq=dq, dk=dk, dv=dv)


TENSORS = ("o", "dq", "dk", "dv")


def row_error(a, r):
    """max over rows (batch, token, head) of |a_row - r_row|_2 / (|r_row|_2 + rms), rms the root mean square of r's row norms:
    a wrong row cannot hide behind a large entry elsewhere, a near-zero row is measured against the tensor's scale."""
    a, r = a.detach().double().cpu(), r.detach().double().cpu()
    assert a.shape == r.shape, (a.shape, r.shape)
    rn = r.norm(dim=-1)
    rms = rn.pow(2).mean().sqrt()
    e = (a - r).norm(dim=-1) / (rn + rms)
    return float(e.max()) if bool(torch.isfinite(a).all()) else math.inf


def bounds(ref, model):
    """Per tensor: (bound, model error).  lse: absolute, 1e-3 + the model's own error."""
    out = {}
    for n in TENSORS:
        me = row_error(model[n], ref[n])
        out[n] = (max(FACTOR * me, FLOOR), me)
    me = float((model["lse"] - ref["lse"]).abs().max())
    out["lse"] = (1e-3 + me, me)
    return out


def mutation_kwargs(Nq, Nk):
    """name -> the arguments of `reference` that build the error in."""
    def keys_without(j):
        m = torch.ones(Nk, dtype=torch.bool)
        m[j] = False
        return m

    def rows(value, base):
        w = torch.full((Nq,), base, dtype=torch.float64)
        w[Nq - 1] = value
        return w

    out = {"twice_last_query": dict(qw=rows(2.0, 1.0)), "drop_last_query": dict(qw=rows(0.0, 1.0)),
           "lse_shift": dict(lse_shift=rows(LN2, 0.0))}
    if Nk > 1:
        out["drop_last_key"] = dict(keys=keys_without(Nk - 1))
        first = 64 * ((Nk - 1) // 64)
        if first != Nk - 1:
            out["drop_first_key_of_last_tile"] = dict(keys=keys_without(first))
    return out


def mutations(q, k, v, do, scale):
    """name -> the reference's dict with that error built in."""
    return {n: reference(q, k, v, do, scale, **kw) for n, kw in mutation_kwargs(q.shape[1], k.shape[1]).items()}


def cross_reference(p, dm, scale, fn=reference, **kw):
    """Both directions of the stacked cross attention with `fn` = reference or rounding_model: dict o [2B,N,H,D], lse [2B,H,N]
    and the two slots of the gradient of p, dqk (as query in one direction + as key in the other) and dv."""
    Bh = p.shape[0] // 2
    qk, v = p[:, :, 0], p[:, :, 1]
    a = fn(qk[:Bh], qk[Bh:], v[Bh:], dm[:Bh], scale, **kw)
    b = fn(qk[Bh:], qk[:Bh], v[:Bh], dm[Bh:], scale, **kw)
    return dict(o=torch.cat((a["o"], b["o"])), lse=torch.cat((a["lse"], b["lse"])),
                dqk=torch.cat((a["dq"] + b["dk"], b["dq"] + a["dk"])), dv=torch.cat((b["dv"], a["dv"])))


def cross_model(p, dm, scale):
    """The rounding model of the cross attention as two launches: the first direction writes its bf16 dq / dk rows, the second
    adds its own to them in fp32 and rounds again (GF_ATTN_ACC_DQ / _DK).  The fused kernel rounds the sum once: no more."""
    m = cross_reference(p, dm, scale, fn=lambda *a: rounding_model(*a, split=False))
    Bh = p.shape[0] // 2
    qk, v = p[:, :, 0], p[:, :, 1]
    first = rounding_model(qk[:Bh], qk[Bh:], v[Bh:], dm[:Bh], scale, False)
    second = rounding_model(qk[Bh:], qk[:Bh], v[:Bh], dm[Bh:], scale, False, round_grads=False)
    m["dqk"] = bf(torch.cat((first["dq"] + second["dk"], first["dk"] + second["dq"])))
    return m
