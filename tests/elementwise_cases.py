"""Shared by tests/test_elementwise_cases_reference.py (CPU) and tests/test_gpu_elementwise.py: case tables, seeded inputs,
float64 references, derived error bounds, fp32 / bf16 emulations in the kernels' own order and named mutations for
  csrc/elementwise.hip   gf_rotary_qk, gf_rotary_qk_bwd, gf_ln_gelu_fwd, gf_ln_gelu_bwd
  csrc/rowdot.hip        gf_rowdot_fwd / _bwd, gf_rowdot2_fwd / _bwd
  csrc/smallops.hip      gf_colsum_f32
(contract in include/gf_amd.h).  No GPU code and no library code here.  Every function works on the device its case lives
on: the CPU test keeps the cases on the CPU, the GPU test moves them (to_device) and so gets its float64 references from
stock torch on the device; the two are the same lines of code.  Inputs are taken as stored: a bf16 tensor is upcast to
float64 and never rounded again.

Bounds (derived, not tuned).  U = 2^-24 is the fp32 rounding unit, gam(n) = n U / (1 - n U) the classic bound of a chain
of n roundings, T the sum of the absolute values of a value's addends.  Every bound has a floor of 1e-30 (flushed
denormals).  One bf16 rounding to nearest is half a bf16 ulp: BF = 2^-9 of the power of two above the value (8
significand bits; relative to the value itself that is between 2^-9 and 2^-8).  A value stored in bf16 gets
bound + BF 2^top with |ref| + bound < 2^top.

  rotary    out = x c -+ x' s: two products and one add, fused or not: 3 U (|x c| + |x' s|).
            dtheta = sum over {q, k} x heads of (g_odd y_even - g_even y_odd) + base.  The scalar kernel adds H terms in
            sequence per lane, then the other half and the base; the vector kernel adds single terms through a butterfly of
            at most 6 steps, then the base; each term carries 2 roundings of its own: gam(max(H, 6) + 4) (T + |base|).
  LN stats  The kernel forms d = x - x0 (x0 = the row's first element), s = sum d, q = sum d^2: every lane adds its
            NCH VEC elements in sequence, the wave sum adds 4 DPP steps and 3 row sums: n = NCH VEC + 7.  With
            A = mean |d|, md = mean d, Q = mean d^2 = var + md^2, e = d - md = x - mu:
              |dmd|   <= gam(n + 3) A                                (d, the sum, 1/C, the product)
              |dmu|   <= |dmd| + U |mu|                              (x0 + md)
              |dvar|  <= gam(n + 4) Q + 2 |md| |dmd| + 3 U md^2      single pass, var = q / C - md^2
            which is (1 + md^2 / var) times worse than the data deserve: the factor is C for one outlier in column 0 (x0 is
            then the outlier, every d as large as it), and on the device that was 1.2e-4 of the normalised values at C = 1024
            -- over the fp32 parity budget -- while the same outlier in the last column gave 1e-7.  So when the computed
            md^2 exceeds LN_GUARD = 63 computed variances (x0 more than 7.9 sigma off the mean) the kernel sums (d - md)^2
            in a second pass over its registers:
              |dvar|  <= gam(n + 6) var + 2 U mean(|e| |d|) + dmd^2  second pass
            (the computed d - md is off by U |d| + |dmd| + U |e|; the error of md enters only in the second order because
            sum e = 0).  A row is held to the larger of the two where the single pass may have been used (md^2 <= 64 var: the
            computed ratio is within 1e-3 of the true one there), to the second alone above that, and
              |drs|/rs <= r / (2 (1 - r)) + 4 U,   r = |dvar| / (var + eps)          (the add of eps, v_rsq)
            r is the variance's conditioning; at the guard the single pass costs at most 64 gam(n + 4) / 2 = 5e-5 of a
            normalised value at n = 23.  On `offset` (mean 1e3, sigma 1) the U |mu| rs term is 6e-5: an fp32 mean at 1e3 cannot
            be better, and only that case pays for it.
  xhat      |dxh| <= rs |dmu| + |xh| (|drs| / rs + 3 U),   xh = (x - mu) rs
  z         z = xh gamma + beta:  |dz| <= |gamma| |dxh| + 2 U (|xh gamma| + |beta|)
  gelu      y = z cdf(z).  erf by Abramowitz-Stegun 7.1.26, |erf error| <= 1.5e-7 absolute, so cdf is off by 0.75e-7 and y
            by |z| 0.75e-7.  Evaluation: t = rcp(1 + p xa) (4 U), the 5-term Horner polynomial with alternating signs
            (30 U S(t), S = sum |a_k| t^k), e = exp(-xa^2) ((4 xa^2 + 4) U relative: the argument's three roundings act
            absolutely on the exponent, plus v_exp), 1 - poly e and 0.5 (1 + .) (2 U):
              cdf_err(z) = 0.5 (1.5e-7 + e S (34 + 4 xa^2) U + U) + U
              |dy| <= (|gelu'(z)| + |dz|) |dz| + |z| cdf_err(z) + 2 U |y|
            In the negative tail cdf cancels in 1 - erf; the absolute term |z| cdf_err is the honest bound there.
  LN bwd    mean / rstd are inputs (the float64 statistics rounded to fp32): |dxh| <= rs U |mu| + 4 U |xh|, z as above,
            gelu' = cdf + z pdf with |dgelu'| <= (|gelu''| + |dz|) |dz| + cdf_err + |z| pdf (4 xa^2 + 6) U + 2 U |gelu'|,
            dz = dy gelu', dxh' = dz gamma (one rounding each), m1 = mean dxh', m2 = mean dxh' xh with the chain n + 2 / n + 3
            on their absolute addends plus the propagated element errors, dx = rs (dxh' - m1 - xh m2) with 5 U on its three
            addends.  dgamma = sum_r dz xh, dbeta = sum_r dz: a wave adds its rows in sequence (ceil(R / (4 nblk)) of them),
            the block adds its 4 waves: gam(rows + 4) T plus the propagated element errors; the partial rows are summed in
            float64 by the tests.
  row-dot   z: a lane adds VEC elements per pass, at most 4 passes, then 6 butterfly steps and the biases:
            gam(4 VEC + 9) (sum |x w| + |b|).  dx = base + dz w: 2 U (|base| + |dz w|).  dw, db: a thread adds
            ceil(M / (nblk rpi)) rows in sequence, the block then rpi = 256 / (C / VEC) of those through the LDS:
            gam(iters + rpi + 1) T.
  colsum    a thread adds ceil(ceil(R / 32) / 4) rows, the block 4 of those, stage 2 the 32 chunks: gam(that + 36) sum |x|.
The two outlier cases are additionally held to the project's fp32 parity budget PARITY = 1e-4 of the row's largest
|normalised value| (fp32 only; a bf16 output is rounded far coarser than that)."""
import functools
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
BF = 2.0 ** -9
FLOOR = 1e-30
EPS = float(torch.tensor(1e-5, dtype=torch.float32))          # eps as the entry receives it: a C float
PARITY = 1e-4
LN_GUARD = 63.0           # the forward's second pass runs when md^2 > LN_GUARD var
STOCK_MU = 4
STOCK_ERF = 6e-7          # absolute error granted to torch's vectorised fp32 erf (unspecified; about 2.6e-7 seen at z = -3.4)
DETECT = 2.0              # a mutation must move an asserted output by this many bounds
DTYPES = [torch.float32, torch.bfloat16]
GF_ERR_UNSUPPORTED, GF_ERR_SHAPE, GF_ERR_DTYPE = -1, -2, -4


def gam(n):
    return n * U / (1.0 - n * U)


def vec_of(dtype):
    return 4 if dtype == torch.float32 else 8


def _stored(bound, ref, dtype):
    """Bound of a value stored in `dtype` from the bound of its fp32 value."""
    if dtype != torch.bfloat16:
        return bound + FLOOR
    a = ref.abs() + bound
    half_ulp = torch.ldexp(torch.full_like(a, BF), torch.frexp(a).exponent)          # |value| < 2^exponent
    return bound + torch.where(a > 0, half_ulp, torch.zeros_like(a)) + FLOOR


def to_device(case, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in case.items()}


def ratio(x, ref, bound):
    """Worst |x - ref| / bound; a NaN (an element never written) is infinitely far off, equal values agree."""
    x, ref = x.detach().double(), ref.detach().double()
    if x.numel() == 0:
        return 0.0
    d = torch.where(x == ref, torch.zeros_like(ref), (x - ref).abs() / bound.double())
    return math.inf if torch.isnan(d).any() else float(d.max())


# ================================================================================================ tables
# ---- rotary (H, D): which kernel and which path each entry pins
ROT_VEC = [(4, 64),      # vector kernel, W = 64: the full wave (the workload's shape)
           (1, 64),      # vector kernel, 16 live lanes, cpd = 8
           (3, 32),      # vector kernel, 24 live lanes (not a power of two), cpd = 4
           (2, 128),     # vector kernel, cpd = 16, full wave
           (16, 16),     # vector kernel, cpd = 2, full wave, 32 lanes per angle chunk
           (1, 8)]       # vector kernel, two live lanes, cpd = 1: the butterfly runs over the whole wave
ROT_SCALAR = [(8, 64),   # scalar kernel (H D = 512 > 256), 2 npair = 64 exactly: one pass, shuffle partner at +32
              (4, 128),  # scalar kernel, npair = 64: two passes, the per-lane carry
              (2, 48),   # scalar kernel (cpd = 6 is no power of two), 48 live lanes in the divergent loop
              (1, 20),   # scalar kernel (D % 8 != 0), 20 live lanes
              (3, 2)]    # scalar kernel, one pair: lanes 0 and 1
ROT_FWD_ONLY = [(2, 96),   # scalar kernel, 96 work items: two passes over the lanes; backward: GF_ERR_UNSUPPORTED
                (1, 256)]  # vector kernel, cpd = 32 (forward); backward: GF_ERR_UNSUPPORTED
ROT_TOKENS = [(1, 1), (3, 1), (1, 4), (1, 5), (1, 37)]        # (B, N): one wave, a ragged block, one block, two blocks, ten
ROT_BIG_TOKENS = (1, 2 * 32768 + 3)                           # the grid-stride loop: 8192 blocks of 4 tokens, three rounds
ROT_BIG_HD = [(1, 8), (1, 20)]
ROT_KINDS = ("rand", "zero", "quarter", "scale")

# ---- LN + GELU channel counts: NCH instance and FULL flag
LN_C = {torch.float32: [256,    # NCH 1 FULL
                        512,    # NCH 2 FULL
                        1024,   # NCH 4 FULL
                        4,      # NCH 1, one live lane
                        252,    # NCH 1 ragged, 63 live lanes
                        260,    # NCH 2 by one chunk
                        516,    # NCH 4 by one chunk
                        1020],  # NCH 4 ragged
        torch.bfloat16: [512, 1024, 2048, 8, 504, 520, 1032, 2040]}     # the same paths at VEC 8
LN_ROWS = [1, 3, 4, 5, 37]                 # one wave, a ragged block, one block, two blocks, ten
LN_BIG_ROWS = [8193, 16389]                # second iteration of one wave; third iteration, waves that stop at different ones
LN_BIG_C = {torch.float32: [256, 1024], torch.bfloat16: [2048]}
LN_REJECT_UNSUPPORTED = {torch.float32: [6, 1028], torch.bfloat16: [12, 2056]}
LN_KINDS = ("rand", "const", "offset", "outlier_first", "outlier_last", "tiny", "tails", "gamma0")
LN_NBLK = [(1, 1), (4, 1), (5, 2), (8192, 2048), (8193, 2048), (10 ** 6, 2048)]

# ---- row-dot channel counts: cpr = C / VEC threads per row, rpi = 256 / cpr rows per sweep
RD_C = {torch.float32: [4,      # cpr 1, 256 rows per sweep
                        12,     # cpr 3, 85 rows, one idle thread
                        96,     # cpr 24, 10 rows, 16 idle threads
                        256,    # cpr 64, 4 rows (the workload's shape)
                        516,    # cpr 129, one row per sweep, 127 idle threads
                        1024],  # cpr 256, one row per sweep, four forward passes
        torch.bfloat16: [8, 24, 192, 256, 1032, 2048]}
RD_ROWS = [1, 3, 5, 255, 257, 5000]
RD_BIG_FWD = 2 * 16384 + 3                 # the forward grid stride (4096 blocks of 4 rows), smallest C of each dtype
RD_BIG_BWD = 131072 + 259                  # the backward sweep at cpr 1: 512 blocks of 256 rows, a second round
RD_REJECT_UNSUPPORTED = {torch.float32: [6, 1028], torch.bfloat16: [6, 2056]}
RD_KINDS = ("rand", "cancel", "spike")
RD_NBLK = [(1, 1), (256, 1), (257, 2), (131072, 512), (10 ** 6, 512)]

# ---- column sums
CS_G, CS_R, CS_C = [1, 2, 3], [1, 31, 32, 33, 2048, 2051], [1, 63, 64, 65, 512]
CS_KINDS = ("rand", "cancel")
CS_CHUNKS = 32


def rotary_vec_ok(H, D):
    cpd = D // 8
    return D % 8 == 0 and 2 * H * D // 8 <= 64 and cpd & (cpd - 1) == 0 and 64 % cpd == 0


def ln_nch(C, dtype):
    chunks = C // vec_of(dtype)
    return -1 if C % vec_of(dtype) or chunks > 256 else (1 if chunks <= 64 else 2 if chunks <= 128 else 4)


def ln_nblk(R):
    return min(max((R + 3) // 4, 1), 2048)


def rd_nblk(M):
    return min(max((M + 255) // 256, 1), 512)


# ================================================================================================ rotary
@functools.lru_cache(maxsize=None)
def rotary_case(kind, B, N, H, D, dtype):
    g = torch.Generator().manual_seed(1000 * H + D + 7 * B * N + ROT_KINDS.index(kind))
    rn = lambda *s: torch.randn(*s, generator=g)                                   # noqa: E731
    qkv, y, grad = rn(B, N, 3, H, D), rn(B, N, 3, H, D), rn(B, N, 3, H, D)
    theta = (torch.rand(B, N, D // 2, generator=g) * 2 - 1) * 4 * math.pi
    cs = torch.stack((torch.cos(theta), torch.sin(theta)), -1).flatten(-2)
    if kind == "zero":
        cs = torch.stack((torch.ones_like(theta), torch.zeros_like(theta)), -1).flatten(-2)
    elif kind == "quarter":               # theta = pi / 2 written as exact (0, 1): a permutation with a sign
        cs = torch.stack((torch.zeros_like(theta), torch.ones_like(theta)), -1).flatten(-2)
    elif kind == "scale":                 # one token of about 1e4 next to tokens of about 1e-3
        sc = torch.full((B, N, 1, 1, 1), 1e-3)
        sc.view(-1)[(B * N) // 2] = 1e4
        qkv, y, grad = qkv * sc, y * sc, grad * sc
    return dict(kind=kind, B=B, N=N, H=H, D=D, dtype=dtype, qkv=qkv.to(dtype), y=y.to(dtype), grad=grad.to(dtype),
                cs=cs.contiguous(), base=rn(B, N, D // 2))


def _rot(x, c, s):
    """rotate_half on adjacent pairs: x [B,N,K,H,D], c / s [B,N,D/2]."""
    c, s = (t.repeat_interleave(2, -1)[:, :, None, None] for t in (c, s))
    r = torch.stack((-x[..., 1::2], x[..., 0::2]), -1).flatten(-2)
    return x * c + r * s, x.abs() * c.abs() + r.abs() * s.abs()


def _rot_half(x, c, s):
    """The mutation: pairs (i, i + D/2) instead of adjacent ones."""
    c, s = (torch.cat((t, t), -1)[:, :, None, None] for t in (c, s))
    h = x.shape[-1] // 2
    return x * c + torch.cat((-x[..., h:], x[..., :h]), -1) * s


def rotary_ref(case, mutation=None):
    """float64: fwd / inv = the q, k thirds rotated by +theta / -theta, dq = the gradient rotated back, dtheta without and
    with the base; bounds under the same names + '_bound'."""
    dt, H = case["dtype"], case["H"]
    cs = case["cs"].double()
    c, s = cs[..., 0::2], cs[..., 1::2]
    if mutation == "sin_sign":
        s = -s
    x, y, gr = (case[k].double()[:, :, :2] for k in ("qkv", "y", "grad"))
    base = case["base"].double()
    out = {}
    for name, src, sgn in (("fwd", x, 1.0), ("inv", x, -1.0), ("dq", gr, -1.0)):
        v, T = _rot(src, c, sgn * s)
        if mutation == "half_pairs":
            v = _rot_half(src, c, sgn * s)
        if mutation == "k_unrotated":
            v = torch.cat((v[:, :, :1], src[:, :, 1:]), 2)
        out[name], out[name + "_bound"] = v, _stored(3 * U * T, v, dt)
    # inverse(forward(x)) against x: the forward errors of a pair (at most the larger of its two bounds each) come back through
    # c and s, then the inverse's own bound at x -- the "twice the forward bound" of a round trip, stated per pair
    b = out["fwd_bound"]
    pm = torch.maximum(b[..., 0::2], b[..., 1::2]).repeat_interleave(2, -1)
    ca, sa = (t.abs().repeat_interleave(2, -1)[:, :, None, None] for t in (c, s))
    out["rt"], out["rt_bound"] = x, pm * (ca + sa) + _stored(3 * U * _rot(out["fwd"], c, -s)[1], x, dt)
    t1, t2 = gr[..., 1::2] * y[..., 0::2], gr[..., 0::2] * y[..., 1::2]                 # [B,N,2,H,D/2]
    terms = t1 - t2
    if mutation == "dtheta_no_k":
        terms = terms[:, :, :1]
    if mutation == "dtheta_one_head_short":
        terms = terms[:, :, :, :-1] if H > 1 else terms * 0
    dth = terms.sum((2, 3))
    T = (t1.abs() + t2.abs()).sum((2, 3))
    n = max(H, 6) + 4
    out["dtheta"], out["dtheta_bound"] = dth, gam(n) * T + FLOOR
    out["dtheta_base"] = dth + (0 if mutation == "base_dropped" else base)
    out["dtheta_base_bound"] = gam(n) * (T + base.abs()) + FLOOR
    return out


ROT_MUTATIONS = {"sin_sign": ("fwd", "inv", "dq"), "half_pairs": ("fwd", "inv", "dq"), "k_unrotated": ("fwd", "inv", "dq"),
                 "dtheta_no_k": ("dtheta",), "dtheta_one_head_short": ("dtheta",), "base_dropped": ("dtheta_base",)}
ROT_OUTPUTS = ("fwd", "inv", "dq", "dtheta", "dtheta_base")


def _tree(p):
    """Pairwise fp32 sum over the last axis (a power of two): the shape of a butterfly."""
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def emulate_rotary(case, stock=False):
    """fp32 arithmetic in the kernels' order (stock: the plain fp32 restatement of rotate_half with torch's own sums)."""
    dt, H, D = case["dtype"], case["H"], case["D"]
    cs = case["cs"].float()
    c, s = cs[..., 0::2], cs[..., 1::2]
    x, y, gr = (case[k].float()[:, :, :2] for k in ("qkv", "y", "grad"))
    out = {"fwd": _rot(x, c, s)[0].to(dt), "inv": _rot(x, c, -s)[0].to(dt), "dq": _rot(gr, c, -s)[0].to(dt)}
    terms = gr[..., 1::2] * y[..., 0::2] - gr[..., 0::2] * y[..., 1::2]                 # [B,N,2,H,D/2]
    if stock:
        dth = terms.sum((2, 3))
    elif rotary_vec_ok(H, D):             # one term per lane, butterfly over the 2H lanes of a chunk (idle lanes hold 0)
        flat = terms.flatten(2, 3)                                                      # [B,N,2H,D/2]
        pad = 1 << max(2 * H - 1, 0).bit_length()
        flat = torch.cat((flat, flat.new_zeros(*flat.shape[:2], pad - 2 * H, D // 2)), 2)
        dth = _tree(flat.transpose(2, 3).contiguous())
    else:                                 # heads in sequence per lane, then q + k
        acc = torch.zeros_like(terms[:, :, :, 0])
        for h in range(H):
            acc = acc + terms[:, :, :, h]
        dth = acc[:, :, 0] + acc[:, :, 1]
    out["dtheta"], out["dtheta_base"] = dth, dth + case["base"]
    return out


# ================================================================================================ LN + GELU
@functools.lru_cache(maxsize=None)
def ln_case(kind, R, C, dtype):
    g = torch.Generator().manual_seed(100 * C + R + LN_KINDS.index(kind))
    rn = lambda *s: torch.randn(*s, generator=g)                                   # noqa: E731
    x = rn(R, C) * 2 + 0.3
    gamma, beta, dy = 1 + 0.2 * rn(C), 0.2 * rn(C), rn(R, C)
    if kind == "const":
        x = (3 * rn(R, 1)).expand(R, C).contiguous()
    elif kind == "offset":
        x = 1e3 + rn(R, C)
    elif kind in ("outlier_first", "outlier_last"):       # 1e2 in the even rows, 1e3 in the odd ones
        x = rn(R, C)
        x[:, 0 if kind == "outlier_first" else C - 1] = torch.where(torch.arange(R) % 2 == 0, 1e2, 1e3)
    elif kind == "tiny":
        x = 1e-4 * rn(R, C)
    elif kind == "tails":                                 # z = xhat gamma + beta covers +-12
        gamma = 3.5 * (1 + 0.1 * rn(C)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    elif kind == "gamma0":
        gamma, beta = torch.zeros(C), rn(C)
    return dict(kind=kind, R=R, C=C, dtype=dtype, x=x.to(dtype), dy=dy.to(dtype), gamma=gamma, beta=beta)


_AS = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
_ASP = 0.3275911


def _gauss(z):
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    return cdf, pdf


def _cdf_err(z, erf_abs=1.5e-7):
    xa = z.abs() / math.sqrt(2.0)
    t = 1 / (1 + _ASP * xa)
    S = sum(abs(a) * t ** (k + 1) for k, a in enumerate(_AS))
    return 0.5 * (erf_abs + torch.exp(-xa * xa) * S * (34 + 4 * xa * xa) * U + U) + U, xa


def _ln_math(x, gamma, beta, dy, R, C, mutation=None):
    """LayerNorm + GELU and its gradients written out in float64 (the mutations live here)."""
    mu = x.mean(1, keepdim=True)
    d = x - x[:, :1]
    md, Q = d.mean(1, keepdim=True), (d * d).mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    if mutation == "var_without_md2":
        var = Q
    if mutation == "mean_without_x0":
        mu = md
    rs = (var + EPS).rsqrt()
    if mutation == "eps_outside_sqrt":
        rs = 1 / (var.sqrt() + EPS)
    xh = (x - mu) * rs
    z = xh * gamma + beta
    cdf, pdf = _gauss(z)
    y, gp = z * cdf, cdf + z * pdf
    if mutation == "tanh_gelu":
        k = math.sqrt(2 / math.pi)
        th = torch.tanh(k * (z + 0.044715 * z ** 3))
        y = 0.5 * z * (1 + th)
        gp = 0.5 * (1 + th) + 0.5 * z * (1 - th * th) * k * (1 + 3 * 0.044715 * z * z)
    dz = dy * gp
    dxh = dz * gamma
    m1, m2 = dxh.mean(1, keepdim=True), (dxh * xh).mean(1, keepdim=True)
    dx = rs * (dxh - m1 - (0 if mutation == "dx_without_m2" else xh * m2))
    keep = torch.ones(R, 1, dtype=x.dtype, device=x.device)
    if mutation == "partial_row_skipped":                  # the last block's partial row is never added
        nb = ln_nblk(R)
        keep = ((torch.arange(R, device=x.device) // 4) % nb != nb - 1).to(x.dtype)[:, None]
    dgamma = (dz * (x if mutation == "dgamma_uses_x" else xh) * keep).sum(0)
    dbeta = (dz * keep).sum(0)
    return dict(y=y, mean=mu[:, 0], rstd=rs[:, 0], dx=dx, dgamma=dgamma, dbeta=dbeta,
                xh=xh, z=z, gp=gp, pdf=pdf, dz=dz, dxh=dxh, m1=m1, m2=m2, d=d, md=md, Q=Q, var=var)


LN_MUTATIONS = {"var_without_md2": ("rstd", "y"), "mean_without_x0": ("mean",), "eps_outside_sqrt": ("rstd", "y"),
                "tanh_gelu": ("y", "dx"), "dx_without_m2": ("dx",), "dgamma_uses_x": ("dgamma",),
                "partial_row_skipped": ("dgamma", "dbeta")}
LN_OUTPUTS = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")


def ln_autograd(case):
    """The reference the issue names: F.gelu(F.layer_norm(...)) and its autograd, float64."""
    C = case["C"]
    x, ga, be = (case[k].double().clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = F.gelu(F.layer_norm(x, (C,), ga, be, EPS))
    (y * case["dy"].double()).sum().backward()
    return dict(y=y.detach(), dx=x.grad, dgamma=ga.grad, dbeta=be.grad)


def ln_ref(case, mutation=None, stock=False):
    """float64 outputs (y, dx, dgamma, dbeta from autograd; mean, rstd directly) and, without a mutation, their bounds under
    name + '_bound', `cond` = the variance's conditioning r per row, `xh_bound` and `xh_max` for the parity budget.
    stock: the bounds for torch's own fp32 layer_norm, which differs from the kernels in two documented ways: it evaluates
    x (rs gamma) + (beta - mu rs gamma), which rounds |mu|-sized quantities STOCK_MU times instead of once, and its backward
    runs on the statistics its own forward computed, not on the rounded float64 ones; its erf is granted STOCK_ERF.  None of
    this enters a bound that a kernel is held to."""
    R, C, dt = case["R"], case["C"], case["dtype"]
    x, gamma, beta, dy = (case[k].double() for k in ("x", "gamma", "beta", "dy"))
    m = _ln_math(x, gamma, beta, dy, R, C, mutation)
    out = {k: m[k] for k in LN_OUTPUTS}
    if mutation is not None:
        return out
    out.update(ln_autograd(case))
    n = ln_nch(C, dt) * vec_of(dt) + 7
    if stock:                              # a CPU vector unit of 8 lanes adds C / 8 elements in sequence per lane
        n = max(n, C // 8 + 8)
    mu, rs, xh, z, var = m["mean"][:, None], m["rstd"][:, None], m["xh"], m["z"], m["var"]
    dsh = x.abs() if stock else m["d"].abs()               # what the sums run over: x - x0 in the kernel, x itself in torch
    A = dsh.mean(1, keepdim=True)
    kmu = STOCK_MU if stock else 1
    dmd = gam(n + 3) * A
    dmu = dmd + kmu * U * mu.abs()
    dvar = gam(n + 6) * var + 2 * U * ((x - mu).abs() * dsh).mean(1, keepdim=True) + dmd ** 2
    if not stock:                          # the single pass, wherever the guard may have let it stand
        single = gam(n + 4) * m["Q"] + 2 * m["md"].abs() * dmd + 3 * U * m["md"] ** 2
        dvar = torch.where(m["md"] ** 2 <= (LN_GUARD + 1) * var, torch.maximum(dvar, single), dvar)
    r = dvar / (var + EPS)
    drs_rel = 0.5 * r / (1 - r.clamp(max=0.5)) + 4 * U
    dxh = rs * dmu + xh.abs() * (drs_rel + 3 * U)
    cerr, xa = _cdf_err(z, STOCK_ERF if stock else 1.5e-7)

    def z_err(dxh_):
        return gamma.abs() * dxh_ + 2 * U * ((xh * gamma).abs() + beta.abs())

    dz = z_err(dxh)
    out.update(cond=r[:, 0], xh=xh, xh_bound=dxh, xh_max=xh.abs().amax(1, keepdim=True),
               mean_bound=dmu[:, 0] + FLOOR, rstd_bound=(rs * drs_rel)[:, 0] + FLOOR,
               y_bound=_stored((m["gp"].abs() + dz) * dz + z.abs() * cerr + 2 * U * out["y"].abs(), out["y"], dt))
    # backward from the stored fp32 statistics
    bxh = dxh if stock else rs * U * mu.abs() + 4 * U * xh.abs()
    bz = z_err(bxh)
    gpp = m["pdf"] * (2 - z * z)
    bgp = (gpp.abs() + bz) * bz + cerr + z.abs() * m["pdf"] * (4 * xa * xa + 6) * U + 2 * U * m["gp"].abs()
    bdz = dy.abs() * bgp + U * m["dz"].abs()
    bdxh = gamma.abs() * bdz + U * m["dxh"].abs()
    mean = lambda t: t.mean(1, keepdim=True)                                          # noqa: E731
    bm1 = mean(bdxh) + gam(n + 2) * mean(m["dxh"].abs())
    bm2 = mean(bdxh * xh.abs() + m["dxh"].abs() * bxh) + gam(n + 3) * mean((m["dxh"] * xh).abs())
    bdx = rs * (bdxh + bm1 + xh.abs() * bm2 + m["m2"].abs() * bxh) \
        + 5 * U * rs * (m["dxh"].abs() + m["m1"].abs() + (xh * m["m2"]).abs())
    nr = -(-R // (4 * ln_nblk(R))) + 4
    out.update(dx_bound=_stored(bdx, out["dx"], dt),
               dgamma_bound=(bdz * xh.abs() + m["dz"].abs() * bxh).sum(0) + gam(nr) * (m["dz"] * xh).abs().sum(0) + FLOOR,
               dbeta_bound=bdz.sum(0) + gam(nr) * m["dz"].abs().sum(0) + FLOOR)
    return out


def _lanes(v, nch, VEC):
    """[R, C] -> [R, nch, 64, VEC], zero padded: lane l of chunk ch owns columns (ch 64 + l) VEC ..."""
    R, C = v.shape
    return torch.cat((v, v.new_zeros(R, nch * 64 * VEC - C)), 1).view(R, nch, 64, VEC)


def _wave_allsum(v, nch, VEC):
    """Per-lane sequential sums, the DPP ladder inside rows of 16 (a pairwise tree), then the four row sums in sequence."""
    p = _lanes(v, nch, VEC)
    s = torch.zeros_like(p[:, 0, :, 0])
    for ch in range(nch):
        for e in range(VEC):
            s = s + p[:, ch, :, e]
    rows = _tree(s.view(-1, 4, 16))
    return (((rows[:, 0] + rows[:, 1]) + rows[:, 2]) + rows[:, 3])[:, None]


def _gelu_parts32(z):
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=z.device)              # noqa: E731
    xa = z.abs() * f(0.70710678118654752)
    t = 1 / (1 + f(_ASP) * xa)
    e = torch.exp(-xa * xa)
    poly = t * (f(_AS[0]) + t * (f(_AS[1]) + t * (f(_AS[2]) + t * (f(_AS[3]) + t * f(_AS[4])))))
    cdf = 0.5 * (1 + torch.copysign(1 - poly * e, z))
    return cdf, f(0.3989422804014327) * e


def emulate_ln(case, mean32, rstd32):
    """fp32 arithmetic in the kernels' order; the backward takes the stored statistics it is given, as the kernel does."""
    R, C, dt = case["R"], case["C"], case["dtype"]
    assert R <= 8192, "one row per wave only"
    VEC, nch = vec_of(dt), ln_nch(C, dt)
    x, dy, g, b = case["x"].float(), case["dy"].float(), case["gamma"].float(), case["beta"].float()
    inv_c = torch.tensor(1.0, dtype=torch.float32) / C
    x0 = x[:, :1]
    d = x - x0
    md = _wave_allsum(d, nch, VEC) * inv_c
    mu = x0 + md
    var = torch.clamp(_wave_allsum(d * d, nch, VEC) * inv_c - md * md, min=0)
    dc = d - md
    var = torch.where(md * md > LN_GUARD * var, _wave_allsum(dc * dc, nch, VEC) * inv_c, var)
    rs = torch.rsqrt(var + EPS)
    z = (x - mu) * rs * g + b
    out = dict(y=(z * _gelu_parts32(z)[0]).to(dt), mean=mu[:, 0], rstd=rs[:, 0])
    mu, rs = mean32[:, None], rstd32[:, None]
    xh = (x - mu) * rs
    z = xh * g + b
    cdf, pdf = _gelu_parts32(z)
    dz = dy * (cdf + z * pdf)
    dxh = dz * g
    m1, m2 = _wave_allsum(dxh, nch, VEC) * inv_c, _wave_allsum(dxh * xh, nch, VEC) * inv_c
    out["dx"] = (rs * (dxh - m1 - xh * m2)).to(dt)
    nb = ln_nblk(R)
    for name, t in (("dgamma_part", dz * xh), ("dbeta_part", dz)):      # one row per wave, the block adds its four waves
        t = torch.cat((t, t.new_zeros(4 * nb - R, C))).view(nb, 4, C)
        out[name] = (((0 + t[:, 0]) + t[:, 1]) + t[:, 2]) + t[:, 3]
    return out


def parity_ratio(case, ref, mean, rstd):
    """Worst error of the normalised values that the given statistics produce, over PARITY times the row's largest one."""
    xh = (case["x"].double() - mean.double()[:, None]) * rstd.double()[:, None]
    return float(((xh - ref["xh"]).abs() / (PARITY * ref["xh_max"])).max())


def stock_ln(case):
    """torch's own fp32 CPU layer_norm + gelu and their autograd on the stored inputs."""
    C, dt = case["C"], case["dtype"]
    x, ga, be = (case[k].float().clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = F.gelu(F.layer_norm(x, (C,), ga, be, EPS))
    (y * case["dy"].float()).sum().backward()
    return dict(y=y.detach().to(dt), dx=x.grad.to(dt), dgamma=ga.grad, dbeta=be.grad)


# ================================================================================================ row-dot
@functools.lru_cache(maxsize=None)
def rd_case(kind, M, C, dtype):
    g = torch.Generator().manual_seed(10 * C + M + RD_KINDS.index(kind))
    rn = lambda *s: torch.randn(*s, generator=g)                                   # noqa: E731
    x, base = rn(M, C), rn(M, C)
    w0, w1, b0, b1 = rn(C) / math.sqrt(C), rn(C) / math.sqrt(C), rn(1), rn(1)
    dz0, dz1 = rn(M), rn(M)
    if kind == "cancel":                  # x . w sums to about 0 from addends of about 1e3
        half = 1e3 * rn(M, C // 2)
        x = torch.stack((half, half), -1).flatten(-2).to(dtype).float() + 0.01 * rn(M, C)
        w0 = torch.stack((torch.ones(C // 2), -torch.ones(C // 2)), -1).flatten()
        w1 = -w0
    elif kind == "spike":                 # dz: mostly zeros and one large entry
        keep = torch.rand(M, generator=g) < 0.25
        dz0, dz1 = dz0 * keep, dz1 * ~keep
        dz0[M // 2] = 1e4
        dz1[0] = -1e4
    return dict(kind=kind, M=M, C=C, dtype=dtype, x=x.to(dtype), base=base.to(dtype), w0=w0, w1=w1, b0=b0, b1=b1,
                dz0=dz0, dz1=dz1)


def rd_ref(case, mutation=None):
    """float64: z0, z1 (b0 / b1 added), z0_nobias, z1_nobias, dx (base + dz0 w0), dx_nobase, dw0, db0, dw1, db1 and bounds."""
    M, C, dt = case["M"], case["C"], case["dtype"]
    VEC = vec_of(dt)
    x, base, w0, w1, b0, b1, dz0, dz1 = (case[k].double() for k in ("x", "base", "w0", "w1", "b0", "b1", "dz0", "dz1"))
    nz = 4 * VEC + 9
    out = {}
    for h, w, b in ((0, w0, b0), (1, w1, b1)):
        T = x.abs() @ w.abs()
        out[f"T{h}"] = T
        out[f"z{h}_nobias"], out[f"z{h}_nobias_bound"] = x @ w, gam(nz) * T + FLOOR
        out[f"z{h}"], out[f"z{h}_bound"] = x @ w + b * (2 if mutation == "bias_twice" else 1), gam(nz) * (T + b.abs()) + FLOOR
    rank1 = dz0[:, None] * w0
    if mutation == "head1_in_dx":
        rank1 = rank1 + dz1[:, None] * w1
    out["dx_nobase"], out["dx_nobase_bound"] = rank1, _stored(2 * U * rank1.abs(), rank1, dt)
    out["dx"] = rank1 + (0 if mutation == "dx_without_base" else base)
    out["dx_bound"] = _stored(2 * U * (base.abs() + rank1.abs()), out["dx"], dt)
    rpi = 256 // (C // VEC)
    nd = -(-M // (rd_nblk(M) * rpi)) + rpi + 1
    keep = torch.ones(M, dtype=x.dtype, device=x.device)
    if mutation == "last_chunk_dropped":
        keep[(M - 1) // rpi * rpi:] = 0
    for h, dz in ((0, dz0), (1, dz1)):
        dzk = dz * keep
        out[f"dw{h}"], out[f"dw{h}_bound"] = dzk @ x, gam(nd) * (dz.abs() @ x.abs()) + FLOOR
        src = (dz1 if h == 0 else dz0) if mutation == "db_wrong_head" else dzk
        out[f"db{h}"], out[f"db{h}_bound"] = src.sum()[None], gam(nd) * dz.abs().sum()[None] + FLOOR
    return out


RD_MUTATIONS = {"bias_twice": ("z0", "z1"), "dx_without_base": ("dx",), "head1_in_dx": ("dx", "dx_nobase"),
                "db_wrong_head": ("db0", "db1"), "last_chunk_dropped": ("dw0", "dw1", "db0", "db1")}
RD_OUTPUTS = ("z0", "z1", "z0_nobias", "z1_nobias", "dx", "dx_nobase", "dw0", "db0", "dw1", "db1")


def emulate_rd(case):
    """fp32 arithmetic in the kernels' order; the partial rows are summed in float64, as the tests do."""
    M, C, dt = case["M"], case["C"], case["dtype"]
    VEC = vec_of(dt)
    x, base, w0, w1, dz0, dz1 = (case[k].float() for k in ("x", "base", "w0", "w1", "dz0", "dz1"))
    passes = -(-C // (64 * VEC))
    out = {}
    for h, w, b in ((0, w0, case["b0"]), (1, w1, case["b1"])):
        p = _lanes(x * w, passes, VEC)
        acc = torch.zeros_like(p[:, 0, :, 0])
        for ps in range(passes):
            for e in range(VEC):
                acc = acc + p[:, ps, :, e]
        while acc.shape[1] > 1:                                           # xor 32, 16, ..., 1
            acc = acc[:, :acc.shape[1] // 2] + acc[:, acc.shape[1] // 2:]
        out[f"z{h}_nobias"], out[f"z{h}"] = acc[:, 0], acc[:, 0] + b.float()
    out["dx_nobase"] = (dz0[:, None] * w0).to(dt)
    out["dx"] = (base + dz0[:, None] * w0).to(dt)
    rpi, nb = 256 // (C // VEC), rd_nblk(M)
    iters = -(-M // (nb * rpi))
    for h, dz in ((0, dz0), (1, dz1)):
        for name, t in ((f"dw{h}", dz[:, None] * x), (f"db{h}", dz[:, None])):
            t = torch.cat((t, t.new_zeros(iters * nb * rpi - M, t.shape[1]))).view(iters, nb, rpi, -1)
            acc = torch.zeros_like(t[0])
            for it in range(iters):
                acc = acc + t[it]
            s = torch.zeros_like(acc[:, 0])
            for l in range(rpi):
                s = s + acc[:, l]
            out[name] = s.double().sum(0)
    return out


# ================================================================================================ column sums
@functools.lru_cache(maxsize=None)
def cs_case(kind, G, R, C):
    g = torch.Generator().manual_seed(100 * R + C + G)
    x = torch.randn(G, R, C, generator=g)
    if kind == "cancel" and R > 1:        # rows of about +-1e3 whose sum is of order 1
        big = 1e3 * torch.randn(G, R // 2, C, generator=g)
        x[:, :R // 2 * 2] += torch.stack((big, -big), 2).flatten(1, 2)
    return dict(kind=kind, G=G, R=R, C=C, x=x)


def cs_chain(R):
    return -(-(-(-R // CS_CHUNKS)) // 4) + 36


def cs_ref(case, mutation=None):
    x = case["x"].double()
    R = case["R"]
    per = -(-R // CS_CHUNKS)
    xs = x[:, :(R - 1) // per * per] if mutation == "last_chunk_dropped" else x
    return dict(out=xs.sum(1), out_bound=gam(cs_chain(R)) * x.abs().sum(1) + FLOOR)


def emulate_cs(case):
    x, G, R, C = case["x"].float(), case["G"], case["R"], case["C"]
    per = -(-R // CS_CHUNKS)
    out = torch.zeros(G, C)
    for k in range(CS_CHUNKS):
        sm = []
        for w in range(4):
            s = torch.zeros(G, C)
            for r in range(k * per + w, min(R, (k + 1) * per), 4):
                s = s + x[:, r]
            sm.append(s)
        out = out + (((sm[0] + sm[1]) + sm[2]) + sm[3])
    return out
