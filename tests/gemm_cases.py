"""Shared by tests/test_gemm_cases_reference.py (CPU) and tests/test_gpu_gemm.py: shape tables, seeded inputs, float64
references, derived error bounds, an fp32 emulation in the kernels' own order and named mutations for
  csrc/gemm_st.hip   the streamed-activation kernel behind gf_gemm / gf_gemm_res2 (14 template instances)
  csrc/gemm_ws.hip   the register-resident kernel behind gf_gemm, bf16 and fp32
  csrc/bgemm.hip     gf_bgemm
(contract in include/gf_amd.h).  No GPU code and no library code here; every function works on the device its case lives
on.  Inputs are taken as stored: a bf16 tensor is upcast to float64 and never rounded again.

The operation.   s = [x0 | x1] W^T + bias + res + res_b (absent terms are 0); channels n < rot_n are then rotated in pairs
(2 i, 2 i + 1) by the token's table row cs[m, n mod 64] = interleaved (cos, sin) of a 64-wide head:
    y[2 i] = s[2 i] c - s[2 i + 1] sn,   y[2 i + 1] = s[2 i + 1] c + s[2 i] sn        -- on the sum INCLUDING the residual;
    C = alpha A B for gf_bgemm.

Bounds (derived, not tuned).  U = 2^-24 is the fp32 rounding unit, gam(n) = n U / (1 - n U) the bound of a chain of n
roundings, BF = 2^-9 half a bf16 ulp relative to the power of two above the value (elementwise_cases.py).
  sum      bf16 x bf16 products are exact in fp32, an fp32 product is rounded once together with its add (fused); the K
           products and the `terms` epilogue addends (bias, res, res_b) enter one fp32 sum in some order, so each addend
           passes through at most K + terms roundings:  |ds| <= gam(K + terms) T,  T = |x| |W|^T + |bias| + |res| + |res_b|.
  rotary   the two computed addends carry their sums' errors through c and sn; each is one product rounding and shares
           the rounding of the add, two more roundings per addend, on their computed size:
           |dy| <= |c| ds + |sn| ds' + gam(2) (|c| (|s| + ds) + |sn| (|s'| + ds')).
  stored   fp32 output: nothing more.  bf16 output: ONE rounding of the final value, BF 2^top with |y| + |dy| < 2^top.
  bgemm    the K products, then the product with alpha: gam(K + 1) |alpha| |A| |B|, stored as above.
On `exact` and `coded` every product and every partial sum is an integer multiple of 1/4 far below 2^24: fp32 arithmetic is
exact in any order and the kernel's output must EQUAL the float64 result rounded once to the output type -- in fp32 mode,
in bf16 mode, and between the streamed and the register-resident kernel.

Launch arithmetic of gemm_st restated (st_plan; the CPU test holds it against the library's gf_gemm_plan):
  rows per tile TR = 32768 / (2 K) = 64 / 32 at K = 256 / 512; ntile = M / TR; grid = (gx, N / 256) with
  gx = min(ST_WGS / (N / 256), ntile), ST_WGS = 256; workgroup x walks the tiles x, x + gx, ...: ceil(ntile / gx) of them
  where x < ntile mod gx (or when that is 0), floor(ntile / gx) elsewhere.
The 14 instances reachable through gf_gemm / gf_gemm_res2 are K in {256, 512} x (one | two sources) x 0 / 1 / 2 residuals
plus the rotary instance (one source, no residual) at each K: ST_INSTANCES.  With N = 2048 the grid is 32 wide and ST_M
gives every instance a smallest launch, one tile everywhere and the ragged sets {2,1}, {3,2}, {4,3}."""
import functools
import math

import torch

from elementwise_cases import BF, DETECT, _stored, gam, ratio  # noqa: F401  (BF, DETECT, ratio: used by the tests)

F32, BF16 = torch.float32, torch.bfloat16
GF_F32, GF_BF16 = 0, 1
GF_ERR_UNSUPPORTED, GF_ERR_SHAPE, GF_ERR_ALIGN, GF_ERR_DTYPE = -1, -2, -3, -4
KINDS = ("rand", "cancel", "exact", "coded")
EXACT_KINDS = ("exact", "coded")

# ================================================================================================ gemm_st tables
ST_WGS, ST_TILE_BYTES = 256, 32768
# (K, two sources, residuals, rotary): every template instance gs_launch is called with
ST_INSTANCES = [(K, two, nres, False) for K in (256, 512) for two in (False, True) for nres in (0, 1, 2)] \
    + [(256, False, 0, True), (512, False, 0, True)]
ST_N = 2048                                   # 8 channel groups: the grid is 256 / 8 = 32 workgroups wide
# M -> the set of tile counts per workgroup at N = 2048 (what st_plan must say; the reason each entry is here)
ST_M = {256: [(64 * 1, {1}),                  # ONE tile, one workgroup per channel group: both prologue DMAs clamped onto it
              (64 * 32, {1}),                 # 32 tiles on 32 workgroups: T = 1 everywhere, the i == 0 wait alone
              (64 * 33, {2, 1}),              # ragged: workgroup 0 reaches the i == 1 wait, the others stop at i == 0
              (64 * 65, {3, 2}),              # workgroup 0 reaches the steady-state wait (i >= 2) and the ring's third stage
              (64 * 97, {4, 3})],             # the ring wraps (stage 0 reused) in workgroup 0 only
        512: [(64, {1}),                      # the smallest M the kernel takes: two 32-row tiles, two workgroups of one
              (1024, {1}),
              (1088, {2, 1}),
              (2112, {3, 2}),
              (3136, {4, 3})]}
ST_RAGGED_M = {256: 64 * 33, 512: 1088}       # where the variants (aliasing, strides, slices, NaN containment) run
# rotary: rot_n % 256 == 0.  N = 2048 = rot_n is one launch; N = 2304 adds a plain launch over the last 256 channels with
# shifted w / bias / y pointers (one channel group: its grid is min(256, ntile) wide, another tile distribution)
ST_ROT_N = [(2048, 2048), (2304, 2048)]
# (M, N) at which blockIdx.y offsets of 1 and 3 channel groups are seen (N = 256: gx = min(256, ntile); N = 768: gx = 85)
ST_NARROW = {256: [(64 * 3, 256, {1}), (64 * 86, 768, {2, 1})],
             512: [(32 * 6, 256, {1}), (32 * 172, 768, {3, 2})]}


def st_plan(M, N, K):
    """(rows per tile, grid x, grid y, fewest, most tiles of a workgroup) of one streamed launch."""
    tr = ST_TILE_BYTES // (2 * K)
    ntile, gy = M // tr, N // 256
    gx = max(1, min(ST_WGS // gy, ntile))
    return tr, gx, gy, ntile // gx, -(-ntile // gx)


def st_serves(M, N, K0, K1, nres, rot_n, dtype):
    K = K0 + K1
    return (dtype == BF16 and K in (256, 512) and N % 256 == 0 and M % 64 == 0 and K1 in (0, K0)
            and (rot_n == 0 or (rot_n % 256 == 0 and rot_n <= N and nres == 0 and K1 == 0)))


# ================================================================================================ gemm_ws tables
WS_K = {BF16: [32, 64, 128, 256, 512], F32: [32, 64, 128, 256]}
WS_N = [32,      # one 32-channel tile: the odd flush alone
        96,      # three tiles: a pair, then an odd last tile (its second accumulator is not flushed)
        160,     # five tiles
        288,     # nine tiles; at K = 32 a slice holds 256 channels: a partial last weight slice of one tile
        768]     # the workload's widest (fused qkv): 2 to 24 slices
WS_M = [1,       # one live row of one wave
        33,      # a second 32-row block with one row
        255,     # one row short of the 256-row workgroup block (fp32 K = 128: 128-row blocks, one short of two)
        257,     # one row into the second workgroup
        513 + 18]   # three workgroups, the last with a tail of 19 rows
WS_TWO_K0 = {BF16: [16, 32, 64, 128, 256], F32: [16, 32, 64, 128]}       # every K0 = K1 the dispatch takes


def ws_rows(K, dtype):
    """Rows of one workgroup block (waves x 32 x blocks per wave) of the instance that serves K."""
    if dtype == BF16:
        return 256
    return 128 if K == 128 else 256


def ws_rot_ns(N):
    """rot_n values for an N: one head, every channel, and all but the last 32 (a multiple of 64 below N)."""
    out = {64, N} | ({N - 32} if (N - 32) % 64 == 0 and N > 32 else set())
    return sorted(r for r in out if r % 64 == 0 and 0 < r <= N)


# ================================================================================================ bgemm tables
BG_MN = [1, 127, 128, 129, 257]               # around the 128 x 128 tile, and a third tile row
BG_KSTEP = {BF16: 64, F32: 32}


def bg_ks(dtype):
    s = BG_KSTEP[dtype]
    return [s // 2 - 3, s - 1, s, s + 1, 2 * s - 8, 2 * s, 2 * s + 5]      # below one step, around one and two steps


# orientation -> how A [M, K] / B [K, N] are laid out: "kc" k-contiguous, "rc" row-contiguous (the kernel's AKC / BKC = true /
# false), "nu" no unit stride (scalar guarded loads, k-contiguous image), "mis" k-contiguous but a slice that starts 2 bytes
# (bf16) / 4 bytes (fp32) off a 16-byte boundary
BG_ORIENT = [("kc", "kc"), ("kc", "rc"), ("rc", "kc"), ("rc", "rc")]
BG_SCALAR = [("nu", "kc"), ("kc", "nu"), ("mis", "rc"), ("rc", "mis"), ("nu", "nu")]


# ================================================================================================ cases
@functools.lru_cache(maxsize=8)
def gemm_case(kind, M, N, K0, K1, nres, rot_n, dtype, device="cpu", bias=True):
    """Seeded inputs of y = [x0 | x1] W^T + bias + res + res_b (+ rotary on [0, rot_n)); rot_n = 0: no table."""
    K = K0 + K1
    g = torch.Generator(device=device).manual_seed(7 * M + 3 * N + K + 11 * nres + rot_n + KINDS.index(kind))
    rn = lambda *s: torch.randn(*s, generator=g, device=device)                                    # noqa: E731
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).float()       # noqa: E731
    theta = (torch.rand(M, 32, generator=g, device=device) * 2 - 1) * math.pi
    cs = torch.stack((torch.cos(theta), torch.sin(theta)), -1).flatten(-2)
    if kind in ("rand", "cancel"):
        x, w, b = rn(M, K), rn(N, K) / math.sqrt(K), rn(N)
        res = [rn(M, N) for _ in range(nres)]
        if kind == "cancel" and nres:         # res = -(the product as bf16 would store it) + a small term
            prod = (x.to(dtype).double() @ w.to(dtype).double().t() + (b.double() if bias else 0)).to(BF16).float()
            res[0] = -prod + (0.01 * rn(M, N) if nres == 1 else 0)
            if nres == 2:
                res[1] = 0.01 * rn(M, N)
    elif kind == "exact":
        x, w, b = ri(-3, 3, M, K), ri(-2, 2, N, K), ri(-8, 8, N)
        res = [ri(-8, 8, M, N) for _ in range(nres)]
        cs = (torch.randint(-2, 3, (M, 64), generator=g, device=device).float() / 2)               # {0, +-1/2, +-1}
    else:                                     # coded: y[m, n] = rowcode(m) (ncode(n) + kcode(hot(m))) + bias + res
        m = torch.arange(M, device=device)
        hot = (5 * m + 3) % K
        x = torch.zeros(M, K, device=device)
        x[m, hot] = (1 + (m // 32) % 2).float()                                                    # 1 / 2 by 32-row block
        w = ((torch.arange(N, device=device) % 256 - 128)[:, None] + (torch.arange(K, device=device) % 256 - 128)[None]).float()
        b = ri(-4, 4, N)
        res = [ri(-8, 8, M, N) for _ in range(nres)]
        cs = (torch.randint(-2, 3, (M, 64), generator=g, device=device).float() / 2)
    x = x.to(dtype)
    return dict(kind=kind, M=M, N=N, K0=K0, K1=K1, nres=nres, rot_n=rot_n, dtype=dtype,
                x0=x[:, :K0].contiguous(), x1=x[:, K0:].contiguous() if K1 else None, w=w.to(dtype),
                bias=b.contiguous() if bias else None, res=res[0].to(dtype) if nres >= 1 else None,
                res_b=res[1].to(dtype) if nres == 2 else None, cs=cs.contiguous() if rot_n else None)


def _rotate(s, cs, rot_n, sign=1.0):
    """Rotate channels [0, rot_n) of s [M, N] in pairs by the [M, 64] table (any float dtype: the arithmetic is s's)."""
    M = s.shape[0]
    c = cs[:, 0::2].repeat(1, rot_n // 64)                     # [M, rot_n / 2]: pair i of a head uses table column i mod 32
    sn = sign * cs[:, 1::2].repeat(1, rot_n // 64)
    a, b = s[:, 0:rot_n:2], s[:, 1:rot_n:2]
    rot = torch.stack((a * c - b * sn, b * c + a * sn), -1).reshape(M, rot_n)
    return torch.cat((rot, s[:, rot_n:]), 1)


def _round(v, dtype):
    """float64 -> rounded ONCE to dtype, back as float64."""
    return v.to(dtype).double()


GEMM_MUTATIONS = {            # name -> what a case needs for the mutation to apply
    "kstep_dropped": lambda c: True,
    "halves_swapped": lambda c: c["K1"] > 0,
    "bias_shifted": lambda c: c["bias"] is not None,
    "res_row32": lambda c: c["nres"] >= 1 and c["M"] > 32,
    "res_b_missing": lambda c: c["nres"] == 2,
    "res_after_rounding": lambda c: c["nres"] >= 1 and c["dtype"] == BF16,
    "rot_before_res": lambda c: c["rot_n"] > 0 and c["nres"] >= 1,
    "rot_sign": lambda c: c["rot_n"] > 0,
    "table_halves_swapped": lambda c: c["rot_n"] > 0,
    "stale_tile": lambda c: c["M"] >= 64,
}


def gemm_ref(case, mutation=None, stale=(32, 1)):
    """float64 y and its bound `y_bound` (no bound under a mutation), `rounded` = y rounded once to the output type.
    stale = (rows per tile, grid x) for the stale_tile mutation: the second tile of workgroup 0 (rows [tr gx, tr gx + tr))
    is computed from the activation rows of its first (rows [0, tr))."""
    dt, M, K0, rot_n = case["dtype"], case["M"], case["K0"], case["rot_n"]
    x0, w = case["x0"].double(), case["w"].double()
    x1 = case["x1"].double() if case["x1"] is not None else None
    if mutation == "halves_swapped":
        x0, x1 = x1, x0
    x = x0 if x1 is None else torch.cat((x0, x1), 1)
    if mutation == "kstep_dropped":           # the second 16-wide k-step never multiplied
        x = x.clone()
        x[:, 16:32] = 0
    if mutation == "stale_tile":
        tr, gx = stale
        x = x.clone()
        x[tr * gx:tr * gx + tr] = x[:tr]
    zero = torch.zeros((), dtype=torch.float64, device=w.device)
    bias = case["bias"].double() if case["bias"] is not None else zero
    if mutation == "bias_shifted":
        bias = bias.roll(8)
    res = case["res"].double() if case["res"] is not None else zero
    res_b = case["res_b"].double() if case["res_b"] is not None else zero
    if mutation == "res_row32":
        res = res.roll(-32, 0)
    if mutation == "res_b_missing":
        res_b = zero
    cs = case["cs"].double() if rot_n else None
    if mutation == "table_halves_swapped":
        cs = torch.cat((cs[:, 32:], cs[:, :32]), 1)
    prod = x @ w.t() + bias
    if mutation == "res_after_rounding":
        prod = _round(prod, BF16)
    if mutation == "rot_before_res":
        y = _rotate(prod, cs, rot_n) + res + res_b
    else:
        s = prod + res + res_b
        y = _rotate(s, cs, rot_n, -1.0 if mutation == "rot_sign" else 1.0) if rot_n else s
    out = dict(y=y, rounded=_round(y, dt))
    if mutation is not None:
        return out
    terms = (case["bias"] is not None) + case["nres"]
    T = x.abs() @ w.abs().t() + bias.abs() + res.abs() + res_b.abs()
    ds = gam(K0 + case["K1"] + terms) * T
    if rot_n:
        sa = s.abs() + ds
        ca = torch.stack((cs[:, 0::2].abs(), cs[:, 0::2].abs()), -1).flatten(1).repeat(1, rot_n // 64)     # |c| per channel
        sna = torch.stack((cs[:, 1::2].abs(), cs[:, 1::2].abs()), -1).flatten(1).repeat(1, rot_n // 64)
        swap = lambda t: torch.stack((t[:, 1:rot_n:2], t[:, 0:rot_n:2]), -1).reshape(M, rot_n)    # noqa: E731  the pair partner
        dr = ca * ds[:, :rot_n] + sna * swap(ds) + gam(2) * (ca * sa[:, :rot_n] + sna * swap(sa))
        ds = torch.cat((dr, ds[:, rot_n:]), 1)
    out["y_bound"] = _stored(ds, y, dt)
    return out


def emulate_gemm(case, stock=False):
    """The kernels' own order: fp32 matmul of the stored operands, epilogue in fp32 (bias, res, res_b, rotation), one rounding.
    stock: torch.nn.functional.linear in fp32, then the same epilogue."""
    x = case["x0"].float() if case["x1"] is None else torch.cat((case["x0"], case["x1"]), 1).float()
    w = case["w"].float()
    if stock:
        s = torch.nn.functional.linear(x, w, case["bias"])
    else:
        s = x @ w.t()
        if case["bias"] is not None:
            s = s + case["bias"]
    for r in (case["res"], case["res_b"]):
        if r is not None:
            s = s + r.float()
    if case["rot_n"]:
        s = _rotate(s, case["cs"], case["rot_n"])
    return s.to(case["dtype"])


# ---- bgemm
def _laid_out(t, how, dtype):
    """A [batch, R, K] tensor (values kept) stored the given way; returns a view of shape [batch, R, K]."""
    Bn, R, K = t.shape
    t = t.to(dtype)
    ld = lambda n: (n + 16 + 7) // 8 * 8      # noqa: E731  a wider row that keeps every row 16-byte aligned in both dtypes
    if how == "kc":                            # k-contiguous inside a wider, sliced buffer: batch stride != R K; 16-byte loads
        buf = torch.zeros(Bn, R + 3, ld(K), dtype=dtype, device=t.device)
        v = buf[:, 1:1 + R, 8:8 + K]
    elif how == "rc":                          # row-contiguous: [batch, K, R] storage, sliced; 16-byte loads
        buf = torch.zeros(Bn, K + 2, ld(R), dtype=dtype, device=t.device)
        v = buf[:, 1:1 + K, 8:8 + R].transpose(1, 2)
    elif how == "nu":                          # no unit stride: every second element along k
        buf = torch.zeros(Bn, R, 2 * K + 2, dtype=dtype, device=t.device)
        v = buf[:, :, 1:1 + 2 * K:2]
    else:                                      # "mis": unit stride along k, rows 16-byte multiples, base one element off
        buf = torch.zeros(Bn, R, ld(K), dtype=dtype, device=t.device)
        v = buf[:, :, 1:1 + K]
    v.copy_(t)
    return v


@functools.lru_cache(maxsize=8)
def bgemm_case(kind, batch, M, N, K, oa, ob, dtype, device="cpu", alpha=0.75):
    g = torch.Generator(device=device).manual_seed(5 * M + 3 * N + K + batch + KINDS.index(kind))
    if kind == "rand":
        a = torch.randn(batch, M, K, generator=g, device=device)
        b = torch.randn(batch, N, K, generator=g, device=device) / math.sqrt(K)
    else:                                      # exact: small integers, alpha a power of two or 3/4
        a = torch.randint(-3, 4, (batch, M, K), generator=g, device=device).float()
        b = torch.randint(-2, 3, (batch, N, K), generator=g, device=device).float()
    return dict(kind=kind, batch=batch, M=M, N=N, K=K, dtype=dtype, alpha=alpha, oa=oa, ob=ob,
                a=_laid_out(a, oa, dtype), b=_laid_out(b, ob, dtype).transpose(1, 2))      # a [batch, M, K], b [batch, K, N]


BGEMM_MUTATIONS = {"alpha_twice": lambda c: True,
                   "last_kstep_dropped": lambda c: True,
                   "a_transposed": lambda c: min(c["M"], c["K"]) > 1}


def bgemm_ref(case, mutation=None):
    dt, K, alpha = case["dtype"], case["K"], case["alpha"]
    a, b = case["a"].double(), case["b"].double()
    if mutation == "last_kstep_dropped":       # the last (partial) k-step never multiplied
        a = a.clone()
        a[:, :, (K - 1) // BG_KSTEP[dt] * BG_KSTEP[dt]:] = 0
    if mutation == "a_transposed":             # element (i, k) read from (k, i) where both exist
        s = min(case["M"], K)
        a = a.clone()
        a[:, :s, :s] = a[:, :s, :s].transpose(1, 2).clone()
    c = alpha * (alpha if mutation == "alpha_twice" else 1.0) * torch.bmm(a, b)
    out = dict(c=c, rounded=_round(c, dt))
    if mutation is None:
        out["c_bound"] = _stored(gam(K + 1) * abs(alpha) * torch.bmm(a.abs(), b.abs()), c, dt)
    return out


def emulate_bgemm(case):
    return (torch.bmm(case["a"].float(), case["b"].float()) * torch.tensor(case["alpha"], dtype=torch.float32)).to(case["dtype"])
