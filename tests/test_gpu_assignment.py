"""The assignment head kernels (csrc/assignment.hip) on their own, through the C ABI of include/gf_amd.h: gf_rows_lse,
gf_rows_argmax, gf_rows_lse_argmax, gf_assign_write, gf_dual_softmax_bwd and gf_filter_matches against float64 references
(tests/assignment_cases.py; its references, mutations, rounding model and margins are held on the CPU by
tests/test_assignment_cases_reference.py), and ops.dual_lse_stacked / ops.assign_write against float64 autograd.

Shapes (B, owner rows, streamed rows) come from the kernels' geometry -- owner blocks of 128, tiles of 64, four splits of the
streamed rows in assign_write / dual_softmax_bwd -- and are used in both roles; every one at D = 256, the multi-block ones
also at D = 64 and 128, all in fp32 and bf16.  Value cases: rand, planted (a winner per owner row with a float64 margin of
GAP), ties (the winner duplicated bit for bit: the lowest index must win), large (|S| about 100: the maximum in the first
tile, in the last ragged tile, every score about -100, matchability logits 0, +-30, +-90) and masked (-inf column bias).
Every output lies between GUARD sentinel elements that must survive and is pre-filled (NaN, or a sentinel index), so an
element that is never written shows.

Bounds (derived in the docstring of assignment_cases, U = 2^-24; `T` = sum of the absolute values of a value's addends):
  value, max, matrix element   |x - ref| <= 1e-5 T + 1e-6
  lse                          the same with T = max_j T_ij + |lse_i|
  dS                           sum over its softmax terms t of |t| (3 U (|S| + |n|) + 8 U + 1e-5 T_S + 1e-6) + 2 U |galpha G|
                               + 1e-12, and 2^-7 |ref| more for a bf16 dS
  expsum                       sum_e exp(out_e) (bound(out_e) + 4 U) + (135 + 16 nob) U expsum   (relative: positive addends)
  filter_matches scores        s (2 U |max0| + 8 U)
  arg-max                      exactly the reference's on planted, ties and large; on rand a row whose float64 gap is below the
                               two value bounds may differ (its picked value within them), at most 0.1 % of the rows
  op-level gradients           _tols(dtype) of the kernel tests (1e-4 fp32, 5e-2 bf16) after dividing by the reference's
                               largest magnitude, as in test_gpu_lg_loss.py: they pass through bf16 products
Every test prints its worst error / bound ratio."""
import functools
import math

import pytest
import torch

import assignment_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from glue_factory_amd import lib as L_
    from glue_factory_amd import ops
    from glue_factory_amd.ops import _dt, _p, _stream

DEV = "cuda"
GF_ERR_UNSUPPORTED, GF_ERR_SHAPE, GF_ERR_DTYPE = -1, -2, -4
GUARD = 64               # sentinel elements on either side of every output
SENTINEL = -776.0        # exact in bf16, and as an index out of every range
CFG_IDS = ["x".join(map(str, c)) for c in C.CONFIGS]
WRITE_COMBOS = [(2.0, 0.0, "head", True), (1.0, -1.75, "head", True), (2.0, -1.75, "none", True), (1.0, 0.0, "plain", False)]
cases = pytest.mark.parametrize("cfg", C.CONFIGS, ids=CFG_IDS)
dtypes = pytest.mark.parametrize("dtype", C.DTYPES, ids=["fp32", "bf16"])


def _tols(dtype):
    return dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=5e-2, atol=5e-2)


def _ratio(x, ref, bound):
    """Worst |x - ref| / bound; a NaN (an element never written) is infinitely far off, two equal infinities agree."""
    x, ref = x.detach().cpu().double(), ref.detach().cpu().double()
    if x.numel() == 0:
        return 0.0
    d = torch.where(x == ref, torch.zeros_like(ref), (x - ref).abs() / bound.cpu().double())
    return math.inf if torch.isnan(d).any() else float(d.max())


class _Worst:
    """Collects error / bound ratios, prints the worst of each name and fails if one exceeds 1."""

    def __init__(self, what):
        self.what, self.worst, self.notes = what, {}, []

    def add(self, name, x, ref, bound):
        assert x.shape == ref.shape, (name, x.shape, ref.shape)
        self.worst[name] = max(self.worst.get(name, 0.0), _ratio(x, ref, bound))

    def finish(self):
        print(f"{self.what}: worst error/bound " + ", ".join(f"{k} {v:.3g}" for k, v in self.worst.items()) + "".join(self.notes))
        bad = {k: v for k, v in self.worst.items() if not v <= 1.0}
        assert not bad, f"{self.what}: over the bound (error / bound): {bad}"


def _guarded(shape, dtype, fill):
    """(buffer, view): `view` of the given shape filled with `fill`, GUARD sentinel elements on either side of it."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return buf, view


def _guards_intact(*bufs):
    torch.cuda.synchronize()
    for buf in bufs:
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "a sentinel next to an output was written"


@functools.lru_cache(maxsize=8)
def _on_device(kind, cfg, dtype):
    case = C.get_case(kind, *cfg, dtype)
    return case, {k: case[k].to(DEV) for k in ("own", "oth", "sbias", "obias", "z", "nrm", "bin_s", "bin_o", "gr", "gc", "r32", "c32")}


def _kinds(Ns):
    return [k for k in C.KINDS if C.has_kind(k, Ns)]


def _what(entry, cfg, dtype):
    return f"{entry} {cfg} {str(dtype)[6:]}"


def _check_arg(w, name, kind, ref, val, idx, Ns):
    """Value within the bound; index exact, except on `rand` where an undecided row (float64 gap below the two bounds) may
    pick the runner-up.  Returns the number of such rows."""
    val, idx = val.cpu(), idx.cpu()
    assert int(idx.min()) >= 0 and int(idx.max()) < Ns, f"{name}: an index outside [0, Ns) or never written"
    w.add(name + "/max", val, ref["val"], ref["bound"])
    differ = idx != ref["idx"]
    if kind != "rand":
        assert not differ.any(), f"{name}: {int(differ.sum())} arg-maxes differ on {kind}"
        return 0
    assert (ref["gap"][differ] <= ref["bound_pair"][differ]).all(), f"{name}: a decided arg-max differs"
    picked = ref["X"].gather(2, idx[..., None]).squeeze(2)
    w.add(name + "/picked", picked, ref["val"], ref["bound_pair"])
    assert float(differ.double().mean()) <= C.MAX_BELOW_MARGIN, f"{name}: too many undecided rows"
    return int(differ.sum())


# =============================================================================================== lse and arg-max entries
@dtypes
@cases
def test_rows_lse(cfg, dtype):
    """gf_rows_lse without and with a column bias (the raw-score `plain` arm and the biased arm), on every value case."""
    B, No, Ns, D = cfg
    lib = L_.load()
    w = _Worst(_what("gf_rows_lse", cfg, dtype))
    for kind in _kinds(Ns):
        case, d = _on_device(kind, cfg, dtype)
        for with_bias in (False, True):
            ref = C.ref_lse(case, with_bias)
            buf, lse = _guarded((B, No), torch.float32, math.nan)
            L_.check(lib.gf_rows_lse(_p(d["own"]), _p(d["oth"]), _p(d["sbias"]) if with_bias else None, _p(lse),
                                     B, No, Ns, D, _dt(d["own"]), _stream()), "gf_rows_lse")
            _guards_intact(buf)
            w.add(f"{kind}/{'bias' if with_bias else 'plain'}", lse, ref["lse"], ref["bound"])
    w.finish()


@dtypes
@cases
def test_rows_argmax(cfg, dtype):
    """gf_rows_argmax with alpha in {1, 2}, without and with a column bias; a -inf bias on every column of the last image
    gives index 0 and maximum -inf, as torch.max does."""
    B, No, Ns, D = cfg
    lib = L_.load()
    w = _Worst(_what("gf_rows_argmax", cfg, dtype))
    undecided = 0

    def run(d, alpha, sbias):
        bv, val = _guarded((B, No), torch.float32, math.nan)
        bi, idx = _guarded((B, No), torch.int64, int(SENTINEL))
        L_.check(lib.gf_rows_argmax(_p(d["own"]), _p(d["oth"]), _p(sbias), alpha, _p(val), _p(idx),
                                    B, No, Ns, D, _dt(d["own"]), _stream()), "gf_rows_argmax")
        _guards_intact(bv, bi)
        return val, idx

    for kind in _kinds(Ns):
        case, d = _on_device(kind, cfg, dtype)
        for v in C.ARG_VARIANTS[:4]:
            val, idx = run(d, v[1], d["sbias"] if v[2] else None)
            undecided += _check_arg(w, f"{kind}/a{v[1]:g}{'b' if v[2] else ''}", kind, C.ref_argmax(case, v), val, idx, Ns)
    case, d = _on_device("rand", cfg, dtype)
    sb = C.masked_bias(case)
    for v in C.ARG_VARIANTS[2:4]:
        val, idx = run(d, v[1], sb.to(DEV))
        ref = C.ref_argmax(case, v, sbias=sb)
        assert (idx[-1] == 0).all() and (val[-1] == -math.inf).all(), "masked image: expected index 0 and maximum -inf"
        undecided += _check_arg(w, f"masked/a{v[1]:g}", "rand", ref, val, idx, Ns)
    w.notes.append(f"; undecided rows on rand: {undecided} of {6 * B * No} ({undecided / (6 * B * No):.4%})")
    w.finish()


@dtypes
@cases
def test_rows_lse_argmax(cfg, dtype):
    """gf_rows_lse_argmax (alpha = 2, bias logsigmoid(z) - n) with the lse and with lse == NULL, whose buffer stays untouched."""
    B, No, Ns, D = cfg
    lib = L_.load()
    w = _Worst(_what("gf_rows_lse_argmax", cfg, dtype))
    v = C.ARG_VARIANTS[4]
    undecided = 0
    for kind in _kinds(Ns):
        case, d = _on_device(kind, cfg, dtype)
        ref, ref_lse = C.ref_argmax(case, v), C.ref_lse(case, False)
        for with_lse in (True, False):
            bl, lse = _guarded((B, No), torch.float32, math.nan if with_lse else SENTINEL)
            bv, val = _guarded((B, No), torch.float32, math.nan)
            bi, idx = _guarded((B, No), torch.int64, int(SENTINEL))
            L_.check(lib.gf_rows_lse_argmax(_p(d["own"]), _p(d["oth"]), _p(d["z"]), _p(d["nrm"]), v[1], _p(lse) if with_lse else None,
                                            _p(val), _p(idx), B, No, Ns, D, _dt(d["own"]), _stream()), "gf_rows_lse_argmax")
            _guards_intact(bl, bv, bi)
            name = f"{kind}/{'lse' if with_lse else 'nolse'}"
            undecided += _check_arg(w, name, kind, ref, val, idx, Ns)
            if with_lse:
                w.add(name + "/lse", lse, ref_lse["lse"], ref_lse["bound"])
            else:
                assert (bl == SENTINEL).all(), "lse == NULL, but the buffer was written"
    w.notes.append(f"; undecided rows on rand: {undecided} of {2 * B * No} ({undecided / (2 * B * No):.4%})")
    w.finish()


# =============================================================================================== split kernels
@dtypes
@cases
def test_assign_write(cfg, dtype):
    """gf_assign_write(a = streamed, b = owner): every element of [B, M+1, N+1] with alpha in {1, 2}, corner in {0, -1.75}, all
    four bias / bin vectors given and all four NULL; expsum NULL, and given pre-filled with garbage, which the call must
    zero."""
    B, No, Ns, D = cfg
    lib = L_.load()
    w = _Worst(_what("gf_assign_write", cfg, dtype))
    for kind in ("rand", "planted"):
        case, d = _on_device(kind, cfg, dtype)
        for alpha, corner, mode, with_expsum in WRITE_COMBOS:
            vecs = C.write_vecs(case, mode)
            ref = C.ref_write(case, alpha, corner, vecs)
            dv = [None] * 4 if vecs is None else [v.to(DEV).contiguous() for v in vecs]
            bo, out = _guarded((B, Ns + 1, No + 1), torch.float32, math.nan)
            be, es = _guarded((B,), torch.float32, 3.0e30)
            L_.check(lib.gf_assign_write(_p(d["oth"]), _p(d["own"]), *(_p(v) for v in dv), alpha, corner, _p(out),
                                         _p(es) if with_expsum else None, B, Ns, No, D, _dt(d["own"]), _stream()), "gf_assign_write")
            _guards_intact(bo, be)
            name = f"{kind}/a{alpha:g}{mode}"
            w.add(name, out, ref["out"], ref["bound"])
            if with_expsum:
                w.add(name + "/expsum", es, ref["expsum"], ref["expsum_bound"])
            else:
                assert (es == 3.0e30).all()
    w.finish()


@dtypes
@cases
def test_dual_softmax_bwd(cfg, dtype):
    """gf_dual_softmax_bwd(a = streamed, b = owner) with G == NULL (ldg and galpha then mean nothing), G with ldg = N + 1 and
    galpha = 1, G with ldg = N + 8 and galpha = 0.5; G's dustbin row, dustbin column and padding hold NaN, so a read
    outside the core shows as a non-finite dS.  dS is written in the operands' dtype."""
    B, No, Ns, D = cfg
    lib = L_.load()
    w = _Worst(_what("gf_dual_softmax_bwd", cfg, dtype))
    for kind in ("rand", "planted"):
        case, d = _on_device(kind, cfg, dtype)
        for ldg, galpha in ((0, 0.37), (No + 1, 1.0), (No + 8, 0.5)):
            ref = C.ref_bwd(case, ldg > 0, galpha, dtype)
            G = C.padded_G(case, ldg).to(DEV) if ldg else None
            bs, dS = _guarded((B, Ns, No), dtype, math.nan)
            L_.check(lib.gf_dual_softmax_bwd(_p(d["oth"]), _p(d["own"]), _p(d["r32"]), _p(d["c32"]), _p(d["gr"]), _p(d["gc"]),
                                             _p(G), ldg, galpha, _p(dS), B, Ns, No, D, _dt(d["own"]), _stream()),
                     "gf_dual_softmax_bwd")
            _guards_intact(bs)
            assert torch.isfinite(dS).all(), "dS is not finite: an element was not written, or G was read outside its core"
            w.add(f"{kind}/ldg{'+%d' % (ldg - No) if ldg else '0'}", dS, ref["dS"], ref["bound"])
    w.finish()


# =============================================================================================== gf_filter_matches
def test_filter_matches():
    """Hand-built arg-max vectors (assignment_cases.filter_case): matches exact, scores within the bound, against a few torch
    lines and against oracle.lightglue_oracle.filter_matches on the materialised matrix."""
    from oracle.lightglue_oracle import filter_matches
    arg0, arg1, max0, la = C.filter_case()
    B, M = arg0.shape
    N = arg1.shape[1]
    lib = L_.load()
    d0, d1, dm = arg0.to(DEV), arg1.to(DEV), max0.to(DEV)
    w = _Worst("gf_filter_matches")
    for th in (0.0, 0.1):
        rm0, rm1, rs0, rs1, b0, b1 = C.ref_filter(arg0, arg1, max0, th)
        om0, om1, _, _ = filter_matches(la, th)
        bm0, m0 = _guarded((B, M), torch.int64, int(SENTINEL))
        bm1, m1 = _guarded((B, N), torch.int64, int(SENTINEL))
        bs0, s0 = _guarded((B, M), torch.float32, math.nan)
        bs1, s1 = _guarded((B, N), torch.float32, math.nan)
        L_.check(lib.gf_filter_matches(_p(dm), _p(d0), _p(d1), th, _p(m0), _p(m1), _p(s0), _p(s1), B, M, N, _stream()),
                 "gf_filter_matches")
        _guards_intact(bm0, bm1, bs0, bs1)
        assert torch.equal(m0.cpu(), rm0) and torch.equal(m1.cpu(), rm1), f"th = {th}: matches"
        assert torch.equal(m0.cpu(), om0) and torch.equal(m1.cpu(), om1), f"th = {th}: matches (oracle)"
        w.add(f"s0/th{th:g}", s0, rs0, b0 + 1e-45)
        w.add(f"s1/th{th:g}", s1, rs1, b1 + 1e-45)
    w.finish()


# =============================================================================================== rejections
def test_rejected_calls_write_nothing():
    """B, M or N <= 0 -> GF_ERR_SHAPE; D in {32, 96, 512} -> GF_ERR_UNSUPPORTED; an unknown dtype -> GF_ERR_DTYPE; a null bias_z /
    rowmax of gf_rows_lse_argmax -> GF_ERR_SHAPE.  No kernel runs on these: every output keeps its fill."""
    cfg = C.CONFIGS[3]
    B, No, Ns, D = cfg
    case, d = _on_device("rand", cfg, torch.float32)
    lib = L_.load()
    st = _stream()
    f = {k: _guarded((B, max(No, Ns) + 1, max(No, Ns) + 1), torch.float32, SENTINEL) for k in ("f0", "f1", "out")}
    i = {k: _guarded((B, max(No, Ns)), torch.int64, int(SENTINEL)) for k in ("i0", "i1")}
    bufs = [v[0] for v in list(f.values()) + list(i.values())]
    own, oth, sb, z, nrm = (_p(d[k]) for k in ("own", "oth", "sbias", "z", "nrm"))
    f0, f1, out, i0, i1 = (_p(v[1]) for v in list(f.values()) + list(i.values()))
    G = C.padded_G(case, No + 1, 0.0).to(DEV)

    def entries(B_, M_, N_, D_, dt):
        """Every entry with the given sizes: (lse / arg-max: a = own, M = No; split kernels: a = oth, M = Ns)."""
        yield "gf_rows_lse", lib.gf_rows_lse(own, oth, sb, f0, B_, M_, N_, D_, dt, st)
        yield "gf_rows_argmax", lib.gf_rows_argmax(own, oth, sb, 2.0, f0, i0, B_, M_, N_, D_, dt, st)
        yield "gf_rows_lse_argmax", lib.gf_rows_lse_argmax(own, oth, z, nrm, 2.0, f1, f0, i0, B_, M_, N_, D_, dt, st)
        yield "gf_assign_write", lib.gf_assign_write(oth, own, sb, _p(d["obias"]), _p(d["bin_s"]), _p(d["bin_o"]), 2.0, 0.0, out, f0,
                                                     B_, N_, M_, D_, dt, st)
        yield "gf_dual_softmax_bwd", lib.gf_dual_softmax_bwd(oth, own, _p(d["r32"]), _p(d["c32"]), _p(d["gr"]), _p(d["gc"]), _p(G),
                                                             No + 1, 1.0, out, B_, N_, M_, D_, dt, st)

    for sizes in ((0, No, Ns), (B, 0, Ns), (B, No, 0), (-1, No, Ns), (B, -3, Ns), (B, No, -1)):
        for name, code in entries(*sizes, D, 0):
            assert code == GF_ERR_SHAPE, (name, sizes, code)
        assert lib.gf_filter_matches(f0, i0, i1, 0.0, i0, i1, f0, f1, *sizes, st) == GF_ERR_SHAPE
    for D_ in (32, 96, 512):
        for dt in (0, 1):
            for name, code in entries(B, No, Ns, D_, dt):
                assert code == GF_ERR_UNSUPPORTED, (name, D_, code)
    for name, code in entries(B, No, Ns, D, 7):
        assert code == GF_ERR_DTYPE, (name, code)
    for bz, bn, rm, ra in ((None, nrm, f0, i0), (z, None, f0, i0), (z, nrm, None, i0), (z, nrm, f0, None)):
        assert lib.gf_rows_lse_argmax(own, oth, bz, bn, 2.0, f1, rm, ra, B, No, Ns, D, 0, st) == GF_ERR_SHAPE
    torch.cuda.synchronize()
    for buf in bufs:
        assert (buf == SENTINEL).all(), "an output was written by a rejected call"


# =============================================================================================== op level
def _scaled_close(name, x, ref, dtype):
    sc = max(float(ref.abs().max()), 1e-2)
    torch.testing.assert_close(x.detach().cpu().double() / sc, ref / sc, msg=lambda m: f"{name}: {m}", **_tols(dtype))


@pytest.mark.parametrize("dtype,D", [(torch.float32, 64), (torch.bfloat16, 128), (torch.bfloat16, 256)],
                         ids=["fp32-dS-bgemm", "bf16-dS-bgemm", "bf16-fused"])
@pytest.mark.parametrize("B,N", [(3, 449), (2, 513)])
def test_dual_lse_stacked(B, N, dtype, D):
    """ops.dual_lse_stacked(md) == ops.dual_lse(md[:B], md[B:]) bit for bit, and its one stacked gradient == float64
    autograd of (r gr + c gc).sum(), through all three backward paths (N0 = N1 variants of the split shapes)."""
    g = torch.Generator().manual_seed(B * N + D)
    md = (torch.randn(2 * B, N, D, generator=g) * math.sqrt(1.5 / math.sqrt(D))).to(dtype)
    gr, gc = torch.randn(B, N, generator=g), torch.randn(B, N, generator=g)
    m64 = md.double().requires_grad_(True)
    S = m64[:B] @ m64[B:].transpose(1, 2)
    ((S.logsumexp(2) * gr.double()).sum() + (S.logsumexp(1) * gc.double()).sum()).backward()
    mds = md.to(DEV).requires_grad_(True)
    r, c = ops.dual_lse_stacked(mds)
    ((r * gr.to(DEV)).sum() + (c * gc.to(DEV)).sum()).backward()
    a, b = md[:B].to(DEV).requires_grad_(True), md[B:].to(DEV).requires_grad_(True)
    r2, c2 = ops.dual_lse(a, b)
    ((r2 * gr.to(DEV)).sum() + (c2 * gc.to(DEV)).sum()).backward()
    assert torch.equal(r, r2) and torch.equal(c, c2)
    assert mds.grad.dtype == dtype and mds.grad.shape == md.shape
    _scaled_close("stacked", mds.grad, m64.grad, dtype)
    _scaled_close("pair", torch.cat([a.grad, b.grad]), m64.grad, dtype)


@pytest.mark.parametrize("corner_shape", [(), (2,)], ids=["corner0d", "cornerB"])
@dtypes
def test_assign_write_backward_with_tensor_corner(dtype, corner_shape):
    """ops.assign_write with a differentiable corner (SuperGlue's bin score) and a dense upstream gradient: the matrix and the
    gradients of a, b, the four bias / bin vectors and the corner against float64 autograd."""
    B, M, N, D, alpha = 2, 65, 130, 64, 1.0
    g = torch.Generator().manual_seed(5)
    s = math.sqrt(1.5 / math.sqrt(D))
    a, b = (torch.randn(B, M, D, generator=g) * s).to(dtype), (torch.randn(B, N, D, generator=g) * s).to(dtype)
    vec = [torch.randn(B, n, generator=g) for n in (M, N, M, N)]
    corner = torch.randn(corner_shape, generator=g)
    G = torch.randn(B, M + 1, N + 1, generator=g)
    leaves = [t.double().requires_grad_(True) for t in [a, b] + vec + [corner]]
    a6, b6, rb, cb, bc, br, co = leaves
    core = alpha * a6 @ b6.transpose(1, 2) + rb[:, :, None] + cb[:, None, :]
    top = torch.cat([core, bc[:, :, None]], 2)
    bottom = torch.cat([br, co.expand(B)[:, None]], 1)[:, None, :]
    ref = torch.cat([top, bottom], 1)
    (ref * G.double()).sum().backward()
    dl = [t.to(DEV).requires_grad_(True) for t in [a, b] + vec + [corner]]
    out = ops.assign_write(*dl[:6], alpha=alpha, corner=dl[6])
    (out * G.to(DEV)).sum().backward()
    T = alpha * (a.double().abs() @ b.double().abs().transpose(1, 2)) + vec[0].double().abs()[:, :, None] + vec[1].double().abs()[:, None, :]
    w = _Worst(f"ops.assign_write backward {str(dtype)[6:]} corner{list(corner_shape)}")
    w.add("core", out[:, :M, :N], ref.detach()[:, :M, :N], C.C_ACC * T + C.FLOOR)
    assert torch.equal(out.detach().cpu()[:, :M, N], vec[2]) and torch.equal(out.detach().cpu()[:, M, :N], vec[3])
    assert torch.equal(out.detach().cpu()[:, M, N], corner.expand(B))
    Ga = G.double().abs()
    sums = {2: Ga[:, :M, :N].sum(2), 3: Ga[:, :M, :N].sum(1)}              # fp32 sums of the core gradient: error ~ U per addend
    for k, name in ((2, "rowbias"), (3, "colbias")):
        w.add(name, dl[k].grad, leaves[k].grad, C.C_ACC * sums[k] + C.FLOOR)
    for k, name in ((4, "bin_col"), (5, "bin_row")):
        assert torch.equal(dl[k].grad.cpu().double(), leaves[k].grad), name
    w.add("corner", dl[6].grad, leaves[6].grad, C.C_ACC * (Ga[:, M, N] if corner_shape else Ga[:, M, N].sum()) + C.FLOOR)
    w.finish()
    _scaled_close("da", dl[0].grad, leaves[0].grad, dtype)
    _scaled_close("db", dl[1].grad, leaves[1].grad, dtype)


@dtypes
def test_strided_a_equals_its_contiguous_copy(dtype):
    """A non-contiguous `a` (every other row of a larger tensor) gives bit for bit what its contiguous copy gives."""
    cfg = C.CONFIGS[3]
    case, d = _on_device("planted", cfg, dtype)
    wide = torch.zeros(cfg[0], 2 * cfg[1], cfg[3], dtype=dtype, device=DEV)
    wide[:, ::2] = d["own"]
    view = wide[:, ::2]
    assert not view.is_contiguous() and torch.equal(view, d["own"])
    assert torch.equal(ops.rows_lse(view, d["oth"]), ops.rows_lse(d["own"], d["oth"]))
    for x, y in zip(ops.rows_argmax(view, d["oth"], d["sbias"], 2.0), ops.rows_argmax(d["own"], d["oth"], d["sbias"], 2.0)):
        assert torch.equal(x, y)
    args = (d["oth"], d["obias"], d["sbias"], d["bin_o"], d["bin_s"])
    assert torch.equal(ops.assign_write(view, *args), ops.assign_write(d["own"], *args))
    r1, c1 = ops.dual_lse(view, d["oth"])
    r2, c2 = ops.dual_lse(d["own"], d["oth"])
    assert torch.equal(r1, r2) and torch.equal(c1, c2)
