"""The GEMM kernels on their own, straight through the C ABI of include/gf_amd.h: the streamed-activation kernel
(csrc/gemm_st.hip) and the register-resident kernel (csrc/gemm_ws.hip) behind gf_gemm / gf_gemm_res2, and gf_bgemm
(csrc/bgemm.hip), against float64 references.

Cases, references and bounds come from tests/gemm_cases.py (derivations in its docstring; held on the CPU by
tests/test_gemm_cases_reference.py, which also proves that the shape tables reach every tile count per workgroup of every
gemm_st instance); nothing measured here enters a bound.  `exact` / `coded` cases must EQUAL the float64 result rounded once
to the output type, `rand` / `cancel` cases must lie inside the entry-by-entry bound.  Every output is a column slice of a
wider NaN-filled buffer with one more row below it: an element never written shows as NaN inside, a stray store as a number
outside.  Every test prints its worst error / bound ratio.

Measured on the MI355X (worst error / bound over all cases of a kernel; zero bit mismatches on every exact case, streamed vs
reference and streamed vs register-resident; the whole file runs in under 4 s):
  gemm_st   K = 256: 0.993 (plain 0.990, one residual 0.993, two 0.991, rotary 0.988; the register-resident kernel on the
            same rows gives the same figures); K = 512: 0.980 (0.972 / 0.980 / 0.979,
            rotary 0.968); the two-source instances give the figures of their one-source twins (same values, same sums)
  gemm_ws   bf16 0.999 (K = 32) ... 0.972 (K = 512), rotary the same, with a residual the same; fp32 0.142 (K = 32, no
            residual) ... 0.018 (K = 256), rotary 0.134 ... 0.019; two sources bf16 0.999, fp32 0.102; K = 768 in pieces 0.984 / 0.015
  bgemm     bf16 0.997, fp32 0.126, the same in all nine layouts
(a bf16 figure just under 1 is a result that sits next to a rounding tie: the bound is half an ulp plus the fp32 sum's error)."""
import ctypes

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from glue_factory_amd import lib as L_
    from glue_factory_amd import ops
    from glue_factory_amd.ops import _p, _stream

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
SENTINEL = -776.0        # exact in bf16


def _code(dtype):
    return G.GF_BF16 if dtype == BF16 else G.GF_F32


class _Worst:
    """Collects error / bound ratios and exact mismatches, prints them and fails if a ratio exceeds 1 or a bit differs."""

    def __init__(self, what):
        self.what, self.worst, self.bad, self.n = what, {}, [], 0

    def check(self, tag, case, y, ref):
        self.n += 1
        if case["kind"] in G.EXACT_KINDS:
            wrong = y.double() != ref["rounded"]          # (NaN != anything: an unwritten element counts)
            if wrong.any():
                m, n = (int(v) for v in wrong.nonzero()[0])
                self.bad.append(f"{tag} {case['kind']} M={case['M']} N={case['N']} K={case['K0']}+{case['K1']}: {int(wrong.sum())} "
                                f"entries differ, first y[{m},{n}] = {float(y[m, n])} for {float(ref['rounded'][m, n])}")
        else:
            r = G.ratio(y, ref["y"], ref["y_bound"])
            self.worst[tag] = max(self.worst.get(tag, 0.0), r)

    def finish(self):
        print(f"{self.what}: {self.n} outputs, worst error/bound " + ", ".join(f"{k} {v:.3g}" for k, v in self.worst.items())
              + f", {len(self.bad)} exact cases with a mismatch")
        over = {k: v for k, v in self.worst.items() if not v <= 1.0}
        assert not over and not self.bad, f"{self.what}: over the bound {over}; exact mismatches: {self.bad[:6]}"


def _wide(t, pad, fill=0.0, extra_rows=0):
    """A copy of t [M, N] as a column slice (16-byte aligned offset) of a buffer `pad` elements wider, filled with `fill`."""
    M, N = t.shape
    buf = torch.full((M + extra_rows, N + pad), fill, dtype=t.dtype, device=t.device)
    v = buf[:M, pad // 2:pad // 2 + N]
    v.copy_(t)
    return buf, v


def _out(M, N, dtype):
    """(buffer, view): the [M, N] output as a column slice of a NaN-filled buffer 128 wider, one sentinel row below."""
    buf = torch.full((M + 1, N + 128), NAN, dtype=dtype, device=DEV)
    return buf, buf[:M, 64:64 + N]


def _outside_untouched(buf, M, N):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:M, 64:64 + N] = False
    assert torch.isnan(buf[mask]).all(), "a store landed outside the M x N block of y"


def _gemm(case, y, M=None, **over):
    """gf_gemm, or gf_gemm_res2 when the case has a second residual; `over` replaces operands by other views of the same values."""
    t = {k: over.get(k, case[k]) for k in ("x0", "x1", "w", "bias", "res", "res_b", "cs")}
    M = case["M"] if M is None else M
    ld = lambda v: 0 if v is None else v.stride(0)                    # noqa: E731
    lib = L_.load()
    if t["res_b"] is not None:
        return lib.gf_gemm_res2(_p(t["x0"]), _p(t["x1"]), _p(t["w"]), _p(t["bias"]), _p(t["res"]), _p(t["res_b"]), _p(y), M,
                                case["N"], case["K0"], case["K1"], ld(t["x0"]), ld(t["x1"]), ld(t["w"]), ld(t["res"]),
                                ld(t["res_b"]), ld(y), _code(case["dtype"]), _stream())
    return lib.gf_gemm(_p(t["x0"]), _p(t["x1"]), _p(t["w"]), _p(t["bias"]), _p(t["res"]), _p(y), _p(t["cs"]), case["rot_n"], M,
                       case["N"], case["K0"], case["K1"], ld(t["x0"]), ld(t["x1"]), ld(t["w"]), ld(t["res"]), ld(y),
                       _code(case["dtype"]), _stream())


def _ok(code, what="gf_gemm"):
    assert code == 0, f"{what} returned {code}" + (" (a hipError_t: the launch was refused)" if code > 0 else "")


def _plan(case, M=None):
    out = (ctypes.c_int64 * 11)()
    return L_.load().gf_gemm_plan(case["M"] if M is None else M, case["N"], case["K0"], case["K1"], int(case["nres"] >= 1),
                                  int(case["nres"] == 2), int(case["rot_n"] > 0), case["rot_n"], _code(case["dtype"]), out)


def _run_sliced(case, w=None, tag=None, ref=None):
    """The call with every operand a slice of a wider buffer of its own and y inside a NaN-filled buffer: every row stride
    differs from ldy (asserted), ld0 from ld1 and ldr from ldr_b, and so do the slices' column offsets (y: 64; 16 / 32 / 48 /
    80 / 24).  Returns y (checked against `ref` when a collector is given)."""
    M, N = case["M"], case["N"]
    buf, y = _out(M, N, case["dtype"])
    over = {}
    for k, pad in (("x0", 32), ("x1", 64), ("res", 96), ("res_b", 160), ("w", 48)):
        if case[k] is not None:
            if case[k].shape[1] + pad == y.stride(0):     # (a K that happens to give x or w the row stride of y)
                pad += 256
            over[k] = _wide(case[k], pad)[1]
            assert over[k].stride(0) != y.stride(0), k
    if case["res_b"] is not None:
        assert over["res"].stride(0) != over["res_b"].stride(0)
    _ok(_gemm(case, y, **over))
    _outside_untouched(buf, M, N)
    if w is not None:
        w.check(tag, case, y, ref)
    return y


def _one_more_row(case):
    """The same rows with one more row appended to every operand: M + 1 is no multiple of 64, so gf_gemm takes the
    register-resident kernel.  Two residuals are added beforehand (that kernel has one residual input)."""
    pad = lambda t: None if t is None else torch.cat((t, torch.zeros_like(t[:1])))          # noqa: E731
    c = dict(case, M=case["M"] + 1, **{k: pad(case[k]) for k in ("x0", "x1", "res", "cs")})
    if case["res_b"] is not None:
        c.update(res=pad(case["res"] + case["res_b"]), res_b=None, nres=1)
    return c


def _nan_containment(case, m, m2, n2):
    """One NaN in row m of x0 and one in res[m2, n2]: NaN in row m, in y[m2, n2] (and its pair partner where rotated), nowhere else."""
    M, N = case["M"], case["N"]
    x0 = case["x0"].clone()
    x0[m, 3] = NAN
    over = dict(x0=x0)
    want = torch.zeros(M, N, dtype=torch.bool, device=DEV)
    want[m] = True
    if case["res"] is not None:
        res = case["res"].clone()
        res[m2, n2] = NAN
        over["res"] = res
        want[m2, n2] = True
        if n2 < case["rot_n"]:
            want[m2, n2 ^ 1] = True
    buf, y = _out(M, N, case["dtype"])
    _ok(_gemm(case, y, **over))
    _outside_untouched(buf, M, N)
    got = torch.isnan(y)
    assert torch.equal(got, want), f"NaN containment: {int((got & ~want).sum())} entries poisoned, {int((want & ~got).sum())} clean " \
                                   f"that should not be (M={M} N={N} K={case['K0']}+{case['K1']})"


# ================================================================================================ gemm_st
def _st_id(inst):
    K, two, nres, rot = inst
    return f"K{K}{'-two' if two else ''}-res{nres}{'-rot' if rot else ''}"


@pytest.mark.parametrize("inst", G.ST_INSTANCES, ids=_st_id)
def test_gemm_streamed_instance(inst):
    """One template instance of gemm_st at every tile count per workgroup of gemm_cases.ST_M (a smallest launch, one tile
    everywhere, ragged {2,1}, {3,2}, {4,3}) and the narrow grids of ST_NARROW, `exact` (bit-equal) and `rand` (inside the
    bound); the same rows through the register-resident kernel (bit-equal on `exact`, within one bf16 ulp of the reference's
    magnitude on `rand`: two summation orders, each rounded once; with two residuals that kernel, which has one residual
    input, gets their bf16 sum and the distance allowed on `rand` grows by that pre-add's known rounding error); at the ragged {2,1} shape also `coded` and `cancel`, y aliasing res, every operand a slice of a wider
    buffer with its own row stride, no bias, and NaN containment.
    Measured on the MI355X: worst error / bound 0.963 ... 0.993 per instance and variant, streamed and register-resident
    alike; no exact case differs in a bit."""
    K, two, nres, rot = inst
    K0, K1 = (K // 2, K // 2) if two else (K, 0)
    w = _Worst(f"gemm_st {_st_id(inst)}")
    shapes = [(M, G.ST_N, G.ST_N if rot else 0) for M, _ in G.ST_M[K]]
    shapes += [(M, N, N - N % 256 if rot else 0) for M, N, _ in G.ST_NARROW[K]]
    if rot:
        shapes.append((G.ST_RAGGED_M[K], 2304, 2048))
    for M, N, rot_n in shapes:
        ragged = M == G.ST_RAGGED_M[K]
        kinds = ("exact", "rand") + (("coded",) + (("cancel",) if nres else ()) if ragged else ())
        for kind in kinds:
            case = G.gemm_case(kind, M, N, K0, K1, nres, rot_n, BF16, DEV)
            assert _plan(case) == 1, "the table's shape is not served by the streamed kernel"
            ref = G.gemm_ref(case)
            buf, y = _out(M, N, BF16)
            _ok(_gemm(case, y))
            _outside_untouched(buf, M, N)
            w.check("streamed", case, y, ref)
            # ---- the register-resident kernel on the same rows
            c1 = _one_more_row(case)
            assert _plan(c1) == 0
            buf1, y1 = _out(M + 1, N, BF16)
            _ok(_gemm(c1, y1))
            _outside_untouched(buf1, M + 1, N)
            if kind in G.EXACT_KINDS:
                assert torch.equal(y1[:M], y), f"streamed and register-resident differ on {kind} at M={M} N={N}"
            elif nres < 2:
                w.check("resident", case, y1[:M], ref)
                a = ref["y"].abs() + ref["y_bound"]                # 2^top = a / mantissa(a), an exact quotient (ldexp on the
                ulp = 2 * G.BF * a / torch.frexp(a).mantissa       # device goes through pow and may come out an ulp short)
                d = (y1[:M].double() - y.double()).abs()
                assert (d <= ulp).all(), f"streamed vs register-resident: {float((d / ulp).max()):.9g} bf16 ulps apart at M={M} N={N}"
            else:
                # two residuals: the register-resident kernel gets res + res_b as ONE bf16 operand.  Its own reference ref1 is
                # the sum with that stored operand, off ref by the pre-add's rounding error delta (known entry by entry);
                # each kernel lies within its bound of its reference, so the two are at most |delta| + bound + bound1 apart
                # (both bounds are half a bf16 ulp plus the fp32 sum's error: "one ulp, two summation orders" moved by delta)
                ref1 = {k: v[:M] for k, v in G.gemm_ref(c1).items()}
                w.check("resident", case, y1[:M], ref1)
                lim = (ref1["y"] - ref["y"]).abs() + ref["y_bound"] + ref1["y_bound"]
                d = (y1[:M].double() - y.double()).abs()
                assert (d <= lim).all(), f"streamed vs register-resident, two residuals: {float((d / lim).max()):.6g} of the limit at M={M} N={N}"
            if not ragged or N != G.ST_N:
                continue
            # ---- variants at the ragged shape
            _run_sliced(case, w, "sliced", ref)
            if nres:
                ya = case["res"].clone()
                _ok(_gemm(case, ya, res=ya))
                w.check("aliased", case, ya, ref)
            nb = G.gemm_case(kind, M, N, K0, K1, nres, rot_n, BF16, DEV, False)
            assert nb["bias"] is None
            buf, y = _out(M, N, BF16)
            _ok(_gemm(nb, y))
            _outside_untouched(buf, M, N)
            w.check("no bias", nb, y, G.gemm_ref(nb))
            if kind == "rand":
                tr, gx = G.st_plan(M, N, K)[:2]
                _nan_containment(case, tr * gx + tr // 2 + 5, 7, 1030)      # the second tile of workgroup 0; a row of tile 0
    w.finish()


# ================================================================================================ gemm_ws
def _ws_params():
    return [pytest.param(dt, K, id=f"{str(dt)[6:]}-K{K}") for dt in (BF16, F32) for K in G.WS_K[dt]]


@pytest.mark.parametrize("dtype,K", _ws_params())
def test_gemm_resident_shapes(dtype, K):
    """gemm_ws at K x every N of WS_N (odd tile counts, a partial last weight slice) x every M of WS_M (around the
    workgroup block), bias, without and with a residual, all operands sliced; `exact` bit-equal, `rand` inside the bound (fp32: the fp32
    bound, at the 1e-5 level the older test demands -- asserted below), `cancel` and `coded` at one M per N; NaN containment.
    Measured on the MI355X: worst error / bound bf16 0.999 / 0.998 / 0.996 / 0.989 / 0.972 at K = 32 ... 512, fp32 0.142 / 0.077 /
    0.043 / 0.018 at K = 32 ... 256."""
    w = _Worst(f"gemm_ws {str(dtype)[6:]} K={K}")
    for i, N in enumerate(G.WS_N):
        for j, M in enumerate(G.WS_M):
            for kind in ("exact", "rand") + (("cancel", "coded") if j == (i + 1) % len(G.WS_M) else ()):
                for nres in (0, 1) if kind in ("exact", "rand") and j % 2 == 0 else (1,):
                    case = G.gemm_case(kind, M, N, K, 0, nres, 0, dtype, DEV)
                    assert _plan(case) == 0
                    ref = G.gemm_ref(case)
                    y = _run_sliced(case, w, f"nres{nres}", ref)
                    if dtype == F32 and kind == "rand":
                        torch.testing.assert_close(y.double(), ref["y"], rtol=1e-5, atol=1e-5)
        if N >= 96:
            case = G.gemm_case("rand", 257, N, K, 0, 1, 0, dtype, DEV)
            _nan_containment(case, 200, 256, N - 31)
    w.finish()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_gemm_resident_two_sources(dtype):
    """TWO at every K0 = K1 the dispatch takes (16 ... 256; fp32 ... 128), 0 and 1 residual."""
    w = _Worst(f"gemm_ws two sources {str(dtype)[6:]}")
    for K0 in G.WS_TWO_K0[dtype]:
        for M, N in ((257, 96), (33, 288)):
            for kind in ("exact", "rand", "coded"):
                for nres in (0, 1):
                    case = G.gemm_case(kind, M, N, K0, K0, nres, 0, dtype, DEV)
                    assert _plan(case) == 0
                    _run_sliced(case, w, f"K0={K0}", G.gemm_ref(case))
    w.finish()


@pytest.mark.parametrize("dtype,K", _ws_params())
def test_gemm_resident_rotary(dtype, K):
    """The rotary epilogue of gemm_ws at rot_n in {64, N} and N - rot_n = 32, without and WITH a residual (the rotation acts
    on the sum including it: the K-piece plan of ops.gemm relies on that), NaN containment with the pair partner."""
    w = _Worst(f"gemm_ws rotary {str(dtype)[6:]} K={K}")
    for N, M in ((96, 257), (128, 33), (160, 255), (288, 531), (768, 257)):
        for rot_n in G.ws_rot_ns(N):
            for nres in (0, 1):
                for kind in ("exact", "rand", "coded") + (("cancel",) if nres else ()):
                    case = G.gemm_case(kind, M, N, K, 0, nres, rot_n, dtype, DEV)
                    assert _plan(case) == 0
                    _run_sliced(case, w, f"rot{'+res' if nres else ''}", G.gemm_ref(case))
            case = G.gemm_case("rand", M, N, K, 0, 1, rot_n, dtype, DEV)
            _nan_containment(case, M // 2, M - 1, rot_n - 2)
            if rot_n < N:
                _nan_containment(case, 0, M - 1, rot_n)             # the first channel that is not rotated: no partner
    w.finish()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_gemm_k_pieces_rotate_after_the_residual(dtype):
    """ops.gemm at K = 768 with a residual and the rotary table: pieces 512 + 256 (fp32 256 x 3) accumulate through the
    residual input, the rotation rides on the last piece.  The stored intermediate is the result of the same call over the
    first 512 columns; the last piece is then one gf_gemm with that residual, held to its reference entry by entry."""
    w = _Worst(f"ops.gemm K=768 rotary {str(dtype)[6:]}")
    M, N, rot_n = 257, 128, 64
    for kind in ("exact", "rand"):
        a = G.gemm_case(kind, M, N, 512, 0, 1, 0, dtype, DEV)                   # columns [0, 512), bias, residual
        b = G.gemm_case(kind, M, N, 256, 0, 0, rot_n, dtype, DEV, False)        # columns [512, 768), the table
        x, wt = torch.cat((a["x0"], b["x0"]), 1), torch.cat((a["w"], b["w"]), 1)
        y = ops.gemm(x, wt, a["bias"], res2=a["res"], cs=b["cs"], rot_n=rot_n)
        mid = ops.gemm(a["x0"], a["w"], a["bias"], res2=a["res"])
        if dtype == BF16:                                                       # one piece: held to its own reference too
            w.check("first piece", a, mid, G.gemm_ref(a))
        last = dict(b, res=mid, nres=1)
        w.check("rotated", last, y, G.gemm_ref(last))
    w.finish()


def test_gemm_rejections_leave_the_output_alone():
    """Every refused call returns its code, writes nothing, and gf_gemm_plan answers the same for the same arguments."""
    lib = L_.load()
    M, N, K = 64, 256, 256
    x = torch.randn(M, K + 8, device=DEV).to(BF16)
    wt = torch.randn(N, K, device=DEV).to(BF16)
    res = torch.randn(M, N, device=DEV).to(BF16)
    cs = torch.ones(M, 64, device=DEV)
    y = torch.full((M, N), SENTINEL, dtype=BF16, device=DEV)
    out = (ctypes.c_int64 * 11)()

    def gemm(M=M, N=N, K0=K, K1=0, ld0=K + 8, cs_=None, rot_n=0, dt=G.GF_BF16, x1=None):
        return lib.gf_gemm(_p(x), _p(x1), _p(wt), None, _p(res), _p(y), _p(cs_), rot_n, M, N, K0, K1, ld0, ld0, K, N, N, dt, _stream())

    def plan(M=M, N=N, K0=K, K1=0, has_cs=0, rot_n=0, dt=G.GF_BF16, res_b=0):
        return lib.gf_gemm_plan(M, N, K0, K1, 1, res_b, has_cs, rot_n, dt, out)

    assert gemm(N=40) == plan(N=40) == G.GF_ERR_UNSUPPORTED                                    # N % 32
    assert gemm(K0=128, K1=64, x1=x) == plan(K0=128, K1=64) == G.GF_ERR_UNSUPPORTED            # K1 != K0
    assert gemm(K0=128, K1=128) == G.GF_ERR_UNSUPPORTED                                        # two sources, no x1
    assert gemm(ld0=K + 4) == G.GF_ERR_ALIGN                                                   # rows 8 bytes off
    assert gemm(cs_=cs, rot_n=32) == plan(has_cs=1, rot_n=32) == G.GF_ERR_SHAPE                # rot_n % 64
    assert gemm(cs_=cs, rot_n=320) == plan(has_cs=1, rot_n=320) == G.GF_ERR_SHAPE              # rot_n > N
    assert gemm(dt=7) == plan(dt=7) == G.GF_ERR_DTYPE
    assert gemm(K0=48) == plan(K0=48) == G.GF_ERR_UNSUPPORTED                                  # no instance for K = 48
    assert gemm(M=0) == plan(M=0) == G.GF_ERR_SHAPE

    def res2(M=M, N=N, res_b=res, dt=G.GF_BF16, ldr_b=N):
        return lib.gf_gemm_res2(_p(x), None, _p(wt), None, _p(res), _p(res_b), _p(y), M, N, K, 0, K + 8, 0, K, N, ldr_b, N, dt, _stream())

    assert res2(res_b=None) == G.GF_ERR_UNSUPPORTED                                            # no second residual
    assert res2(M=63) == plan(M=63, res_b=1) == G.GF_ERR_UNSUPPORTED and plan(M=63) == 0       # outside the streamed shapes:
    assert res2(N=128) == plan(N=128, res_b=1) == G.GF_ERR_UNSUPPORTED and plan(N=128) == 0    # gf_gemm's resident kernel
    assert res2(dt=G.GF_F32) == plan(dt=G.GF_F32, res_b=1) == G.GF_ERR_UNSUPPORTED
    assert res2(ldr_b=N + 4) == G.GF_ERR_ALIGN
    torch.cuda.synchronize()
    assert (y == SENTINEL).all(), "a refused call wrote to its output"
    assert plan() == 1 and plan(res_b=1) == 1                                                  # and the calls it would take


# ================================================================================================ bgemm
def _bg_shapes(dtype):
    """(batch, M, N, K): every M, N of BG_MN and every K of bg_ks occurs; batch 3 on every second entry."""
    ks = G.bg_ks(dtype)
    return [(3 if i % 2 else 1, G.BG_MN[i % 5], G.BG_MN[(i + 2) % 5], k) for i, k in enumerate(ks)]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("oa,ob", G.BG_ORIENT + G.BG_SCALAR, ids=lambda v: v)
def test_bgemm_orientations(oa, ob, dtype):
    """gf_bgemm: the four orientation instances and the scalar guarded-load paths (no unit stride, a slice that starts off a
    16-byte boundary) x M, N in {1, 127, 128, 129, 257} x K below, at and around one and two k-steps, batch 3 with sliced
    batch strides, alpha = 0.75, C a strided slice of a NaN-filled buffer (row-major and, on every second shape, transposed);
    `exact` bit-equal, `rand` inside the bound.  Measured on the MI355X: worst error / bound bf16 0.997, fp32 0.126 in every layout."""
    lib = L_.load()
    worst, bad = 0.0, []
    for i, (batch, M, N, K) in enumerate(_bg_shapes(dtype)):
        for kind in ("exact", "rand"):
            case = G.bgemm_case(kind, batch, M, N, K, oa, ob, dtype, DEV)
            ref = G.bgemm_ref(case)
            a, b = case["a"], case["b"]
            if i % 2:
                cbuf = torch.full((batch, N + 2, M + 5), NAN, dtype=dtype, device=DEV)
                c = cbuf[:, 1:1 + N, 2:2 + M].transpose(1, 2)
            else:
                cbuf = torch.full((batch, M + 2, N + 5), NAN, dtype=dtype, device=DEV)
                c = cbuf[:, 1:1 + M, 2:2 + N]
            _ok(lib.gf_bgemm(_p(a), _p(b), _p(c), batch, M, N, K, L_.strides(*a.stride()), L_.strides(*b.stride()),
                             L_.strides(*c.stride()), case["alpha"], _code(dtype), _stream()), "gf_bgemm")
            assert int(torch.isnan(cbuf).sum()) == cbuf.numel() - batch * M * N and not torch.isnan(c).any(), \
                f"gf_bgemm wrote outside C or left an entry unwritten ({batch}, {M}, {N}, {K})"
            if kind == "exact":
                wrong = int((c.double() != ref["rounded"]).sum())
                if wrong:
                    bad.append((batch, M, N, K, wrong))
            else:
                worst = max(worst, G.ratio(c, ref["c"], ref["c_bound"]))
    print(f"bgemm {oa}/{ob} {str(dtype)[6:]}: worst error/bound {worst:.3g}, exact mismatches {bad}")
    assert worst <= 1.0 and not bad, (worst, bad)
