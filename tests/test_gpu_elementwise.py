"""The per-layer streaming kernels on their own, through the C ABI of include/gf_amd.h: gf_rotary_qk / gf_rotary_qk_bwd,
gf_ln_gelu_fwd / gf_ln_gelu_bwd (csrc/elementwise.hip), gf_rowdot_* / gf_rowdot2_* (csrc/rowdot.hip) and gf_colsum_f32
(csrc/smallops.hip) against float64 references, then ops.ln_gelu / ops.rowdot / ops.rowdot2 against float64 autograd.

Cases, references and bounds come from tests/elementwise_cases.py (derivations in its docstring; held on the CPU by
tests/test_elementwise_cases_reference.py); nothing measured here enters a bound.  Shapes are the smallest at which each
dispatch path exists (the tables of elementwise_cases say which), in fp32 and bf16, on every value case.  Every output and
every buffer rewritten in place lies between GUARD sentinel elements that must survive; every pure output is pre-filled with
NaN, so an element that is never written shows; every call is made twice and must give the same bits.  Every test prints
its worst error / bound ratio.

Measured on the MI355X (worst error / bound over all cases of a kernel; the CPU test prints the emulation's figures):
  rotary        fp32: fwd / inv / dq 0.65, round trip 0.66, dtheta 0.29; bf16: the stored values 1.00 (a rounding tie), dtheta 0.20
  ln_gelu       fp32: y 0.51, mean 0.51, rstd 0.40, dx 0.43, dgamma 0.50, dbeta 0.48; bf16: y and dx 1.00, mean 0.51,
                rstd 0.41, dgamma 0.78, dbeta 0.47; past 8192 rows no figure above those
  outliers      normalised-value error over the fp32 parity budget, outlier_first / outlier_last: 0.0023 / 0.0015 at worst
                (fp32 C = 1024; bf16 at most 0.0027 / 0.0015).  With the single-pass variance this suite was first run
                against, outlier_first gave 0.21 (C = 256), 0.55 (C = 512) and 1.23 (C = 1024) in fp32, outlier_last 0.001.
  rowdot        z 0.11, dx 0.50 (fp32) / 1.00 (bf16), dw 0.46, db 0.31
  colsum        0.07
  dynamic LDS   gf_ln_gelu_bwd at bf16 C in (1024, 2048] asks for 65536 bytes without an opt-in: the launch is accepted."""
import functools
import math

import pytest
import torch

import elementwise_cases as E

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from glue_factory_amd import lib as L_
    from glue_factory_amd import ops
    from glue_factory_amd.ops import _dt, _p, _stream

DEV = "cuda"
GUARD = 64               # sentinel elements on either side of every output (a multiple of 16 bytes in both dtypes)
SENTINEL = -776.0        # exact in bf16
F32, BF16 = torch.float32, torch.bfloat16
dtypes = pytest.mark.parametrize("dtype", E.DTYPES, ids=["fp32", "bf16"])


def _tols(dtype):
    return dict(rtol=1e-4, atol=1e-4) if dtype == F32 else dict(rtol=5e-2, atol=5e-2)


class _Worst:
    """Collects error / bound ratios, prints the worst of each name and fails if one exceeds 1."""

    def __init__(self, what):
        self.what, self.worst, self.notes = what, {}, []

    def add(self, name, x, ref, bound):
        assert x.shape == ref.shape, (name, x.shape, ref.shape)
        self.worst[name] = max(self.worst.get(name, 0.0), E.ratio(x, ref, bound))

    def finish(self):
        print(f"{self.what}: worst error/bound " + ", ".join(f"{k} {v:.3g}" for k, v in self.worst.items()) + "".join(self.notes))
        bad = {k: v for k, v in self.worst.items() if not v <= 1.0}
        assert not bad, f"{self.what}: over the bound (error / bound): {bad}"


def _guarded(shape, dtype, fill):
    """(buffer, view): `view` of the given shape filled with `fill` (a number or a tensor to copy), GUARD sentinels around it."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    if torch.is_tensor(fill):
        view.copy_(fill)
    else:
        view.fill_(fill)
    return buf, view


def _guards_intact(*bufs):
    torch.cuda.synchronize()
    for buf in bufs:
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "a sentinel next to an output was written"


def _same_bits(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _ok(code, what):
    assert code == 0, f"{what} returned {code}" + (" (a hipError_t: the launch was refused)" if code > 0 else "")


def _name(dtype):
    return str(dtype)[6:]


@functools.lru_cache(maxsize=4)
def _dev(maker, *key):
    return E.to_device(maker(*key), DEV)


# ================================================================================================ rotary
def _rotary_fwd(w, tag, d, ref, lib):
    B, N, H, D, dt = d["B"], d["N"], d["H"], d["D"], d["dtype"]
    runs = []
    for _ in range(2):
        buf, q = _guarded((B, N, 3, H, D), dt, d["qkv"])
        _ok(lib.gf_rotary_qk(_p(q), _p(d["cs"]), B, N, H, D, 0, _dt(q), _stream()), "gf_rotary_qk")
        _guards_intact(buf)
        runs.append(buf)
    assert _same_bits(*runs), "gf_rotary_qk: two runs differ"
    assert _same_bits(q[:, :, 2].contiguous(), d["qkv"][:, :, 2].contiguous()), "the v third was touched by the forward"
    w.add(tag + "fwd", q[:, :, :2], ref["fwd"], ref["fwd_bound"])
    if d["kind"] == "quarter":
        assert torch.equal(q[:, :, :2].double(), ref["fwd"]), "theta = pi / 2 as exact (0, 1) is a signed permutation"
    _ok(lib.gf_rotary_qk(_p(q), _p(d["cs"]), B, N, H, D, 1, _dt(q), _stream()), "gf_rotary_qk inverse")     # back again
    _guards_intact(buf)
    w.add(tag + "roundtrip", q[:, :, :2], ref["rt"], ref["rt_bound"])
    assert _same_bits(q[:, :, 2].contiguous(), d["qkv"][:, :, 2].contiguous()), "the v third was touched by the inverse"
    buf, q = _guarded((B, N, 3, H, D), dt, d["qkv"])
    _ok(lib.gf_rotary_qk(_p(q), _p(d["cs"]), B, N, H, D, 1, _dt(q), _stream()), "gf_rotary_qk inverse")
    _guards_intact(buf)
    w.add(tag + "inv", q[:, :, :2], ref["inv"], ref["inv_bound"])


def _rotary_bwd(w, tag, d, ref, lib, modes=("null", "separate", "alias")):
    B, N, H, D, dt = d["B"], d["N"], d["H"], d["D"], d["dtype"]
    for mode in modes:
        runs = []
        for _ in range(2):
            bg, g = _guarded((B, N, 3, H, D), dt, d["grad"])
            bt, dth = _guarded((B, N, D // 2), F32, d["base"] if mode == "alias" else math.nan)
            base = {"null": None, "separate": d["base"], "alias": dth}[mode]
            _ok(lib.gf_rotary_qk_bwd(_p(g), _p(d["y"]), _p(d["cs"]), _p(dth), _p(base), B, N, H, D, _dt(g), _stream()),
                "gf_rotary_qk_bwd")
            _guards_intact(bg, bt)
            runs.append((bg, bt))
        assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1]), "gf_rotary_qk_bwd: two runs differ"
        assert _same_bits(g[:, :, 2].contiguous(), d["grad"][:, :, 2].contiguous()), "the v third was touched by the backward"
        w.add(tag + "dq", g[:, :, :2], ref["dq"], ref["dq_bound"])
        name = "dtheta" if mode == "null" else "dtheta_base"
        w.add(tag + name + ("/alias" if mode == "alias" else ""), dth, ref[name], ref[name + "_bound"])


@dtypes
@pytest.mark.parametrize("H,D", E.ROT_VEC + E.ROT_SCALAR + E.ROT_FWD_ONLY, ids=lambda v: str(v))
def test_rotary(H, D, dtype):
    """Forward, inverse, round trip and (where the backward takes the shape) the backward with dtheta_base NULL, separate and
    aliasing dtheta, on every token count and value case; the forward-only shapes must be rejected by the backward."""
    lib = L_.load()
    w = _Worst(f"rotary ({H},{D}) {_name(dtype)}")
    for B, N in E.ROT_TOKENS:
        for kind in E.ROT_KINDS:
            d = _dev(E.rotary_case, kind, B, N, H, D, dtype)
            ref = E.rotary_ref(d)
            _rotary_fwd(w, "", d, ref, lib)
            if (H, D) in E.ROT_FWD_ONLY:
                bg, g = _guarded((B, N, 3, H, D), dtype, d["grad"])
                bt, dth = _guarded((B, N, D // 2), F32, math.nan)
                assert lib.gf_rotary_qk_bwd(_p(g), _p(d["y"]), _p(d["cs"]), _p(dth), None, B, N, H, D, _dt(g),
                                            _stream()) == E.GF_ERR_UNSUPPORTED
                _guards_intact(bg, bt)
                assert _same_bits(g, d["grad"]) and torch.isnan(dth).all(), "a rejected backward wrote"
            else:
                _rotary_bwd(w, "", d, ref, lib)
    w.finish()


@dtypes
@pytest.mark.parametrize("H,D", E.ROT_BIG_HD, ids=lambda v: str(v))
def test_rotary_grid_stride(H, D, dtype):
    """2 * 32768 + 3 tokens: 8192 blocks of four waves take three rounds, the last one ragged."""
    B, N = E.ROT_BIG_TOKENS
    lib = L_.load()
    w = _Worst(f"rotary grid stride ({H},{D}) {_name(dtype)}")
    d = E.to_device(E.rotary_case.__wrapped__("rand", B, N, H, D, dtype), DEV)
    ref = E.rotary_ref(d)
    _rotary_fwd(w, "", d, ref, lib)
    _rotary_bwd(w, "", d, ref, lib, modes=("null", "alias"))
    w.finish()


def test_rotary_rejections():
    """B, N, H, D <= 0 or an odd D -> GF_ERR_SHAPE; an unknown dtype -> GF_ERR_DTYPE; nothing is written."""
    lib = L_.load()
    d = _dev(E.rotary_case, "rand", 1, 5, 3, 32, F32)
    B, N, H, D = 1, 5, 3, 32
    bq, q = _guarded((B, N, 3, H, D), F32, d["qkv"])
    bt, dth = _guarded((B, N, D // 2), F32, math.nan)
    st = _stream()
    for sizes in ((0, N, H, D), (B, 0, H, D), (B, N, 0, D), (B, N, H, 0), (-1, N, H, D), (B, N, H, 31), (B, N, H, -2)):
        assert lib.gf_rotary_qk(_p(q), _p(d["cs"]), *sizes, 0, 0, st) == E.GF_ERR_SHAPE, sizes
        assert lib.gf_rotary_qk_bwd(_p(q), _p(d["y"]), _p(d["cs"]), _p(dth), None, *sizes, 0, st) == E.GF_ERR_SHAPE, sizes
    assert lib.gf_rotary_qk(_p(q), _p(d["cs"]), B, N, H, D, 0, 7, st) == E.GF_ERR_DTYPE
    assert lib.gf_rotary_qk_bwd(_p(q), _p(d["y"]), _p(d["cs"]), _p(dth), None, B, N, H, D, 7, st) == E.GF_ERR_DTYPE
    _guards_intact(bq, bt)
    assert _same_bits(q, d["qkv"]) and torch.isnan(dth).all(), "a rejected call wrote"


# ================================================================================================ LN + GELU
def _ln_fwd(w, tag, d, ref, lib, parity=None):
    R, C, dt = d["R"], d["C"], d["dtype"]
    runs = []
    for _ in range(2):
        by, y = _guarded((R, C), dt, math.nan)
        bm, mean = _guarded((R,), F32, math.nan)
        br, rstd = _guarded((R,), F32, math.nan)
        _ok(lib.gf_ln_gelu_fwd(_p(d["x"]), _p(d["gamma"]), _p(d["beta"]), _p(y), _p(mean), _p(rstd), R, C, E.EPS, _dt(y),
                               _stream()), "gf_ln_gelu_fwd")
        _guards_intact(by, bm, br)
        runs.append((by, bm, br))
    assert all(_same_bits(a, b) for a, b in zip(*runs)), "gf_ln_gelu_fwd: two runs differ"
    for name, t in (("y", y), ("mean", mean), ("rstd", rstd)):
        w.add(tag + name, t, ref[name], ref[name + "_bound"])
    if parity is not None and d["kind"] in parity:
        parity[d["kind"]] = max(parity[d["kind"]], E.parity_ratio(d, ref, mean, rstd))


def _ln_bwd(w, tag, d, ref, lib):
    R, C, dt = d["R"], d["C"], d["dtype"]
    nblk = lib.gf_ln_gelu_nblk(R)
    assert nblk == E.ln_nblk(R)
    mean, rstd = ref["mean"].float(), ref["rstd"].float()
    runs = []
    for _ in range(2):
        bx, dx = _guarded((R, C), dt, math.nan)
        bg, dgp = _guarded((nblk, C), F32, math.nan)
        bb, dbp = _guarded((nblk, C), F32, math.nan)
        _ok(lib.gf_ln_gelu_bwd(_p(d["x"]), _p(d["gamma"]), _p(d["beta"]), _p(mean), _p(rstd), _p(d["dy"]), _p(dx), _p(dgp),
                               _p(dbp), R, C, _dt(dx), _stream()), "gf_ln_gelu_bwd")
        _guards_intact(bx, bg, bb)
        runs.append((bx, bg, bb))
    assert all(_same_bits(a, b) for a, b in zip(*runs)), "gf_ln_gelu_bwd: two runs differ"
    assert torch.isfinite(dgp).all() and torch.isfinite(dbp).all(), "a partial element was not written"
    w.add(tag + "dx", dx, ref["dx"], ref["dx_bound"])
    w.add(tag + "dgamma", dgp.double().sum(0), ref["dgamma"], ref["dgamma_bound"])
    w.add(tag + "dbeta", dbp.double().sum(0), ref["dbeta"], ref["dbeta_bound"])


def _ln_ids(dtype):
    return [(dtype, C) for C in E.LN_C[dtype]]


@pytest.mark.parametrize("dtype,C", _ln_ids(F32) + _ln_ids(BF16), ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_ln_gelu(dtype, C):
    """Forward (y, mean, rstd) and backward (dx, float64 column sums of the partials) on every row count and value case.  The two
    outlier cases are printed side by side against the fp32 parity budget (1e-4 of the row's largest normalised value), which
    the fp32 statistics must meet."""
    lib = L_.load()
    w = _Worst(f"ln_gelu C={C} {_name(dtype)}")
    parity = {"outlier_first": 0.0, "outlier_last": 0.0}
    for R in E.LN_ROWS:
        for kind in E.LN_KINDS:
            d = _dev(E.ln_case, kind, R, C, dtype)
            ref = E.ln_ref(d)
            _ln_fwd(w, "", d, ref, lib, parity)
            _ln_bwd(w, "", d, ref, lib)
    w.notes.append(f"; normalised-value error / parity budget: outlier_first {parity['outlier_first']:.3g}, "
                   f"outlier_last {parity['outlier_last']:.3g}")
    w.finish()
    if dtype == F32:
        assert max(parity.values()) <= 1.0, f"over the fp32 parity budget: {parity}"


def _scaled_close(name, x, ref, dtype):
    sc = max(float(ref.abs().max()), 1e-2)
    torch.testing.assert_close(x.detach().double() / sc, ref / sc, msg=lambda m: f"{name}: {m}", **_tols(dtype))


@pytest.mark.parametrize("R", E.LN_BIG_ROWS)
@pytest.mark.parametrize("dtype,C", [(dt, C) for dt in E.DTYPES for C in E.LN_BIG_C[dt]],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_ln_gelu_row_loop(dtype, C, R):
    """More than 8192 rows: the prefetch of the next row, the second and third iteration of the row loop and waves that stop
    at different iterations; then the same gradients through ops.ln_gelu on a non-contiguous x, whose dgamma / dbeta go through
    gf_colsum_f32 (2048 partial rows)."""
    lib = L_.load()
    w = _Worst(f"ln_gelu row loop R={R} C={C} {_name(dtype)}")
    d = E.to_device(E.ln_case.__wrapped__("rand", R, C, dtype), DEV)          # not kept in the cache of cases
    ref = E.ln_ref(d)
    ref = {k: ref[k] for k in ("y", "mean", "rstd", "dx", "dgamma", "dbeta") + tuple(
        k + "_bound" for k in ("y", "mean", "rstd", "dx", "dgamma", "dbeta"))}
    _ln_fwd(w, "", d, ref, lib)
    _ln_bwd(w, "", d, ref, lib)
    wide = torch.zeros(R, 2, C, dtype=dtype, device=DEV)
    wide[:, 0] = d["x"]
    xs = wide[:, 0].requires_grad_(True)
    assert not xs.is_contiguous()
    ga, be = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
    y = ops.ln_gelu(xs, ga, be, E.EPS)
    gx, gg, gb = torch.autograd.grad((y * d["dy"]).sum(), (xs, ga, be))
    w.add("ops/y", y, ref["y"], ref["y_bound"])
    w.finish()
    for name, t in (("dx", gx), ("dgamma", gg), ("dbeta", gb)):
        _scaled_close("ops.ln_gelu " + name, t, ref[name], dtype)


def test_ln_gelu_rejections():
    """C not a multiple of VEC or above 256 VEC -> GF_ERR_UNSUPPORTED; R, C <= 0 -> GF_ERR_SHAPE; an unknown dtype ->
    GF_ERR_DTYPE; every (guarded, pre-filled) output keeps its fill."""
    lib = L_.load()
    R, CM = 4, 2056
    st = _stream()
    for dtype in E.DTYPES:
        x = torch.randn(R, CM, device=DEV).to(dtype)
        ga, be, mean, rstd = (torch.randn(n, device=DEV) for n in (CM, CM, R, R))
        outs = [_guarded((R, CM), dtype, math.nan)] + [_guarded(s, F32, math.nan) for s in ((R,), (R,), (R, CM), (R, CM))]
        y, m, r, gp, bp = (_p(v) for _, v in outs)

        def both(R_, C_, dt):
            yield lib.gf_ln_gelu_fwd(_p(x), _p(ga), _p(be), y, m, r, R_, C_, E.EPS, dt, st)
            yield lib.gf_ln_gelu_bwd(_p(x), _p(ga), _p(be), _p(mean), _p(rstd), _p(x), y, gp, bp, R_, C_, dt, st)

        for C in E.LN_REJECT_UNSUPPORTED[dtype]:
            assert list(both(R, C, _dt(x))) == [E.GF_ERR_UNSUPPORTED] * 2, C
        for R_, C_ in ((0, 256), (-1, 256), (R, 0), (R, -8)):
            assert list(both(R_, C_, _dt(x))) == [E.GF_ERR_SHAPE] * 2, (R_, C_)
        assert list(both(R, 256, 7)) == [E.GF_ERR_DTYPE] * 2
        torch.cuda.synchronize()
        for buf, view in outs:
            assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all() and torch.isnan(view).all(), \
                "an output was written by a rejected call"
    for R_, nb in E.LN_NBLK:
        assert lib.gf_ln_gelu_nblk(R_) == nb


# ================================================================================================ row-dot
def _rd_fwd(w, tag, d, ref, lib):
    M, C = d["M"], d["C"]
    b0, b1 = float(d["b0"]), float(d["b1"])
    b0d, b1d = d["b0"].double(), d["b1"].double()
    nz = E.gam(4 * E.vec_of(d["dtype"]) + 9)
    variants = [("host", b0, None, ref["z0"], ref["z0_bound"]), ("dev", 0.0, d["b0"], ref["z0"], ref["z0_bound"]),
                ("both", b0, d["b1"], ref["z0_nobias"] + b0d + b1d, nz * (ref["T0"] + b0d.abs() + b1d.abs()) + E.FLOOR),
                ("none", 0.0, None, ref["z0_nobias"], ref["z0_nobias_bound"])]
    for name, bias, bias_dev, zref, zb in variants:
        runs = []
        for _ in range(2):
            bz, z = _guarded((M,), F32, math.nan)
            _ok(lib.gf_rowdot_fwd(_p(d["x"]), _p(d["w0"]), bias, _p(bias_dev), _p(z), M, C, _dt(d["x"]), _stream()), "gf_rowdot_fwd")
            _guards_intact(bz)
            runs.append(bz)
        assert _same_bits(*runs), "gf_rowdot_fwd: two runs differ"
        w.add(tag + "z/" + name, z, zref, zb)
    for name, pb0, pb1 in (("both", d["b0"], d["b1"]), ("b0null", None, d["b1"]), ("b1null", d["b0"], None)):
        runs = []
        for _ in range(2):
            bz0, z0 = _guarded((M,), F32, math.nan)
            bz1, z1 = _guarded((M,), F32, math.nan)
            _ok(lib.gf_rowdot2_fwd(_p(d["x"]), _p(d["w0"]), _p(d["w1"]), _p(pb0), _p(pb1), _p(z0), _p(z1), M, C, _dt(d["x"]),
                                   _stream()), "gf_rowdot2_fwd")
            _guards_intact(bz0, bz1)
            runs.append((bz0, bz1))
        assert all(_same_bits(a, b) for a, b in zip(*runs)), "gf_rowdot2_fwd: two runs differ"
        k0, k1 = ("z0_nobias" if pb0 is None else "z0"), ("z1_nobias" if pb1 is None else "z1")
        w.add(tag + "z0/two", z0, ref[k0], ref[k0 + "_bound"])
        w.add(tag + "z1/two", z1, ref[k1], ref[k1 + "_bound"])


def _rd_bwd(w, tag, d, ref, lib):
    M, C, dt = d["M"], d["C"], d["dtype"]
    nblk = lib.gf_rowdot_nblk(M)
    assert nblk == E.rd_nblk(M)
    for two in (False, True):
        for mode in ("nodx", "nobase", "separate", "alias"):
            runs = []
            for _ in range(2):
                bx, dx = _guarded((M, C), dt, d["base"] if mode == "alias" else math.nan)
                bp, part = _guarded((nblk, 2, C + 1) if two else (nblk, C + 1), F32, math.nan)
                pdx = None if mode == "nodx" else dx
                base = {"nodx": dx, "nobase": None, "separate": d["base"], "alias": dx}[mode]    # nodx: base must be ignored
                if two:
                    code = lib.gf_rowdot2_bwd(_p(d["x"]), _p(d["dz0"]), _p(d["dz1"]), _p(d["w0"]), _p(pdx), _p(base), _p(part),
                                              M, C, _dt(d["x"]), _stream())
                else:
                    code = lib.gf_rowdot_bwd(_p(d["x"]), _p(d["dz0"]), _p(d["w0"]), _p(pdx), _p(base), _p(part), M, C,
                                             _dt(d["x"]), _stream())
                _ok(code, "gf_rowdot2_bwd" if two else "gf_rowdot_bwd")
                _guards_intact(bx, bp)
                runs.append((bx, bp))
            assert _same_bits(runs[0][1], runs[1][1]), "rowdot backward: two runs differ (partials)"
            assert torch.isfinite(part).all(), "a partial element (the bias slot included) was not written"
            t = tag + ("two/" if two else "one/")
            if mode == "nodx":
                assert torch.isnan(dx).all(), "dx == NULL, but the stand-in buffer was written"
            else:
                assert _same_bits(runs[0][0], runs[1][0]), "rowdot backward: two runs differ (dx)"
                k = "dx_nobase" if mode == "nobase" else "dx"
                w.add(t + "dx/" + mode, dx, ref[k], ref[k + "_bound"])
            s = part.double().sum(0)
            heads = ((0, s[0]), (1, s[1])) if two else ((0, s),)
            for h, sh in heads:
                w.add(t + f"dw{h}", sh[:C], ref[f"dw{h}"], ref[f"dw{h}_bound"])
                w.add(t + f"db{h}", sh[C:], ref[f"db{h}"], ref[f"db{h}_bound"])


def _rd_ids(dtype):
    return [(dtype, C) for C in E.RD_C[dtype]]


@pytest.mark.parametrize("dtype,C", _rd_ids(F32) + _rd_ids(BF16), ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_rowdot(dtype, C):
    """Both forward entries with every bias combination and both backward entries with dx NULL, base NULL / separate / aliasing dx,
    on every row count and value case."""
    lib = L_.load()
    w = _Worst(f"rowdot C={C} {_name(dtype)}")
    for M in E.RD_ROWS:
        for kind in E.RD_KINDS:
            d = _dev(E.rd_case, kind, M, C, dtype)
            ref = E.rd_ref(d)
            _rd_fwd(w, "", d, ref, lib)
            _rd_bwd(w, "", d, ref, lib)
    w.finish()


@dtypes
def test_rowdot_grid_stride(dtype):
    """Forward with 2 * 16384 + 3 rows (4096 blocks of four waves, three rounds) at the smallest C, both entries; in fp32 also the
    backward sweep at cpr = 1 with 131072 + 259 rows (512 blocks of 256 rows, a ragged second round)."""
    lib = L_.load()
    C = E.RD_C[dtype][0]
    w = _Worst(f"rowdot grid stride C={C} {_name(dtype)}")
    d = E.to_device(E.rd_case("rand", E.RD_BIG_FWD, C, dtype), DEV)
    _rd_fwd(w, "", d, E.rd_ref(d), lib)
    if dtype == F32:
        d = E.to_device(E.rd_case("rand", E.RD_BIG_BWD, C, dtype), DEV)
        _rd_bwd(w, "big/", d, E.rd_ref(d), lib)
    w.finish()


def test_rowdot_rejections():
    """C not a multiple of VEC or above 256 VEC -> GF_ERR_UNSUPPORTED; M, C <= 0 -> GF_ERR_SHAPE; an unknown dtype -> GF_ERR_DTYPE."""
    lib = L_.load()
    M, CM = 4, 2056
    st = _stream()
    for dtype in E.DTYPES:
        x = torch.randn(M, CM, device=DEV).to(dtype)
        wv, dz, b = torch.randn(CM, device=DEV), torch.randn(M, device=DEV), torch.randn(1, device=DEV)
        outs = [_guarded((M, CM), dtype, math.nan)] + [_guarded(s, F32, math.nan) for s in ((M,), (M,), (1, 2, CM + 1))]
        dx, z0, z1, part = (_p(v) for _, v in outs)

        def every(M_, C_, dt):
            yield lib.gf_rowdot_fwd(_p(x), _p(wv), 0.5, _p(b), z0, M_, C_, dt, st)
            yield lib.gf_rowdot2_fwd(_p(x), _p(wv), _p(wv), _p(b), _p(b), z0, z1, M_, C_, dt, st)
            yield lib.gf_rowdot_bwd(_p(x), _p(dz), _p(wv), dx, None, part, M_, C_, dt, st)
            yield lib.gf_rowdot2_bwd(_p(x), _p(dz), _p(dz), _p(wv), dx, None, part, M_, C_, dt, st)

        for C in E.RD_REJECT_UNSUPPORTED[dtype]:
            assert list(every(M, C, _dt(x))) == [E.GF_ERR_UNSUPPORTED] * 4, C
        for M_, C_ in ((0, 256), (-1, 256), (M, 0), (M, -8)):
            assert list(every(M_, C_, _dt(x))) == [E.GF_ERR_SHAPE] * 4, (M_, C_)
        assert list(every(M, 256, 7)) == [E.GF_ERR_DTYPE] * 4
        torch.cuda.synchronize()
        for buf, view in outs:
            assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all() and torch.isnan(view).all(), \
                "an output was written by a rejected call"
    for M_, nb in E.RD_NBLK:
        assert lib.gf_rowdot_nblk(M_) == nb


@dtypes
@pytest.mark.parametrize("M,C", [(257, 96), (5000, 256)])
def test_ops_rowdot_against_float64_autograd(M, C, dtype):
    """ops.rowdot and ops.rowdot2 (head 1 sees x detached) against float64 autograd."""
    if dtype == BF16 and C == 96:
        C = 192
    d = _dev(E.rd_case, "rand", M, C, dtype)
    x64, w0, b0, w1, b1 = (d[k].double().clone().requires_grad_(True) for k in ("x", "w0", "b0", "w1", "b1"))
    ((x64 @ w0 + b0) * d["dz0"].double()).sum().backward()
    ((x64.detach() @ w1 + b1) * d["dz1"].double()).sum().backward()
    xs = d["x"].clone().requires_grad_(True)
    ps = [d[k].clone().requires_grad_(True) for k in ("w0", "b0", "w1", "b1")]
    z0, z1 = ops.rowdot2(xs, ps[0][None], ps[1], ps[2][None], ps[3])
    ((z0 * d["dz0"]).sum() + (z1 * d["dz1"]).sum()).backward()
    ref = E.rd_ref(d)
    w = _Worst(f"ops.rowdot2 M={M} C={C} {_name(dtype)}")
    w.add("z0", z0, ref["z0"], ref["z0_bound"])
    w.add("z1", z1, ref["z1"], ref["z1_bound"])
    w.add("dx", xs.grad, x64.grad, ref["dx_nobase_bound"])
    w.finish()
    for name, t, r in (("dw0", ps[0].grad, w0.grad), ("db0", ps[1].grad, b0.grad), ("dw1", ps[2].grad, w1.grad),
                       ("db1", ps[3].grad, b1.grad)):
        _scaled_close("ops.rowdot2 " + name, t, r, F32)
    xs1 = d["x"].clone().requires_grad_(True)
    w1s, b1s = d["w0"].clone().requires_grad_(True), d["b0"].clone().requires_grad_(True)
    z = ops.rowdot(xs1, w1s[None], b1s)
    (z * d["dz0"]).sum().backward()
    w = _Worst(f"ops.rowdot M={M} C={C} {_name(dtype)}")
    w.add("z", z, ref["z0"], ref["z0_bound"])
    w.add("dx", xs1.grad, x64.grad, ref["dx_nobase_bound"])
    w.finish()
    _scaled_close("ops.rowdot dw", w1s.grad, w0.grad, F32)
    _scaled_close("ops.rowdot db", b1s.grad, b0.grad, F32)


# ================================================================================================ column sums
@pytest.mark.parametrize("G", E.CS_G)
def test_colsum(G):
    """gf_colsum_f32 with the workspace of gf_colsum_ws_floats: fewer rows than chunks (empty chunks), the real 2048, ragged
    column groups, several matrices."""
    lib = L_.load()
    w = _Worst(f"colsum G={G}")
    for R in E.CS_R:
        for C in E.CS_C:
            for kind in E.CS_KINDS:
                d = _dev(E.cs_case, kind, G, R, C)
                ref = E.cs_ref(d)
                n = lib.gf_colsum_ws_floats(G, C)
                assert n == G * E.CS_CHUNKS * C
                runs = []
                for _ in range(2):
                    bw, ws = _guarded((n,), F32, math.nan)
                    bo, out = _guarded((G, C), F32, math.nan)
                    _ok(lib.gf_colsum_f32(_p(d["x"]), _p(ws), _p(out), G, R, C, _stream()), "gf_colsum_f32")
                    _guards_intact(bw, bo)
                    runs.append(bo)
                assert _same_bits(*runs), "gf_colsum_f32: two runs differ"
                w.add(kind, out, ref["out"], ref["out_bound"])
    bo, out = _guarded((G, 64), F32, math.nan)
    for sizes in ((0, 4, 64), (G, 0, 64), (G, 4, 0)):
        assert lib.gf_colsum_f32(_p(d["x"]), _p(out), _p(out), *sizes, _stream()) == E.GF_ERR_SHAPE
    _guards_intact(bo)
    assert torch.isnan(out).all()
    w.finish()
