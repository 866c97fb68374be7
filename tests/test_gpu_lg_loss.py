"""The fused LightGlue layer loss (csrc/lg_loss.hip) on its own: ops.lg_layer_loss against dense float64 autograd, and the
three C-ABI entries gf_lg_loss_fwd / _bwd_tokens / _bwd_rows on stated statistics against the closed forms of
include/gf_amd.h (references, inputs and their conditions: tests/lg_loss_cases.py, held by tests/test_lg_loss_reference.py).

Bounds (derived, not tuned; `T` = the sum of the absolute values of a value's elementary addends, lg_loss_cases):
  acc                  |x - ref| <= 1e-5 T + 1e-6     fp32 accumulation of at most a few hundred addends and the exp / log1p
                                                      intrinsics are each good to a few 1e-7 relative per addend; the same in
                                                      bf16, whose stored values the reference upcasts and the kernels multiply
                                                      in fp32
  dz, dt, gr, gc       |x - ref| <= 1e-5 T + 1e-7     fp32 outputs of fp32 inputs in both dtypes
  d(md), op level      _tols(dtype) of the kernel tests (1e-4 fp32, 5e-2 bf16) after dividing by the reference's largest
                       magnitude: the dense double-softmax part dominates there
  dmd, gf_lg_loss_bwd_rows on a base:  fp32 1e-5 (|base| + sum |term|) + 1e-7;  bf16 2 h 2^-7 (|base| + sum |term|) for h
                       adds on the element (each add rounds its addend and then the sum to bf16; one ulp, 2^-7 relative,
                       covers nearest and truncating rounding alike) -- 1.6 % at h = 1, a missing or doubled term fails.
Every test prints its worst error / bound ratio."""
import functools
import math

import pytest
import torch

import lg_loss_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from glue_factory_amd import lib as L_
    from glue_factory_amd import ops
    from glue_factory_amd.ops import _dt, _p, _stream

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
GF_ERR_SHAPE, GF_ERR_ALIGN, GF_ERR_DTYPE = -2, -3, -4
GUARD = 64               # sentinel elements on either side of every output
SENTINEL = -776.0        # exact in bf16


def _tols(dtype):
    return dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=5e-2, atol=5e-2)


def _ratio(x, ref, bound):
    """Worst |x - ref| / bound; a non-finite x is infinitely far off."""
    x, ref = x.detach().cpu().double(), ref.detach().cpu().double()
    if x.numel() == 0:
        return 0.0
    if not torch.isfinite(x).all():
        return math.inf
    return float(((x - ref).abs() / bound.cpu().double()).max())


class _Worst:
    """Collects error / bound ratios, prints the worst of each name and fails if one exceeds 1."""

    def __init__(self, what):
        self.what, self.worst = what, {}

    def add(self, name, x, ref, bound):
        assert x.shape == ref.shape, (name, x.shape, ref.shape)
        self.worst[name] = max(self.worst.get(name, 0.0), _ratio(x, ref, bound))

    def finish(self):
        print(f"{self.what}: worst error/bound " + ", ".join(f"{k} {v:.3g}" for k, v in self.worst.items()))
        bad = {k: v for k, v in self.worst.items() if not v <= 1.0}
        assert not bad, f"{self.what}: over the bound (error / bound): {bad}"


def _dev(x):
    return None if x is None else x.to(DEV)


# =============================================================================================== ops.lg_layer_loss
@functools.lru_cache(maxsize=None)
def _dense_reference(B, N, D, dtype, kind, with_t):
    """reference_dense of a planted case with autograd's gradients of (acc * gacc).sum(); computed once per variant."""
    case = C.planted_case(B, N, D, dtype)
    pos = C.positives(case, kind)
    leaves = [case[k].double().requires_grad_(True) for k in ("md0", "md1", "z0", "z1")]
    ts = [case[k].double().requires_grad_(True) for k in ("t0", "t1")] if with_t else [None, None]
    ref = C.reference_dense(*leaves, *ts, pos, case["neg0"], case["neg1"], case["fin0"], case["fin1"])
    (ref["acc"] * case["gacc"].double()).sum().backward()
    lse = C.dense_stats(case["md0"], case["md1"], case["z0"], case["z1"])
    return {"pos": pos, "tgt0": ref["tgt0"], "tgt1": ref["tgt1"], "dmd": torch.cat([leaves[0].grad, leaves[1].grad]),
            "dz": torch.cat([leaves[2].grad, leaves[3].grad]),
            "dt": torch.cat([ts[0].grad, ts[1].grad]) if with_t else None, "r": lse["r"], "c": lse["c"]}


def _expected_forward(case, pos, with_t, r, c):
    """acc, T and the gradient T's for the normalisers the op actually used (float64 statistics from those r, c)."""
    st = C.dense_stats(case["md0"], case["md1"], case["z0"], case["z1"], r, c)
    t0, t1 = (case["t0"], case["t1"]) if with_t else (None, None)
    return C.reference_stats(case["md0"], case["md1"], case["z0"], case["z1"], t0, t1, pos, case["neg0"], case["neg1"],
                             case["fin0"], case["fin1"], st["r"], st["c"], st["v0"], st["a0"], st["v1"], st["a1"], case["gacc"])


def _run_layer_loss(B, N, D, dtype, kind, with_t, with_rc):
    case = C.planted_case(B, N, D, dtype)
    ref = _dense_reference(B, N, D, dtype, kind, with_t)
    pos = ref["pos"]
    md = torch.cat([case["md0"], case["md1"]]).to(DEV)
    z = torch.cat([case["z0"], case["z1"]]).to(DEV)
    t = torch.cat([case["t0"], case["t1"]]).to(DEV) if with_t else None
    a, b = md[:B], md[B:]
    if with_rc:                       # the float64 log-sum-exp rounded to fp32
        r, c = ref["r"].float().to(DEV), ref["c"].float().to(DEV)
        rc = (r, c)
    else:                             # the op computes its own: expect what the (separately tested) gf_rows_lse gives
        r, c = ops.rows_lse(a, b), ops.rows_lse(b, a)
        rc = None
    exp = _expected_forward(case, pos, with_t, r.cpu(), c.cpu())
    # the statistics of the normalisers in use decide every target as the dense reference does (the inputs keep a margin of
    # C.GAP; a normaliser far enough off to break this fails test_rows_lse_normalisers)
    assert torch.equal(exp["tgt0"], ref["tgt0"]) and torch.equal(exp["tgt1"], ref["tgt1"])
    gacc = case["gacc"].to(DEV)
    args = (rc, tuple(x.to(DEV) for x in pos), _dev(case["neg0"]), _dev(case["neg1"]), _dev(case["fin0"]), _dev(case["fin1"]))
    w = _Worst(f"lg_layer_loss ({B},{N},{D}) {str(dtype)[6:]} {kind} t={'y' if with_t else 'n'} rc={'y' if with_rc else 'n'}")
    empty_images = [i for i in range(B) if not ((pos[0] == i) & (pos[2] >= 0)).any()]
    scale = max(float(ref["dmd"].abs().max()), 1e-2)
    tol = _tols(dtype)
    for _ in range(2):                # twice: the order of the atomics is free, so both runs are held to the bounds, not to each other
        mdg, zg = md.clone().requires_grad_(True), z.clone().requires_grad_(True)
        tg = None if t is None else t.clone().requires_grad_(True)
        acc = ops.lg_layer_loss(mdg, zg, tg, *args)
        (acc * gacc).sum().backward()
        assert acc.shape == (B, 4) and acc.dtype == torch.float32
        w.add("acc", acc, exp["acc"], 1e-5 * exp["T_acc"] + 1e-6)
        for i in empty_images:
            assert float(acc.detach()[i, 0]) == 0.0, f"image {i} has no positive: acc[{i},0] must be exactly 0"
        if not with_t:
            assert tg is None and (acc[:, 2:] == 0).all()
        w.add("dz", zg.grad, ref["dz"], 1e-5 * torch.cat([exp["T_dz0"], exp["T_dz1"]]) + 1e-7)
        if with_t:
            w.add("dt", tg.grad, ref["dt"], 1e-5 * torch.cat([exp["T_dt0"], exp["T_dt1"]]) + 1e-7)
        assert mdg.grad.dtype == dtype
        w.add("dmd", mdg.grad, ref["dmd"], tol["atol"] * scale + tol["rtol"] * ref["dmd"].abs())
    w.finish()


@pytest.mark.parametrize("kind", C.OPS_LISTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,D", C.OPS_CASES)
def test_layer_loss_lists(B, N, D, dtype, kind):
    """Every kind of positives list with token logits and rc=None (the three-pass form of a middle layer)."""
    _run_layer_loss(B, N, D, dtype, kind, with_t=True, with_rc=False)


@pytest.mark.parametrize("with_t,with_rc", [(False, True), (False, False), (True, True)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,D", C.OPS_CASES)
def test_layer_loss_forms(B, N, D, dtype, with_t, with_rc):
    """The fixed list in the remaining forms: t=None with rc (the last layer), t=None without, t with rc."""
    _run_layer_loss(B, N, D, dtype, "fixed", with_t, with_rc)


def test_layer_loss_returns_no_dt_without_t():
    B, N, D = C.OPS_CASES[0]
    case = C.planted_case(B, N, D, torch.float32)
    md = torch.cat([case["md0"], case["md1"]]).to(DEV).requires_grad_(True)
    z = torch.cat([case["z0"], case["z1"]]).to(DEV).requires_grad_(True)
    pos = tuple(x.to(DEV) for x in C.positives(case, "fixed"))
    acc = ops.lg_layer_loss(md, z, None, None, pos, _dev(case["neg0"]), _dev(case["neg1"]), None, None)
    from glue_factory_amd.ops._assignment import _LGLayerLoss
    grads = _LGLayerLoss.backward(acc.grad_fn, case["gacc"].to(DEV))      # (the node of a torch.autograd.Function is its ctx)
    assert len(grads) == 9 and grads[0] is not None and grads[1] is not None and all(g is None for g in grads[2:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,D", C.OPS_CASES)
def test_rows_lse_normalisers(B, N, D, dtype):
    """The two vectors the rc=None expectations are built on, held to test_assignment_head's own tolerance."""
    case = C.planted_case(B, N, D, dtype)
    lse = C.dense_stats(case["md0"], case["md1"], case["z0"], case["z1"])
    a, b = case["md0"].to(DEV), case["md1"].to(DEV)
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=2e-2, atol=8e-2)
    w = _Worst(f"rows_lse ({B},{N},{D}) {str(dtype)[6:]}")
    for name, x, ref in (("r", ops.rows_lse(a, b), lse["r"]), ("c", ops.rows_lse(b, a), lse["c"])):
        w.add(name, x, ref, tol["atol"] + tol["rtol"] * ref.abs())
    w.finish()


# =============================================================================================== the C-ABI entries
def _guarded(shape, dtype, fill):
    """(buffer, view): `view` of the given shape filled with `fill`, GUARD sentinel elements on either side of it."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    if torch.is_tensor(fill):
        view.copy_(fill)
    else:
        view.fill_(fill)
    return buf, view


def _guards_intact(bufs):
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        for part in (buf[:GUARD], buf[-GUARD:]):
            assert (part == SENTINEL).all(), f"{name}: a sentinel next to the output was written"


def _abi_inputs(case):
    return {k: case[k].to(DEV) for k in ("md0", "md1", "z0", "z1", "t0", "t1", "neg0", "neg1", "r", "c", "v0", "a0", "v1", "a1",
                                         "fin0", "fin1", "gacc")}


def _fwd(lib, d, pos, P, with_t, tgt0, tgt1, acc, B, M, N, D, dtype_code, t0="t0", t1="t1"):
    ts = (_p(d[t0]) if t0 else None, _p(d[t1]) if t1 else None) if with_t else (None, None)
    return lib.gf_lg_loss_fwd(_p(d["md0"]), _p(d["md1"]), _p(d["z0"]), _p(d["z1"]), _p(d["r"]), _p(d["c"]),
                              _p(pos[0]), _p(pos[1]), _p(pos[2]), P, _p(d["neg0"]), _p(d["neg1"]), ts[0], ts[1],
                              _p(d["v0"]), _p(d["a0"]), _p(d["v1"]), _p(d["a1"]), _p(d["fin0"]), _p(d["fin1"]),
                              _p(tgt0), _p(tgt1), _p(acc), B, M, N, D, dtype_code, _stream())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,M,N,D", C.ABI_CASES)
def test_abi_fwd(B, M, N, D, dtype):
    """gf_lg_loss_fwd on stated statistics: acc within 1e-5 T + 1e-6, targets exactly the reference's 0/1 values; with
    t0 = t1 = NULL acc[:, 2:] is exactly 0 and tgt is not touched; nothing next to an output is written."""
    case = C.abi_case(B, M, N, D, dtype)
    d = _abi_inputs(case)
    lib = L_.load()
    w = _Worst(f"gf_lg_loss_fwd ({B},{M},{N},{D}) {str(dtype)[6:]}")
    for kind in C.ABI_LISTS:
        pos_cpu = C.positives(case, kind)
        pos = tuple(x.to(DEV) for x in pos_cpu)
        P = pos_cpu[0].shape[0]
        for with_t in (True, False):
            exp = C.stats_of(case, pos_cpu, with_t=with_t, gacc=False)
            bufs, views = {}, {}
            for name, shape in (("acc", (B, 4)), ("tgt0", (B, M)), ("tgt1", (B, N))):
                bufs[name], views[name] = _guarded(shape, torch.float32, SENTINEL if name != "acc" else float("nan"))
            L_.check(_fwd(lib, d, pos, P, with_t, views["tgt0"], views["tgt1"], views["acc"], B, M, N, D, _dt(d["md0"])),
                     "gf_lg_loss_fwd")
            _guards_intact(bufs)
            w.add(f"acc/{kind}", views["acc"], exp["acc"], 1e-5 * exp["T_acc"] + 1e-6)
            if with_t:
                assert torch.equal(views["tgt0"].cpu().double(), exp["tgt0"]), f"{kind}: tgt0"
                assert torch.equal(views["tgt1"].cpu().double(), exp["tgt1"]), f"{kind}: tgt1"
            else:
                assert (views["acc"][:, 2:] == 0).all()
                assert (views["tgt0"] == SENTINEL).all() and (views["tgt1"] == SENTINEL).all(), "tgt written without t"
            if kind == "empty":
                assert (views["acc"][:, 0] == 0).all()
    w.finish()


def test_abi_fwd_rejects_bad_arguments():
    """D = 6 -> GF_ERR_ALIGN, exactly one of t0 / t1 NULL -> GF_ERR_SHAPE, an unknown dtype -> GF_ERR_DTYPE; no kernel
    runs on these (acc and tgt keep their fill)."""
    B, M, N, D = C.ABI_CASES[0]
    case = C.abi_case(B, M, N, D, torch.float32)
    d = _abi_inputs(case)
    pos = tuple(x.to(DEV) for x in C.positives(case, "fixed"))
    P = pos[0].shape[0]
    lib = L_.load()
    bufs, views = {}, {}
    for name, shape in (("acc", (B, 4)), ("tgt0", (B, M)), ("tgt1", (B, N))):
        bufs[name], views[name] = _guarded(shape, torch.float32, SENTINEL)
    out = (views["tgt0"], views["tgt1"], views["acc"])
    assert _fwd(lib, d, pos, P, True, *out, B, M, N, 6, 0) == GF_ERR_ALIGN          # (rows of D = 36: reads would stay in bounds)
    assert _fwd(lib, d, pos, P, True, *out, B, M, N, D, 0, t1=None) == GF_ERR_SHAPE
    assert _fwd(lib, d, pos, P, True, *out, B, M, N, D, 0, t0=None) == GF_ERR_SHAPE
    assert _fwd(lib, d, pos, P, True, *out, B, M, N, D, 7) == GF_ERR_DTYPE
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        assert (buf == SENTINEL).all(), f"{name} was written by a rejected call"


@pytest.mark.parametrize("B,M,N,D", C.ABI_CASES)
def test_abi_bwd_tokens(B, M, N, D):
    """gf_lg_loss_bwd_tokens into NaN-filled outputs: dz, dt, gr, gc equal the closed forms within 1e-5 T + 1e-7, and
    gr / gc are EXACTLY -g count (gacc is dyadic, so the sum is exact in any order)."""
    case = C.abi_case(B, M, N, D, torch.float32)
    d = _abi_inputs(case)
    lib = L_.load()
    w = _Worst(f"gf_lg_loss_bwd_tokens ({B},{M},{N})")
    for kind in C.ABI_LISTS:
        pos_cpu = C.positives(case, kind)
        pos = tuple(x.to(DEV) for x in pos_cpu)
        P = pos_cpu[0].shape[0]
        for with_t in (True, False):
            exp = C.stats_of(case, pos_cpu, with_t=with_t)
            bufs, v = {}, {}
            for name, n in (("dz0", M), ("dz1", N), ("dt0", M), ("dt1", N), ("gr", M), ("gc", N)):
                bufs[name], v[name] = _guarded((B, n), torch.float32, float("nan") if with_t or name[:2] != "dt" else SENTINEL)
            tp = (None,) * 4
            if with_t:
                tgt0, tgt1 = exp["tgt0"].float().to(DEV), exp["tgt1"].float().to(DEV)
                tp = (_p(d["t0"]), _p(d["t1"]), _p(tgt0), _p(tgt1))
            dtp = (_p(v["dt0"]), _p(v["dt1"])) if with_t else (None, None)
            L_.check(lib.gf_lg_loss_bwd_tokens(_p(d["z0"]), _p(d["z1"]), _p(d["neg0"]), _p(d["neg1"]), *tp,
                                               _p(pos[0]), _p(pos[1]), _p(pos[2]), P, _p(d["gacc"]), _p(v["dz0"]), _p(v["dz1"]),
                                               *dtp, _p(v["gr"]), _p(v["gc"]), B, M, N, _stream()), "gf_lg_loss_bwd_tokens")
            _guards_intact(bufs)
            for name in ("dz0", "dz1") + (("dt0", "dt1") if with_t else ()):
                w.add(f"{name[:2]}/{kind}", v[name], exp[name], 1e-5 * exp["T_" + name] + 1e-7)
            for name in ("gr", "gc"):
                assert torch.equal(v[name].cpu().double(), exp[name]), f"{kind}: {name} != -g count"
    w.finish()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,M,N,D", C.ABI_CASES)
def test_abi_bwd_rows(B, M, N, D, dtype):
    """gf_lg_loss_bwd_rows accumulating into a seeded base: base + sum of the terms within the bound of the module
    docstring; rows that no positive names stay bit-identical to the base."""
    case = C.abi_case(B, M, N, D, dtype)
    d = _abi_inputs(case)
    lib = L_.load()
    w = _Worst(f"gf_lg_loss_bwd_rows ({B},{M},{N},{D}) {str(dtype)[6:]}")
    for kind in C.ABI_LISTS:
        pos_cpu = C.positives(case, kind)
        pos = tuple(x.to(DEV) for x in pos_cpu)
        P = pos_cpu[0].shape[0]
        exp = C.stats_of(case, pos_cpu, with_t=False)
        bufs, v = {}, {}
        for name in ("0", "1"):
            bufs[name], v[name] = _guarded(case["base" + name].shape, dtype, case["base" + name].to(DEV))
        L_.check(lib.gf_lg_loss_bwd_rows(_p(d["md0"]), _p(d["md1"]), _p(pos[0]), _p(pos[1]), _p(pos[2]), P, _p(d["gacc"]),
                                         _p(v["0"]), _p(v["1"]), B, M, N, D, _dt(d["md0"]), _stream()), "gf_lg_loss_bwd_rows")
        _guards_intact(bufs)
        for name in ("0", "1"):
            base, out = case["base" + name], v[name].cpu()
            hits = exp["hits" + name]
            named = hits > 0
            assert torch.equal(out[~named], base[~named]), f"{kind}: rows of dmd{name} that no positive names changed"
            if kind == "empty":
                assert not named.any()
                continue
            T = base.double().abs() + exp["T_sp" + name]
            if dtype == torch.float32:
                bound = 1e-5 * T + 1e-7
            else:
                bound = 2.0 * hits[..., None] * 2.0 ** -7 * T
            w.add(f"dmd{name}/{kind}", out[named], (base.double() + exp["sp" + name])[named], bound[named])
    w.finish()
