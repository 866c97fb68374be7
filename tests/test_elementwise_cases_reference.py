"""CPU: keeps tests/elementwise_cases.py honest in both directions on every shape and value case (small row counts): the
fp32 / bf16 emulations in the kernels' order and the stock fp32 implementations lie inside every bound (ratios printed),
every named mutation lands outside one, the written-out float64 LayerNorm gradients equal autograd's, and the host
entries of the library match the tables."""
import pytest
import torch

import elementwise_cases as E

dtypes = pytest.mark.parametrize("dtype", E.DTYPES, ids=["fp32", "bf16"])


class _Worst:
    def __init__(self, what):
        self.what, self.worst = what, {}

    def add(self, name, x, ref, bound):
        assert x.shape == ref.shape, (name, x.shape, ref.shape)
        self.worst[name] = max(self.worst.get(name, 0.0), E.ratio(x, ref, bound))

    def finish(self):
        print(f"{self.what}: worst error/bound " + ", ".join(f"{k} {v:.3g}" for k, v in self.worst.items()))
        bad = {k: v for k, v in self.worst.items() if not v <= 1.0}
        assert not bad, f"{self.what}: over the bound (error / bound): {bad}"


def _detected(what, hits, mutations, outputs):
    """hits[mutation][output] = worst ratio over the cases."""
    print(what + ": " + "; ".join(f"{m} " + ", ".join(f"{o} {r:.3g}" for o, r in hits[m].items()) for m in mutations))
    covered = set()
    for m, outs in mutations.items():
        for o in outs:
            assert hits[m][o] > E.DETECT, f"{what}: mutation {m} stays inside the bound of {o} ({hits[m][o]:.3g})"
            covered.add(o)
    assert covered >= set(outputs), f"{what}: no mutation moves {set(outputs) - covered}"


# ================================================================================================ rotary
def _rot_cases(dtype, hds=None):
    for H, D in hds or E.ROT_VEC + E.ROT_SCALAR + E.ROT_FWD_ONLY:
        for B, N in E.ROT_TOKENS:
            for kind in E.ROT_KINDS:
                yield E.rotary_case(kind, B, N, H, D, dtype)


@dtypes
def test_rotary_emulation_and_stock_inside(dtype):
    for stock in (False, True):
        w = _Worst(f"rotary {'stock fp32' if stock else 'emulation'} {str(dtype)[6:]}")
        for case in _rot_cases(dtype):
            ref, em = E.rotary_ref(case), E.emulate_rotary(case, stock)
            for name in E.ROT_OUTPUTS:
                w.add(name, em[name], ref[name], ref[name + "_bound"])
            if case["kind"] == "quarter":             # an exact permutation with a sign
                assert torch.equal(em["fwd"].double(), ref["fwd"]) and torch.equal(em["dq"].double(), ref["dq"])
        w.finish()


def test_rotary_reference_is_rotate_half_and_its_autograd():
    """The restated reference against the rotation written with complex numbers, and dq / dtheta against autograd."""
    case = E.rotary_case("rand", 3, 1, 3, 32, torch.float32)
    th = torch.atan2(case["cs"][..., 1::2], case["cs"][..., 0::2]).double().requires_grad_(True)
    case2 = dict(case, cs=torch.stack((torch.cos(th), torch.sin(th)), -1).flatten(-2).detach())       # float64 cos / sin
    ref = E.rotary_ref(case2)
    x = case["qkv"].double()[:, :, :2].clone().requires_grad_(True)
    xc = torch.view_as_complex(x.reshape(*x.shape[:-1], -1, 2))
    yc = xc * torch.polar(torch.ones_like(th), th)[:, :, None, None]
    y = torch.view_as_real(yc).flatten(-2)
    torch.testing.assert_close(y.detach(), ref["fwd"], rtol=1e-12, atol=1e-12)
    g = case["grad"].double()[:, :, :2]
    (y * g).sum().backward()
    torch.testing.assert_close(x.grad, ref["dq"], rtol=1e-12, atol=1e-12)
    # dtheta of the entry is stated on the saved rotated values: feed them as y
    case2 = dict(case2, y=torch.cat((y.detach(), case["y"].double()[:, :, 2:]), 2))
    torch.testing.assert_close(th.grad, E.rotary_ref(case2)["dtheta"], rtol=1e-11, atol=1e-11)


def test_rotary_mutations_outside():
    hits = {m: {o: 0.0 for o in outs} for m, outs in E.ROT_MUTATIONS.items()}
    for dtype in E.DTYPES:
        for case in _rot_cases(dtype, E.ROT_VEC + E.ROT_SCALAR):
            if case["kind"] in ("zero", "quarter") or case["H"] * case["D"] <= 2:
                continue
            ref = E.rotary_ref(case)
            for m, outs in E.ROT_MUTATIONS.items():
                mut = E.rotary_ref(case, m)
                for o in outs:
                    hits[m][o] = max(hits[m][o], E.ratio(mut[o], ref[o], ref[o + "_bound"]))
    _detected("rotary mutations", hits, E.ROT_MUTATIONS, E.ROT_OUTPUTS)


# ================================================================================================ LN + GELU
def _ln_cases(dtype, rows=E.LN_ROWS):
    for C in E.LN_C[dtype]:
        for R in rows:
            for kind in E.LN_KINDS:
                yield E.ln_case(kind, R, C, dtype)


def _ln_add(w, ref, out, names):
    for name in names:
        w.add(name, out[name], ref[name], ref[name + "_bound"])


@dtypes
def test_ln_gelu_emulation_inside(dtype):
    """Also: the conditioning r stays far below 1 (the first-order model holds), the written-out gradients equal autograd's,
    and the two outlier cases side by side against the fp32 parity budget."""
    w = _Worst(f"ln_gelu emulation {str(dtype)[6:]}")
    parity = {"outlier_first": 0.0, "outlier_last": 0.0}
    for case in _ln_cases(dtype):
        ref = E.ln_ref(case)
        assert float(ref["cond"].max()) < 0.1, (case["kind"], case["C"], float(ref["cond"].max()))
        x, ga, be, dy = (case[k].double() for k in ("x", "gamma", "beta", "dy"))
        hand = E._ln_math(x, ga, be, dy, case["R"], case["C"])
        for name in ("y", "dx", "dgamma", "dbeta"):
            assert E.ratio(hand[name], ref[name], ref[name + "_bound"]) < 1e-3, f"written-out {name} differs from autograd's"
        em = E.emulate_ln(case, ref["mean"].float(), ref["rstd"].float())
        em["dgamma"], em["dbeta"] = em["dgamma_part"].double().sum(0), em["dbeta_part"].double().sum(0)
        _ln_add(w, ref, em, E.LN_OUTPUTS)
        if case["kind"] in parity:
            parity[case["kind"]] = max(parity[case["kind"]], E.parity_ratio(case, ref, em["mean"], em["rstd"]))
    print(f"ln_gelu emulation {str(dtype)[6:]}: normalised-value error / (1e-4 of the row's largest): "
          f"outlier_first {parity['outlier_first']:.3g}, outlier_last {parity['outlier_last']:.3g}")
    w.finish()                 # the parity figures are the emulation's (no fused multiply-add), printed for the record only


@dtypes
def test_ln_gelu_stock_fp32_inside(dtype):
    w = _Worst(f"ln_gelu stock fp32 {str(dtype)[6:]}")
    for case in _ln_cases(dtype):
        _ln_add(w, E.ln_ref(case, stock=True), E.stock_ln(case), ("y", "dx", "dgamma", "dbeta"))
    w.finish()


def test_ln_gelu_mutations_outside():
    hits = {m: {o: 0.0 for o in outs} for m, outs in E.LN_MUTATIONS.items()}
    for dtype in E.DTYPES:
        for case in _ln_cases(dtype, rows=[5, 37]):
            ref = E.ln_ref(case)
            for m, outs in E.LN_MUTATIONS.items():
                mut = E.ln_ref(case, m)
                for o in outs:
                    hits[m][o] = max(hits[m][o], E.ratio(mut[o], ref[o], ref[o + "_bound"]))
    _detected("ln_gelu mutations", hits, E.LN_MUTATIONS, E.LN_OUTPUTS)


# ================================================================================================ row-dot
def _rd_cases(dtype):
    for C in E.RD_C[dtype]:
        for M in E.RD_ROWS:
            if M > 1000 and C > 256:
                continue
            for kind in E.RD_KINDS:
                yield E.rd_case(kind, M, C, dtype)


@dtypes
def test_rowdot_emulation_and_stock_inside(dtype):
    w = _Worst(f"rowdot emulation {str(dtype)[6:]}")
    ws = _Worst(f"rowdot F.linear fp32 {str(dtype)[6:]}")
    for case in _rd_cases(dtype):
        ref, em = E.rd_ref(case), E.emulate_rd(case)
        for name in E.RD_OUTPUTS:
            w.add(name, em[name], ref[name], ref[name + "_bound"])
        x = case["x"].float().clone().requires_grad_(True)
        ps = [case[k].float().clone().requires_grad_(True) for k in ("w0", "b0", "w1", "b1")]
        z0 = torch.nn.functional.linear(x, ps[0][None], ps[1])[:, 0]
        z1 = torch.nn.functional.linear(x.detach(), ps[2][None], ps[3])[:, 0]
        ((z0 * case["dz0"]).sum() + (z1 * case["dz1"]).sum()).backward()
        ws.add("z0", z0, ref["z0"], ref["z0_bound"])
        ws.add("z1", z1, ref["z1"], ref["z1_bound"])
        ws.add("dx_nobase", x.grad.to(case["dtype"]), ref["dx_nobase"], ref["dx_nobase_bound"])
        for k, name in enumerate(("dw0", "db0", "dw1", "db1")):
            ws.add(name, ps[k].grad, ref[name], ref[name + "_bound"])
    w.finish()
    ws.finish()


def test_rowdot_mutations_outside():
    hits = {m: {o: 0.0 for o in outs} for m, outs in E.RD_MUTATIONS.items()}
    for dtype in E.DTYPES:
        for case in _rd_cases(dtype):
            if case["M"] < 3:
                continue
            ref = E.rd_ref(case)
            for m, outs in E.RD_MUTATIONS.items():
                mut = E.rd_ref(case, m)
                for o in outs:
                    hits[m][o] = max(hits[m][o], E.ratio(mut[o], ref[o], ref[o + "_bound"]))
    _detected("rowdot mutations", hits, E.RD_MUTATIONS, [o for o in E.RD_OUTPUTS if "nobias" not in o])


# ================================================================================================ column sums
def test_colsum_emulation_stock_and_mutation():
    w, ws, worst_mut = _Worst("colsum emulation"), _Worst("colsum torch fp32 sum"), 0.0
    for G in E.CS_G:
        for R in E.CS_R:
            for C in E.CS_C:
                if G == 3 and R > 33 and C != 65:       # the large row counts once per G are enough on the CPU
                    continue
                for kind in E.CS_KINDS:
                    case = E.cs_case(kind, G, R, C)
                    ref = E.cs_ref(case)
                    w.add(kind, E.emulate_cs(case), ref["out"], ref["out_bound"])
                    ws.add(kind, case["x"].sum(1), ref["out"], ref["out_bound"])
                    worst_mut = max(worst_mut, E.ratio(E.cs_ref(case, "last_chunk_dropped")["out"], ref["out"], ref["out_bound"]))
    print(f"colsum mutation last_chunk_dropped: {worst_mut:.3g}")
    assert worst_mut > E.DETECT
    w.finish()
    ws.finish()


# ================================================================================================ host entries and tables
def test_host_entries_match_the_tables():
    from glue_factory_amd import lib
    L = lib.load()
    for R, nb in E.LN_NBLK:
        assert L.gf_ln_gelu_nblk(R) == nb == E.ln_nblk(R), R
    for M, nb in E.RD_NBLK:
        assert L.gf_rowdot_nblk(M) == nb == E.rd_nblk(M), M
    for G in E.CS_G:
        for C in E.CS_C:
            assert L.gf_colsum_ws_floats(G, C) == G * E.CS_CHUNKS * C


def test_tables_pin_the_paths_they_name():
    assert all(E.rotary_vec_ok(*hd) for hd in E.ROT_VEC) and not any(E.rotary_vec_ok(*hd) for hd in E.ROT_SCALAR)
    assert [E.rotary_vec_ok(*hd) for hd in E.ROT_FWD_ONLY] == [False, True]
    assert [E.ln_nch(C, torch.float32) for C in E.LN_C[torch.float32]] == [1, 2, 4, 1, 1, 2, 4, 4]
    assert [E.ln_nch(C, torch.bfloat16) for C in E.LN_C[torch.bfloat16]] == [1, 2, 4, 1, 1, 2, 4, 4]
    for dt in E.DTYPES:
        assert all(E.ln_nch(C, dt) == -1 for C in E.LN_REJECT_UNSUPPORTED[dt])
        assert [256 // (C // E.vec_of(dt)) for C in E.RD_C[dt]] == [256, 85, 10, 4 if dt == torch.float32 else 8, 1, 1]
