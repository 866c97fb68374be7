"""CPU checks of what tests/test_gpu_assignment.py relies on (tests/assignment_cases.py): the float64 references agree with
autograd of the oracle's log_double_softmax, every mutation of a reference that a wrong kernel would amount to moves an
asserted output by DETECT bounds (or changes an index), the fp32 rounding model of the kernels lies inside every bound,
and the planted margins, the bit-identical ties and the split geometry hold.  These are conditions on the INPUTS and on
the bounds; a failure here means a case or a derivation has to change, never the bound alone."""
import math

import pytest
import torch

import assignment_cases as C
from oracle.lightglue_oracle import filter_matches, log_double_softmax

CFG_IDS = ["x".join(map(str, c)) for c in C.CONFIGS]
WRITE_COMBOS = [(2.0, 0.0, "head"), (1.0, -1.75, "head"), (2.0, -1.75, "none"), (1.0, 0.0, "plain")]
BWD_COMBOS = [(False, 0.0), (True, 1.0), (True, 0.5)]           # (with G, galpha)


def _ratio(x, ref, bound):
    """Worst |x - ref| / bound; a NaN (an element never written) or an infinite difference is infinitely far off; two equal
    infinities agree."""
    x, ref = x.double(), ref.double()
    same = (x == ref)
    d = torch.where(same, torch.zeros_like(ref), (x - ref).abs() / bound.double())
    if torch.isnan(d).any():
        return math.inf
    return float(d.max()) if d.numel() else 0.0


def test_geometry_of_the_shapes():
    """The split ranges the shapes were chosen for."""
    assert C.split_ranges(257) == [(0, 128), (128, 256), (256, 257)]
    assert C.split_ranges(449) == [(0, 128), (128, 256), (256, 384), (384, 449)]
    assert C.split_ranges(513) == [(0, 192), (192, 384), (384, 513)]
    assert C.split_ranges(1024) == [(0, 256), (256, 512), (512, 768), (768, 1024)]
    assert C.split_ranges(65) == [(0, 64), (64, 65)] and C.split_ranges(63) == [(0, 63)] and C.split_ranges(1) == [(0, 1)]
    assert C.tie_pairs(449) == [(3, 11), (1, 5), (6, 10), (2, 70), (0, 448)]
    assert C.tie_pairs(200)[-1] == (135, 192)
    assert C.tie_pairs(63) == [(3, 11), (1, 5), (6, 10), (0, 62)] and C.tie_pairs(1) == []


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cfg", C.CONFIGS, ids=CFG_IDS)
def test_references_equal_oracle_autograd(cfg, dtype):
    """With W a weight on the core, L = sum W * log_double_softmax(sim, z0, z1)[core] has dL/dsim = 2 W - rowsum(W) P_row -
    colsum(W) P_col: ref_bwd with G = W, galpha = 2, gr = -rowsum, gc = -colsum on the exact normalisers must equal
    autograd, ref_lse both normalisers, and ref_write (alpha = 2, LightGlue's vectors) the oracle's matrix, all to 1e-11."""
    case = C.get_case("rand", *cfg, dtype)
    B, No, Ns = case["B"], case["No"], case["Ns"]
    tol = dict(rtol=1e-11, atol=1e-11)
    sim = (case["oth"].double() @ case["own"].double().transpose(1, 2)).requires_grad_(True)      # [B,Ns,No]: a = oth, b = own
    z0, z1 = case["z"].double().requires_grad_(True), case["bin_o"].double().requires_grad_(True)
    la = log_double_softmax(sim, z0, z1)
    W = case["G"].double()
    (la * W).sum().backward()
    c = C.ref_lse(case, False)["lse"]                              # over the streamed axis, per owner row
    r = C.ref_lse(C.swapped(case), False)["lse"]                   # over the owner axis, per streamed row
    torch.testing.assert_close(r, sim.detach().logsumexp(2), **tol)
    torch.testing.assert_close(c, sim.detach().logsumexp(1), **tol)
    ls = torch.nn.functional.logsigmoid
    vecs = (ls(z0.detach()) - r, ls(z1.detach()) - c, ls(-z0.detach()), ls(-z1.detach()))
    out = C.ref_write(case, 2.0, 0.0, vecs)
    torch.testing.assert_close(out["out"], la.detach(), **tol)
    assert (out["T"] >= out["out"].abs() * (1 - 1e-12)).all()
    torch.testing.assert_close(out["expsum"], la.detach().exp()[:, :-1].sum((1, 2)), **tol)
    Wc = W[:, :Ns, :No]
    exact = dict(case, gr=-Wc.sum(2), gc=-Wc.sum(1), r32=r, c32=c)
    ref = C.ref_bwd(exact, True, 2.0, torch.float32)
    torch.testing.assert_close(ref["dS"], sim.grad, **tol)
    assert (ref["T"] >= ref["dS"].abs() * (1 - 1e-12)).all()
    # the gradients of the assignment with respect to its vectors: what ops.assign_write's backward returns
    torch.testing.assert_close(z0.grad, (Wc.sum(2) * torch.sigmoid(-z0.detach()) - W[:, :Ns, No] * torch.sigmoid(z0.detach())), **tol)


def _arg_moved(ref, mut):
    """An index changed, or (where no other index exists) the value moved by DETECT bounds."""
    if not torch.equal(ref["idx"], mut["idx"]):
        return math.inf
    return _ratio(mut["val"], ref["val"], ref["bound"])


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cfg", C.CONFIGS, ids=CFG_IDS)
def test_every_mutation_is_detected(cfg, dtype):
    """Each mutation of a reference stands for a kernel bug (a streamed row dropped or counted twice, an owner row shifted,
    a tile-local index, the wrong tie, the dustbin column missing from expsum, G read with the wrong stride, galpha
    ignored, a normaliser off by ln 2).  Against the unmutated reference it must exceed DETECT times the bound the GPU
    test allows, in the entry and case named; the worst (smallest) ratio of each is printed."""
    B, No, Ns, D = cfg
    rand, planted = C.get_case("rand", *cfg, dtype), C.get_case("planted", *cfg, dtype)
    found = {}

    def note(name, ratio):
        found[name] = min(found.get(name, math.inf), ratio)

    lse_p, lse_r = C.ref_lse(planted, False), C.ref_lse(rand, True)
    args_p = {v: C.ref_argmax(planted, v) for v in C.ARG_VARIANTS}
    # ---- streaming kernels (no split): lse and arg-max of the planted case, whose first owner rows win at the special rows
    drops = [(j,) for j in C.special_rows(Ns, False)] + [tuple(C.special_rows(Ns, False))]
    for rows in drops:
        m = ("drop", rows)
        note("drop/lse", _ratio(C.ref_lse(planted, False, m)["lse"], lse_p["lse"], lse_p["bound"]))
        for v in C.ARG_VARIANTS:
            note("drop/arg", _arg_moved(args_p[v], C.ref_argmax(planted, v, m)))
    j = int(planted["win"].view(-1)[0])
    note("twice/lse", _ratio(C.ref_lse(planted, False, ("twice", j))["lse"], lse_p["lse"], lse_p["bound"]))
    note("ln2_row/lse", _ratio(C.ref_lse(rand, True, ("ln2_row",))["lse"], lse_r["lse"], lse_r["bound"]))
    if No > 1:
        note("owner_shift/lse", _ratio(C.ref_lse(rand, True, ("owner_shift",))["lse"], lse_r["lse"], lse_r["bound"]))
        for v in C.ARG_VARIANTS:
            note("owner_shift/arg", _arg_moved(args_p[v], C.ref_argmax(planted, v, ("owner_shift",))))
    if Ns > C.TILE:
        for v in C.ARG_VARIANTS:
            note("tile_local/arg", _arg_moved(args_p[v], C.ref_argmax(planted, v, ("tile_local",))))
    if C.has_kind("ties", Ns):
        ties = C.get_case("ties", *cfg, dtype)
        for v in C.ARG_VARIANTS:
            a, b = C.ref_argmax(ties, v), C.ref_argmax(ties, v, ("tie_highest",))
            assert not torch.equal(a["idx"], b["idx"])
            note("tie_highest/arg", math.inf)
    # ---- split kernels: every element of the matrix and of dS, and expsum
    sp = C.special_rows(Ns, True)
    for alpha, corner, mode in WRITE_COMBOS:
        vecs = C.write_vecs(rand, mode)
        ref = C.ref_write(rand, alpha, corner, vecs)
        for rows in [(j,) for j in sp]:
            note("drop/write", _ratio(C.ref_write(rand, alpha, corner, vecs, ("drop", rows))["out"], ref["out"], ref["bound"]))
        if No > 1:
            note("owner_shift/write", _ratio(C.ref_write(rand, alpha, corner, vecs, ("owner_shift",))["out"], ref["out"], ref["bound"]))
        share = ref["out"][:, :Ns].exp().sum(2)                  # the row of each image that weighs most in expsum, counted twice
        for b in range(B):
            jb = int(share[b].argmax())
            m = C.ref_write(rand, alpha, corner, vecs, ("twice", jb))
            note("twice/expsum", float(((m["expsum"] - ref["expsum"]).abs() / ref["expsum_bound"])[b]))
        if mode == "head" and alpha == 2.0:                      # the log assignment: entries <= 0, the dustbin column a visible share
            m = C.ref_write(rand, alpha, corner, vecs, ("no_dustbin",))
            note("no_dustbin/expsum", float(((m["expsum"] - ref["expsum"]).abs() / ref["expsum_bound"]).min()))
    for out_dtype in {torch.float32, dtype}:
        for with_G, galpha in BWD_COMBOS:
            ref = C.ref_bwd(rand, with_G, galpha, out_dtype)
            muts = [("drop", (j,)) for j in sp] + [("ln2_row",)] + ([("owner_shift",)] if No > 1 else [])
            if with_G and galpha != 1.0:
                muts.append(("galpha_one",))
            if with_G and Ns > 1:
                muts.append(("ldg_n",))
            for m in muts:
                note(m[0] + "/dS", _ratio(C.ref_bwd(rand, with_G, galpha, out_dtype, m)["dS"], ref["dS"], ref["bound"]))
    print(f"mutations {cfg} {str(dtype)[6:]}: smallest change / bound " + ", ".join(f"{k} {v:.3g}" for k, v in found.items()))
    bad = {k: v for k, v in found.items() if not v >= C.DETECT}
    assert not bad, f"mutations that the bounds would let pass: {bad}"


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cfg", C.CONFIGS, ids=CFG_IDS)
def test_rounding_model_is_inside_the_bounds(cfg, dtype):
    """The references evaluated the way the kernels evaluate them (stored inputs, sequential fp32 accumulation, exp2 / log2 in
    fp32, dS rounded to bf16 where the kernel does) pass every check of the GPU test: values within the bound, indices
    exact on planted / ties / large, at most MAX_BELOW_MARGIN undecided rows on rand."""
    B, No, Ns, D = cfg
    worst = {}

    def note(name, ratio):
        worst[name] = max(worst.get(name, 0.0), ratio)

    for kind in C.KINDS:
        if not C.has_kind(kind, Ns):
            continue
        case = C.get_case(kind, *cfg, dtype)
        for with_bias in (False, True):
            ref = C.ref_lse(case, with_bias)
            note("lse", _ratio(C.model_lse(case, with_bias), ref["lse"], ref["bound"]))
        for v in C.ARG_VARIANTS:
            ref = C.ref_argmax(case, v)
            val, idx = C.model_argmax(case, v)
            note("argmax", _ratio(val, ref["val"], ref["bound"]))
            differ = idx != ref["idx"]
            if kind == "rand":
                assert (ref["gap"][differ] <= ref["bound_pair"][differ]).all(), "a decided arg-max differs in the model"
                picked = ref["X"].gather(2, idx[..., None]).squeeze(2)
                note("picked", _ratio(picked, ref["val"], ref["bound_pair"]))
                assert float(differ.double().mean()) <= C.MAX_BELOW_MARGIN
            else:
                assert not differ.any(), f"{kind} {v}: the model's arg-max differs"
        if kind in ("rand", "planted"):
            for alpha, corner, mode in WRITE_COMBOS:
                vecs = C.write_vecs(case, mode)
                ref = C.ref_write(case, alpha, corner, vecs)
                out, es = C.model_write(case, alpha, corner, vecs)
                note("write", _ratio(out, ref["out"], ref["bound"]))
                note("expsum", _ratio(es, ref["expsum"], ref["expsum_bound"]))
            for out_dtype in {torch.float32, dtype}:
                for with_G, galpha in BWD_COMBOS:
                    ref = C.ref_bwd(case, with_G, galpha, out_dtype)
                    note("dS/" + str(out_dtype)[6:], _ratio(C.model_bwd(case, with_G, galpha, out_dtype), ref["dS"], ref["bound"]))
    masked = C.get_case("rand", *cfg, dtype)
    for v in C.ARG_VARIANTS[2:4]:
        sb = C.masked_bias(masked)
        ref = C.ref_argmax(masked, v, sbias=sb)
        val, idx = C.model_argmax(masked, v, sbias=sb)
        assert (ref["idx"][-1] == 0).all() and (ref["val"][-1] == -math.inf).all()
        assert (idx[-1] == 0).all() and (val[-1] == -math.inf).all()
    print(f"model {cfg} {str(dtype)[6:]}: worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"the rounding model leaves the bound: {bad}"


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cfg", C.CONFIGS, ids=CFG_IDS)
def test_margins_ties_and_edges(cfg, dtype):
    """planted and large: every arg-max keeps GAP in float64, bias included, and GAP exceeds the two value bounds; ties: the
    duplicate is bit-identical, biases included, scores equally in float64, and both the stated rule and torch.max give
    the lowest index; rand: at most MAX_BELOW_MARGIN undecided rows; every image of a batch has its own data."""
    B, No, Ns, D = cfg
    for kind in C.KINDS:
        if not C.has_kind(kind, Ns):
            continue
        case = C.get_case(kind, *cfg, dtype)
        assert case["own"].dtype == dtype and case["own"].shape == (B, No, D) and case["oth"].shape == (B, Ns, D)
        if B > 1:
            assert not torch.equal(case["oth"][0], case["oth"][1]) and not torch.equal(case["sbias"][0], case["sbias"][1])
        for v in C.ARG_VARIANTS:
            ref = C.ref_argmax(case, v)
            if kind == "rand":
                assert float((ref["gap"] <= ref["bound_pair"]).double().mean()) <= C.MAX_BELOW_MARGIN
                continue
            assert float(ref["gap"].min()) >= C.GAP > float(ref["bound_pair"].max()), (kind, v)
            assert torch.equal(ref["idx"], ref["X"].max(2).indices), "torch.max does not return the lowest index"
            if kind in ("planted", "ties", "first_dominates", "late_spike"):
                assert torch.equal(ref["idx"], case["win"])
            if kind == "ties":
                hi = case["tie_hi"]
                assert (ref["X"].gather(2, hi[..., None]).squeeze(2) == ref["val"]).all() and (hi > ref["idx"]).all()
        if kind == "ties":
            for lo, hi in C.tie_pairs(Ns):
                assert torch.equal(case["oth"][:, lo], case["oth"][:, hi])
                for k in ("sbias", "z", "nrm"):
                    assert torch.equal(case[k][:, lo], case[k][:, hi])
            assert set(case["win"].view(-1).tolist()) == {p[0] for p in C.tie_pairs(Ns)} or B * No < len(C.tie_pairs(Ns))
        if kind in ("first_dominates", "late_spike"):
            S = case["own"].double() @ case["oth"].double().transpose(1, 2)
            assert 85.0 < float(S.max()) < 105.0
            tile = C.ref_argmax(case, C.ARG_VARIANTS[0])["idx"] // C.TILE
            assert (tile == (0 if kind == "first_dominates" else (Ns - 1) // C.TILE)).all()
        if kind == "all_negative":
            S = case["own"].double() @ case["oth"].double().transpose(1, 2)
            assert float(S.max()) < -50.0 and (Ns == 1 or float(S.median()) < -85.0)     # (a single score is the winner's)
        if kind == "huge_bias":
            e = min(Ns, len(C.Z_EDGES))
            assert torch.equal(case["z"][:, :e], torch.tensor(C.Z_EDGES[:e]).expand(B, e))
        if kind == "planted":                                    # the special rows are winners: a dropped one shows in lse and arg-max
            sp = C.special_rows(Ns, False)[:B * No]
            assert case["win"].view(-1)[:len(sp)].tolist() == sp


def test_filter_case_has_every_category():
    arg0, arg1, max0, la = C.filter_case()
    B, M = arg0.shape
    N = arg1.shape[1]
    assert B == 2 and M != N
    for th in (0.0, 0.1):
        m0, m1, s0, s1, b0, b1 = C.ref_filter(arg0, arg1, max0, th)
        o0, o1, os0, os1 = filter_matches(la, th)
        assert torch.equal(m0, o0) and torch.equal(m1, o1)
        torch.testing.assert_close(s0, os0, rtol=1e-7, atol=0.0)       # (max0 is stored in fp32)
        torch.testing.assert_close(s1, os1, rtol=1e-7, atol=0.0)
        mutual = arg1.gather(1, arg0) == torch.arange(M)[None]
        assert (m0 >= 0).any() and (~mutual).any() and (mutual & (m0 < 0)).any()
        assert ((arg0.gather(1, arg1) != torch.arange(N)[None])).any()
        assert ((s0 - th).abs() > 10 * b0 + 1e-30)[mutual & torch.isfinite(max0)].all()
    assert max0[1, 0] == -math.inf and arg0[1, 0] == 0 and arg1[1, 0] == 0
    assert C.ref_filter(arg0, arg1, max0, 0.0)[0][1, 0] == -1
