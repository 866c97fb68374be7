"""CPU checks of the references and inputs of tests/test_gpu_lg_loss.py (tests/lg_loss_cases.py): the references agree with
the oracle's loss and with each other, and every case keeps the conditions the GPU tests rely on -- decisive arg-maxes,
both branches of the target taken about equally often, a COO list with duplicates and a column named several times.
These are conditions on the INPUTS; nothing on the GPU side skips or masks a row."""
import pytest
import torch
import torch.nn.functional as F

import lg_loss_cases as C
from oracle import lightglue_oracle as lgo

DTYPES = [torch.float32, torch.bfloat16]


def _leaves(case):
    return [case[k].double().requires_grad_(True) for k in ("md0", "md1", "z0", "z1", "t0", "t1")]


def _dense(case, pos, leaves):
    return C.reference_dense(*leaves, pos, case["neg0"], case["neg1"], case["fin0"], case["fin1"])


def _final_with_rows(fin, n_cols):
    """A log assignment [B, n+1, n_cols+1] whose rows 0..n-1 have their arg-max (incl. dustbin) at `fin`."""
    B, n = fin.shape
    la = torch.full((B, n + 1, n_cols + 1), -1000.0, dtype=torch.float64)
    la[:, :n].scatter_(2, fin[..., None], 0.0)
    return la


def test_reference_dense_equals_oracle_nll_and_token_confidence():
    """acc composed as LightGlue._loss_fused composes it (/ num_pos, / (n0 + n1), / 2n) == oracle nll and
    token_confidence_loss on the dense ground truth of the `fixed` list, to 1e-12 relative.  One log assignment cannot
    in general have a prescribed arg-max in every row AND every column, so the final one is built twice: with the case's
    fin0 in its rows (its columns then give that run's fin1), and transposed for fin1."""
    B, N, D = C.OPS_CASES[0]
    case = C.planted_case(B, N, D, torch.float32)
    pos = C.positives(case, "fixed")
    match = case["match"]
    gt = torch.zeros(B, N, N, dtype=torch.bool)
    bi, ii = (match >= 0).nonzero(as_tuple=True)
    gt[bi, ii, match[bi, ii]] = True
    gt_m1 = torch.full((B, N), -1, dtype=torch.int64)
    gt_m1[bi, match[bi, ii]] = ii
    leaves = _leaves(case)
    S = leaves[0] @ leaves[1].transpose(1, 2)
    la = lgo.log_double_softmax(S, leaves[2], leaves[3])
    _, stats = lgo.nll(la, gt, match, gt_m1)
    p = {"token_confidence.0.token.0.weight": torch.ones(1, 1, dtype=torch.float64),
         "token_confidence.0.token.0.bias": torch.zeros(1, dtype=torch.float64)}
    rel = dict(rtol=1e-12, atol=0.0)
    for side in (0, 1):
        if side == 0:
            final = _final_with_rows(case["fin0"], N)
        else:
            final = _final_with_rows(case["fin1"], N).transpose(1, 2).contiguous()
        fin0, fin1 = final[:, :-1, :].argmax(-1), final[:, :, :-1].argmax(-2)
        assert torch.equal((fin0, fin1)[side], case["fin" + str(side)])
        ref = C.reference_dense(*leaves, pos, case["neg0"], case["neg1"], fin0, fin1)
        acc = ref["acc"]
        num_pos = gt.sum((1, 2)).clamp(min=1).double()
        n0, n1 = (match < 0).sum(1).clamp(min=1).double(), (gt_m1 < 0).sum(1).clamp(min=1).double()
        torch.testing.assert_close(-acc[:, 0] / num_pos, stats["nll_pos"], **rel)
        torch.testing.assert_close(-acc[:, 1] / (n0 + n1), stats["nll_neg"], **rel)
        conf = lgo.token_confidence_loss(p, 0, leaves[4][..., None], leaves[5][..., None], la, final)
        torch.testing.assert_close((acc[:, 2] + acc[:, 3]) / (2.0 * N), conf, **rel)
        assert 0.3 < float(ref["tgt" + str(side)].mean()) < 0.7


@pytest.mark.parametrize("kind", ["fixed", "coo"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_stats_equals_reference_dense(dtype, kind):
    """reference_stats on the exact float64 r, c, v, a of a case == reference_dense: sums, targets, the closed-form dz and
    dt against autograd, and sparse terms + dense double-softmax part (dS = P_row gr + P_col gc) == autograd's d(md)."""
    B, N, D = C.OPS_CASES[0]
    case = C.planted_case(B, N, D, dtype)
    pos = C.positives(case, kind)
    leaves = _leaves(case)
    ref = _dense(case, pos, leaves)
    gacc = case["gacc"].double()
    (ref["acc"] * gacc).sum().backward()
    st = C.dense_stats(case["md0"], case["md1"], case["z0"], case["z1"])
    out = C.reference_stats(case["md0"], case["md1"], case["z0"], case["z1"], case["t0"], case["t1"], pos, case["neg0"],
                            case["neg1"], case["fin0"], case["fin1"], st["r"], st["c"], st["v0"], st["a0"], st["v1"], st["a1"],
                            gacc)
    tol = dict(rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(out["acc"], ref["acc"].detach(), **tol)
    assert torch.equal(out["tgt0"], ref["tgt0"]) and torch.equal(out["tgt1"], ref["tgt1"])
    assert torch.equal(out["full0"], ref["full0"]) and torch.equal(out["full1"], ref["full1"])
    assert (out["T_acc"] >= out["acc"].abs() * (1 - 1e-12)).all()
    for name, leaf in (("dz0", leaves[2]), ("dz1", leaves[3]), ("dt0", leaves[4]), ("dt1", leaves[5])):
        torch.testing.assert_close(out[name], leaf.grad, **tol)
        assert (out["T_" + name] >= out[name].abs() * (1 - 1e-12)).all()
    md0, md1 = case["md0"].double(), case["md1"].double()
    S = md0 @ md1.transpose(1, 2)
    dS = torch.softmax(S, 2) * out["gr"][:, :, None] + torch.softmax(S, 1) * out["gc"][:, None, :]
    torch.testing.assert_close(out["sp0"] + dS @ md1, leaves[0].grad, **tol)
    torch.testing.assert_close(out["sp1"] + dS.transpose(1, 2) @ md0, leaves[1].grad, **tol)
    if kind == "coo":
        assert out["hits0"].max() >= 2 and out["hits1"].max() >= 3


def _check_coo(pos, P):
    pb, pi, pj = pos
    assert pb.shape[0] == P and P % 4 != 0 and (pj >= 0).all()
    triples = list(zip(pb.tolist(), pi.tolist(), pj.tolist()))
    assert len(set(triples)) <= P - 5, "the list must name some pairs twice"
    cols = {}
    for b, _, j in triples:
        cols[(b, j)] = cols.get((b, j), 0) + 1
    assert max(cols.values()) >= 3, "one column of md1 must be named at least 3 times"
    assert (pb[1:] < pb[:-1]).any() or len(set(pb.tolist())) == 1, "the list must not be sorted by image"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,D", C.OPS_CASES)
def test_planted_cases_keep_their_conditions(B, N, D, dtype):
    case = C.planted_case(B, N, D, dtype)
    print(f"planted ({B},{N},{D}) {dtype}: seed {case['seed']}, min gap {min(float(case['gap0'].min()), float(case['gap1'].min())):.4f}")
    assert float(case["gap0"].min()) >= C.GAP and float(case["gap1"].min()) >= C.GAP
    for k in ("0", "1"):
        full, fin = case["full" + k], case["fin" + k]
        assert 0.3 < float((full == N).double().mean()) < 0.7, "dustbin share of the arg-maxes"
        tgt = full == fin
        assert 0.3 < float(tgt.double().mean()) < 0.7, "share of ones among the targets"
        assert (fin[tgt] == N).any() and (fin[~tgt] == N).any(), "dustbin on the agreeing and the disagreeing side"
        assert (fin[tgt] < N).any() and (fin[~tgt] < N).any()
        assert int(fin.min()) >= 0 and int(fin.max()) <= N
    fixed = C.positives(case, "fixed")
    assert fixed[0].shape[0] == B * N and (fixed[0][1:] >= fixed[0][:-1]).all()
    assert (fixed[2] < 0).any() and (fixed[2] >= 0).any()
    _check_coo(C.positives(case, "coo"), 157)
    last = C.positives(case, "last_image")
    assert (last[2][last[0] < B - 1] < 0).all() and (last[2][last[0] == B - 1] >= 0).any()
    assert (C.positives(case, "all_skipped")[2] < 0).all() and C.positives(case, "all_skipped")[2].shape[0] == B * N
    assert C.positives(case, "empty")[0].shape[0] == 0
    for kind in C.OPS_LISTS:                                  # every index in range: the kernels read where the list points
        pb, pi, pj = C.positives(case, kind)
        assert all(x.dtype == torch.int64 for x in (pb, pi, pj))
        if pb.numel():
            assert 0 <= int(pb.min()) and int(pb.max()) < B and 0 <= int(pi.min()) and int(pi.max()) < N and int(pj.max()) < N


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,M,N,D", C.ABI_CASES)
def test_abi_cases_keep_their_conditions(B, M, N, D, dtype):
    case = C.abi_case(B, M, N, D, dtype)
    assert case["md0"].shape == (B, M, D) and case["md1"].shape == (B, N, D) and case["md0"].dtype == dtype
    ones = []
    for kind in C.ABI_LISTS:
        pos = C.positives(case, kind)
        pb, pi, pj = pos
        if pb.numel():
            assert 0 <= int(pb.min()) and int(pb.max()) < B and 0 <= int(pi.min()) and int(pi.max()) < M and int(pj.max()) < N
        out = C.stats_of(case, pos)
        assert float(out["margin0"].min()) >= C.GAP and float(out["margin1"].min()) >= C.GAP
        ones += [out["tgt0"].reshape(-1), out["tgt1"].reshape(-1)]
        for k in ("acc", "dz0", "dz1", "dt0", "dt1", "gr", "gc", "sp0", "sp1"):
            assert torch.isfinite(out[k]).all()
    if M > 1:                                                  # (the one-token image has three targets in all)
        assert 0.3 < float(torch.cat(ones).mean()) < 0.7
    assert case["coo_P"] == C.abi_P(B, M, N) and case["coo_P"] <= 157 and case["coo_P"] <= B * M * N
    _check_coo(C.positives(case, "coo"), case["coo_P"])
    e = min(M, len(C.Z_EDGES))
    assert torch.equal(case["z0"][:, :e], torch.tensor(C.Z_EDGES[:e]).expand(B, e))
    assert torch.equal(case["z1"][:, :5], torch.tensor(C.Z_EDGES).expand(B, 5))
    for k in ("0", "1"):
        other = N if k == "0" else M
        assert int(case["a" + k].min()) >= 0 and int(case["a" + k].max()) < other
        assert int(case["fin" + k].min()) >= 0 and int(case["fin" + k].max()) <= other
    g = case["gacc"].double()
    assert (g != 0).all() and torch.equal(g * 64, (g * 64).round())
    assert F.logsigmoid(case["z0"].double()).isfinite().all()
