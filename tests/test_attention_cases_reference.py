"""The inputs of tests/test_gpu_attention_edges.py discriminate (CPU, no library code): for every shape, case and kernel
setting the GPU module runs, each mutation of the fp64 reference -- a dropped key, a dropped or doubled query row, one row's
lse off by ln 2 (tests/attention_cases.py) -- moves at least one of o, dq, dk, dv by 5 times the bound the GPU test allows,
`max(3 * row_error(rounding_model, reference), 4e-3)`.  A condition on the INPUTS: where it fails, the case has to change."""
import math

import pytest
import torch

import attention_cases as ac


def _check(what, ref, model, muts, names=ac.TENSORS):
    bd = {n: max(ac.FACTOR * ac.row_error(model[n], ref[n]), ac.FLOOR) for n in names}
    for n in names:
        assert torch.isfinite(ref[n]).all() and torch.isfinite(model[n]).all(), (what, n)
    worst = {}
    for name, mut in muts.items():
        worst[name] = max(ac.row_error(mut[n], ref[n]) / bd[n] for n in names)
    print(f"{what}: bounds " + ", ".join(f"{n} {bd[n]:.2e}" for n in names) + "; mutation / bound " +
          ", ".join(f"{k} {v:.1f}" for k, v in worst.items()))
    weak = {k: v for k, v in worst.items() if not v >= ac.DETECT}
    assert not weak, f"{what}: mutations closer than {ac.DETECT} bounds to the reference: {weak}"


def _attention(case, Nq, Nk, D, pre, split, b=ac.B):
    q, k, v, do, sc = ac.make_case(case, Nq, Nk, D, pre, b=b)
    for t in (q, k, v, do):
        assert torch.equal(ac.bf(t), t)
    _check(f"{case} {Nq}x{Nk} D={D} pre={pre} split={split}", ac.reference(q, k, v, do, sc),
           ac.rounding_model(q, k, v, do, sc, split), ac.mutations(q, k, v, do, sc))


@pytest.mark.parametrize("case", ac.BASIC)
@pytest.mark.parametrize("Nq,Nk", ac.SHAPES_D64 + ac.SHAPES_ACC)
def test_basic_cases_at_head_dim_64(case, Nq, Nk):
    for pre in (False, True):
        for split in (False, True):
            _attention(case, Nq, Nk, 64, pre, split)
    if (Nq, Nk) == (65, 65):
        _attention(case, Nq, Nk, 64, False, False, b=1)       # the register-staged arm runs one image


@pytest.mark.parametrize("case", ac.HARD)
def test_hard_cases(case):
    for pre in (False, True):
        for split in (False, True):
            _attention(case, ac.HARD_N, ac.HARD_N, 64, pre, split)


@pytest.mark.parametrize("case", ac.BASIC)
@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("Nq,Nk", ac.SHAPES_GENERIC)
def test_basic_cases_at_head_dim_32_and_128(case, D, Nq, Nk):
    _attention(case, Nq, Nk, D, False, False)


@pytest.mark.parametrize("case", ["last_key", "last_query"])
@pytest.mark.parametrize("N,h", [(n, h) for n in ac.CROSS_N for h in ac.CROSS_H] + ac.CROSS_TWO_LAUNCH)
def test_cross_cases(case, N, h):
    for b2 in ac.CROSS_B2:
        for pre in (False, True):
            p, dm, sc = ac.cross_case(case, N, h, b2, pre)
            ref = ac.cross_reference(p, dm, sc)
            model = ac.cross_model(p, dm, sc)
            muts = {n: ac.cross_reference(p, dm, sc, **kw) for n, kw in ac.mutation_kwargs(N, N).items()}
            _check(f"cross {case} N={N} H={h} 2B={b2} pre={pre}", ref, model, muts, names=("o", "dqk", "dv"))


def test_metric_and_model_properties():
    """row_error sees one wrong row next to large ones and measures a zero row against the tensor's scale; the split model is
    closer to the reference than the plain one; the closed-form gradients are autograd's."""
    r = torch.ones(1, 4, 1, 8, dtype=torch.float64)
    r[0, 0] *= 1000.0
    r[0, 3] = 0.0
    a = r.clone()
    a[0, 1, 0, 0] += 1.0
    rms = math.sqrt((8e6 + 8 + 8) / 4)
    assert ac.row_error(a, r) == pytest.approx(1.0 / (math.sqrt(8) + rms))
    a = r.clone()
    a[0, 3, 0, 0] = 1.0
    assert ac.row_error(a, r) == pytest.approx(1.0 / rms)
    a[0, 2, 0, 0] = math.nan
    assert ac.row_error(a, r) == math.inf

    q, k, v, do, sc = ac.make_case("rand", 65, 129)
    ref = ac.reference(q, k, v, do, sc)
    plain, split = (ac.rounding_model(q, k, v, do, sc, s) for s in (False, True))
    for n in ("dq", "dk"):
        assert ac.row_error(split[n], ref[n]) < ac.row_error(plain[n], ref[n])
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", qa, ka) * sc
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), va)
    (o * do).sum().backward()
    torch.testing.assert_close(ref["o"], o.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["lse"], torch.logsumexp(s, -1).detach(), rtol=1e-12, atol=1e-12)
    for n, t in (("dq", qa), ("dk", ka), ("dv", va)):
        torch.testing.assert_close(ref[n], t.grad, rtol=1e-11, atol=1e-11)
