"""The kernels of csrc/batchnorm.hip on their own (inputs, float64 references and bounds: tests/batchnorm_cases.py).

A. gf_bn_finalize_fwd / _bwd, gf_bn_pack_sums, gf_bn_finalize_sets_fwd / _bwd and the two replay kernels through the C ABI on
   stated partial sums, at every block count where bn_block_sums enters or leaves one of its three loop stages, at channel
   counts that end inside a block, and with two synthetic ranks whose packed buffers are added with torch.  Bounds: derived
   (batchnorm_cases: 64 x 2^-24 x sum |part| on a channel's sum, pushed through the float64 formulas).
B. ops.batch_norm_act_sets against a float64 torch.nn.BatchNorm1d called once per set.  Tolerances: `_tols(dtype)` of
   tests/test_gpu_kernels.py for y and the scaled dx; the statistic tolerances of test_batch_norm_act_at_benchmarked_row_counts
   for dgamma, dbeta and the running buffers (2e-5 of the reference's largest magnitude; bf16 dgamma / dbeta 4e-3).  The inputs
   keep every float64 pre-activation of a relu case GATE_MARGIN away from zero, so the gates must agree exactly.
Every test prints its worst error / bound ratio."""
import math

import pytest
import torch

import batchnorm_cases as cases
from batchnorm_cases import EPS, MOMENTUM, exact

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from glue_factory_amd import lib as L_
    from glue_factory_amd import ops
    from test_gpu_kernels import _tols

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
GF_ERR_UNSUPPORTED, GF_ERR_SHAPE = -1, -2                # include/gf_amd.h
GF_F32, GF_BF16 = 0, 1
GUARD = 256              # sentinel elements on either side of every output: a whole block of the widest kernel
SENTINEL = -776.0
NBLK = [1, 2, 8, 9, 16, 17, 24, 25, 56, 57, 64, 65, 72, 73, 120, 121, 128, 129, 511, 512]
NBLK_THIN = [1, 9, 57, 73, 512]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Worst:
    """Collects error / bound ratios, prints the worst of each name and fails if one exceeds 1."""

    def __init__(self, what):
        self.what, self.worst = what, {}

    def add(self, name, x, ref, bound):
        x, ref, bound = x.detach().cpu().double(), ref.detach().cpu().double(), bound.detach().cpu().double()
        assert x.shape == ref.shape == bound.shape, (name, x.shape, ref.shape, bound.shape)
        r = float(((x - ref).abs() / bound).max()) if bool(torch.isfinite(x).all()) else math.inf
        self.worst[name] = max(self.worst.get(name, 0.0), r)

    def pair(self, name, x, ref_and_bound):
        self.add(name, x, *ref_and_bound)

    def close(self, name, x, ref, rtol, atol, scaled=True):
        """torch.testing.assert_close's criterion |x - ref| <= atol + rtol |ref|, after dividing both by the reference's
        largest magnitude when `scaled`."""
        x, ref = x.detach().cpu().double(), ref.detach().cpu().double()
        sc = float(ref.abs().max()) if scaled else 1.0
        self.add(name, x / sc, ref / sc, atol + rtol * (ref / sc).abs())

    def finish(self):
        print(f"{self.what}: worst error/bound " + ", ".join(f"{k} {v:.3g}" for k, v in self.worst.items()))
        bad = {k: v for k, v in self.worst.items() if not v <= 1.0}
        assert not bad, f"{self.what}: over the bound (error / bound): {bad}"


class _Guarded:
    """`rows` fp32 vectors of `width` elements on the device, each between GUARD sentinel elements on either side."""

    def __init__(self, rows, width, init=None):
        self.width = width
        self.buf = torch.full((rows, GUARD + width + GUARD), SENTINEL, device=DEV)
        if init is not None:
            self.inner.copy_(init)

    @property
    def inner(self):
        return self.buf[:, GUARD:GUARD + self.width]

    def ptr(self, row=0):
        return self.buf[row, GUARD:].data_ptr()

    def intact(self):
        return bool((self.buf[:, :GUARD] == SENTINEL).all()) and bool((self.buf[:, GUARD + self.width:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def _padded(t):
    """t (fp32, CPU) at the start of a longer zero-filled device buffer: its data_ptr() is the kernel argument."""
    buf = torch.zeros(t.numel() + 2 * GUARD, device=DEV)
    buf[:t.numel()] = t.flatten().to(DEV)
    return buf


def _running_init(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)])


# ------------------------------------------------------------------------------------------- A. the C ABI on stated partials
@pytest.mark.parametrize("C", [8, 40, 300])
def test_finalize_fwd_over_every_loop_stage(C):
    """gf_bn_finalize_fwd on part [nblk, 2, C]: mean, biased variance, rstd and the running update against the float64 sums,
    with running buffers and with both NULL; n = 1 keeps the unbiased factor at 1; nothing outside [0, C) is written."""
    L, st, worst = L_.load(), _stream(), _Worst(f"finalize_fwd C={C}")
    run0 = _running_init(C, C)
    for nblk in NBLK:
        part = cases.synthetic_part(nblk, C, 1000 * nblk + C, variance_like=True)
        s, B = cases.sum_bound(part)
        dpart = _padded(part)
        for n in [2.0 * nblk] + ([1.0] if nblk == 1 else []):
            mean, var, rstd = cases.forward_stats(s, B, n)
            for running in (True, False):
                out = _Guarded(5, C)
                out.inner[3:].copy_(run0)
                rc = L.gf_bn_finalize_fwd(dpart.data_ptr(), nblk, C, n, EPS, MOMENTUM, out.ptr(0), out.ptr(1), out.ptr(2),
                                          out.ptr(3) if running else None, out.ptr(4) if running else None, st)
                assert rc == 0, (nblk, n, running, rc)
                got = out.inner.cpu()
                assert out.intact(), (nblk, n, running)
                for name, x, rb in (("mean", got[0], mean), ("var", got[1], var), ("rstd", got[2], rstd)):
                    worst.pair(name, x, rb)
                if running:
                    rm, rv = cases.running_update(exact(run0[0].double()), exact(run0[1].double()), mean, var, n, MOMENTUM)
                    worst.pair("running_mean", got[3], rm)
                    worst.pair("running_var", got[4], rv)
                else:
                    assert torch.equal(got[3:], run0), (nblk, n)
    worst.finish()


@pytest.mark.parametrize("C", [8, 40, 300])
def test_finalize_bwd_over_every_loop_stage(C):
    """gf_bn_finalize_bwd: dbeta / dgamma are the sums, m1 / m2 the sums times fl(1 / n) (two roundings)."""
    L, st, worst = L_.load(), _stream(), _Worst(f"finalize_bwd C={C}")
    for nblk in NBLK:
        part = cases.synthetic_part(nblk, C, 2000 * nblk + C)
        s, B = cases.sum_bound(part)
        dpart = _padded(part)
        n = 2.0 * nblk + 1.0
        out = _Guarded(4, C)
        rc = L.gf_bn_finalize_bwd(dpart.data_ptr(), nblk, C, n, out.ptr(0), out.ptr(1), out.ptr(2), out.ptr(3), st)
        assert rc == 0, (nblk, rc)
        got = out.inner.cpu()
        assert out.intact(), nblk
        worst.add("dbeta", got[0], s[0], B[0])
        worst.add("dgamma", got[1], s[1], B[1])
        worst.add("m1", got[2], s[0] / n, B[0] / n + 2 * cases.U * (s[0] / n).abs())
        worst.add("m2", got[3], s[1] / n, B[1] / n + 2 * cases.U * (s[1] / n).abs())
    worst.finish()


@pytest.mark.parametrize("with_local", [True, False])
@pytest.mark.parametrize("C", [40, 300])
def test_pack_sums(C, with_local):
    """gf_bn_pack_sums on three sets: [sets][2][C] sums, then the row count once per set; `local` takes the same sums."""
    L, st, worst, sets = L_.load(), _stream(), _Worst(f"pack_sums C={C} local={with_local}"), 3
    for nblk in NBLK_THIN:
        part = cases.synthetic_part(nblk, C, 3000 * nblk + C, sets=sets)
        dpart = _padded(part)
        n_local = 1.0 + nblk
        packed, local = _Guarded(1, sets * 2 * C + sets), _Guarded(1, sets * 2 * C)
        rc = L.gf_bn_pack_sums(dpart.data_ptr(), sets, nblk, C, n_local, packed.ptr(), local.ptr() if with_local else None, st)
        assert rc == 0, (nblk, rc)
        got = packed.inner[0].cpu()
        assert packed.intact(), nblk
        for h in range(sets):
            s, B = cases.sum_bound(part[h])
            worst.add("sums", got[2 * h * C:(2 * h + 2) * C].view(2, C), s, B)
        assert got[sets * 2 * C:].tolist() == [n_local] * sets, nblk
        if with_local:
            assert local.intact() and torch.equal(local.inner[0].cpu(), got[:sets * 2 * C]), nblk
        else:
            assert local.untouched(), nblk
    worst.finish()


RANK_ROWS = ((288, 1, 1), (96, 5, 0))            # rows of each set on rank 0 / rank 1: the reduced counts are 384, 6 and 1


@pytest.mark.parametrize("C", [40, 300])
def test_two_synthetic_ranks_through_the_exchange_kernels(C):
    """What _BatchNormActSetsSync does around its all-reduce, in one process: every rank packs the block sums of its rows with
    its row count (gf_bn_pack_sums), torch adds the ranks' buffers, gf_bn_finalize_sets_fwd / _bwd read the sum.  Reference:
    the float64 statistics of the concatenated rows (rows on a 1 / 32 grid: their fp32 partial sums are exact).  The sets have
    different reduced counts; the one with a single row keeps n / max(n - 1, 1) = 1."""
    L, st, worst, sets, nblk = L_.load(), _stream(), _Worst(f"two ranks C={C}"), 3, 3
    x = [[cases.quantised_rows(n, C, 100 * r + h) for h, n in enumerate(rows)] for r, rows in enumerate(RANK_ROWS)]
    d = [[(cases.quantised_rows(n, C, 300 * r + h + 50, spread=False), cases.quantised_rows(n, C, 500 * r + h + 70, spread=False))
          for h, n in enumerate(rows)] for r, rows in enumerate(RANK_ROWS)]

    def exchange(part_of, counted):
        """-> the reduced buffer [sets][2][C] + [sets] counts, float64 sums [sets, 2, C] and their bounds."""
        reduced, sums, bounds = [], [], []
        for h in range(sets):
            acc, s, b = None, 0.0, 0.0
            for r in range(2):
                part = part_of(r, h)
                dpart, packed = _padded(part), _Guarded(1, 2 * C + 1)
                rc = L.gf_bn_pack_sums(dpart.data_ptr(), 1, nblk, C, float(RANK_ROWS[r][h]) if counted else 0.0, packed.ptr(),
                                       None, st)
                assert rc == 0 and packed.intact(), (r, h, rc)
                acc = packed.inner[0].clone() if acc is None else acc + packed.inner[0]        # the all-reduce
                s, b = s + part.double().sum(0), b + 64 * cases.U * part.double().abs().sum(0)
            reduced.append(acc)
            sums.append(s)
            bounds.append(b + cases.U * s.abs())                                                # (the addition above)
        buf = torch.cat([r[:2 * C] for r in reduced] + [r[2 * C:] for r in reduced]).contiguous()
        return buf, torch.stack(sums), torch.stack(bounds)

    fwd, s, B = exchange(lambda r, h: cases.part_of_rows(x[r][h], x[r][h] ** 2, nblk), True)
    n = [float(RANK_ROWS[0][h] + RANK_ROWS[1][h]) for h in range(sets)]
    assert fwd[sets * 2 * C:].tolist() == n == [384.0, 6.0, 1.0]
    stats = []
    for h in range(sets):
        rows = torch.cat([x[0][h], x[1][h]])
        assert torch.equal(s[h], torch.stack([rows.sum(0), (rows ** 2).sum(0)]))               # the concatenated rows' own sums
        stats.append(cases.forward_stats(s[h], B[h], n[h]))
    run0 = _running_init(C, C + 1)
    for momentum in (MOMENTUM, 1.0):
        for running in (True, False):
            mvr, run = _Guarded(1, sets * 3 * C), _Guarded(2, C, run0)
            rc = L.gf_bn_finalize_sets_fwd(fwd.data_ptr(), sets, C, EPS, momentum, mvr.ptr(), run.ptr(0) if running else None,
                                           run.ptr(1) if running else None, st)
            assert rc == 0, (momentum, running, rc)
            got, got_run = mvr.inner[0].cpu().view(sets, 3, C), run.inner.cpu()
            assert mvr.intact() and run.intact(), (momentum, running)
            rm, rv = exact(run0[0].double()), exact(run0[1].double())
            for h in range(sets):
                for i, name in enumerate(("mean", "var", "rstd")):
                    worst.pair(name, got[h, i], stats[h][i])
                rm, rv = cases.running_update(rm, rv, stats[h][0], stats[h][1], n[h], momentum)
            if running:
                worst.pair("running_mean", got_run[0], rm)
                worst.pair("running_var", got_run[1], rv)
            else:
                assert torch.equal(got_run, run0), momentum

    bwd, s, B = exchange(lambda r, h: cases.part_of_rows(d[r][h][0], d[r][h][1], nblk), False)
    m12 = _Guarded(1, sets * 2 * C)
    rc = L.gf_bn_finalize_sets_bwd(bwd.data_ptr(), fwd[sets * 2 * C:].data_ptr(), sets, C, m12.ptr(), st)
    assert rc == 0, rc
    got = m12.inner[0].cpu().view(sets, 2, C)
    assert m12.intact()
    for h in range(sets):
        rows = [torch.cat([d[0][h][i], d[1][h][i]]) for i in range(2)]
        m = torch.stack([rows[0].sum(0), rows[1].sum(0)]) / n[h]
        worst.add("m12", got[h], m, B[h] / n[h] + 2 * cases.U * m.abs())                        # fl(1 / n), one product
    worst.finish()


@pytest.mark.parametrize("C", [40, 300])
@pytest.mark.parametrize("sets", [1, 2, 3])
def test_replay_kernels_and_their_skip_flag(sets, C):
    """gf_bn_replay_running / _n against the float64 recurrence, set after set; a skip flag of 1.0 or NaN leaves both buffers
    bit for bit, NULL and 0.0 replay; with every count equal to n the two kernels agree bit for bit."""
    L, st, worst = L_.load(), _stream(), _Worst(f"replay sets={sets} C={C}")
    g = torch.Generator().manual_seed(10 * sets + C)
    mvr = torch.randn(sets, 3, C, generator=g)
    mvr[:, 1] = 0.2 + torch.rand(sets, C, generator=g)
    mvr[:, 2] = torch.rsqrt(mvr[:, 1] + EPS)
    run0, dmvr = _running_init(C, C + 2), _padded(mvr)
    for flag in (None, 0.0, 1.0, float("nan")):
        skip = None if flag is None else torch.tensor(flag, device=DEV)
        skips = flag is not None and not flag == 0.0
        sp = None if skip is None else skip.data_ptr()

        def check(run, counts):
            got = run.inner.cpu()
            assert run.intact(), (flag, counts)
            if skips:
                assert torch.equal(got, run0), (flag, counts)
            else:
                rm, rv = cases.replay_reference(run0[0], run0[1], mvr, counts, MOMENTUM)
                worst.pair("running_mean", got[0], rm)
                worst.pair("running_var", got[1], rv)
            return got

        for n in (7.0, 1.0):
            plain, by_count = _Guarded(2, C, run0), _Guarded(2, C, run0)
            counts = torch.full((sets,), n, device=DEV)
            rc = L.gf_bn_replay_running(dmvr.data_ptr(), sets, C, n, MOMENTUM, plain.ptr(0), plain.ptr(1), sp, st)
            assert rc == 0, (flag, n, rc)
            rc = L.gf_bn_replay_running_n(dmvr.data_ptr(), counts.data_ptr(), sets, C, MOMENTUM, by_count.ptr(0), by_count.ptr(1), sp, st)
            assert rc == 0, (flag, n, rc)
            assert torch.equal(check(plain, [n] * sets), check(by_count, [n] * sets)), (flag, n)
        mixed = [384.0, 6.0, 1.0][:sets]
        counts, by_count = torch.tensor(mixed, device=DEV), _Guarded(2, C, run0)
        rc = L.gf_bn_replay_running_n(dmvr.data_ptr(), counts.data_ptr(), sets, C, MOMENTUM, by_count.ptr(0), by_count.ptr(1), sp, st)
        assert rc == 0, (flag, rc)
        check(by_count, mixed)
    worst.finish()


def test_rejected_calls_launch_nothing():
    """C % VEC != 0 and C / VEC > 256 in gf_bn_stats (GF_ERR_UNSUPPORTED); sets = 0, exactly one running buffer NULL and n = 0
    (GF_ERR_SHAPE): the code comes back and no output element changes."""
    L, st, C = L_.load(), _stream(), 40
    src = torch.ones(64 * 2056, device=DEV)                    # every input below, in either dtype
    out = [_Guarded(1, 2 * 2056) for _ in range(5)]
    i, o = src.data_ptr(), [t.ptr() for t in out]
    for c, dt in ((36, GF_BF16), (34, GF_F32), (1028, GF_F32), (2056, GF_BF16)):
        assert L.gf_bn_stats(i, o[0], 64, c, dt, st) == GF_ERR_UNSUPPORTED, (c, dt)
    assert L.gf_bn_pack_sums(i, 0, 1, C, 1.0, o[0], o[1], st) == GF_ERR_SHAPE
    assert L.gf_bn_finalize_sets_fwd(i, 0, C, EPS, MOMENTUM, o[0], o[1], o[2], st) == GF_ERR_SHAPE
    assert L.gf_bn_finalize_sets_bwd(i, i, 0, C, o[0], st) == GF_ERR_SHAPE
    assert L.gf_bn_replay_running(i, 0, C, 7.0, MOMENTUM, o[0], o[1], None, st) == GF_ERR_SHAPE
    assert L.gf_bn_replay_running_n(i, i, 0, C, MOMENTUM, o[0], o[1], None, st) == GF_ERR_SHAPE
    assert L.gf_bn_finalize_fwd(i, 1, C, 2.0, EPS, MOMENTUM, o[0], o[1], o[2], o[3], None, st) == GF_ERR_SHAPE
    assert L.gf_bn_finalize_fwd(i, 1, C, 2.0, EPS, MOMENTUM, o[0], o[1], o[2], None, o[4], st) == GF_ERR_SHAPE
    assert L.gf_bn_finalize_sets_fwd(i, 1, C, EPS, MOMENTUM, o[0], o[1], None, st) == GF_ERR_SHAPE
    assert L.gf_bn_finalize_sets_fwd(i, 1, C, EPS, MOMENTUM, o[0], None, o[2], st) == GF_ERR_SHAPE
    assert L.gf_bn_finalize_fwd(i, 1, C, 0.0, EPS, MOMENTUM, o[0], o[1], o[2], o[3], o[4], st) == GF_ERR_SHAPE
    torch.cuda.synchronize()
    assert all(t.untouched() for t in out)


# -------------------------------------------------------------------- B. ops.batch_norm_act_sets against float64 BatchNorm1d
SETS_CASES = [(1, 333, 32, 32),          # the H = 1 dgamma branch
              (2, 2100, 96, 48),         # nblk = 9; 256 is no multiple of the 24 / 6 chunks of a row
              (3, 18500, 32, 32),        # nblk = 73: all three loop stages; the buffers chained over three sets
              (2, 30800, 32, 32),        # nblk = 121
              (2, 300, 1024, 2048),      # 256 chunks per row: one row lane
              (2, 5, 32, 32)]            # fewer rows than rows in flight: every load of a thread but one is clamped
STAT_TOL = 2e-5                          # test_batch_norm_act_at_benchmarked_row_counts: statistics, of the largest magnitude
STAT_TOL_BF16_GRADS = 4e-3               # the same test's dgamma / dbeta in bf16


def _module(case, training=True):
    bn = torch.nn.BatchNorm1d(case["x"].shape[-1], momentum=0.1).to(DEV)
    bn.load_state_dict(case["state"])
    return bn.train(training)


def _check_gate_precondition(case, relu):
    assert not relu or case["gate_distance"] >= cases.GATE_MARGIN, case["gate_distance"]


def _check_forward(worst, case, y, bn, relu):
    dtype = case["x"].dtype
    worst.close("y", y, case["y"], scaled=False, **_tols(dtype))
    if relu:
        assert torch.equal(y.detach().cpu() > 0, case["y"] > 0), "the ReLU gates differ"
    worst.close("running_mean fwd", bn.running_mean, case["rm_fwd"], STAT_TOL, STAT_TOL)
    worst.close("running_var fwd", bn.running_var, case["rv_fwd"], STAT_TOL, STAT_TOL)


def _check_backward(worst, case, xs, bn):
    dtype = case["x"].dtype
    worst.close("dx", xs.grad, case["dx"], **_tols(dtype))
    grad_tol = STAT_TOL if dtype == torch.float32 else STAT_TOL_BF16_GRADS
    worst.close("dgamma", bn.weight.grad, case["dgamma"], grad_tol, grad_tol)
    worst.close("dbeta", bn.bias.grad, case["dbeta"], grad_tol, grad_tol)


def _check_buffers(worst, case, bn, replayed):
    H, tag = case["x"].shape[0], "replayed" if replayed else "fwd"
    worst.close("running_mean end", bn.running_mean, case["rm_" + tag], STAT_TOL, STAT_TOL)
    worst.close("running_var end", bn.running_var, case["rv_" + tag], STAT_TOL, STAT_TOL)
    assert int(bn.num_batches_tracked) == (2 * H if replayed else H)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,M,C32,C16", SETS_CASES)
def test_batch_norm_act_sets(H, M, C32, C16, dtype, relu):
    """y, the chained running buffers after the forward, dx / dgamma / dbeta, and buffers and counter after the backward,
    without and with the replayed update."""
    C = C32 if dtype == torch.float32 else C16
    case = cases.sets_case(dtype, H, M, C, relu)
    _check_gate_precondition(case, relu)
    worst = _Worst(f"sets {H}x{M}x{C} {dtype} relu={relu}")
    for replay in (False, True):
        bn = _module(case)
        xs = case["x"].to(DEV).requires_grad_(True)
        y = ops.batch_norm_act_sets(xs, bn, relu, replay=replay)
        assert int(bn.num_batches_tracked) == H
        _check_forward(worst, case, y, bn, relu)
        y.backward(case["dy"].to(DEV))
        _check_backward(worst, case, xs, bn)
        _check_buffers(worst, case, bn, replay)
    worst.finish()


@pytest.mark.parametrize("flag", [0.0, 1.0, float("nan")])
def test_replay_gate_values(flag, monkeypatch):
    """ops.REPLAY_GATE around the backward of a replaying call: 0.0 replays (buffers and counter as the replayed reference),
    1.0 and NaN leave the buffers bit for bit as the forward left them and the counter at H."""
    H, M, C = 3, 18500, 32
    case = cases.sets_case(torch.float32, H, M, C, True)
    _check_gate_precondition(case, True)
    worst = _Worst(f"replay gate {flag}")
    bn = _module(case)
    xs = case["x"].to(DEV).requires_grad_(True)
    y = ops.batch_norm_act_sets(xs, bn, True, replay=True)
    _check_forward(worst, case, y, bn, True)
    after_fwd = bn.running_mean.clone(), bn.running_var.clone()
    monkeypatch.setattr(ops, "REPLAY_GATE", torch.tensor(flag, device=DEV))
    y.backward(case["dy"].to(DEV))
    _check_backward(worst, case, xs, bn)
    if flag == 0.0:
        _check_buffers(worst, case, bn, True)
    else:
        assert torch.equal(bn.running_mean, after_fwd[0]) and torch.equal(bn.running_var, after_fwd[1])
        assert int(bn.num_batches_tracked) == H
    worst.finish()


def test_stats_out_route_replays_like_the_node():
    """stats_out=[] collects (module, [(mean, unbiased var) per set]); ops.replay_running_stats attaches the replay: buffers
    and counter as replay=True gives them."""
    H, M, C = 2, 2100, 96
    case = cases.sets_case(torch.float32, H, M, C, True)
    _check_gate_precondition(case, True)
    worst, ends = _Worst("stats_out route"), []
    for route in ("stats_out", "replay"):
        bn = _module(case)
        xs = case["x"].to(DEV).requires_grad_(True)
        if route == "stats_out":
            stats = []
            y = ops.batch_norm_act_sets(xs, bn, True, stats_out=stats)
            assert len(stats) == 1 and stats[0][0] is bn and len(stats[0][1]) == H
            _check_forward(worst, case, y, bn, True)
            y = ops.replay_running_stats(y, stats)
        else:
            y = ops.batch_norm_act_sets(xs, bn, True, replay=True)
        y.backward(case["dy"].to(DEV))
        _check_backward(worst, case, xs, bn)
        _check_buffers(worst, case, bn, True)
        ends.append((bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)))
    worst.close("running_mean, route against node", ends[0][0], ends[1][0], STAT_TOL, STAT_TOL)
    worst.close("running_var, route against node", ends[0][1], ends[1][1], STAT_TOL, STAT_TOL)
    assert ends[0][2] == ends[1][2] == 2 * H
    worst.finish()


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_norm_act_sets_in_eval_mode(dtype):
    """bn.eval(): the stacked ops.batch_norm_act route with the running statistics; y, dx, dgamma and dbeta against float64,
    buffers and counter untouched (also with replay requested)."""
    H, M, C = 2, 2100, 96 if dtype == torch.float32 else 48
    case = cases.sets_case(dtype, H, M, C, True, False)
    _check_gate_precondition(case, True)
    worst = _Worst(f"eval {dtype}")
    bn = _module(case, training=False)
    xs = case["x"].to(DEV).requires_grad_(True)
    y = ops.batch_norm_act_sets(xs, bn, True, replay=True)
    worst.close("y", y, case["y"], scaled=False, **_tols(dtype))
    assert torch.equal(y.detach().cpu() > 0, case["y"] > 0), "the ReLU gates differ"
    y.backward(case["dy"].to(DEV))
    _check_backward(worst, case, xs, bn)
    assert torch.equal(bn.running_mean.cpu(), case["state"]["running_mean"])
    assert torch.equal(bn.running_var.cpu(), case["state"]["running_var"])
    assert int(bn.num_batches_tracked) == 0
    worst.finish()
