"""CPU side of tests/test_gpu_batchnorm.py: inputs, float64 references and the derived error bounds for the kernels of
csrc/batchnorm.hip.  Nothing here touches a GPU, so the input conditions can be checked wherever torch runs.

Part A (the finalize / pack / exchange / replay kernels on stated partial sums): every bound is DERIVED.  `U` = 2^-24 is the
relative rounding of one fp32 operation.  A channel's sum over the partial rows carries `sum_bound`; every derived quantity
carries that bound pushed through its float64 formula (first order, plus the product of two errors where one appears) and
`k U |value|` for the k fp32 operations the kernel spends on it.  Each function below returns (reference, bound) pairs.

Part B (ops.batch_norm_act_sets against a float64 torch.nn.BatchNorm1d): `sets_case` builds inputs whose float64
pre-activations stay clear of the ReLU gate and the reference results of every stage."""
import functools

import torch

U = 2.0 ** -24
GATE_MARGIN = 1e-4       # no reference pre-activation of a relu case is closer to 0 than this


def f32(v):
    """The value a C `float` argument takes."""
    return float(torch.tensor(v, dtype=torch.float32))


EPS, MOMENTUM = f32(1e-5), f32(0.1)


# ---------------------------------------------------------------------------------------------------------------- part A
def synthetic_part(nblk, C, seed, variance_like=False, sets=None):
    """fp32 part [nblk, 2, C] ([sets, nblk, 2, C]): row k has magnitude (1 + k / nblk) x [0.5, 1.5), one sign per statistic
    and channel -- a skipped or repeated row moves a channel's sum by at least 1 / (6 nblk) of it.  variance_like: the second
    statistic is positive and three times as large, so that s1 / n - (s0 / n)^2 is a variance."""
    g = torch.Generator().manual_seed(seed)
    lead = () if sets is None else (sets,)
    mag = (1 + torch.arange(nblk, dtype=torch.float64) / nblk)[:, None, None] * (0.5 + torch.rand(*lead, nblk, 2, C, generator=g,
                                                                                               dtype=torch.float64))
    sign = torch.where(torch.rand(*lead, 1, 2, C, generator=g) < 0.5, -1.0, 1.0).double()
    if variance_like:
        sign[..., 1, :] = 1.0
        mag[..., 1, :] *= 3.0
    return (mag * sign).float()


def sum_bound(part):
    """part [nblk, 2, C] fp32 -> (float64 sums [2, C], bound [2, C]).
    bn_block_sums: <= 32 serial adds in a chain, one a + b, 8 combines = 41 roundings of partial sums <= sum |part|; 64 covers it."""
    p = part.double()
    return p.sum(0), 64 * U * p.abs().sum(0)


def forward_stats(s, B, n, eps=EPS):
    """(mean, biased var, rstd) of sums s [2, C] +- B over n rows, each as (reference, bound).
    The variance s1 / n - m^2 is formed by cancellation, so its bound is at E[x^2] scale: B1 / n + 2 |m| em + em^2 from the inputs and
    4 U (E[x^2] + m^2) for the division, the square, the subtraction and a possible contraction; max(., 0) does not increase it."""
    m = s[0] / n
    em = B[0] / n + 2 * U * m.abs()                                   # the division (+ one spare)
    e2 = s[1] / n
    v = (e2 - m * m).clamp(min=0.0)
    ev = B[1] / n + 2 * m.abs() * em + em * em + 4 * U * (e2.abs() + m * m)
    rstd = torch.rsqrt(v + eps)
    lo, hi = torch.rsqrt((v - ev).clamp(min=0.0) + eps), torch.rsqrt(v + ev + eps)
    er = torch.maximum(lo - rstd, rstd - hi) + 6 * U * lo             # v + eps (half a U on the result), rsqrtf within 2 ulp = 4 U
    return (m, em), (v, ev), (rstd, er)


def unbias(n):
    return n / max(n - 1.0, 1.0)


def running_update(rm, rv, mean, var, n, momentum):
    """One running-statistics update, as torch.nn.BatchNorm1d applies it: rm, rv, mean, var are (value, bound) pairs.
    fp32 operations: 1 - momentum, two products, one sum (4 U); the variance also n / max(n - 1, 1) and one more product (6 U)."""
    keep = 1.0 - momentum
    out = []
    for (r, er), (x, ex), k, f in ((rm, mean, 4, 1.0), (rv, var, 6, unbias(n))):
        new = r * keep + x * f * momentum
        out.append((new, er * keep + ex * f * momentum + k * U * (r.abs() * keep + x.abs() * f * momentum)))
    return out


def exact(t):
    return t, torch.zeros_like(t)


def quantised_rows(n, C, seed, scale=0.7, spread=True):
    """[n, C] float64 rows on a 1 / 32 grid inside (-4, 4): sums of up to 1000 rows and of their squares are exact in fp32, so
    fp32 partial sums of them ARE the float64 statistics of the rows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g, dtype=torch.float64) * scale
    if spread:
        x = x + torch.linspace(-1.0, 2.0, C, dtype=torch.float64)
    return (x * 32).round().clamp(-127, 127) / 32


def part_of_rows(a, b, nblk):
    """fp32 part [nblk, 2, C] of the column sums of a and b [n, C] over nblk row chunks (empty chunks give zeros)."""
    part = torch.stack([torch.stack([ca.sum(0), cb.sum(0)]) for ca, cb in zip(torch.tensor_split(a, nblk), torch.tensor_split(b, nblk))])
    out = part.float()
    assert torch.equal(out.double(), part), "the partial sums must be exact in fp32"
    return out


def replay_reference(rm, rv, mvr, counts, momentum):
    """The float64 recurrence of the replay kernels, set after set: mvr [sets, 3, C], counts one row count per set."""
    rm, rv = exact(rm.double()), exact(rv.double())
    for h, n in enumerate(counts):
        rm, rv = running_update(rm, rv, exact(mvr[h, 0].double()), exact(mvr[h, 1].double()), float(n), momentum)
    return rm, rv


# ---------------------------------------------------------------------------------------------------------------- part B
def _pre_activation(x, w, b, training, rm, rv, eps):
    xd = x.double()
    if training:
        m, v = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    else:
        m, v = rm.double(), rv.double()
    rstd = torch.rsqrt(v + eps)
    return (xd - m) * rstd * w.double() + b.double()


def _clear_of_gate(x, w, b, training, rm, rv, eps):
    """x with the few elements whose float64 pre-activation lies within 2 GATE_MARGIN of zero moved away from it.
    (Reseeding alone cannot do this: at 10^6 elements about a hundred fall inside the band whatever the seed.  Moving them
    shifts the batch statistics by ~1e-6, hence the wider band here and the loop.)"""
    for _ in range(8):
        z = _pre_activation(x, w, b, training, rm, rv, eps)
        near = z.abs() < 2 * GATE_MARGIN
        if not bool(near.any()):
            return x
        away = torch.where(z < 0, -1.0, 1.0) * torch.where(w.double() < 0, -1.0, 1.0)
        x = torch.where(near, x.double() + 0.0625 * away, x.double()).to(x.dtype)      # (two bf16 steps at |x| in [4, 8))
    raise AssertionError("could not move the inputs clear of the ReLU gate")


@functools.lru_cache(maxsize=2)
def sets_case(dtype, H, M, C, relu, training=True):
    """Inputs (rounded to `dtype`) and the float64 torch.nn.BatchNorm1d results of ops.batch_norm_act_sets on x [H, M, C]:
    one module call per set in order, relu, backward of the stack with dy, and -- `replayed` -- one more call per set under
    no_grad.  Channel means span +-3 standard deviations.  The returned tensors are shared between tests: read only."""
    g = torch.Generator().manual_seed(1000 * H + M + C)
    x = (torch.randn(H, M, C, generator=g) * 0.7 + torch.linspace(-2.1, 2.1, C)).to(dtype)
    dy = torch.randn(H, M, C, generator=g).to(dtype)
    state = {"weight": 1 + 0.2 * torch.randn(C, generator=g), "bias": 0.2 * torch.randn(C, generator=g),
             "running_mean": 0.3 * torch.randn(C, generator=g), "running_var": 0.5 + torch.rand(C, generator=g),
             "num_batches_tracked": torch.tensor(0)}
    ref = torch.nn.BatchNorm1d(C, momentum=0.1).double()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in state.items()})
    ref.train(training)
    if relu:
        x = _clear_of_gate(x, state["weight"], state["bias"], training, state["running_mean"], state["running_var"], ref.eps)
    xr = x.double().requires_grad_(True)
    zs = [ref(xr[h]) for h in range(H)]
    z = torch.stack(zs)
    out = {"x": x, "dy": dy, "state": state, "gate_distance": float(z.detach().abs().min()),
           "rm_fwd": ref.running_mean.clone(), "rv_fwd": ref.running_var.clone()}
    y = torch.relu(z) if relu else z
    y.backward(dy.double())
    out.update(y=y.detach(), dx=xr.grad, dgamma=ref.weight.grad.clone(), dbeta=ref.bias.grad.clone())
    with torch.no_grad():
        for h in range(H):
            ref(xr[h].detach())
    out.update(rm_replayed=ref.running_mean.clone(), rv_replayed=ref.running_var.clone())
    return out
