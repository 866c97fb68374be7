"""Shared by tools/gen_golden_nn_matcher.py and the nearest-neighbour matcher tests: the fixture's cases, a float64 numpy
restatement of find_nn / mutual_check (gluefactory/models/matchers/nearest_neighbor_matcher.py:15-35), and the rows whose
decisions are safe against the fp32 tolerance."""
import numpy as np

TOL = 1e-4            # the project's fp32 tolerance: a decision closer than this to its boundary is not compared
MAX_EXCLUDED = 0.01   # ... and at most this share of all rows may be excluded that way

# fixture cases: name -> configuration of the matcher
CASES = {
    "a": {},
    "b": {"ratio_thresh": 0.8, "distance_thresh": 0.9, "mutual_check": True},
    "c": {"ratio_thresh": 0.8, "distance_thresh": 0.9, "mutual_check": False},
    "d": {"loss": "N_pair"},
}
TEMPERATURE_D = 1.7


def _top2(sim):
    """(best, arg, second) along the last axis; lowest index on ties, second as a multiset."""
    arg = sim.argmax(-1)
    best = np.take_along_axis(sim, arg[..., None], -1)[..., 0]
    rest = sim.copy()
    np.put_along_axis(rest, arg[..., None], -np.inf, -1)
    second = rest.max(-1) if sim.shape[-1] > 1 else np.full(best.shape, -np.inf)
    return best, arg, second


def _find_nn(sim, ratio, dist):
    best, arg, second = _top2(sim)
    d0, d1 = 2 * (1 - best), 2 * (1 - second)
    mask = np.ones(best.shape, bool)
    if ratio:
        mask &= d0 <= ratio ** 2 * d1
    if dist:
        mask &= d0 <= dist ** 2
    return np.where(mask, arg, -1)


def ref_matches(sim, ratio_thresh=None, distance_thresh=None, mutual_check=True, **_):
    """(matches0, matches1) of a [B,M,N] similarity in float64."""
    sim = np.asarray(sim, np.float64)
    m0 = _find_nn(sim, ratio_thresh, distance_thresh)
    m1 = _find_nn(sim.transpose(0, 2, 1), ratio_thresh, distance_thresh)
    if mutual_check:      # i keeps j only if j, after its own thresholds, points back at i (both sides from the SAME m0, m1)
        back0 = np.take_along_axis(m1, np.maximum(m0, 0), -1) == np.arange(m0.shape[-1])
        back1 = np.take_along_axis(m0, np.maximum(m1, 0), -1) == np.arange(m1.shape[-1])
        m0, m1 = np.where(back0, m0, -1), np.where(back1, m1, -1)
    return m0, m1


def _own_safe(sim, ratio, dist):
    best, arg, second = _top2(sim)
    d0, d1 = 2 * (1 - best), 2 * (1 - second)
    safe = (best - second) > TOL
    if ratio:
        safe &= np.abs(d0 - ratio ** 2 * d1) > TOL
    if dist:
        safe &= np.abs(d0 - dist ** 2) > TOL
    return safe, arg


def safe_rows(sim, ratio_thresh=None, distance_thresh=None, mutual_check=True, **_):
    """(safe0 [B,M], safe1 [B,N]): rows whose every decision (arg-max, ratio, distance -- and with the mutual check the same
    three of the row's nearest neighbour on the other side) has a margin above TOL in `sim`."""
    sim = np.asarray(sim, np.float64)
    s0, a0 = _own_safe(sim, ratio_thresh, distance_thresh)
    s1, a1 = _own_safe(sim.transpose(0, 2, 1), ratio_thresh, distance_thresh)
    if mutual_check:
        s0, s1 = s0 & np.take_along_axis(s1, a0, -1), s1 & np.take_along_axis(s0, a1, -1)
    return s0, s1


def excluded_share(safe0, safe1):
    return 1.0 - (safe0.sum() + safe1.sum()) / float(safe0.size + safe1.size)


def check_mutual_invariant(sim, m0, m1, ratio_thresh=None, distance_thresh=None, mutual_check=True, **_):
    """Properties every output of the matcher has, from `sim` alone: a match points at a row maximum (within TOL), and with
    the mutual check the two vectors are inverse to each other."""
    sim = np.asarray(sim, np.float64)
    for b in range(sim.shape[0]):
        for m, s in ((m0[b], sim[b]), (m1[b], sim[b].T)):
            i = np.nonzero(m > -1)[0]
            assert np.all(s[i, m[i]] >= s[i].max(-1) - TOL)
        if mutual_check:
            i = np.nonzero(m0[b] > -1)[0]
            assert np.array_equal(m1[b][m0[b][i]], i)
            j = np.nonzero(m1[b] > -1)[0]
            assert np.array_equal(m0[b][m1[b][j]], j)


# rows_top2 kernel cases: (B, M, N) x D x dtype; M ragged against the 128-row owner block, N against the 64-row tile
TOP2_SHAPES = [(2, 150, 201), (1, 1, 2), (1, 130, 64), (1, 64, 129)]
TOP2_DIMS = [64, 128, 256]


def top2_inputs(shape, dim, bf16):
    """Seeded L2-normalised descriptors as torch CPU tensors (rounded to bf16 when asked: the reference then sees exactly
    the values the kernel sees) and the float64 (best, arg, second) of a b^T.  The seed is the first one for which the
    float64 reference ALONE keeps the rows with a top-1 / top-2 gap within TOL under the cap (at M = 64 one such row would
    already exceed it); the kernel under test has no part in the choice."""
    import torch
    B, M, N = shape
    for seed in range(50):
        g = torch.Generator().manual_seed(1000 * seed + 10 * dim + M + N)
        a = torch.nn.functional.normalize(torch.randn(B, M, dim, generator=g), dim=-1)
        b = torch.nn.functional.normalize(torch.randn(B, N, dim, generator=g), dim=-1)
        if bf16:
            a, b = a.bfloat16(), b.bfloat16()
        top = _top2(np.einsum("bmd,bnd->bmn", a.double().numpy(), b.double().numpy()))
        if ((top[0] - top[2]) <= TOL).mean() <= MAX_EXCLUDED:
            return a, b, top
    raise AssertionError("no seed keeps the float64 reference within the cap")
