"""Host restatement of the RANSAC skeleton shared by the two-view solvers (csrc/ransac_common.h), from that header's
comment: the counter-based sampling (bit for bit) and the ordered compaction.  numpy only, no torch.
tests/h_solver_cases.py and tests/e_solver_cases.py bind their own names to these; tests/test_ransac_cases.py tests them."""
import numpy as np


def hash32(seed, pair, hyp, draw):
    m = 0xFFFFFFFF
    x = (seed * 0x9E3779B1 + pair * 0x85EBCA77 + hyp * 0xC2B2AE3D + draw * 0x27D4EB2F + 0x165667B1) & m
    x ^= x >> 16
    x = (x * 0x7FEB352D) & m
    x ^= x >> 15
    x = (x * 0x846CA68B) & m
    x ^= x >> 16
    return x


def sample_distinct(n, seed, pair, hyp, K, off_by_one=False):
    """The n indices of hypothesis `hyp` of pair `pair` with K >= n matches.  off_by_one: the mutated skip mapping
    (`>` for `>=`), which can return an index twice."""
    out = []
    for d in range(n):
        r = (hash32(seed, pair, hyp, d) * (K - d)) >> 32
        for p in sorted(out):
            if (r > p) if off_by_one else (r >= p):
                r += 1
        out.append(r)
    return out


def samples(n, seed, pair, T, K, **kw):
    """[T,n] int32; -1 everywhere when K < n (what the kernels write)."""
    if K < n:
        return np.full((T, n), -1, np.int32)
    return np.array([sample_distinct(n, seed, pair, t, K, **kw) for t in range(T)], np.int32)


def compact(kpts0, kpts1, matches0, dtype=None):
    """Ordered matched indices of view 0 and their correspondences [K,4] = (x0, y0, x1, y1), in `dtype` where given (an
    index outside [0, N) is no match)."""
    idx = np.nonzero((matches0 >= 0) & (matches0 < kpts1.shape[0]))[0]
    corr = np.concatenate([kpts0[idx], kpts1[matches0[idx]]], -1).reshape(-1, 4)
    return idx, corr if dtype is None else corr.astype(dtype)
