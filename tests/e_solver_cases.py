"""Yardstick of the relative-pose solver (csrc/e_solver.hip, csrc/e_fivept.h): numpy fp64 restatements, planted scenes,
derived bounds and the mutations the bounds must catch.  No GPU, no torch.  tests/test_e_solver_cases_reference.py tests
this module itself; tests/test_gpu_e_solver.py compares the kernels with it.

Restated here from the header comments of the two files: the Sampson rule, the refit and the decomposition with the depth
test; the 5-draw counter-based sampling (bit for bit) and the compaction are restated from the header comment of
csrc/ransac_common.h in tests/ransac_cases.py.  The 5-point solver goes ANOTHER ROUTE than the kernel's: null space by
numpy.linalg.svd (the kernel: elimination), the ten cubic constraints in graded order reduced by numpy.linalg.solve, the
10 x 10 action matrix of multiplication by x and numpy.linalg.eig (the kernel: a hidden variable, a degree-10 polynomial in
z and bisection).  The depth test goes another route too: homogeneous DLT triangulation through a 4 x 4 SVD."""
import functools
import os
import re

import numpy as np

import ransac_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constants():
    text = open(os.path.join(ROOT, "include", "gf_amd.h")).read()
    get = lambda name: re.search(r"#define\s+" + name + r"\s+([0-9.eE+-]+)f?\b", text).group(1)
    return int(get("GF_E_TILE")), int(get("GF_E_HYPS")), int(get("GF_E_MAXSOL")), float(get("GF_E_EPS_PIVOT"))


TILE, HYPS, MAXSOL, EPS_PIVOT = _header_constants()
RANSAC_TH = 0.5               # pixels, the reference default (relative_pose/opencv.py:12)
SEED = 11                     # the solver seed of every case
U32 = 2.0 ** -24              # unit roundoff of fp32

# ---- recorded measurements (tests/test_e_solver_cases_reference.py re-measures them and checks they are not exceeded) -------
# Worst residual of the RESTATEMENT's own solutions over the kept samples of candidate_samples(): max over the five sample
# residuals |x1^T E x0| and the cubic residual ||2 E E^T E - tr(E E^T) E||_F + |det E| with ||E||_F = 1.  Measured on the host
# (numpy fp64): 1.7e-10.  The kernel is allowed 16 x that (its elimination order differs) plus the derived storage part.
RESTATED_RESIDUAL = 1.7e-10
# Worst Frobenius distance (up to sign) between the restatement's solutions on a kept sample and on the same sample with the
# five correspondences in reversed order (another elimination / SVD order of the same problem).  Measured on the host: 8.4e-10.
RESTATED_DISTANCE = 8.4e-10
SOLVER_FACTOR = 16.0
# fp32 storage of nine entries of a unit-norm E: every entry moves by at most U32 |E_k| <= U32, the Frobenius norm by at most
# 3 U32; a residual that is a sum of at most nine products with |x| <= PT_MAX coordinates moves by at most
STORAGE_DISTANCE = 3 * U32
PT_MAX = 1.5                  # bound on |x|, |y| of the normalised coordinates of every scene here (asserted by the tests)
STORAGE_RESIDUAL = 9 * U32 * PT_MAX ** 2 + 30 * U32      # sample residuals; the cubic terms: d(2EE^TE - tr E) <= ~10 |dE|
# the kept samples: smallest separation of the restatement's real solutions >= SEP_MIN and the conditioning of its reduced
# cubic system <= COND_MAX; at most 10 % of the samples may be left out (asserted)
SEP_MIN = 1e-3
COND_MAX = 1e7
# margin of the noisy planted scenes: the kernel pipeline may end in another local optimum of the same count rule than the
# restated one when a count ties; both are refits over >= 90 % the same inliers, whose poses differ by less than this
# (degrees; measured on the host between lo_iters = 1 and lo_iters = 2 of the restated pipeline on the noisy PLANTED
# scenes: at most 0.09)
NOISY_MARGIN_DEG = 0.1


# ---- sampling and compaction: the shared skeleton with five draws (samples: [T,5] int32, -1 everywhere when K < 5) --------
hash32 = rc.hash32
sample5 = functools.partial(rc.sample_distinct, 5)
samples = functools.partial(rc.samples, 5)
compact = rc.compact


# ---- 5-point solver, fp64, by the action matrix ----------------------------------------------------------------------------
_MONO3 = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
_BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _pmul(p, q):
    out = np.zeros((4, 4, 4))
    for i, j, k in np.argwhere(p != 0):
        out[i:, j:, k:] += p[i, j, k] * q[:4 - i, :4 - j, :4 - k]
    return out


def _hom(p):
    return np.concatenate([p, np.ones(p.shape[:-1] + (1,))], -1)


def constraints(E):
    """(cubic residual, det) of one or more E [...,3,3]."""
    EEt = E @ np.swapaxes(E, -1, -2)
    tr = np.trace(EEt, axis1=-2, axis2=-1)[..., None, None]
    return np.linalg.norm(2 * EEt @ E - tr * E, axis=(-2, -1)), np.linalg.det(E)


def solve5(pts, with_info=False):
    """pts [5,4] fp64 -> candidates [n,3,3] with ||E||_F = 1 (n <= 10).  with_info: also the conditioning of the reduced
    cubic system."""
    pts = np.asarray(pts, np.float64)
    x0, x1 = _hom(pts[:, :2]), _hom(pts[:, 2:])
    Q = (x1[:, :, None] * x0[:, None, :]).reshape(5, 9)
    _, sq, Vt = np.linalg.svd(Q)
    if not sq[4] > 1e-12 * sq[0]:                                 # fewer than five independent rows
        return (np.zeros((0, 3, 3)), np.inf) if with_info else np.zeros((0, 3, 3))
    N = Vt[5:]                                                    # four null vectors
    Ep = np.zeros((3, 3, 4, 4, 4))
    for l, e in enumerate([(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]):
        Ep[(slice(None), slice(None)) + e] = N[l].reshape(3, 3)
    EEt = [[sum(_pmul(Ep[i, k], Ep[j, k]) for k in range(3)) for j in range(3)] for i in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    rows = []
    for i in range(3):
        for j in range(3):
            rows.append(sum(_pmul(2 * EEt[i][k] - (tr if i == k else 0), Ep[k, j]) for k in range(3)))
    det = sum(_pmul(_pmul(Ep[1, (k + 1) % 3], Ep[2, (k + 2) % 3]) - _pmul(Ep[1, (k + 2) % 3], Ep[2, (k + 1) % 3]), Ep[0, k])
              for k in range(3))
    rows.append(det)
    A = np.array([[r[m] for m in _MONO3 + _BASIS] for r in rows])
    A /= np.abs(A).max(1, keepdims=True)
    cond = np.linalg.cond(A[:, :10])
    if not np.isfinite(cond) or cond > 1e14:
        return (np.zeros((0, 3, 3)), np.inf) if with_info else np.zeros((0, 3, 3))
    Bm = np.linalg.solve(A[:, :10], A[:, 10:])                   # monomial_i = -Bm[i] . basis
    Mx = np.zeros((10, 10))
    Mx[:6] = -Bm[[0, 1, 2, 3, 4, 5]]
    Mx[6, 0] = Mx[7, 1] = Mx[8, 2] = Mx[9, 6] = 1.0
    w, V = np.linalg.eig(Mx)
    out = []
    for k in np.nonzero(w.imag == 0)[0]:
        v = V[:, k].real
        x, y, z = v[6] / v[9], v[7] / v[9], v[8] / v[9]
        E = (x * N[0] + y * N[1] + z * N[2] + N[3]).reshape(3, 3)
        E = E / np.linalg.norm(E)
        if np.isfinite(E).all():
            out.append(E)
    out = np.array(out).reshape(-1, 3, 3)
    return (out, cond) if with_info else out


def sample_residual(E, pts):
    """max |x1^T E x0| over the sample, for E [...,3,3] and pts [5,4]."""
    x0, x1 = _hom(pts[:, :2]), _hom(pts[:, 2:])
    return np.abs(np.einsum("ni,...ij,nj->...n", x1, E, x0)).max(-1)


def residual(E, pts):
    c, d = constraints(E)
    return np.maximum(sample_residual(E, pts), c + np.abs(d))


def sign_distance(E, F):
    """Frobenius distance up to sign between E [...,3,3] and F [...,3,3] (broadcast)."""
    return np.minimum(np.linalg.norm(E - F, axis=(-2, -1)), np.linalg.norm(E + F, axis=(-2, -1)))


def separation(Es):
    if len(Es) < 2:
        return np.inf
    d = sign_distance(Es[:, None], Es[None]) + np.eye(len(Es)) * 1e9
    return d.min()


# ---- Sampson rule ----------------------------------------------------------------------------------------------------
def sampson_terms(E, corr):
    """(e^2, |a|^2 + |b|^2) in fp64 of E [3,3] over corr [K,4]."""
    E = np.asarray(E, np.float64)
    corr = np.asarray(corr, np.float64)
    x0, x1 = _hom(corr[:, :2]), _hom(corr[:, 2:])
    a, b = x0 @ E.T, x1 @ E
    e = (x1 * a).sum(-1)
    return e * e, a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2


def inlier_mask(E, corr, th, mutate=None):
    """mutate: 'transpose' (E^T for E) or 'one_denominator' (|b|^2 dropped)."""
    E = np.asarray(E, np.float64)
    if mutate == "transpose":
        E = E.T
    e2, den = sampson_terms(E, corr)
    if mutate == "one_denominator":
        x0 = _hom(np.asarray(corr, np.float64)[:, :2])
        a = x0 @ E.T
        den = a[:, 0] ** 2 + a[:, 1] ** 2
    rhs = float(th) ** 2 * den
    return (e2 < rhs) & (rhs > 0) & np.isfinite(rhs)


def sampson_distance(E, corr):
    e2, den = sampson_terms(E, corr)
    return np.sqrt(e2 / den)


def count_band(E32, corr32, th32):
    """(sure, maybe): correspondences that are inliers whatever the fp32 rounding, and those within the rounding bound of the
    rule  e^2 < th^2 (|a|^2 + |b|^2)  as the kernel evaluates it.  Derivation, with u = U32 and g(k) = k u / (1 - k u), every
    fused multiply-add counted as if it rounded twice (an upper bound either way):
      a_i = E_i0 x + E_i1 y + E_i2: two products, two sums, at most 3 roundings on a path: |da_i| <= g(3) Sa_i with
            Sa_i = |E_i0||x| + |E_i1||y| + |E_i2|;  b_j likewise with Sb_j.
      e = x1 a_0 + y1 a_1 + a_2: the three inherited errors and 3 more roundings: |de| <= g(6) Se,
            Se = |x1| Sa_0 + |y1| Sa_1 + Sa_2.
      e^2: one product: |d(e^2)| <= 2 |e| de + de^2 + u (|e| + de)^2.
      den = a_0^2 + a_1^2 + b_0^2 + b_1^2: each square 2 g(3) + u relative to S^2, three sums: |d den| <= g(10) Sden,
            Sden = Sa_0^2 + Sa_1^2 + Sb_0^2 + Sb_1^2.
      rhs = (th th) den: two more roundings: |d rhs| <= g(12) th^2 Sden."""
    g = lambda k: k * U32 / (1 - k * U32)
    E = np.asarray(E32, np.float64)
    c = np.asarray(corr32, np.float64)
    th2 = float(th32) ** 2
    x0, x1 = _hom(c[:, :2]), _hom(c[:, 2:])
    Sa, Sb = np.abs(x0) @ np.abs(E).T, np.abs(x1) @ np.abs(E)
    Se = (np.abs(x1) * Sa).sum(-1)
    Sden = Sa[:, 0] ** 2 + Sa[:, 1] ** 2 + Sb[:, 0] ** 2 + Sb[:, 1] ** 2
    e2, den = sampson_terms(E, c)
    e, de = np.sqrt(e2), g(6) * Se
    slack = 2 * e * de + de * de + U32 * (e + de) ** 2 + g(12) * th2 * Sden
    gap = th2 * den - e2                                          # > 0: inlier
    return int((gap > slack).sum()), int((np.abs(gap) <= slack).sum())


# ---- refit ---------------------------------------------------------------------------------------------------------------
def _hartley(p):
    c = p.mean(0)
    s = np.sqrt(2.0) / np.linalg.norm(p - c, axis=1).mean()
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def project_essential(E):
    U, _, Vt = np.linalg.svd(E)
    return U @ np.diag([1.0, 1.0, 0.0]) @ Vt / np.sqrt(2.0)


def refit(corr, mask):
    """Hartley-normalised eight-point fit over corr[mask], projected to singular values (1, 1, 0) / sqrt 2; None under 8."""
    c = np.asarray(corr, np.float64)[mask]
    if len(c) < 8:
        return None
    T0, T1 = _hartley(c[:, :2]), _hartley(c[:, 2:])
    x0, x1 = _hom(c[:, :2]) @ T0.T, _hom(c[:, 2:]) @ T1.T
    A = (x1[:, :, None] * x0[:, None, :]).reshape(-1, 9)
    G = np.linalg.svd(A)[2][-1].reshape(3, 3)
    return project_essential(T1.T @ G @ T0)


# ---- decomposition and the depth test -----------------------------------------------------------------------------------
def decompose(E):
    """R1, R2, t of gluefactory/geometry/epipolar.py:97-122 (numpy.linalg.svd for torch.svd)."""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64))
    if np.linalg.det(U) < 0:
        U = U * np.array([1, 1, -1.0])
    if np.linalg.det(Vt) < 0:
        Vt = Vt * np.array([[1], [1], [-1.0]])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    return U @ W @ Vt, U @ W.T @ Vt, U[:, 2]


def front_count(R, t, corr):
    """Correspondences whose homogeneous DLT triangulation has positive depth in both cameras."""
    P1 = np.concatenate([R, t[:, None]], 1)
    n = 0
    for x0, y0, x1, y1 in np.asarray(corr, np.float64):
        A = np.array([[-1, 0, x0, 0], [0, -1, y0, 0], x1 * P1[2] - P1[0], y1 * P1[2] - P1[1]])
        X = np.linalg.svd(A)[2][-1]
        if X[3] == 0:
            continue
        X = X / X[3]
        n += bool(X[2] > 0 and (P1 @ X)[2] > 0)
    return n


def four_poses(E):
    R1, R2, t = decompose(E)
    return [(R1, t), (R1, -t), (R2, t), (R2, -t)]


def choose_pose(E, corr, mutate=None):
    """-> (R, t, counts of the four candidates in this function's order).  mutate: 'no_cheirality' takes the first."""
    poses = four_poses(E)
    counts = [front_count(R, t, corr) for R, t in poses]
    k = 0 if mutate == "no_cheirality" else int(np.argmax(counts))           # argmax: ties to the lowest index
    return poses[k][0], poses[k][1], counts


def angle_R(R, R_gt):
    return np.degrees(np.arccos(np.clip((np.trace(R.T @ R_gt) - 1) / 2, -1, 1)))


def angle_t(t, t_gt):
    n = max(np.linalg.norm(t) * np.linalg.norm(t_gt), 1e-10)
    a = np.degrees(np.arccos(np.clip(t @ t_gt / n, -1, 1)))
    return min(a, 180 - a)


def pose_error(R, t, R_gt, t_gt):
    return max(angle_R(np.asarray(R, np.float64), R_gt), angle_t(np.asarray(t, np.float64), t_gt))


def E_of(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])
    E = tx @ R
    return E / np.linalg.norm(E)


# ---- restated pipeline ------------------------------------------------------------------------------------------------------
def select(counts, mutate=None):
    """counts [T, MAXSOL] (-1 = no candidate) -> flat index of the winner or -1.  mutate: 'ties_high'."""
    flat = np.asarray(counts).reshape(-1)
    if (flat < 0).all():
        return -1
    best = flat.max()
    hits = np.nonzero(flat == best)[0]
    return int(hits[-1] if mutate == "ties_high" else hits[0])


def pipeline(corr, th, T, seed=SEED, pair=0, lo_iters=2):
    """The whole solver in fp64 on corr [K,4] (normalised): dict(E, R, t, mask, count, success)."""
    corr = np.asarray(corr, np.float64)
    K = len(corr)
    fail = dict(E=np.zeros((3, 3)), R=np.eye(3), t=np.zeros(3), mask=np.zeros(K, bool), count=0, success=False)
    if K < 5:
        return fail
    best = (-1, None)
    for s in samples(seed, pair, T, K):
        for E in solve5(corr[s])[:MAXSOL]:
            c = int(inlier_mask(E, corr, th).sum())
            if c > best[0]:
                best = (c, E)
    if best[1] is None:
        return fail
    count, E = best
    mask = inlier_mask(E, corr, th)
    for _ in range(lo_iters):
        En = refit(corr, mask)
        if En is None:
            break
        mn = inlier_mask(En, corr, th)
        if mn.sum() >= count:
            E, mask, count = En, mn, int(mn.sum())
    R, t, _ = choose_pose(E, corr[mask])
    return dict(E=E, R=R, t=t, mask=mask, count=count, success=True)


@functools.lru_cache(maxsize=None)
def restated(spec, noise=0.0, lo_iters=2, pair=0):
    """The restated pipeline on scene(*spec, noise) as pair `pair` of its batch (the pair index is an argument of the sampling
    hash) with PLANTED_T hypotheses (cached: several tests share it)."""
    s = scene(*spec, noise=noise)
    return pipeline(scene_corr(s)[1], s["th"], PLANTED_T, pair=pair, lo_iters=lo_iters)


# ---- scenes -----------------------------------------------------------------------------------------------------------
def _rotation(rng, max_deg):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.radians(rng.uniform(min(5.0, max_deg / 2), max_deg))
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0.0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def camera(rng):
    """(f [2], c [2]) of a pinhole camera: focal lengths 600-1200, principal point near the centre of a 1024 x 768 frame."""
    f = rng.uniform(600, 1200)
    return np.array([f, f * rng.uniform(0.97, 1.03)]), np.array([512.0, 384.0]) + rng.uniform(-30, 30, 2)


def normalise(kpts, cam):
    """fp32 (kpts - c) / f, the arithmetic of Camera.image2cam."""
    f, c = cam
    return (np.asarray(kpts, np.float32) - c.astype(np.float32)) / f.astype(np.float32)


def norm_threshold(cam0, cam1, ransac_th=RANSAC_TH):
    f = np.concatenate([cam0[0], cam1[0]]).astype(np.float32)
    return np.float32(ransac_th) / f.mean(dtype=np.float32)


@functools.lru_cache(maxsize=None)
def scene(seed, n_in, n_out, M, N, noise=0.0, mode="general"):
    """One planted pair.  mode: 'general', 'planar' (all points on one plane) or 'rotation' (t = 0).  Keys: kpts0 [M,2],
    kpts1 [N,2] fp32 pixels, matches0 [M] int64, planted [M] bool (the inlier matches), cam0, cam1, R, t, E (unit norm),
    th (normalised, fp32), p0n [M,2], p1n [N,2] fp32 normalised coordinates."""
    rng = np.random.default_rng(1000 + seed)
    K = n_in + n_out
    assert K <= M and K <= N
    R = _rotation(rng, 30.0)
    t = rng.normal(size=3)
    t[2] *= 0.3                                                  # not along the optical axis
    t /= np.linalg.norm(t)
    cam0, cam1 = camera(rng), camera(rng)
    th = norm_threshold(cam0, cam1)
    tt = np.zeros(3) if mode == "rotation" else t
    pts0, pts1 = [], []
    while len(pts0) < n_in:
        uv = rng.uniform([40, 40], [984, 728])
        ray = np.append((uv - cam0[1]) / cam0[0], 1.0)
        if mode == "planar":
            nrm, dist = np.array([0.2, -0.1, 1.0]), 5.0           # the plane n . X = d
            X = ray * dist / (nrm @ ray)
        else:
            X = ray * rng.uniform(2.0, 10.0)
        Y = R @ X + tt
        if X[2] < 1.0 or Y[2] < 1.0:
            continue
        q = Y[:2] / Y[2] * cam1[0] + cam1[1]
        if not (0 <= q[0] <= 1023 and 0 <= q[1] <= 767):
            continue
        pts0.append(uv)
        pts1.append(q + rng.normal(size=2) * noise)
    E = E_of(R, t)
    while len(pts0) < K:                                         # outliers: Sampson distance to the TRUE E >= 10 th
        uv, q = rng.uniform([40, 40], [984, 728]), rng.uniform([40, 40], [984, 728])
        c = np.concatenate([normalise(uv, cam0), normalise(q, cam1)])[None].astype(np.float64)
        if sampson_distance(E, c)[0] >= 10 * float(th):
            pts0.append(uv)
            pts1.append(q)
    order0, order1 = rng.permutation(M)[:K], rng.permutation(N)[:K]
    kpts0 = rng.uniform([0, 0], [1023, 767], (M, 2))
    kpts1 = rng.uniform([0, 0], [1023, 767], (N, 2))
    kpts0[order0], kpts1[order1] = np.array(pts0).reshape(-1, 2), np.array(pts1).reshape(-1, 2)
    matches0 = np.full(M, -1, np.int64)
    matches0[order0] = order1
    planted = np.zeros(M, bool)
    planted[order0[:n_in]] = True
    kpts0, kpts1 = kpts0.astype(np.float32), kpts1.astype(np.float32)
    return dict(kpts0=kpts0, kpts1=kpts1, matches0=matches0, planted=planted, cam0=cam0, cam1=cam1, R=R, t=t, E=E, th=th,
                p0n=normalise(kpts0, cam0), p1n=normalise(kpts1, cam1), K=K)


def scene_corr(s):
    """(idx, corr fp32 [K,4]) of a scene in normalised coordinates."""
    return compact(s["p0n"], s["p1n"], s["matches0"])


# planted scenes of the GPU tests: (seed, inliers, outliers, M, N); 50 % outliers, unequal K_b, K across the tile edge
PLANTED = [(0, 130, 130, 300, 280), (1, 100, 100, 300, 280), (2, 40, 40, 300, 280)]
PLANTED_T = 512


def refit_bound_deg(s):
    """First-order bound (degrees) on the pose error of the refit over the planted inliers of a noise-free scene whose
    keypoints were rounded to fp32.  A pixel coordinate below 1024 moves by at most 2^-14 px in the rounding, that is
    2^-14 / f in normalised units, and the fp32 evaluation of (p - c) / f adds 2 U32 |x|: eps per coordinate, s eps after the
    Hartley scaling s.  The row (u x, u y, u, v x, v y, v, x, y, 1) of the normalised design matrix A then moves by at most
    s eps (|(x, y, 1)| + |(u, v, 1)|) sqrt 2 in norm, A by the root of the sum of the squares, and the singular vector of its
    smallest singular value by at most ||dA|| / (sigma_8 - sigma_9) (Wedin), sigma_8 the second smallest singular value of
    the noise-free A and sigma_9 ~ 0.  De-normalisation G -> T1^T G T0 is linear: it amplifies a relative error by at most
    cond(T0) cond(T1); the projection onto the essential manifold at most doubles it, the fp32 storage adds 3 U32, and a
    unit-norm E that moves by dE turns R and t by at most 2 sqrt 2 dE.  The returned R is fp32: its trace is off by up to
    3 U32, which the arccos of angle_R near zero turns into sqrt(2 . 3 U32) rad (0.034 degrees), added last."""
    idx, corr = scene_corr(s)
    c = corr[s["planted"][idx]].astype(np.float64)
    T0, T1 = _hartley(c[:, :2]), _hartley(c[:, 2:])
    x0, x1 = _hom(c[:, :2]) @ T0.T, _hom(c[:, 2:]) @ T1.T
    A = (x1[:, :, None] * x0[:, None, :]).reshape(-1, 9)
    sv = np.linalg.svd(A, compute_uv=False)
    eps = 2.0 ** -14 / min(s["cam0"][0].min(), s["cam1"][0].min()) + 2 * U32 * PT_MAX
    sc = max(T0[0, 0], T1[0, 0])
    rows = sc * eps * np.sqrt(2.0) * (np.linalg.norm(x0, axis=1) + np.linalg.norm(x1, axis=1))
    dA = np.sqrt((rows ** 2).sum())
    dE = 2 * np.linalg.cond(T0) * np.linalg.cond(T1) * dA / sv[-2] + 3 * U32
    return float(np.degrees(2 * np.sqrt(2.0) * dE + np.sqrt(6 * U32)))


# ---- samples of the candidate test -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def candidate_samples(T=HYPS + 1):
    """The samples the candidate test looks at: scene PLANTED[2]'s inliers only (noise-free, so the true E solves every
    sample), T hypotheses.  dict(corr [K,4] fp32, samples [T,5], sols: list of [n,3,3], keep [T] bool)."""
    sc = scene(7, 60, 0, 64, 64)
    idx, corr = scene_corr(sc)
    smp = samples(SEED, 0, T, len(corr))
    sols, keep = [], []
    for s in smp:
        Es, cond = solve5(corr[s].astype(np.float64), with_info=True)
        sols.append(Es)
        keep.append(bool(len(Es) > 0 and cond <= COND_MAX and separation(Es) >= SEP_MIN))
    return dict(scene=sc, corr=corr, samples=smp, sols=sols, keep=np.array(keep))


# ---- metrics fixture --------------------------------------------------------------------------------------------------------
def eval_inputs():
    """Seeded inputs of the metric tests (tests/golden/relative_pose_eval.npz holds the reference's answers): 4 pairs of 40
    correspondences, ground-truth poses, estimated (R, t) including a 0 degree and a 180 degree rotation error, translations
    either side of the 90 degree fold and a near-zero t_gt, and two error lists for the AUC (one all above 20)."""
    rng = np.random.default_rng(99)
    out = dict(R_gt=[], t_gt=[], R=[], t=[], p0=[], p1=[])
    for i in range(4):
        s = scene(20 + i, 40, 0, 40, 40, noise=0.3 * i)
        idx, corr = scene_corr(s)
        out["p0"].append(corr[:, :2])
        out["p1"].append(corr[:, 2:])
        out["R_gt"].append(s["R"])
        out["t_gt"].append(s["t"] if i != 3 else s["t"] * 1e-12)
        Rd = [np.eye(3), _rotation(rng, 20.0), np.diag([1.0, -1.0, -1.0]), _rotation(rng, 3.0)][i]
        out["R"].append(Rd @ s["R"])
        td = [s["t"], -s["t"] + 0.1 * rng.normal(size=3), s["t"] + 0.8 * rng.normal(size=3), rng.normal(size=3)][i]
        out["t"].append(td)
    out = {k: np.array(v).astype(np.float32 if k in ("p0", "p1") else np.float64) for k, v in out.items()}
    out["errors_a"] = np.array([0.5, 3.0, 7.5, 12.0, 19.0, 25.0, np.inf, 1.0, 4.9, 10.0])
    out["errors_b"] = np.array([21.0, 40.0, np.inf, 90.0])
    return out


MUTATIONS = ["transpose", "one_denominator", "no_cheirality", "ties_high", "ragged_tile", "t_not_normalised"]
