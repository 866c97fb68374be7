"""Yardstick of the homography solver (csrc/h_solver.hip): numpy fp64 restatements, planted scenes, derived bounds and the
mutations the bounds must catch.  No GPU, no torch.  tests/test_h_solver_cases_reference.py tests this module itself;
tests/test_gpu_h_solver.py compares the kernels with it.

Restated here, from the header comment of csrc/h_solver.hip: the degeneracy tests, the closed-form 4-point fit and the
forward transfer error; the counter-based sampling (bit for bit) and the compaction are restated from the header comment of
csrc/ransac_common.h in tests/ransac_cases.py.  The weighted DLT is restated through
numpy.linalg.svd: kornia is not available here, so `dlt` restates the PUBLISHED meaning of its find_homography_dlt
(normalise both point sets to zero mean and mean distance sqrt 2 without the weights, stack the two rows per point, weight
the rows, take the right singular vector of the smallest singular value, de-normalise, divide by h22)."""
import functools
import os
import re

import numpy as np

import ransac_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constants():
    text = open(os.path.join(ROOT, "include", "gf_amd.h")).read()
    get = lambda name: re.search(r"#define\s+" + name + r"\s+([0-9.eE+-]+)f?\b", text).group(1)
    return int(get("GF_H_TILE")), int(get("GF_H_HYPS")), float(get("GF_H_EPS_AREA")), float(get("GF_H_H22_FRAC"))


TILE, HYPS, EPS_AREA, H22_FRAC = _header_constants()
TH = 3.0                      # ransac_th of every case (the reference default)
SEED = 7                      # the solver seed of every case
U32 = 2.0 ** -24              # unit roundoff of fp32
SIZE = (640.0, 480.0)         # frame of the corner error


# ---- sampling and compaction: the shared skeleton with four draws (samples: [T,4] int32, -1 everywhere when K < 4) --------
hash32 = rc.hash32
sample4 = functools.partial(rc.sample_distinct, 4)
samples = functools.partial(rc.samples, 4)
compact = functools.partial(rc.compact, dtype=np.float64)


# ---- 4-point fit, vectorised over hypotheses -------------------------------------------------------------------------------
def _area(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def fit4(c, dtype=np.float64, eps=EPS_AREA):
    """c [T,4,4] = (x0, y0, x1, y1) of the four sampled correspondences.  Returns dict(H [T,3,3] with h22 == 1, ok [T]
    (not rejected), band [T] (an area or the h22 test lies so close to its threshold that fp32 may decide either way),
    kappa [T] (the cancellation of the worst area: extent^2 / |area|), extent [T]).  dtype = float32 follows the kernel's
    operation order in numpy fp32 (no fused multiply-add): used only to check the derived bound on the host."""
    c = np.asarray(c, dtype)
    z = np.zeros(c.shape[0], dtype)
    one = dtype(1)
    rel = c[:, 1:, :] - c[:, :1, :]
    x2, y2, u2, v2 = (rel[:, 0, i] for i in range(4))
    x3, y3, u3, v3 = (rel[:, 1, i] for i in range(4))
    x4, y4, u4, v4 = (rel[:, 2, i] for i in range(4))
    with np.errstate(all="ignore"):
        s, d = _area(z, z, x2, y2, x3, y3), _area(z, z, u2, v2, u3, v3)
        l1, l2, l3 = _area(x2, y2, x3, y3, x4, y4), _area(x3, y3, z, z, x4, y4), _area(z, z, x2, y2, x4, y4)
        m1, m2, m3 = _area(u2, v2, u3, v3, u4, v4), _area(u3, v3, z, z, u4, v4), _area(z, z, u2, v2, u4, v4)
        src, dst = np.stack([s, l1, l2, l3]), np.stack([d, m1, m2, m3])
        areas = np.concatenate([src, dst])
        ok = (np.abs(areas) >= dtype(eps)).all(0) & ((src > 0) == (dst > 0)).all(0)
        e0 = np.abs(rel[:, :, :2]).max((1, 2)).astype(np.float64)
        e1 = np.abs(rel[:, :, 2:]).max((1, 2)).astype(np.float64)
        kappa = np.maximum(e0 ** 2 / np.abs(src.astype(np.float64)).min(0), e1 ** 2 / np.abs(dst.astype(np.float64)).min(0))
        # an area within the rounding of its two products of the threshold may fall either way in fp32
        slack = 8 * U32 * np.concatenate([np.broadcast_to(e0 ** 2, src.shape), np.broadcast_to(e1 ** 2, dst.shape)])
        band = (np.abs(np.abs(areas.astype(np.float64)) - eps) <= slack).any(0)
        ln = one / np.abs(src[1:]).max(0)
        mn = one / np.abs(dst[1:]).max(0)
        l1, l2, l3, m1, m2, m3 = l1 * ln, l2 * ln, l3 * ln, m1 * mn, m2 * mn, m3 * mn
        g1, g2, g3 = m1 * l2 * l3, m2 * l1 * l3, m3 * l1 * l2
        a00, a01, a02, a10, a11, a20, a21 = y2 - y3, x3 - x2, s, y3, -x3, -y2, x2
        k = [u2 * g2 * a10 + u3 * g3 * a20, u2 * g2 * a11 + u3 * g3 * a21, z.copy(),
             v2 * g2 * a10 + v3 * g3 * a20, v2 * g2 * a11 + v3 * g3 * a21, z.copy(),
             g1 * a00 + g2 * a10 + g3 * a20, g1 * a01 + g2 * a11 + g3 * a21, g1 * a02]
        inv = one / np.abs(np.stack(k)).max(0)
        k = [v * inv for v in k]
        px, py, qx, qy = c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 0, 3]
        k[2] = k[2] - (k[0] * px + k[1] * py)
        k[5] = k[5] - (k[3] * px + k[4] * py)
        k[8] = k[8] - (k[6] * px + k[7] * py)
        for i in range(3):
            k[i] = k[i] + qx * k[6 + i]
            k[3 + i] = k[3 + i] + qy * k[6 + i]
        fro = np.sqrt(sum(v * v for v in k))
        ratio = np.abs(k[8]) / fro
        ok &= ratio >= dtype(H22_FRAC)
        band |= np.abs(ratio.astype(np.float64) - H22_FRAC) <= 1e-2 * H22_FRAC + 64 * U32 * kappa
        H = np.stack([v / k[8] for v in k], -1)
        ok &= np.isfinite(H).all(-1)
    return {"H": H.reshape(-1, 3, 3), "ok": ok, "band": band & np.isfinite(kappa), "kappa": kappa, "extent": np.minimum(e0, e1)}


# ---- transfer error -------------------------------------------------------------------------------------------------------
def transfer(H, corr, backward=False, dtype=np.float64):
    """(err [.., K], w [.., K]) of models H [.., 3, 3] on corr [K, 4]: forward |pi(H x0) - x1|; backward (the mutation)
    |pi(H^-1 x1) - x0|."""
    H, corr = np.asarray(H, dtype), np.asarray(corr, dtype)
    a, b = (corr[:, 2:], corr[:, :2]) if backward else (corr[:, :2], corr[:, 2:])
    with np.errstate(all="ignore"):
        if backward:
            H = np.linalg.inv(H)
        Hm = H[..., None, :, :]
        x, y = a[:, 0:1], a[:, 1:2]
        p = Hm[..., 0] * x + Hm[..., 1] * y + Hm[..., 2]
        w = p[..., 2]
        q = p[..., :2] / w[..., None]
        err = np.sqrt(((q - b) ** 2).sum(-1))
    return err, w


def inlier_mask(H, corr, th=TH, **kw):
    err, w = transfer(H, corr, **kw)
    with np.errstate(invalid="ignore"):
        return (w > 0) & np.isfinite(w) & (err < th)


# ---- derived bound of the scoring comparison -----------------------------------------------------------------------------
FIT_FACTOR = 32.0


def delta(fit, coord_range):
    """Band of the inlier threshold inside which fp32 may decide either way, per hypothesis [T], in pixels.
    The fit's fp32 error is dominated by the cancellation inside the eight signed areas: each is a difference of two
    products of coordinate differences of size <= extent, so its relative error is about 2^-24 * kappa with
    kappa = extent^2 / min |area| (the condition number of the fit).  That relative error reaches the entries of H in the
    sample's own frame; a point at distance r from the sample sees it amplified by (r / extent)^2 through the projective
    division, and r <= coord_range.  Hence delta = FIT_FACTOR * 2^-24 * kappa * max(1, coord_range / extent)^2 *
    coord_range.  FIT_FACTOR = 32 stands for the number of rounded operations between the areas and a transfer error
    (about 30: 3 products in g, 3-term sums with 2 products, the normalisation, 2 translations, the division by h22 and
    the 11 operations of the inlier test).  Checked on the host against a numpy fp32 run of the same formulas
    (test_h_solver_cases_reference.py); never tuned on the GPU."""
    rho = np.maximum(1.0, coord_range / np.maximum(fit["extent"], 1e-30))
    with np.errstate(all="ignore"):
        return FIT_FACTOR * U32 * fit["kappa"] * rho ** 2 * coord_range


def count_band(H, corr, dlt_, th=TH, coord_range=1.0):
    """[lo, hi] of the inlier count of every model H [T,3,3] with threshold band dlt_ [T]: lo counts what is an inlier
    whatever fp32 decides, hi what may be one (a denominator within its own band of 0 included)."""
    err, w = transfer(H, corr)
    wband = (dlt_ / coord_range)[:, None]
    with np.errstate(invalid="ignore"):
        lo = ((w > wband) & (err < (th - dlt_)[:, None])).sum(-1)
        hi = (((w > -wband) & (err < (th + dlt_)[:, None])) | (np.abs(w) <= wband) | ~np.isfinite(err)).sum(-1)
    return lo, hi


# ---- Hartley-normalised weighted DLT ------------------------------------------------------------------------------------
def dlt(p0, p1, w=None, denormalise=True, use_weights=True, transposed=False):
    """Restates the published meaning of kornia's find_homography_dlt (see the module docstring) in fp64 through
    numpy.linalg.svd.  p0, p1 [K,2], w [K] or None.  Returns H [3,3] with h22 == 1, or None with fewer than 4 points or
    |h22| < H22_FRAC ||H||_F.  denormalise=False, use_weights=False, transposed=True are the mutations."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    if p0.shape[0] < 4:
        return None
    w = np.ones(p0.shape[0]) if (w is None or not use_weights) else np.asarray(w, np.float64)

    def norm(p):
        c = p.mean(0)
        s = np.sqrt(2.0) / np.sqrt(((p - c) ** 2).sum(-1)).mean()
        return (p - c) * s, np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])

    with np.errstate(all="ignore"):
        (a, T0), (b, T1) = norm(p0), norm(p1)
        x, y, u, v = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
        o, z = np.ones_like(x), np.zeros_like(x)
        r0 = np.stack([z, z, z, -x, -y, -o, v * x, v * y, v], -1)
        r1 = np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], -1)
        A = np.concatenate([r0, r1]) * np.sqrt(np.concatenate([w, w]))[:, None]
        if not np.isfinite(A).all():
            return None
        G = np.linalg.svd(A, full_matrices=True)[2][-1].reshape(3, 3)
        H = np.linalg.inv(T1) @ G @ T0 if denormalise else G
        if not np.isfinite(H).all() or abs(H[2, 2]) < H22_FRAC * np.linalg.norm(H):
            return None
        H = H / H[2, 2]
    return H.T.copy() if transposed else H


def warp(H, p):
    q = np.concatenate([p, np.ones_like(p[:, :1])], -1) @ np.asarray(H, np.float64).T
    return q[:, :2] / q[:, 2:]


def corner_error(H, H_gt, size=SIZE):
    """homography_corner_error of the reference (geometry/homography.py:336-342) in fp64."""
    W, Hh = size
    c = np.array([[0, 0], [W, 0], [W, Hh], [0, Hh]], np.float64)
    return float(np.sqrt(((warp(H, c) - warp(H_gt, c)) ** 2).sum(-1)).mean())


def sym_error(p0, p1, H):
    """sym_homography_error of the reference (:314-323) in fp64."""
    d01 = np.sqrt(((warp(H, p0) - p1) ** 2).sum(-1))
    d10 = np.sqrt(((warp(np.linalg.inv(H), p1) - p0) ** 2).sum(-1))
    return (d01 + d10) / 2


DLT_FACTOR = 4.0


def corner_bound(p0, p1, w=None, size=SIZE):
    """Bound on the corner error between two correct evaluations of the DLT on these points, one of which sees its fp32
    inputs perturbed by half an ulp each and rounds its nine outputs to fp32: the first-order sum
        sum_j |d corner / d input_j| ulp32(input_j) / 2  +  sum_e |d corner / d h_e| ulp32(h_e) / 2
    (central differences of the fp64 restatement, the worst corner), times DLT_FACTOR = 4 for the second-order terms and the
    fp64 arithmetic of two different eigen-solvers (Jacobi sweeps against an SVD), which is 2^-29 of the first sum."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    W, Hh = size
    corners = np.array([[0, 0], [W, 0], [W, Hh], [0, Hh]], np.float64)
    H = dlt(p0, p1, w)
    total = np.zeros(4)
    pts = [p0, p1]
    for which in range(2):
        for k in range(p0.shape[0]):
            for a in range(2):
                v = pts[which][k, a]
                step = max(abs(v), 1.0) * 1e-6
                out = []
                for sgn in (1, -1):
                    q = [p0.copy(), p1.copy()]
                    q[which][k, a] = v + sgn * step
                    out.append(warp(dlt(q[0], q[1], w), corners))
                deriv = np.sqrt((((out[0] - out[1]) / (2 * step)) ** 2).sum(-1))
                total += deriv * np.spacing(np.float32(abs(v))) / 2
    for e in range(8):
        Hp, Hm = H.copy(), H.copy()
        step = max(abs(H.flat[e]), 1e-6) * 1e-6
        Hp.flat[e] += step
        Hm.flat[e] -= step
        deriv = np.sqrt((((warp(Hp, corners) - warp(Hm, corners)) / (2 * step)) ** 2).sum(-1))
        total += deriv * np.spacing(np.float32(abs(H.flat[e]))) / 2
    return DLT_FACTOR * float(total.max())


# ---- host RANSAC (fp64): what the kernels are compared with --------------------------------------------------------------
def host_ransac(kpts0, kpts1, matches0, pair, T, lo_iters=2, seed=SEED, th=TH, backward=False, off_by_one=False):
    """The solver in fp64.  Returns dict(H, inliers [M] bool, num, success, samples [T,4], fit (see fit4), counts [T],
    models: the winning and every refitted model (for the band check of the scenes))."""
    idx, corr = compact(kpts0, kpts1, matches0)
    K, M = len(idx), kpts0.shape[0]
    smp = samples(seed, pair, T, K, off_by_one=off_by_one)
    none = {"H": np.eye(3), "inliers": np.zeros(M, bool), "num": 0, "success": False, "samples": smp, "fit": None,
            "counts": np.full(T, -1), "models": [], "corr": corr, "idx": idx}
    if K < 4:
        return none
    fit = fit4(corr[smp])
    counts = np.where(fit["ok"], inlier_mask(np.where(fit["ok"][:, None, None], fit["H"], np.eye(3)), corr, th, backward=backward).sum(-1), -1)
    none.update(fit=fit, counts=counts)
    if not fit["ok"].any():
        return none
    best = int(np.argmax(counts))                                   # the first maximum: the lowest index of a tie
    H = fit["H"][best]
    mask = inlier_mask(H, corr, th, backward=backward)
    models = [H]
    for _ in range(lo_iters):
        Hn = dlt(corr[mask, :2], corr[mask, 2:])
        if Hn is None:
            continue
        models.append(Hn)
        mn = inlier_mask(Hn, corr, th, backward=backward)
        if mn.sum() >= mask.sum():
            H, mask = Hn, mn
    inl = np.zeros(M, bool)
    inl[idx[mask]] = True
    return {"H": H, "inliers": inl, "num": int(mask.sum()), "success": True, "samples": smp, "fit": fit, "counts": counts,
            "models": models, "corr": corr, "idx": idx, "best": best}


# ---- planted scenes -------------------------------------------------------------------------------------------------------
RANGE = 256                                   # lattice [0, RANGE)^2 in view 0
H_AFFINE = np.array([[1.25, 0.25, 8.0], [-0.25, 1.5, 40.0], [0.0, 0.0, 1.0]])            # dyadic: view 1 is exact too
H_PROJ = np.array([[1.1, 0.08, 12.0], [-0.05, 1.2, 20.0], [2.0e-4, -1.0e-4, 1.0]])        # view 1 = fp32(H x0)
MODELS = {"affine": H_AFFINE, "proj": H_PROJ}
MEDIUM = 3.25
# (model, K, M, N) of the planted-truth scenes: one match more than the scoring tile, and a small one
PLANTED = [("affine", TILE + 1, TILE + 38, TILE + 51), ("proj", TILE + 1, TILE + 38, TILE + 51), ("proj", 40, 64, 50)]


def _build_scene(model, K, M, N, seed):
    """K matches among M / N keypoints (M != N): ceil(K / 2) planted inliers x1 = fp32(H x0) on distinct integer lattice
    points; the rest displaced by 50..120 px in a random direction on the 1/4-pixel grid, except (K >= 16) four "medium"
    ones displaced by (0, MEDIUM) px: outliers of the forward error, inliers of the backward one under either model (the
    linear parts shrink that displacement to 2.2 / 2.7 px), which is what catches the backward-error mutation.  Unmatched
    keypoints of both views are random; the matched slots and their partners are scattered by random permutations."""
    rng = np.random.RandomState(seed)
    H = MODELS[model]
    flat = rng.choice(RANGE * RANGE, size=M, replace=False)
    kp0 = np.stack([flat % RANGE, flat // RANGE], -1).astype(np.float32)
    slots = np.sort(rng.choice(M, size=K, replace=False))
    partner = rng.permutation(N)[:K]
    kp1 = (rng.randint(0, 4 * 600, size=(N, 2)) / 4.0).astype(np.float32)
    matches0 = np.full(M, -1, np.int64)
    planted = np.zeros(M, bool)
    n_in = (K + 1) // 2
    order = rng.permutation(K)
    inl = set(order[:n_in].tolist())
    medium = set(order[n_in:n_in + 4].tolist()) if K >= 16 else set()
    for k in range(K):
        i, j = slots[k], partner[k]
        x1 = warp(H, kp0[i:i + 1].astype(np.float64))[0]
        if k in inl:
            planted[i] = True
        elif k in medium:
            x1 = x1 + np.array([0.0, MEDIUM])
        else:
            ang, r = rng.uniform(0, 2 * np.pi), rng.uniform(50, 120)
            x1 = np.round((x1 + r * np.array([np.cos(ang), np.sin(ang)])) * 4) / 4
            if np.hypot(*(x1 - warp(H, kp0[i:i + 1].astype(np.float64))[0])) < 50:
                x1 = x1 + np.array([60.0, 0.0])
        kp1[j] = x1.astype(np.float32)
        matches0[i] = j
    return {"kpts0": kp0, "kpts1": kp1, "matches0": matches0, "planted": planted, "H": H, "model": model, "seed": seed,
            "range": float(max(np.abs(kp0).max(), np.abs(kp1).max()))}


def scene_is_clean(scene, pair, T, lo_iters=2):
    """The conditions a planted scene has to meet (checked again by test_h_solver_cases_reference.py): an all-inlier sample
    that is not rejected and not in a decision band exists among the T hypotheses; no correspondence's error under the
    winning or a refitted model lies within that model's band of the threshold; the host solver recovers the planted set."""
    res = host_ransac(scene["kpts0"], scene["kpts1"], scene["matches0"], pair, T, lo_iters)
    if not res["success"]:
        return False, res
    fit, idx = res["fit"], res["idx"]
    good = scene["planted"][idx][res["samples"]].all(-1) & fit["ok"] & ~fit["band"]
    dl = delta(fit, scene["range"])
    if not (good & (dl < 0.5)).any():
        return False, res
    band = max(float(dl[res["best"]]), 1e-3)
    for Hm in res["models"]:
        err, w = transfer(Hm, res["corr"])
        if (np.abs(err - TH) <= band).any() or (np.abs(w) < 1e-3).any():
            return False, res
    return bool((res["inliers"] == scene["planted"]).all()), res


@functools.lru_cache(maxsize=None)
def planted_scene(model, K, M, N, pair=0, T=2 * HYPS + 5, seed0=100):
    """The first seed >= seed0 whose scene is clean (scene_is_clean) for hypotheses `T` of pair index `pair`: a scene with
    an error inside a band is regenerated with the next seed, here, deterministically."""
    for seed in range(seed0, seed0 + 50):
        scene = _build_scene(model, K, M, N, seed)
        ok, res = scene_is_clean(scene, pair, T)
        if ok:
            scene["host"] = res
            return scene
    raise AssertionError("no clean scene in 50 seeds")


def small_scene(model, K, M, N, seed=0):
    """A scene for the sampling / scoring comparisons where nothing has to be found (K may be < 4)."""
    return _build_scene(model, K, M, N, 1000 + seed)


# ---- inputs of the metric comparison (tools/gen_homography_eval_golden.py, test_h_solver_cases_reference.py) ----------------
def eval_inputs():
    """Seeded inputs of sym_homography_error / homography_corner_error: 3 homographies, 50 point pairs each, (W, H) sizes."""
    rng = np.random.RandomState(11)
    Hs = np.stack([H_AFFINE, H_PROJ, np.array([[0.9, -0.2, 30.0], [0.15, 1.05, -12.0], [-1e-4, 3e-4, 1.0]])]).astype(np.float32)
    p0 = rng.uniform(0, 600, size=(3, 50, 2)).astype(np.float32)
    p1 = np.stack([warp(Hs[i], p0[i].astype(np.float64)) for i in range(3)]) + rng.normal(0, 2.0, size=(3, 50, 2))
    T = (Hs.astype(np.float64) + rng.normal(0, 1.0, size=(3, 3, 3)) * np.array([[1e-2, 1e-2, 2.0], [1e-2, 1e-2, 2.0], [1e-5, 1e-5, 0.0]]))
    sizes = np.array([[640.0, 480.0], [1024.0, 768.0], [320.0, 240.0]], np.float32)
    return {"H_gt": Hs, "kpts0": p0, "kpts1": p1.astype(np.float32), "T": T.astype(np.float32), "image_size": sizes}


# ---- DLT cases --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dlt_case(name):
    """(p0 [K,2] fp32, p1 [K,2] fp32, weights [K] fp32 or None).  'clean': 40 planted inliers of H_PROJ; 'weighted': the same
    with half of the points moved by 0.5..2 px and weight 1/16 on those (the weights change the answer measurably:
    test_h_solver_cases_reference.py asserts by how much); 'four': exactly four points."""
    rng = np.random.RandomState({"clean": 1, "weighted": 2, "four": 3}[name])
    K = 4 if name == "four" else 40
    flat = rng.choice(RANGE * RANGE, size=K, replace=False)
    p0 = np.stack([flat % RANGE, flat // RANGE], -1).astype(np.float32)
    if name == "four":
        p0 = np.array([[10, 20], [200, 30], [220, 210], [15, 180]], np.float32)
    p1 = warp(H_PROJ, p0.astype(np.float64))
    w = None
    if name == "weighted":
        noisy = np.arange(K) % 2 == 1
        p1[noisy] += np.round(rng.uniform(0.5, 2.0, size=(int(noisy.sum()), 2)) * rng.choice([-1, 1], size=(int(noisy.sum()), 2)) * 8) / 8
        w = np.where(noisy, 1.0 / 16, 1.0).astype(np.float32)
    return p0, p1.astype(np.float32), w


@functools.lru_cache(maxsize=None)
def planted_bound(model, K, M, N):
    """corner_bound on the planted inliers of a planted scene (pair 0): what the solver's result may differ from the truth
    by.  The fp64 restatement reaches 2e-13 px (affine: exact inputs) and 2e-5 .. 1e-4 px (proj: view 1 is rounded to fp32)
    against bounds of 3e-3 .. 2e-2 px; test_h_solver_cases_reference.py prints and asserts both."""
    scene = planted_scene(model, K, M, N, 0)
    idx, corr = compact(scene["kpts0"], scene["kpts1"], scene["matches0"])
    inl = scene["planted"][idx]
    return corner_bound(corr[inl, :2], corr[inl, 2:])
