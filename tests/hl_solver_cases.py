"""Yardstick of the point-and-line homography solver (csrc/hl_solver.hip, csrc/hl_fit.h): numpy fp64 restatements, planted
scenes, derived bounds and the mutations the bounds must catch.  No GPU, no torch.  tests/test_hl_solver_cases_reference.py
tests this module itself; tests/test_gpu_hl_solver.py compares the kernels with it.

The reference's estimator (homography_est) is a CPU package that is not available, so nothing here is compared with it: the
header comments of csrc/hl_solver.hip and csrc/hl_fit.h DEFINE the solver, and this module restates that text.  The sampling
(bit for bit) and the point compaction are tests/ransac_cases.py's; the 8 x 9 fit is restated through numpy.linalg.svd (the
null vector of an 8 x 9 system does not depend on how it is found), with the kernel's own Gauss-Jordan elimination restated
beside it (`fit_gj`) for the pivot test and for the host check of the residual bound."""
import functools
import os
import re

import numpy as np

import h_solver_cases as hc
import ransac_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants():
    text = open(os.path.join(ROOT, "include", "gf_amd.h")).read()
    get = lambda name: re.search(r"#define\s+" + name + r"\s+([0-9.eE+-]+)f?\b", text).group(1)
    return {"TILE": int(get("GF_HL_TILE")), "HYPS": int(get("GF_HL_HYPS")), "EPS_LEN": float(get("GF_HL_EPS_LEN")),
            "EPS_PIVOT": float(get("GF_HL_EPS_PIVOT")), "H22_FRAC": float(get("GF_HL_H22_FRAC")),
            "JACOBI": int(get("GF_HL_JACOBI"))}


_C = header_constants()
TILE, HYPS, EPS_LEN, EPS_PIVOT, H22_FRAC = _C["TILE"], _C["HYPS"], _C["EPS_LEN"], _C["EPS_PIVOT"], _C["H22_FRAC"]
TH = 2.0                      # ransac_th of every case (the reference's default for this estimator)
SEED = 7                      # the solver seed of every case
U32 = 2.0 ** -24              # unit roundoff of fp32: the scoring
U64 = 2.0 ** -53              # unit roundoff of fp64: the in-lane fit (the choice stated in csrc/hl_fit.h)
SIZE = hc.SIZE
warp, corner_error = hc.warp, hc.corner_error
H_AFFINE, H_PROJ = hc.H_AFFINE, hc.H_PROJ
MODELS = hc.MODELS


# ---- compaction of both lists and the index mapping -----------------------------------------------------------------------
def compact_lines(lines0, lines1, line_matches0):
    """Ordered matched indices of the segments of view 0 and their matches [K_l,8] = (p, q, r, s) in fp64.  No match: an
    index outside [0, L1), a non-finite coordinate, a segment shorter than EPS_LEN in either view."""
    lines0 = np.asarray(lines0, np.float64).reshape(-1, 4)
    lines1 = np.asarray(lines1, np.float64).reshape(-1, 4)
    lm = np.asarray(line_matches0)
    ok = (lm >= 0) & (lm < lines1.shape[0])
    if lines1.shape[0] == 0 or lines0.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros((0, 8))
    seg = np.concatenate([lines0, lines1[np.where(ok, lm, 0)]], -1)
    with np.errstate(all="ignore"):
        n0 = (seg[:, 2] - seg[:, 0]) ** 2 + (seg[:, 3] - seg[:, 1]) ** 2
        n1 = (seg[:, 6] - seg[:, 4]) ** 2 + (seg[:, 7] - seg[:, 5]) ** 2
        ok &= np.isfinite(n0) & np.isfinite(n1) & (n0 >= EPS_LEN ** 2) & (n1 >= EPS_LEN ** 2)
    idx = np.nonzero(ok)[0]
    return idx, seg[idx]


def features(scene):
    """Both ordered lists of a scene dict(kpts0 [M,2], kpts1 [N,2], matches0 [M], lines0 [L,2,2], lines1 [L1,2,2],
    line_matches0 [L]) and the joint feature list: feat [K,8] (a point match is (x, y, x, y, u, v, u, v)), isline [K];
    index s < K_p is ordered point match s, otherwise ordered line match s - K_p."""
    if scene["kpts0"].shape[0] and scene["kpts1"].shape[0]:
        idx, corr = rc.compact(scene["kpts0"], scene["kpts1"], scene["matches0"], dtype=np.float64)
    else:
        idx, corr = np.zeros(0, np.int64), np.zeros((0, 4))
    lidx, seg = compact_lines(scene["lines0"], scene["lines1"], scene["line_matches0"])
    pf = np.concatenate([corr[:, :2], corr[:, :2], corr[:, 2:], corr[:, 2:]], -1).reshape(-1, 8)
    return {"idx": idx, "corr": corr, "lidx": lidx, "seg": seg, "Kp": len(idx), "Kl": len(lidx),
            "feat": np.concatenate([pf, seg]), "isline": np.arange(len(idx) + len(lidx)) >= len(idx)}


def samples(seed, pair, T, K, **kw):
    return rc.samples(4, seed, pair, T, K, **kw)


def take(ft, smp, kp_off_by_one=False):
    """The sampled features: (feat [T,4,8], isline [T,4]).  kp_off_by_one: the mutated mapping `s <= K_p` is a point."""
    if not kp_off_by_one:
        return ft["feat"][smp], ft["isline"][smp]
    Kp, Kl = ft["Kp"], ft["Kl"]
    isline = smp > Kp
    pidx = np.minimum(smp, max(Kp - 1, 0))
    lidx = np.clip(smp - Kp - 1, 0, max(Kl - 1, 0))
    pf = ft["feat"][:Kp][pidx] if Kp else np.zeros(smp.shape + (8,))
    lf = ft["feat"][Kp:][lidx] if Kl else np.zeros(smp.shape + (8,))
    return np.where(isline[..., None], lf, pf), isline


def line_of(r, s):
    """Unit-normal line (a, b, c) through r and s [.., 2]: a x + b y + c = 0."""
    with np.errstate(all="ignore"):
        a, b = r[..., 1] - s[..., 1], s[..., 0] - r[..., 0]
        c = r[..., 0] * s[..., 1] - s[..., 0] * r[..., 1]
        n = np.sqrt(a * a + b * b)
        return np.stack([a / n, b / n, c / n], -1)


# ---- the 8 x 9 system ----------------------------------------------------------------------------------------------------
def design(feat, isline, mutation=None):
    """The conditioned system of every sample: (A [T,8,9], T0 [T,3,3], T1 [T,3,3]) with H = T1^-1 G T0.
    mutation = 'swap_views': line rows built from the view-0 LINE and the view-1 ENDPOINTS; 'raw_normal': the line normal
    is not scaled to unit length (the null vector does not notice: only the inlier rule does)."""
    f = np.asarray(feat, np.float64)
    with np.errstate(all="ignore"):
        p0 = f[:, :, :4].reshape(-1, 8, 2)
        p1 = f[:, :, 4:].reshape(-1, 8, 2)
        c0, c1 = p0.mean(1), p1.mean(1)
        s0 = np.sqrt(2.0) / np.sqrt(((p0 - c0[:, None]) ** 2).sum(-1)).mean(1)
        s1 = np.sqrt(2.0) / np.sqrt(((p1 - c1[:, None]) ** 2).sum(-1)).mean(1)
        q0 = ((p0 - c0[:, None]) * s0[:, None, None]).reshape(-1, 4, 2, 2)     # [T, feature, endpoint, xy]
        q1 = ((p1 - c1[:, None]) * s1[:, None, None]).reshape(-1, 4, 2, 2)
        x, y = q0[..., 0], q0[..., 1]                                          # [T,4,2]
        u, v = q1[:, :, 0, 0], q1[:, :, 0, 1]
        one, zero = np.ones_like(u), np.zeros_like(u)
        if mutation == "swap_views":
            ln = line_of(q0[:, :, 0], q0[:, :, 1])
            x, y = np.where(isline[..., None], q1[..., 0], x), np.where(isline[..., None], q1[..., 1], y)
        else:
            ln = line_of(q1[:, :, 0], q1[:, :, 1])
            if mutation == "raw_normal":
                ln = ln * np.sqrt(((q1[:, :, 0] - q1[:, :, 1]) ** 2).sum(-1))[..., None]
        il = isline
        abc = [[np.where(il, ln[..., 0], zero), np.where(il, ln[..., 1], -one), np.where(il, ln[..., 2], v)],
               [np.where(il, ln[..., 0], one), np.where(il, ln[..., 1], zero), np.where(il, ln[..., 2], -u)]]
        rows = []
        for e in range(2):
            xe, ye = x[..., e], y[..., e]
            rows.append(np.stack([k * t for k in abc[e] for t in (xe, ye, one)], -1))       # [T,4,9]
        A = np.stack(rows, 2).reshape(-1, 8, 9)
    T = f.shape[0]
    T0, T1 = np.zeros((T, 3, 3)), np.zeros((T, 3, 3))
    for Tm, s, c in ((T0, s0, c0), (T1, s1, c1)):
        Tm[:, 0, 0] = Tm[:, 1, 1] = s
        Tm[:, 0, 2], Tm[:, 1, 2], Tm[:, 2, 2] = -s * c[:, 0], -s * c[:, 1], 1.0
    return A, T0, T1


def gauss_jordan(A):
    """The kernel's elimination on A [T,8,9] in numpy fp64: full pivoting in place, the first largest entry in row-major
    order.  Returns (g [T,9] null vector with the free entry 1, pivots [T,8] magnitudes in the order taken)."""
    A = np.array(A, np.float64)
    T = A.shape[0]
    rows_used, cols_used = np.zeros((T, 8), bool), np.zeros((T, 9), bool)
    pcol = np.full((T, 8), -1)
    pivots = np.zeros((T, 8))
    ar = np.arange(T)
    with np.errstate(all="ignore"):
        for step in range(8):
            mag = np.where(rows_used[:, :, None] | cols_used[:, None, :], -1.0, np.abs(A))
            mag = np.where(np.isnan(mag), -1.0, mag)
            flat = mag.reshape(T, -1).argmax(1)
            br, bc = flat // 9, flat % 9
            best = mag.reshape(T, -1)[ar, flat]
            pivots[:, step] = np.where(best < 0, np.nan, best)
            rows_used[ar, br], cols_used[ar, bc] = True, True
            pcol[ar, br] = bc
            row = A[ar, br] / A[ar, br, bc][:, None]
            row[ar, bc] = 1.0
            fac = A[ar, :, bc]                                   # [T,8]
            A = A - fac[:, :, None] * row[:, None, :]
            A[ar, :, bc] = 0.0
            A[ar, br] = row
        fc = (~cols_used).argmax(1)
        g = np.zeros((T, 9))
        g[ar, fc] = 1.0
        for i in range(8):
            g[ar, pcol[:, i]] = -A[ar, i, fc]
    return g, pivots


def _finish(g, T0, T1, feat, isline, cond, pivots):
    """De-normalisation, the rejections and their decision bands, from the conditioned null vector g [T,9].  A sample of two
    point matches and two line matches is rejected outright (csrc/hl_fit.h: its system always has a rank-one solution)."""
    two_two = np.asarray(isline).sum(-1) == 2
    with np.errstate(all="ignore"):
        G = g.reshape(-1, 3, 3)
        T1i = np.zeros_like(T1)                                  # T1^-1 = [[1/s, 0, cx], [0, 1/s, cy], [0, 0, 1]]
        T1i[:, 0, 0] = T1i[:, 1, 1] = 1.0 / T1[:, 0, 0]
        T1i[:, 0, 2], T1i[:, 1, 2], T1i[:, 2, 2] = -T1[:, 0, 2] / T1[:, 0, 0], -T1[:, 1, 2] / T1[:, 0, 0], 1.0
        H = T1i @ G @ T0
        fro = np.sqrt((H ** 2).sum((-1, -2)))
        ratio = np.abs(H[:, 2, 2]) / fro
        Hn = H / H[:, 2:, 2:]
        pts = np.asarray(feat, np.float64)[:, :, :4].reshape(-1, 8, 2)
        wabs = np.abs(Hn[:, 2, :1] * pts[..., 0]) + np.abs(Hn[:, 2, 1:2] * pts[..., 1]) + 1.0
        w = Hn[:, 2, :1] * pts[..., 0] + Hn[:, 2, 1:2] * pts[..., 1] + 1.0
        pmin = np.nanmin(np.where(np.isnan(pivots), -1.0, pivots), 1)
        finite = np.isfinite(Hn.astype(np.float32)).all((-1, -2))
        ok = (pmin >= EPS_PIVOT) & (ratio >= H22_FRAC) & finite & (w > 0).all(-1) & ~two_two
        # decision bands.  The pivots: a different order of equal candidates, or a fused multiply-add, changes the later
        # pivots by the growth of the elimination, so a smallest pivot within a factor 100 of the threshold may fall either
        # way; so may everything computed from a system too ill-conditioned for fp64 to say (cond > 1e10).  The h22 test:
        # 1 % of the threshold plus the fit's error 1e3 u cond.  The w test: the fit's error on w, relative to its terms.
        err = 1e3 * U64 * np.where(np.isfinite(cond), cond, 1e300)
        band = ((pmin >= EPS_PIVOT / 100) & (pmin <= EPS_PIVOT * 100)) | ((pmin >= EPS_PIVOT / 100) & ~(cond <= 1e10))
        live = pmin >= EPS_PIVOT / 100
        band |= live & (np.abs(ratio - H22_FRAC) <= 1e-2 * H22_FRAC + err)
        band |= live & (np.abs(w) <= (1e-9 + err[:, None]) * wabs).any(-1)
        band &= np.isfinite(pmin) & ~two_two
    return {"H": Hn, "ok": ok, "band": band, "cond": cond, "pivot": pmin}


def fit(feat, isline, mutation=None):
    """The fit of every sample through numpy.linalg.svd: dict(H [T,3,3] with h22 == 1, ok [T], band [T] (a rejection that
    may fall either way on the device), cond [T] = s_1 / s_8 of the conditioned design matrix, pivot [T])."""
    A, T0, T1 = design(feat, isline, mutation)
    bad = ~np.isfinite(A).all((-1, -2))
    As = np.where(bad[:, None, None], 0.0, A)
    with np.errstate(all="ignore"):
        _, S, Vt = np.linalg.svd(As, full_matrices=True)
        cond = np.where(bad, np.inf, S[:, 0] / S[:, 7])
        _, pivots = gauss_jordan(A)
    pivots[bad] = np.nan
    return _finish(Vt[:, -1], T0, T1, feat, isline, cond, pivots)


def fit_gj(feat, isline, mutation=None):
    """The same fit by the kernel's own algorithm in numpy fp64 (the chosen arithmetic): for the host check of fit_bound."""
    A, T0, T1 = design(feat, isline, mutation)
    g, pivots = gauss_jordan(A)
    with np.errstate(all="ignore"):
        S = np.linalg.svd(np.where(np.isfinite(A), A, 0.0), compute_uv=False)
        cond = S[:, 0] / S[:, 7]
    return _finish(g, T0, T1, feat, isline, cond, pivots)


# ---- both inlier rules ---------------------------------------------------------------------------------------------------
def project(H, pts):
    """(X [..,K], Y, w, terms) of models H [..,3,3] on points [K,2]; terms = the magnitudes the fp32 error scales with."""
    H = np.asarray(H, np.float64)[..., None, :, :]
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(all="ignore"):
        nx = H[..., 0, 0] * x + H[..., 0, 1] * y + H[..., 0, 2]
        ny = H[..., 1, 0] * x + H[..., 1, 1] * y + H[..., 1, 2]
        w = H[..., 2, 0] * x + H[..., 2, 1] * y + H[..., 2, 2]
        sx = np.abs(H[..., 0, 0] * x) + np.abs(H[..., 0, 1] * y) + np.abs(H[..., 0, 2])
        sy = np.abs(H[..., 1, 0] * x) + np.abs(H[..., 1, 1] * y) + np.abs(H[..., 1, 2])
        sw = np.abs(H[..., 2, 0] * x) + np.abs(H[..., 2, 1] * y) + np.abs(H[..., 2, 2])
        X, Y = nx / w, ny / w
        # rounding of X and Y: three rounded operations in each numerator and in w, the reciprocal and the product
        dxy = 4 * U32 * ((sx + sy) / np.abs(w) + (np.abs(X) + np.abs(Y)) * (sw / np.abs(w) + 1.0))
    return X, Y, w, {"dxy": dxy, "sw": sw}


def point_errors(H, corr):
    """(err [..,K_p], w, delta): forward transfer error, the denominator, and the fp32 band of err (see `delta`)."""
    X, Y, w, t = project(H, corr[:, :2])
    with np.errstate(all="ignore"):
        err = np.sqrt((X - corr[:, 2]) ** 2 + (Y - corr[:, 3]) ** 2)
        dl = 2 * (t["dxy"] + 4 * U32 * (err + TH))
    return err, w, dl, 8 * U32 * t["sw"]


def line_errors(H, seg, one_endpoint=False, raw_normal=False):
    """(err [..,K_l] = max of the two endpoint-to-line distances, w = min of the two denominators, delta, wband).
    one_endpoint / raw_normal: the mutations (only p is tested; the normal keeps the segment's length)."""
    ln = line_of(seg[:, 4:6], seg[:, 6:8])
    if raw_normal:
        ln = ln * np.sqrt(((seg[:, 4:6] - seg[:, 6:8]) ** 2).sum(-1))[:, None]
    out = []
    for e in range(2):
        X, Y, w, t = project(H, seg[:, 2 * e:2 * e + 2])
        with np.errstate(all="ignore"):
            d = np.abs(ln[:, 0] * X + ln[:, 1] * Y + ln[:, 2])
            # |a|, |b| <= 1 carry X's and Y's error; (a, b, c) are rounded to fp32; three rounded operations in the sum
            dl = 2 * (t["dxy"] + 4 * U32 * (np.abs(X) + np.abs(Y) + np.abs(ln[:, 2]) + TH))
        out.append((d, w, dl, 8 * U32 * t["sw"]))
    if one_endpoint:
        return out[0]
    with np.errstate(all="ignore"):
        return (np.maximum(out[0][0], out[1][0]), np.minimum(out[0][1], out[1][1]), np.maximum(out[0][2], out[1][2]),
                np.maximum(out[0][3], out[1][3]))


def _mask(err, w, th):
    with np.errstate(invalid="ignore"):
        return (w > 0) & np.isfinite(w) & (err < th)


def inlier_masks(H, ft, th=TH, **kw):
    """(point mask [..,K_p], line mask [..,K_l]) of models H."""
    pe, pw = point_errors(H, ft["corr"])[:2]
    le, lw = line_errors(H, ft["seg"], **kw)[:2]
    return _mask(pe, pw, th), _mask(le, lw, th)


def counts(H, ft, th=TH, ignore_lines=False, **kw):
    """[T,2] (point inliers, line inliers) of models H [T,3,3]."""
    pm, lm = inlier_masks(H, ft, th, **kw)
    nl = lm.sum(-1)
    return np.stack([pm.sum(-1), np.zeros_like(nl) if ignore_lines else nl], -1)


def delta(H, ft):
    """The scoring band around th, per (model, feature): (point deltas [T,K_p], line deltas [T,K_l]) in pixels.
    Derivation (fp32, unit roundoff u = 2^-24, evaluated on the model the kernel itself scores, so no error of the fit
    enters).  w and the two numerators are sums of three terms, each with at most three rounded operations:
    |dw| <= 3 u Sw, |dnx| <= 3 u Sx with S. the sum of the terms' magnitudes.  X = nx (1 / w) adds two roundings:
    |dX| <= (3 u Sx + |X| 3 u Sw) / |w| + 2 u |X|, the same for Y; together <= 4 u ((Sx + Sy) / |w| + (|X| + |Y|) (Sw / |w| + 1)).
    Point rule: the differences, squares, sum and the comparison with th^2 add at most 4 u (err + th) on the error itself.
    Line rule: with |a|, |b| <= 1 the distance carries |dX| + |dY|; a, b, c are fp32 roundings of fp64 values and the
    three-term sum rounds three times: 4 u (|X| + |Y| + |c| + th).  Both are doubled for the second-order terms.  A
    denominator within 8 u Sw of zero may take either sign.  Nothing here is tuned on a GPU."""
    return point_errors(H, ft["corr"])[2], line_errors(H, ft["seg"])[2]


def count_band(H, ft, th=TH):
    """(lo [T,2], hi [T,2]): what is an inlier whatever fp32 decides, and what may be one, for models H [T,3,3]."""
    out = []
    for err, w, dl, wb in (point_errors(H, ft["corr"]), line_errors(H, ft["seg"])):
        with np.errstate(invalid="ignore"):
            lo = ((w > wb) & (err < th - dl)).sum(-1)
            hi = (((w > -wb) & (err < th + dl)) | (np.abs(w) <= wb) | ~np.isfinite(err)).sum(-1)
        out.append((lo, hi))
    return np.stack([out[0][0], out[1][0]], -1), np.stack([out[0][1], out[1][1]], -1)


# ---- the residual of a fit on its own sample and its bound -------------------------------------------------------------------
def sample_residual(H, feat, isline):
    """[T] the largest residual of model H [T,3,3] on its own four features [T,4,8]: the transfer error of a point match,
    the endpoint-to-line distances of a line match, in pixels."""
    out = np.zeros(len(H))
    for t in range(len(H)):
        r = 0.0
        for i in range(4):
            f = feat[t, i]
            if isline[t, i]:
                r = max(r, float(line_errors(H[t], f[None])[0][0]))
            else:
                r = max(r, float(point_errors(H[t], f[None, [0, 1, 4, 5]])[0][0]))
        out[t] = r
    return out


FIT_FACTOR = 256.0


def fit_bound(ft_fit, feat, coord_range):
    """Bound on sample_residual of an accepted fit whose nine entries were rounded to fp32, per hypothesis [T], in pixels:
        FIT_FACTOR u64 cond coord_range  +  the rounding of the nine fp32 entries.
    First term: the null vector of the conditioned 8 x 9 system from a backward-stable elimination (full pivoting) has a
    relative error of order u cond(A), cond = s_1 / s_8 from the fp64 singular values of the sample's design matrix; in the
    conditioned frame coordinates are of order one, so that is the residual there, and a conditioned unit is at most
    coord_range pixels.  FIT_FACTOR = 256 is the operation count: every entry passes through at most 8 eliminations of two
    rounded operations, 3 more build the row, 6 the de-normalisation and the division by h22, 4 the residual, about 32;
    times sqrt(72) ~ 8 from the norm-wise error of the 72 entries to one component.  u64 = 2^-53: the fit is fp64.
    Second term: h_e (1 + d_e), |d_e| <= 2^-24, moves X by at most u32 (Sx + |X| Sw) / |w| (first order, see `delta`), summed
    over X and Y, the worst of the sample's eight view-0 points, doubled for the second order."""
    H = ft_fit["H"]
    rnd = np.zeros(len(H))
    for t in range(len(H)):
        pts = np.asarray(feat[t], np.float64)[:, :4].reshape(8, 2)
        with np.errstate(all="ignore"):
            rnd[t] = np.nanmax(project(H[t], pts)[3]["dxy"]) / 4 * 2
    with np.errstate(all="ignore"):
        return FIT_FACTOR * U64 * ft_fit["cond"] * coord_range + rnd


# ---- the refit ---------------------------------------------------------------------------------------------------------------
def refit_batch(corr, seg):
    """`refit` on P feature sets at once: corr [P,n_p,4], seg [P,n_l,8] -> (H [P,3,3], ok [P])."""
    corr, seg = np.asarray(corr, np.float64), np.asarray(seg, np.float64)
    P = corr.shape[0]
    if corr.shape[1] + seg.shape[1] < 4:
        return np.tile(np.eye(3), (P, 1, 1)), np.zeros(P, bool)
    p0 = np.concatenate([corr[:, :, :2], seg[:, :, 0:2], seg[:, :, 2:4]], 1)
    p1 = np.concatenate([corr[:, :, 2:], seg[:, :, 4:6], seg[:, :, 6:8]], 1)

    def norm(p):
        c = p.mean(1)
        s = np.sqrt(2.0) / np.sqrt(((p - c[:, None]) ** 2).sum(-1)).mean(1)
        return c[:, None], s[:, None, None]

    with np.errstate(all="ignore"):
        (c0, s0), (c1, s1) = norm(p0), norm(p1)
        n0, n1 = lambda p: (p - c0) * s0, lambda p: (p - c1) * s1
        a, b = n0(corr[:, :, :2]), n1(corr[:, :, 2:])
        x, y, u, v = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
        o, z = np.ones_like(x), np.zeros_like(x)
        rows = [np.stack([z, z, z, -x, -y, -o, v * x, v * y, v], -1), np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], -1)]
        ln = line_of(n1(seg[:, :, 4:6]), n1(seg[:, :, 6:8]))
        for e in range(2):
            q = n0(seg[:, :, 2 * e:2 * e + 2])
            rows.append(np.stack([ln[..., k] * t for k in range(3) for t in (q[..., 0], q[..., 1], np.ones(seg.shape[:2]))], -1))
        A = np.concatenate(rows, 1)
        bad = ~np.isfinite(A).all((-1, -2))
        G = np.linalg.svd(np.where(bad[:, None, None], 0.0, A), full_matrices=A.shape[1] < 9)[2][:, -1].reshape(P, 3, 3)
        T0, T1i = np.zeros((P, 3, 3)), np.zeros((P, 3, 3))
        T0[:, 0, 0] = T0[:, 1, 1] = s0[:, 0, 0]
        T0[:, 0, 2], T0[:, 1, 2], T0[:, 2, 2] = -s0[:, 0, 0] * c0[:, 0, 0], -s0[:, 0, 0] * c0[:, 0, 1], 1.0
        T1i[:, 0, 0] = T1i[:, 1, 1] = 1.0 / s1[:, 0, 0]
        T1i[:, 0, 2], T1i[:, 1, 2], T1i[:, 2, 2] = c1[:, 0, 0], c1[:, 0, 1], 1.0
        H = T1i @ G @ T0
        ok = ~bad & np.isfinite(H).all((-1, -2)) & (np.abs(H[:, 2, 2]) >= H22_FRAC * np.sqrt((H ** 2).sum((-1, -2))))
        H = H / H[:, 2:, 2:]
        ok &= np.isfinite(H.astype(np.float32)).all((-1, -2))
    return H, ok


def refit(corr, seg):
    """Hartley-normalised DLT over point matches corr [n_p,4] and line matches seg [n_l,8] in fp64 through numpy.linalg.svd:
    view 0 is normalised over the points and the endpoints p, q, view 1 over the points and the endpoints r, s; the view-1
    lines are rebuilt from the normalised endpoints with unit normal; two rows per feature.  H [3,3] with h22 == 1, or None
    with fewer than 4 features, |h22| < H22_FRAC ||H||_F or a non-finite entry."""
    H, ok = refit_batch(np.asarray(corr, np.float64)[None], np.asarray(seg, np.float64)[None])
    return H[0] if ok[0] else None


# ---- host RANSAC (fp64): what the kernels are compared with ----------------------------------------------------------------
def host_ransac(scene, pair, T, lo_iters=2, seed=SEED, th=TH, fit_mutation=None, kp_off_by_one=False, **rule):
    """The solver in fp64.  rule: ignore_lines / one_endpoint / raw_normal (the mutations of the scoring).  Returns
    dict(H, inliers [M] bool, line_inliers [L] bool, num (points, lines), success, samples [T,4], fit (see `fit`), counts
    [T,2] (-1 where rejected), models, ft, best)."""
    ft = features(scene)
    K, M, L = ft["Kp"] + ft["Kl"], scene["kpts0"].shape[0], np.asarray(scene["lines0"]).reshape(-1, 4).shape[0]
    smp = samples(seed, pair, T, K)
    none = {"H": np.eye(3), "inliers": np.zeros(M, bool), "line_inliers": np.zeros(L, bool), "num": (0, 0), "success": False,
            "samples": smp, "fit": None, "counts": np.full((T, 2), -1), "models": [], "ft": ft}
    if K < 4:
        return none
    feat, isline = take(ft, smp, kp_off_by_one)
    fr = fit(feat, isline, fit_mutation)
    flag_rule = {k: v for k, v in rule.items() if k != "ignore_lines"}
    cnt = counts(np.where(fr["ok"][:, None, None], fr["H"], np.zeros((3, 3))), ft, th, **rule)
    cnt = np.where(fr["ok"][:, None], cnt, -1)
    none.update(fit=fr, counts=cnt, feat=feat, isline=isline)
    if not fr["ok"].any():
        return none
    best = int(np.argmax(cnt.sum(-1)))                               # the first maximum: the lowest index of a tie
    H = fr["H"][best]
    pm, lm = inlier_masks(H, ft, th, **flag_rule)
    total = lambda a, b: int(a.sum()) + (0 if rule.get("ignore_lines") else int(b.sum()))
    models = [H]
    for _ in range(lo_iters):
        Hn = refit(ft["corr"][pm], ft["seg"][lm])
        if Hn is None:
            continue
        models.append(Hn)
        pn, ln = inlier_masks(Hn, ft, th, **flag_rule)
        if total(pn, ln) >= total(pm, lm):
            H, pm, lm = Hn, pn, ln
    inl, linl = np.zeros(M, bool), np.zeros(L, bool)
    inl[ft["idx"][pm]] = True
    linl[ft["lidx"][lm]] = True
    return {"H": H, "inliers": inl, "line_inliers": linl, "num": (int(pm.sum()), int(lm.sum())), "success": True, "samples": smp,
            "fit": fr, "counts": cnt, "models": models, "ft": ft, "best": best, "feat": feat, "isline": isline}


# ---- planted scenes ----------------------------------------------------------------------------------------------------------
RANGE = 256                                   # lattice [0, RANGE)^2 in view 0


def _dist(ln, p):
    return abs(ln[0] * p[0] + ln[1] * p[1] + ln[2])


def build_scene(model, Kp, Kl, M, N, L, L1, seed, n_in_p=None, n_in_l=None):
    """Kp point matches among M / N keypoints and Kl line matches among L / L1 segments under the planted homography, with
    50 % outliers in both lists (ceil(K / 2) inliers unless n_in_* says otherwise).
    Points: inliers x1 = fp32(H x0) on distinct integer lattice points; outliers displaced by 50..120 px.
    Lines: view-0 segments of 20..80 px from a lattice point; an inlier's view-1 endpoints are H p, H q SLID ALONG THE LINE by
    random amounts (from -60 % to +60 % of the segment at either end, partial overlaps included, at least 10 px left), so the
    endpoints do not correspond, only the lines do; an outlier's view-1 line lies at least 50 px from both H p and H q.
    Unmatched keypoints and segments are random; matched slots and partners are scattered by random permutations."""
    rng = np.random.RandomState(seed)
    H = MODELS[model]
    flat = rng.choice(RANGE * RANGE, size=max(M, 1), replace=False)[:M]
    kp0 = np.stack([flat % RANGE, flat // RANGE], -1).astype(np.float32).reshape(M, 2)
    kp1 = (rng.randint(0, 4 * 600, size=(N, 2)) / 4.0).astype(np.float32)
    m0, planted = np.full(M, -1, np.int64), np.zeros(M, bool)
    slots, partner = np.sort(rng.choice(M, size=Kp, replace=False)) if Kp else [], rng.permutation(N)[:Kp]
    n_in = (Kp + 1) // 2 if n_in_p is None else n_in_p
    inl = set(rng.permutation(Kp)[:n_in].tolist())
    for k in range(Kp):
        i, j = slots[k], partner[k]
        x1 = warp(H, kp0[i:i + 1].astype(np.float64))[0]
        if k in inl:
            planted[i] = True
        else:
            ang, r = rng.uniform(0, 2 * np.pi), rng.uniform(50, 120)
            x1 = np.round((x1 + r * np.array([np.cos(ang), np.sin(ang)])) * 4) / 4
            if np.hypot(*(x1 - warp(H, kp0[i:i + 1].astype(np.float64))[0])) < 50:
                x1 = x1 + np.array([60.0, 0.0])
        kp1[j] = x1.astype(np.float32)
        m0[i] = j

    def segment():
        p = rng.randint(0, RANGE, size=2).astype(np.float64)
        ang, ln = rng.uniform(0, 2 * np.pi), rng.uniform(20, 80)
        return np.stack([p, np.round((p + ln * np.array([np.cos(ang), np.sin(ang)])) * 4) / 4])

    l0 = np.array([segment() for _ in range(L)], np.float32).reshape(L, 2, 2)
    l1 = np.array([segment() * 2 for _ in range(L1)], np.float32).reshape(L1, 2, 2)
    lm0, lplanted = np.full(L, -1, np.int64), np.zeros(L, bool)
    lslots, lpartner = np.sort(rng.choice(L, size=Kl, replace=False)) if Kl else [], rng.permutation(L1)[:Kl]
    n_in = (Kl + 1) // 2 if n_in_l is None else n_in_l
    linl = set(rng.permutation(Kl)[:n_in].tolist())
    for k in range(Kl):
        i, j = lslots[k], lpartner[k]
        r, s = warp(H, l0[i].astype(np.float64))
        if k in linl:
            lplanted[i] = True
            while True:
                al, be = rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6)
                r2, s2 = r + al * (s - r), s + be * (s - r)
                if np.hypot(*(s2 - r2)) >= 10.0 and np.dot(s2 - r2, s - r) > 0:
                    break
        else:
            while True:
                mid, d = (r + s) / 2, (s - r) / np.hypot(*(s - r))
                nrm = np.array([-d[1], d[0]])
                ang = np.arctan2(d[1], d[0]) + rng.uniform(-0.5, 0.5)
                c = mid + rng.choice([-1, 1]) * rng.uniform(60, 120) * nrm
                half = rng.uniform(10, 40) * np.array([np.cos(ang), np.sin(ang)])
                r2, s2 = np.round((c - half) * 4) / 4, np.round((c + half) * 4) / 4
                ln = line_of(r2.astype(np.float32).astype(np.float64), s2.astype(np.float32).astype(np.float64))
                if min(_dist(ln, r), _dist(ln, s)) >= 50.0:
                    break
        l1[j] = np.stack([r2, s2]).astype(np.float32)
        lm0[i] = j
    rng_all = [np.abs(a).max() for a in (kp0, kp1, l0, l1) if a.size]
    return {"kpts0": kp0, "kpts1": kp1, "matches0": m0, "lines0": l0, "lines1": l1, "line_matches0": lm0, "planted": planted,
            "line_planted": lplanted, "H": H, "model": model, "seed": seed, "range": float(max(rng_all))}


SCENE_BAND = 1e-2             # pixels: the least band a scene keeps clear of the threshold; a larger fp32 delta (see `delta`) replaces it


def scene_is_clean(scene, pair, T, lo_iters=2):
    """The conditions a planted scene has to meet, so that the host restatement alone decides the result:
    the host recovers exactly the planted sets; the winner's margin holds -- every hypothesis that could reach the winner's
    count, once the features within SCENE_BAND (or their own fp32 delta, if larger) of the threshold under it are granted to it, has none such and is in no
    rejection band (its count and its rejection are certain, so the device ranks it as the host does); no feature lies within
    SCENE_BAND of the threshold under the winning or a refitted model; no matched segment's length lies at EPS_LEN."""
    res = host_ransac(scene, pair, T, lo_iters)
    if not res["success"]:
        return False, res
    ft, fr = res["ft"], res["fit"]
    if not ((res["inliers"] == scene["planted"]).all() and (res["line_inliers"] == scene["line_planted"]).all()):
        return False, res
    Hs = np.where((fr["ok"] | fr["band"])[:, None, None], fr["H"], np.zeros((3, 3)))
    pe, pw, pd, _ = point_errors(Hs, ft["corr"])
    le, lw, ld, _ = line_errors(Hs, ft["seg"])
    with np.errstate(invalid="ignore"):
        near = lambda e, w, d: ((np.abs(e - TH) <= np.maximum(d, SCENE_BAND)) | (np.abs(w) <= 1e-3) |
                                (~np.isfinite(e) & np.isfinite(w))).sum(-1)
        nb = near(pe, pw, pd) + near(le, lw, ld)
        reach = (_mask(pe, pw, TH).sum(-1) + _mask(le, lw, TH).sum(-1) + nb) * (fr["ok"] | fr["band"])
    top = int(res["counts"][res["best"]].sum())
    rivals = reach >= top
    if (nb[rivals] > 0).any() or fr["band"][rivals].any():
        return False, res
    for Hm in res["models"]:
        for e, w, d, _ in (point_errors(Hm, ft["corr"]), line_errors(Hm, ft["seg"])):
            if (np.abs(e - TH) <= np.maximum(d, SCENE_BAND)).any() or (np.abs(w) < 1e-3).any():
                return False, res
    raw = np.concatenate([np.asarray(scene["lines0"], np.float64).reshape(-1, 4)[scene["line_matches0"] >= 0],
                          np.asarray(scene["lines1"], np.float64).reshape(-1, 4)[scene["line_matches0"][scene["line_matches0"] >= 0]]])
    lens = np.hypot(raw[:, 2] - raw[:, 0], raw[:, 3] - raw[:, 1])
    return bool((np.abs(lens - EPS_LEN) > 1e-3).all()), res


# (model, Kp, Kl, M, N, L, L1, point inliers or None, line inliers or None): points only, lines only, mixed with one feature
# more than a scoring tile in either list, and the scene that needs its lines: 3 point inliers, 40 line inliers
PLANTED = {
    "points": ("proj", 40, 0, 64, 50, 6, 5, None, None),
    "lines": ("proj", 0, 40, 9, 7, 55, 48, None, None),
    "mixed": ("proj", TILE + 1, TILE + 1, TILE + 38, TILE + 51, TILE + 20, TILE + 9, None, None),
    "lines_needed": ("affine", 6, 80, 12, 10, 90, 85, 3, 40),
}
T_FULL = 2 * HYPS + 5


@functools.lru_cache(maxsize=None)
def planted_scene(name, pair=0, T=T_FULL, seed0=100):
    """The first seed >= seed0 whose scene is clean (scene_is_clean) for hypotheses `T` of pair index `pair`."""
    model, Kp, Kl, M, N, L, L1, nip, nil = PLANTED[name]
    for seed in range(seed0, seed0 + 50):
        scene = build_scene(model, Kp, Kl, M, N, L, L1, seed, nip, nil)
        ok, res = scene_is_clean(scene, pair, T)
        if ok:
            scene["host"] = res
            return scene
    raise AssertionError("no clean scene in 50 seeds")


BAND_CAP = 0.01               # share of the hypotheses that may be decided differently inside a rejection band


@functools.lru_cache(maxsize=None)
def small_scene(Kp, Kl, M, N, L, L1, pair=0, T=HYPS + 1, seed0=0):
    """A scene for the sampling / fit / scoring comparisons where nothing has to be found (Kp + Kl may be < 4): the first
    seed whose share of hypotheses inside a rejection band stays under half of BAND_CAP on the host."""
    for seed in range(1000 + seed0, 1050 + seed0):
        scene = build_scene("proj", Kp, Kl, M, N, L, L1, seed)
        ft = features(scene)
        if ft["Kp"] + ft["Kl"] < 4:
            return scene
        feat, isline = take(ft, samples(SEED, pair, T, ft["Kp"] + ft["Kl"]))
        if fit(feat, isline)["band"].sum() <= 0.5 * BAND_CAP * T:
            return scene
    raise AssertionError("no scene under the band cap in 50 seeds")


# ---- the refit's first-order bound ---------------------------------------------------------------------------------------------
DLT_FACTOR = 4.0


def corner_bound(corr, seg, size=SIZE):
    """hc.corner_bound for the two-part refit: the bound on the corner error between two correct evaluations of `refit` on
    these features, one of which sees its fp32 inputs perturbed by half an ulp each and rounds its nine outputs to fp32:
        sum_j |d corner / d input_j| ulp32(input_j) / 2  +  sum_e |d corner / d h_e| ulp32(h_e) / 2
    (central differences of the fp64 restatement, the worst corner), times DLT_FACTOR = 4 for the second-order terms and the
    fp64 arithmetic of two different eigen-solvers (Jacobi sweeps against an SVD)."""
    corr, seg = np.asarray(corr, np.float64), np.asarray(seg, np.float64)
    W, Hh = size
    corners = np.array([[0, 0], [W, 0], [W, Hh], [0, Hh]], np.float64)
    H = refit(corr, seg)
    total = np.zeros(4)
    warp_all = lambda Hs: np.stack([warp(Hm, corners) for Hm in Hs])
    for which, arr in enumerate((corr, seg)):
        n, width = arr.shape
        if n == 0:
            continue
        v = arr.reshape(-1)
        step = np.maximum(np.abs(v), 1.0) * 1e-6
        out = []
        for sgn in (1, -1):                               # every input perturbed on its own: n * width feature sets at once
            pert = np.tile(arr.reshape(1, -1), (n * width, 1))
            pert[np.arange(n * width), np.arange(n * width)] += sgn * step
            q = [np.tile(corr[None], (n * width, 1, 1)), np.tile(seg[None], (n * width, 1, 1))]
            q[which] = pert.reshape(n * width, n, width)
            out.append(warp_all(refit_batch(q[0], q[1])[0]))
        deriv = np.sqrt((((out[0] - out[1]) / (2 * step[:, None, None])) ** 2).sum(-1))           # [inputs, 4]
        total += (deriv * (np.spacing(np.abs(v).astype(np.float32)).astype(np.float64) / 2)[:, None]).sum(0)
    for e in range(8):
        Hp, Hm = H.copy(), H.copy()
        step = max(abs(H.flat[e]), 1e-6) * 1e-6
        Hp.flat[e] += step
        Hm.flat[e] -= step
        deriv = np.sqrt((((warp(Hp, corners) - warp(Hm, corners)) / (2 * step)) ** 2).sum(-1))
        total += deriv * np.spacing(np.float32(abs(H.flat[e]))) / 2
    return DLT_FACTOR * float(total.max())


def planted_features(scene):
    """(corr, seg) of the planted inliers of a scene, in the order of the ordered lists."""
    ft = features(scene)
    return ft["corr"][scene["planted"][ft["idx"]]], ft["seg"][scene["line_planted"][ft["lidx"]]]


@functools.lru_cache(maxsize=None)
def planted_bound(name, pair=0):
    return corner_bound(*planted_features(planted_scene(name, pair)))


@functools.lru_cache(maxsize=None)
def four_feature_scene(M, N, L, L1, pair, Kp=3, Kl=1, T=T_FULL, seed0=300):
    """Exactly four matches, all planted (every hypothesis is a permutation of the same sample): the first seed whose sample
    the host accepts outside every band and whose four errors keep clear of the threshold."""
    for seed in range(seed0, seed0 + 50):
        scene = build_scene("proj", Kp, Kl, M, N, L, L1, seed, Kp, Kl)
        ok, res = scene_is_clean(scene, pair, T)
        if ok and res["fit"]["ok"].all() and not res["fit"]["band"].any():
            scene["host"] = res
            return scene
    raise AssertionError("no clean scene in 50 seeds")
