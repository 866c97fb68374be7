"""What tests/test_gpu_homography_views.py measures csrc/hviews.hip with: seeded inputs, fp64 restatements of both kernels
(contract: include/gf_amd.h, arithmetic: the header comment of csrc/hviews.hip), the error bound of every output pixel and the
mutations each bound has to reject.  No GPU code and no library code here; tests/test_homography_views_reference.py holds
this file against independent formulations (grid_sample, conv2d).

THE BOUND (u = 2^-24, the unit roundoff of fp32).  Nothing below is a tolerance chosen by hand; each term is a rounding the
device performs, carried through the stage that follows it.
 1. Coordinates.  nx = fmaf(h00, x, fmaf(h01, y, h02)) rounds twice, each by at most u times the magnitude of a partial sum
    that never exceeds Mx = |h00 x| + |h01 y| + |h02|: |dnx| <= 2 u Mx, likewise |dd| <= 2 u Md.  sx = nx / d is one more
    rounding, so to first order |dsx| <= (2 u Mx + |sx| 2 u Md) / |d| + u |sx|.  E_x is TWICE that (second-order terms and a
    division that is within 1 ulp rather than correctly rounded); E_y alike.  fx = sx - floorf(sx) is exact.
 2. Sampling.  Bilinear interpolation of the zero-extended image is continuous and piecewise bilinear; inside one cell its
    x-slope is at most the larger horizontal tap difference.  A coordinate error below a quarter pixel keeps the point in its
    cell or moves it to a neighbour (a floorf that flips between device and host), so with Gx, Gy the largest horizontal /
    vertical differences of zero-extended taps in the 4 x 4 neighbourhood around the cell, |dv| <= Gx E_x + Gy E_y.  Pixels
    with E > 1/4 px or |d| < 1e-6 (next to a horizon) get an infinite bound: only their finiteness is checked.
 3. The three fmaf of the interpolation and their three differences: 12 u Tmax (Tmax = the largest tap), and u |v| for the
    division by 255 of a uint8 source.
 4. powf: monotone on v >= 0, so the input interval [v - e, v + e] maps to an output interval exactly; plus 4 u |result| for
    a powf within 2 ulp.
 5. Value shift: C = 1 is 1-Lipschitz (+ 2 u); C = 3 is v_c k(m), k(m) = clamp(m + s, 0, 1) / m: e <- k e_c + v_c |dk| with dk
    from the interval of m, + 4 u |result|.  For s < 0, k vanishes on m <= -s, so black stays black and k is continuous; s > 0 at
    m -> 0 is not, and gets an infinite bound (the presets never draw s > 0).
 6. Post stage clamp(fmaf(a, v, b), 0, 1): e <- |a| e + 2 u (|a v| + |b|).  Gray: e <- sum w_c e_c + 4 u sum w_c |v_c|.
 7. Filter: the input is given exactly; n chained fmaf give (n + 1) u sum_t |w_t x_t| (the standard running-sum bound), then 6."""
import numpy as np

U = 2.0 ** -24
NPARAM, MAXTAPS, RADIUS = 4, 81, 12
EPS_D = 1e-8
GRAY = np.array([0.299, 0.587, 0.114])
IDENT_PARAMS = np.array([1.0, 0.0, 1.0, 0.0], np.float32)

# the measured number of positive ground-truth matches of the train-step test (tests/test_gpu_homography_views.py:
# test_two_view_pipeline_train_step prints it); the test's condition is "> 0", this is a record
TRAIN_STEP_POSITIVES = 25      # of 512 keypoints, MI355X


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
SIZES = np.array([[37, 29], [16, 50]], np.int32)            # (w, h) of the two sources; the padded buffer is 50 x 37
HMAX, WMAX = 50, 37
VIEW_SRC = np.array([1, 0, 0, 1, 1, 0], np.int32)           # out of order, repeated
PATCHES = [(40, 24), (33, 19), (70, 60)]                    # (pw, ph); the last is larger than either source and spans 2 x 4 tiles


def sources(dtype, C, kind="random", seed=0):
    """[2, HMAX, WMAX, C]; the padding outside each source's own size holds 255 (uint8) or NaN (fp32).
    kind "ramp": a + b x + c y per channel (integers for uint8, so that bilinear sampling reproduces them exactly)."""
    rng = np.random.RandomState(seed)
    out = np.full((2, HMAX, WMAX, C), 255 if dtype == np.uint8 else np.nan, dtype)
    for s, (w, h) in enumerate(SIZES):
        if kind == "ramp":
            ys, xs = np.mgrid[0:h, 0:w]
            img = np.stack([(3 + c) + (2 + c) * xs + (1 + s) * ys for c in range(C)], -1).astype(np.float64)
            img = img if dtype == np.uint8 else img / 255.0
        elif dtype == np.uint8:
            img = rng.randint(0, 256, size=(h, w, C))
            img[:3, :3] = 0                                 # black pixels: gamma at 0, value shift on black
        else:
            img = rng.uniform(0, 1, size=(h, w, C))
            img[:3, :3] = 0
        out[s, :h, :w] = img.astype(dtype)
    return out


def ramp_value(s, c, x, y, dtype):
    """The closed form of sources(kind="ramp") in output units (uint8 / 255)."""
    return ((3 + c) + (2 + c) * x + (1 + s) * y) / 255.0


def view_matrices(patch, seed=0):
    """Hinv [6,3,3] fp32: patch pixel -> source pixel.  Rotations up to 60 degrees, scales that look beyond the source,
    a mild perspective; view 0 is the identity."""
    rng = np.random.RandomState(100 + seed)
    pw, ph = patch
    out = []
    for v, s in enumerate(VIEW_SRC):
        w, h = SIZES[s]
        th = np.deg2rad(rng.uniform(-60, 60))
        sc = rng.uniform(0.5, 1.4) * max(w / pw, h / ph)
        A = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]) * np.array([sc, sc, 1])[:, None]
        P = np.eye(3)
        P[2, :2] = rng.uniform(-1e-3, 1e-3, 2)
        T0 = np.array([[1, 0, -(pw - 1) / 2], [0, 1, -(ph - 1) / 2], [0, 0, 1.0]])
        T1 = np.array([[1, 0, (w - 1) / 2], [0, 1, (h - 1) / 2], [0, 0, 1.0]])
        out.append(np.eye(3) if v == 0 else T1 @ A @ P @ T0)
    return np.stack(out).astype(np.float32)


def horizon_matrix(patch):
    """d = 0 along a line that crosses the patch."""
    pw, ph = patch
    return np.array([[1, 0, 0], [0, 1, 0], [1.0 / pw, 1.0 / ph, -1.0]], np.float32)


def photometric_params(seed=0):
    """[6,4]: every stage on for some view and off for some (gamma, value shift < 0, a, b)."""
    p = np.tile(IDENT_PARAMS, (6, 1))
    p[1, 0] = 0.4
    p[2, 1] = -0.3
    p[3] = [0.6, -0.2, 0.8, -0.1]
    p[4, 2:] = [0.75, -0.35]
    p[5] = [1.0, -60.0 / 255.0, 1.0, -0.05]
    return p.astype(np.float32)


def tap_tables(kinds):
    """kinds: one per view of "id", ("box", k), ("line", k, "h" | "v" | "d"), "full" (81 random taps, unit sum)."""
    V = len(kinds)
    off, wgt, n = np.zeros((V, MAXTAPS, 2), np.int32), np.zeros((V, MAXTAPS), np.float32), np.zeros((V,), np.int32)
    rng = np.random.RandomState(5)
    for v, kind in enumerate(kinds):
        if kind == "id":
            o, w = [(0, 0)], [1.0]
        elif kind[0] == "box":
            r = kind[1] // 2
            o = [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
            w = [1.0 / len(o)] * len(o)
        elif kind[0] == "line":
            r = kind[1] // 2
            o = [{"h": (i, 0), "v": (0, i), "d": (i, i)}[kind[2]] for i in range(-r, r + 1)]
            w = [1.0 / len(o)] * len(o)
        else:
            o = rng.randint(-RADIUS, RADIUS + 1, size=(MAXTAPS, 2)).tolist()
            w = rng.uniform(0, 1, MAXTAPS)
            w = (w / w.sum()).tolist()
        n[v] = len(o)
        off[v, :len(o)] = o
        wgt[v, :len(o)] = w
    return off, wgt, n


# ---- restatements ---------------------------------------------------------------------------------------------------------------
def _post(v, e, a, b):
    a, b = float(a), float(b)
    return np.clip(a * v + b, 0, 1), abs(a) * e + 2 * U * (np.abs(a * v) + abs(b))


def _gray(v, e, weights=GRAY):
    """v, e [C=3, ...] -> [1, ...]"""
    w = weights.reshape(3, *([1] * (v.ndim - 1)))
    return (w * v).sum(0, keepdims=True), (w * e).sum(0, keepdims=True) + 4 * U * (w * np.abs(v)).sum(0, keepdims=True)


def _pre(v, e, gamma, shift):
    """gamma, then the value shift, on v [C, ...] >= 0 with error e."""
    gamma, shift = float(gamma), float(shift)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if gamma != 1.0:
            f = v ** gamma
            hi, lo = (v + e) ** gamma, np.maximum(v - e, 0) ** gamma
            e = np.where(np.isfinite(e), np.maximum(hi - f, f - lo), np.inf) + 4 * U * f
            v = f
        if shift != 0.0:
            if v.shape[0] == 1:
                v, e = np.clip(v + shift, 0, 1), e + 2 * U * (np.abs(v) + abs(shift))
            else:
                def k(m):
                    return np.where(m > 0, np.clip(m + shift, 0, 1) / np.where(m > 0, m, 1), 0.0 if shift < 0 else 1.0)
                m, em = v.max(0, keepdims=True), e.max(0, keepdims=True)
                km = k(m)
                m_lo = m - em
                dk = np.maximum(np.abs(k(m + em) - km), np.abs(k(np.maximum(m_lo, 0)) - km))
                if shift > 0:
                    dk = np.where(m_lo <= 0, np.inf, dk)
                dk = np.where(np.isfinite(em), dk, np.inf)
                out = v * km
                part = np.where(v > 0, v * dk, 0.0)
                e = km * e + part + 4 * U * np.abs(out)
                v = out
    return v, e


def _fetch(img, w, h, xi, yi, border):
    """img [H,W,C] float64 -> [C, ...] taps at integer (xi, yi); zero outside [0,w) x [0,h) unless border == "replicate"."""
    xc, yc = np.clip(xi, 0, w - 1), np.clip(yi, 0, h - 1)
    t = np.moveaxis(img[yc, xc], -1, 0)
    if border == "replicate":
        return t
    inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    return np.where(inside[None], t, 0.0)


def warp_ref(src, sizes, view_src, Hinv, params, patch, finish, gray, mutate=None):
    """-> (out [V,Cout,ph,pw] fp64, bound [V,Cout,ph,pw]).  mutate: None, "half_pixel", "H_for_Hinv", "transposed", "replicate",
    "padded_size", "bgr"."""
    pw, ph = patch
    S, Hm, Wm, C = src.shape
    scale = 255.0 if src.dtype == np.uint8 else 1.0
    imgs = src.astype(np.float64) / scale
    ys, xs = np.mgrid[0:ph, 0:pw].astype(np.float64)
    outs, bounds = [], []
    for v in range(len(view_src)):
        s = int(view_src[v])
        w, h = (Wm, Hm) if mutate == "padded_size" else (int(sizes[s, 0]), int(sizes[s, 1]))
        M = Hinv[v].astype(np.float64).reshape(3, 3)
        if mutate == "H_for_Hinv":
            M = np.linalg.inv(M)
        elif mutate == "transposed":
            M = M.T
        px, py = (xs + 0.5, ys + 0.5) if mutate == "half_pixel" else (xs, ys)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            d = M[2, 0] * px + M[2, 1] * py + M[2, 2]
            sx = (M[0, 0] * px + M[0, 1] * py + M[0, 2]) / d
            sy = (M[1, 0] * px + M[1, 1] * py + M[1, 2]) / d
            if mutate == "half_pixel":
                sx, sy = sx - 0.5, sy - 0.5
            Md = np.abs(M[2, 0] * px) + np.abs(M[2, 1] * py) + abs(M[2, 2])
            Ex = 2 * ((2 * U * (np.abs(M[0, 0] * px) + np.abs(M[0, 1] * py) + abs(M[0, 2])) + np.abs(sx) * 2 * U * Md) / np.abs(d)
                      + U * np.abs(sx))
            Ey = 2 * ((2 * U * (np.abs(M[1, 0] * px) + np.abs(M[1, 1] * py) + abs(M[1, 2])) + np.abs(sy) * 2 * U * Md) / np.abs(d)
                      + U * np.abs(sy))
            ok = np.isfinite(d) & (np.abs(d) >= EPS_D) & (sx >= -1) & (sx <= w) & (sy >= -1) & (sy <= h)
        # a pixel outside is 0; its neighbourhood (for Gx, Gy) is taken at the nearest point of the valid range, where a device
        # coordinate that lands just inside would sample
        with np.errstate(invalid="ignore"):
            sxc = np.where(np.isfinite(sx) & np.isfinite(sy), np.clip(sx, -1.0, w), -1.0)
            syc = np.where(np.isfinite(sx) & np.isfinite(sy), np.clip(sy, -1.0, h), -1.0)
        x0, y0 = np.floor(sxc).astype(np.int64), np.floor(syc).astype(np.int64)
        fx, fy = sxc - x0, syc - y0
        border = "replicate" if mutate == "replicate" else "zero"
        nb = np.stack([np.stack([_fetch(imgs[s], w, h, x0 + i, y0 + j, border) for i in range(-1, 3)]) for j in range(-1, 3)])
        t00, t10, t01, t11 = nb[1, 1], nb[1, 2], nb[2, 1], nb[2, 2]         # nb[j, i] -> [C, ph, pw]
        top, bot = t00 + fx * (t10 - t00), t01 + fx * (t11 - t01)
        val = np.where(ok[None], top + fy * (bot - top), 0.0)
        Gx = np.abs(np.diff(nb, axis=1)).max((0, 1))
        Gy = np.abs(np.diff(nb, axis=0)).max((0, 1))
        Tmax = np.abs(nb[1:3, 1:3]).max((0, 1))
        with np.errstate(invalid="ignore"):
            e = Gx * Ex[None] + Gy * Ey[None] + 12 * U * Tmax + U * np.abs(val)
            wild = ~np.isfinite(d) | (np.abs(d) < 1e-6) | ~(Ex <= 0.25) | ~(Ey <= 0.25)
        e = np.where(wild[None], np.inf, e)
        val, e = _pre(val, e, params[v, 0], params[v, 1])
        if finish:
            val, e = _post(val, e, params[v, 2], params[v, 3])
            if gray and C == 3:
                val, e = _gray(val, e, GRAY[::-1] if mutate == "bgr" else GRAY)
        outs.append(val)
        bounds.append(e)
    return np.stack(outs), np.stack(bounds)


def _reflect(i, n, edge):
    if edge:                                        # the mutation: "reflect" repeats the edge pixel (-1 -> 0, n -> n-1)
        i = np.where(i < 0, -i - 1, i)
        return np.where(i >= n, 2 * n - 1 - i, i)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def filter_ref(x, tap_off, tap_w, ntaps, params, gray, mutate=None):
    """x [V,C,ph,pw] -> (out [V,Cout,ph,pw] fp64, bound).  mutate: None, "reflect", "flipped", "bgr", "post_before_blur"."""
    V, C, ph, pw = x.shape
    ys, xs = np.arange(ph), np.arange(pw)
    outs, bounds = [], []
    for v in range(V):
        a, b = params[v, 2], params[v, 3]
        src = x[v].astype(np.float64)
        if mutate == "post_before_blur":
            src = _post(src, 0.0, a, b)[0]
        acc, mag = np.zeros((C, ph, pw)), np.zeros((C, ph, pw))
        n = int(ntaps[v])
        for t in range(n):
            dx, dy = (-tap_off[v, t] if mutate == "flipped" else tap_off[v, t]).tolist()
            yi, xi = _reflect(ys + dy, ph, mutate == "reflect"), _reflect(xs + dx, pw, mutate == "reflect")
            term = float(tap_w[v, t]) * src[:, yi][:, :, xi]
            acc += term
            mag += np.abs(term)
        e = (n + 1) * U * mag
        val, e = (acc, e) if mutate == "post_before_blur" else _post(acc, e, a, b)
        if gray and C == 3:
            val, e = _gray(val, e, GRAY[::-1] if mutate == "bgr" else GRAY)
        outs.append(val)
        bounds.append(e)
    return np.stack(outs), np.stack(bounds)


WARP_MUTATIONS = ["half_pixel", "H_for_Hinv", "transposed", "replicate", "padded_size", "bgr"]
FILTER_MUTATIONS = ["reflect", "flipped", "bgr", "post_before_blur"]


def violations(got, ref, bound):
    """How many pixels lie outside their (finite) bound, and the worst ratio; a non-finite value always counts."""
    got = np.asarray(got, np.float64)
    finite = np.isfinite(bound)
    with np.errstate(invalid="ignore", divide="ignore"):
        bad = finite & ~(np.abs(got - ref) <= bound)
        ratio = np.where(finite & (bound > 0), np.abs(got - ref) / bound, 0.0)
    bad |= ~np.isfinite(got)
    return int(bad.sum()), float(np.nanmax(ratio)) if ratio.size else 0.0


def textured_image(w, h, seed=0):
    """A synthetic source with corners for a detector to find: random rectangles over a smooth gradient, uint8 [h,w,3]."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    img = np.stack([64 + 64 * xs / w, 64 + 64 * ys / h, 96 + 32 * (xs + ys) / (w + h)], -1)
    for _ in range(400):
        x0, y0 = rng.randint(0, w - 8), rng.randint(0, h - 8)
        ww, hh = rng.randint(8, 96), rng.randint(8, 96)
        img[y0:y0 + hh, x0:x0 + ww] = rng.randint(0, 256, 3)
    return img.clip(0, 255).astype(np.uint8)


# ---- sampler settings shared by tools/gen_homography_views_golden.py and the reference tests ------------------------------------
# (seed, image (w, h), patch (pw, ph), keyword arguments); two consecutive views are drawn from one RandomState(seed)
SAMPLER_SETTINGS = [
    (0, (1024, 768), (640, 480), dict(difficulty=0.8, translation=1.0, n_angles=10, max_angle=60, min_convexity=0.05)),
    (1, (1024, 1024), (640, 480), dict(difficulty=0.7, translation=1.0, n_angles=10, max_angle=60, min_convexity=0.05)),
    (2, (640, 480), (320, 240), dict(difficulty=0.0, translation=1.0, n_angles=10, max_angle=60, min_convexity=0.05)),
    (3, (500, 333), (64, 48), dict(difficulty=0.8, translation=1.0, n_angles=0, max_angle=60, min_convexity=0.05)),
    (4, (333, 500), (64, 48), dict(difficulty=0.8, translation=0.0, n_angles=10, max_angle=60, min_convexity=0.05)),
    (5, (37, 29), (16, 12), dict(difficulty=0.8, translation=1.0, n_angles=10, max_angle=60, min_convexity=0.05)),
    (6, (37, 29), (40, 24), dict(difficulty=0.7, translation=0.5, n_angles=5, max_angle=90, min_convexity=0.05)),
    (7, (1024, 768), (640, 480), dict(difficulty=0.8, translation=1.0, n_angles=10, max_angle=60, min_convexity=0.2)),
]


def run_sampler(sample, compute):
    """{name: array} of what `sample` (a sample_homography_corners) and `compute` (a compute_homography) give on
    SAMPLER_SETTINGS: H, coords of two consecutive views, the homography between them from the fp32 corners, the next draw."""
    out = {}
    for i, (seed, shape, patch, kw) in enumerate(SAMPLER_SETTINGS):
        rng = np.random.RandomState(seed)
        coords = []
        for k in range(2):
            H, full, warped, _ = sample(shape, patch, rng=rng, **kw)
            out[f"s{i}_H{k}"], out[f"s{i}_coords{k}"] = np.asarray(H), np.asarray(warped)
            coords.append(np.asarray(warped).astype(np.float32))
        out[f"s{i}_H01"] = np.asarray(compute(coords[0], coords[1], [1, 1]))
        out[f"s{i}_next"] = np.array(rng.uniform())
    return out
