"""Shared cases of the SIFT tests: seeded images with planted blobs, an fp64 restatement of every stage of
glue_factory_amd/extractors/sift.py written independently of its code (numpy, direct loops over taps / window pixels, a
library solve for the refinement, tent weights instead of floor-based interpolation), the margins that tell which
decisions fp32 can take differently, and the named mutations the bounds must catch.  test_sift_cases_reference.py holds
the stock path to this on the CPU; test_gpu_sift.py holds the kernels of csrc/sift.hip to it.

Rounding model (u = 2^-24; the images here lie in [0, VMAX = 0.5], the Gaussian taps are positive and sum to 1)
-----------------------------------------------------------------------------------------------
* One separable pass with radius R is R + 1 multiply-adds and R pair sums on values <= VMAX: at most (R + 2) u VMAX.  A
  level is two passes on top of the level below (a blur does not amplify an incoming error), the base adds the bilinear
  upsampling (4 u VMAX).  With the radii 5, 5, 7, 8, 10, 13 of the base and the five increments the level errors
  accumulate in octave 0 to E_LEVEL = (4 + 2 (7 + 7 + 9 + 10 + 12 + 15)) u VMAX = 124 u VMAX = 3.7e-6 at level 5 (70 u VMAX
  at level 3).  The base of octave o + 1 is level 3 of octave o and the five increments follow again, so level 5 of octave
  o errs by at most e_level(o) = (124 + 52 o) u VMAX (level 3: (70 + 52 o) u VMAX), used for EVERY level of that octave;
  a DoG value, the difference of two levels, by e_dog(o) = 2 e_level(o): 7.4e-6 in octave 0, 1.7e-5 in octave 3.  (Measured
  errors are some 20 times smaller; the bound is not fitted.)  Below, E_LEVEL and E_DOG stand for e_level(o), e_dog(o) of
  the candidate's octave.
* Extremum test and the two |D| thresholds compare DoG values: margin band E_DOG (a gap between two values: 2 E_DOG).
* Refinement: offset = -H^-1 g.  g errs by E_DOG per entry; a diagonal entry of H by 4 E_DOG, a mixed one by E_DOG, so
  (dH offset)_j <= 0.5 (4 + 1 + 1) E_DOG = 3 E_DOG for |offset| <= 0.5; to first order offset_i errs by at most
  4 E_DOG sum_j |H^-1|_ij: OFFSET band, per candidate and axis.  D^ = D + g . offset / 2 errs by at most 2 E_DOG
  (|offset| <= 0.5 per axis, three axes): band 3 E_DOG with the rounding of the product chain.
* Edge test tr^2 r < (r + 1)^2 det: tr errs by 8 E_DOG, det by 4 E_DOG (|dxx| + |dyy| + |dxy|); the margin is the
  distance of (r + 1)^2 det - tr^2 r to zero against the propagated error, per candidate.
* Orientation histogram: every term w m t (window weight, gradient magnitude, tent weight) is positive.  m errs by
  2 sqrt(2) E_LEVEL absolutely: 2.9 E_LEVEL w per pixel, spread over its two bins.  The bin coordinate errs by
  36 / (2 pi) * 2 sqrt(2) E_LEVEL / m, which MOVES at most 16.3 E_LEVEL w between two adjacent bins and conserves their
  sum.  The six box passes are one circular kernel K (K_PEAK its largest tap, K_SLOPE its largest difference of adjacent
  taps): a smoothed bin sees at most K_PEAK of every magnitude error and K_SLOPE of every move.  Bound per smoothed bin:
  (2.9 K_PEAK + 16.3 K_SLOPE) E_LEVEL sum w + 40 u max(hist).  The second peak's margin is its distance to 0.8 max (and
  to the third peak) against twice that bound.
* Descriptor: same terms with the cell and orientation tents (derivative <= 1 in each of the three coordinates); the
  normalised vector errs by at most the un-normalised relative error, bound per entry:
  (30 E_LEVEL * sum w + 60 u * |d|) / |d| after normalisation, + 4 u for the square roots.
A candidate is DECISIVE when every margin exceeds its band.

Mutations the bounds must catch (test_mutations_are_caught): blur radius off by one; zero border instead of reflect-101;
orientation window sigma 1.0 instead of 1.5; descriptor clip omitted; descriptor bins in the wrong (transposed) cell order.
The missing 0.8 prefilter changes the ACCEPTED list only where |D| <= 0.8 thr and |D^| >= thr.  No cell of the images here
is of that kind, so prefilter_stack() builds one: the restatement accepts it only without the prefilter, and the stock
path and gf_sift_extrema are held to the restatement's accepted list on that stack.
"""
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
VMAX = 0.5
E_LEVEL = 124 * U * VMAX
E_DOG = 2 * E_LEVEL


def e_level(octave):
    return (124 + 52 * octave) * U * VMAX


def e_dog(octave):
    return 2 * e_level(octave)


# a stage fed fp32 inputs that are exact in fp64 (the kernel tests): a gradient is one subtraction of values <= VMAX (u VMAX);
# atan2f, expf, sinf, cosf are allowed 4 ulp, which moves a bin coordinate by less than a gradient error of 7 u VMAX does
E_STAGE = 8 * U * VMAX
SIGMA0, LAYERS, LEVELS = 1.6, 3, 6
# A blob of standard deviation s peaks in the DoG level labelled 0.885 s (see test_planted_blobs_are_found); an octave
# holds refined layers 0.5 .. 3.5, i.e. labels 1.6 * 2^(0.5 / 3) .. 1.6 * 2^(3.5 / 3) octave pixels: blobs of
# s = 2.03 * 2^k input pixels sit on the seam between two octaves, where either octave may see the peak outside its layers.
OCTAVE_SEAM = 0.5 * 1.6 * 2.0 ** (3.5 / 3) / 0.885
_K = np.zeros(36)
_K[0] = 1.0
for _ in range(6):
    _K = (np.roll(_K, 1) + _K + np.roll(_K, -1)) / 3.0
K_PEAK, K_SLOPE = float(_K.max()), float(np.abs(_K - np.roll(_K, 1)).max())
THR, EDGE = 0.0066667, 10.0

# fp64 stock path on the CPU, 160 x 128 shift image (test_sift_cases_reference.py asserts it): share of the keypoints farther
# than the largest descriptor radius from the border that are recovered at the position shifted by 16 px with an equal
# descriptor
SHIFT_RECOVERED_FP64 = 1.0

SIZES = [(48, 64), (61, 97), (33, 40)]          # (h, w): plain, odd, early-ending pyramid
E2E_SIZE = (128, 160)


# ------------------------------------------------------------------------------------------------ images
def make_image(h, w, seed, n_blobs=None, margin=10.0, offset=(0.0, 0.0), asym=0.3, texture=True, avoid_seams=False, sigmas=None):
    """-> (image [h,w] float64 in [0, VMAX], blobs [(x, y, sigma, sign)]) in the corner convention (pixel centres at
    +0.5).  A blob is sign A (1 + 0.3 t) exp(-r^2 / 2 sigma^2), t the coordinate along a random direction in units of
    sigma: the odd term gives it one dominant gradient direction.  Amplitudes keep the negative ring of a blob's DoG
    response well under 0.8 x the detection threshold."""
    rng = np.random.RandomState(seed)
    n_blobs = n_blobs if n_blobs is not None else max(4, (h * w) // 400)
    yy, xx = np.meshgrid(np.arange(h) + 0.5 - offset[1], np.arange(w) + 0.5 - offset[0], indexing="ij")
    img = np.full((h, w), 0.25)
    blobs = []
    for i in range(n_blobs):
        for _ in range(50):
            x, y = rng.uniform(margin, w - margin), rng.uniform(margin, h - margin)
            s = rng.uniform(1.2, 3.2) if sigmas is None else sigmas[i % len(sigmas)] * rng.uniform(0.9, 1.1)
            if avoid_seams and abs(np.log2(s / OCTAVE_SEAM) - np.round(np.log2(s / OCTAVE_SEAM))) < 0.12:
                continue
            if all((x - bx) ** 2 + (y - by) ** 2 > (3.5 * (s + bs)) ** 2 for bx, by, bs, _ in blobs):
                break
        else:
            continue
        sign = 1.0 if i % 2 else -1.0
        th = rng.uniform(0, 2 * np.pi)
        t = ((xx - x) * np.cos(th) + (yy - y) * np.sin(th)) / s
        blobs.append((x, y, s, sign))
        img += sign * rng.uniform(0.13, 0.2) * (1 + asym * t) * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))
    for _ in range(3 if texture else 0):                   # low-amplitude smooth texture
        fx, fy, ph = rng.uniform(0.02, 0.06), rng.uniform(0.02, 0.06), rng.uniform(0, 6.28)
        img += 0.004 * np.sin(6.283 * (fx * xx + fy * yy) + ph)
    assert img.min() >= 0.0 and img.max() <= VMAX
    return img, blobs


# seeds chosen so that at most 10 % of an image's candidates are non-decisive (asserted in test_sift_cases_reference.py)
CASE_SEEDS = [117, 129, 101]
COARSE_SEED = 501
E2E_SEEDS = [(203, 22), (207, 22), (210, 22)]
SHIFT = 16


def case_images():
    """plain, odd, early-ending, coarse."""
    return [make_image(h, w, seed)[0] for seed, (h, w) in zip(CASE_SEEDS, SIZES)] + [coarse_image()]


def coarse_image():
    """128 x 160 with blobs of sigma 5 .. 10 px next to small ones: accepted candidates in octaves 2 and 3 as well."""
    return make_image(E2E_SIZE[0], E2E_SIZE[1], COARSE_SEED, n_blobs=12, margin=22.0, sigmas=[7.0, 2.2, 5.5, 1.5, 9.0, 2.8])[0]


def e2e_batch():
    """[3,1,128,160] float64 and per-image (w, h) sizes."""
    imgs = np.stack([make_image(E2E_SIZE[0], E2E_SIZE[1], seed, n_blobs=n)[0] for seed, n in E2E_SEEDS])
    return torch.from_numpy(imgs)[:, None], torch.tensor([[160, 128], [150, 100], [120, 128]])


def shift_pair():
    """An image and the same content moved by (SHIFT, SHIFT) px: blobs on a constant background (no texture), every blob
    at least 30 px inside both images, so that in exact arithmetic the two pyramids are shifted copies of each other."""
    h, w = E2E_SIZE
    a, blobs = make_image(h - SHIFT, w - SHIFT, 313, n_blobs=14, margin=30.0, texture=False)
    pair = []
    for off in (0, SHIFT):
        img = np.full((h, w), 0.25)
        img[off:off + h - SHIFT, off:off + w - SHIFT] = a
        pair.append(img)
    return pair, blobs


# ------------------------------------------------------------------------------------------------ pyramid
def ref_taps(sigma, radius_delta=0):
    r = int(math.ceil(4.0 * sigma)) + radius_delta
    k = np.exp(-np.arange(-r, r + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return k / k.sum()


def _reflect(i, n):
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def ref_blur(img, sigma, radius_delta=0, border="reflect"):
    k = ref_taps(sigma, radius_delta)
    r = (len(k) - 1) // 2
    out = img
    for axis in (1, 0):
        n = out.shape[axis]
        acc = np.zeros_like(out)
        for t in range(-r, r + 1):
            idx = np.arange(n) + t
            taken = np.take(out, _reflect(idx, n), axis=axis)
            if border == "zero":
                ok = ((idx >= 0) & (idx < n)).astype(np.float64)
                taken = taken * (ok[None, :] if axis == 1 else ok[:, None])
            acc = acc + k[t + r] * taken
        out = acc
    return out


def ref_upsample2(img):
    def axis_weights(n):
        u = np.arange(2 * n)
        c = np.maximum(0.5 * (u + 0.5) - 0.5, 0.0)
        i0 = np.floor(c).astype(int)
        return i0, np.minimum(i0 + 1, n - 1), c - i0
    y0, y1, ly = axis_weights(img.shape[0])
    x0, x1, lx = axis_weights(img.shape[1])
    rows = img[y0] * (1 - ly)[:, None] + img[y1] * ly[:, None]
    return rows[:, x0] * (1 - lx)[None] + rows[:, x1] * lx[None]


def ref_pyramid(img, first_octave=-1, num_octaves=4, **mut):
    """-> (gauss, dog): per octave [6,h,w], [5,h,w] float64."""
    if first_octave == -1:
        img = ref_upsample2(img)
    base = ref_blur(img, math.sqrt(SIGMA0 ** 2 - (0.5 * 2.0 ** -first_octave) ** 2), **mut)
    gauss, dog = [], []
    for _ in range(num_octaves):
        if min(base.shape) < 8:
            break
        lv = [base]
        for i in range(1, LEVELS):
            s1, s0 = SIGMA0 * 2.0 ** (i / LAYERS), SIGMA0 * 2.0 ** ((i - 1) / LAYERS)
            lv.append(ref_blur(lv[-1], math.sqrt(s1 * s1 - s0 * s0), **mut))
        g = np.stack(lv)
        gauss.append(g)
        dog.append(g[1:] - g[:-1])
        base = lv[LAYERS][::2, ::2]
    return gauss, dog


# ------------------------------------------------------------------------------------------------ detection
def _hessian(D, s, y, x):
    v = D[s, y, x]
    g = 0.5 * np.array([D[s, y, x + 1] - D[s, y, x - 1], D[s, y + 1, x] - D[s, y - 1, x], D[s + 1, y, x] - D[s - 1, y, x]])
    H = np.empty((3, 3))
    H[0, 0] = D[s, y, x + 1] + D[s, y, x - 1] - 2 * v
    H[1, 1] = D[s, y + 1, x] + D[s, y - 1, x] - 2 * v
    H[2, 2] = D[s + 1, y, x] + D[s - 1, y, x] - 2 * v
    H[0, 1] = H[1, 0] = 0.25 * (D[s, y + 1, x + 1] - D[s, y + 1, x - 1] - D[s, y - 1, x + 1] + D[s, y - 1, x - 1])
    H[0, 2] = H[2, 0] = 0.25 * (D[s + 1, y, x + 1] - D[s + 1, y, x - 1] - D[s - 1, y, x + 1] + D[s - 1, y, x - 1])
    H[1, 2] = H[2, 1] = 0.25 * (D[s + 1, y + 1, x] - D[s + 1, y - 1, x] - D[s - 1, y + 1, x] + D[s - 1, y - 1, x])
    return v, g, H


def ref_detect(D, thr=THR, edge=EDGE, prefilter=0.8, e_dog=E_DOG):
    """One octave's DoG stack [5,h,w] -> list of dicts in (layer, y, x) order of the cell where the extremum was found.
    Every cell whose extremum / prefilter decision is within the band is reported too (accepted or not), so that a test
    can tell a legitimate fp32 difference from a wrong one: entries carry 'accepted' and 'margin' (the smallest distance of
    any decision to its threshold, in units of its band: decisive when > 1)."""
    n, h, w = D.shape
    out = []
    for s in range(1, 4):
        cube = np.stack([D[s + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx] for ds in (-1, 0, 1) for dy in (-1, 0, 1)
                         for dx in (-1, 0, 1) if (ds, dy, dx) != (0, 0, 0)])
        c = D[s, 1:h - 1, 1:w - 1]
        gap = np.maximum(c - cube.max(0), cube.min(0) - c)           # > 0: strict extremum
        pre = np.abs(c) - prefilter * thr
        near = (gap > -2 * e_dog) & (pre > -e_dog)
        for yy, xx in zip(*np.nonzero(near)):
            m0 = min(gap[yy, xx] / (2 * e_dog), pre[yy, xx] / e_dog)
            ent = {"cell0": (s, yy + 1, xx + 1), "accepted": False, "margin": abs(m0)}
            out.append(ent)
            if m0 <= 0:
                continue
            ss, y, x = s, yy + 1, xx + 1
            margins = [m0]
            ok = False
            for _ in range(5):
                v, g, H = _hessian(D, ss, y, x)
                if np.linalg.det(H) == 0:
                    break
                off = -np.linalg.solve(H, g)
                band = 4 * e_dog * np.abs(np.linalg.inv(H)).sum(1)
                margins.append(np.min(np.abs(np.abs(off) - 0.5) / band))
                step = (off > 0.5).astype(int) - (off < -0.5).astype(int)
                if not step.any():
                    ok = True
                    break
                x, y, ss = x + step[0], y + step[1], ss + step[2]
                if not (1 <= ss <= 3 and 1 <= y <= h - 2 and 1 <= x <= w - 2):
                    break
            ent["margin"] = float(min(margins))
            if not ok:
                continue
            dhat = v + 0.5 * g.dot(off)
            tr, det = H[0, 0] + H[1, 1], H[0, 0] * H[1, 1] - H[0, 1] ** 2
            edge_val = (edge + 1) ** 2 * det - tr * tr * edge
            edge_err = (edge + 1) ** 2 * 4 * e_dog * (abs(H[0, 0]) + abs(H[1, 1]) + abs(H[0, 1])) + 2 * abs(tr) * 8 * e_dog * edge
            margins += [abs(abs(dhat) - thr) / (3 * e_dog), abs(det) / (4 * e_dog * (abs(H[0, 0]) + abs(H[1, 1]) + abs(H[0, 1])) + 1e-300),
                        abs(edge_val) / (edge_err + 1e-300)]
            ent.update(accepted=bool(abs(dhat) >= thr and det > 0 and edge_val > 0), margin=float(min(margins)), cell=(ss, y, x),
                       offset=off, dhat=dhat, offset_band=band)
    return out


def accepted(cands):
    return [c for c in cands if c["accepted"]]


# ------------------------------------------------------------------------------------------------ orientation / descriptor
def _window(L, cx, cy, rad):
    """Interior pixels of the (2 rad + 1)^2 window: integer coordinates and central-difference gradients."""
    h, w = L.shape
    ys, xs = np.meshgrid(np.arange(cy - rad, cy + rad + 1), np.arange(cx - rad, cx + rad + 1), indexing="ij")
    ok = (ys >= 1) & (ys <= h - 2) & (xs >= 1) & (xs <= w - 2)
    ys, xs = ys[ok], xs[ok]
    return xs, ys, L[ys, xs + 1] - L[ys, xs - 1], L[ys + 1, xs] - L[ys - 1, xs]


def ref_orient(L, cx, cy, sigma, window=1.5, e_level=E_LEVEL):
    """-> (oris (strongest first, <= 2), bound per bin, second-peak margin in units of its band (None: no second
    local maximum))."""
    sw = window * sigma
    rad = int(np.round(3.0 * 1.5 * sigma))
    xs, ys, gx, gy = _window(L, cx, cy, rad)
    wgt = np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * sw * sw))
    mag = np.hypot(gx, gy)
    fb = np.mod(np.arctan2(gy, gx), 2 * np.pi) * 36 / (2 * np.pi)
    hist = np.zeros(36)
    for k in range(36):
        d = np.abs(fb - k)
        hist[k] = np.sum(wgt * mag * np.maximum(0.0, 1.0 - np.minimum(d, 36 - d)))
    bound = (2.9 * K_PEAK + 16.3 * K_SLOPE) * e_level * wgt.sum() + 40 * U * hist.max()
    for _ in range(6):
        hist = (np.roll(hist, 1) + hist + np.roll(hist, -1)) / 3.0
    peaks = [k for k in range(36) if hist[k] > hist[k - 1] and hist[k] > hist[(k + 1) % 36]]
    peaks.sort(key=lambda k: (-hist[k], k))
    oris, margin = [], None
    for k in peaks[:2]:
        if hist[k] >= 0.8 * hist.max():
            l, c, r = hist[k - 1], hist[k], hist[(k + 1) % 36]
            oris.append(np.mod((k + 0.5 * (l - r) / (l - 2 * c + r)) * 2 * np.pi / 36, 2 * np.pi))
    if len(peaks) >= 2:
        margin = abs(hist[peaks[1]] - 0.8 * hist.max()) / (2 * bound)
        if len(peaks) >= 3:       # the third peak must not compete with the second
            margin = min(margin, abs(hist[peaks[1]] - hist[peaks[2]]) / (2 * bound))
    return oris, bound, margin, hist


def ori_bound(hist, k, bound):
    """Error bound of a refined orientation: the parabola's offset errs by the bin bound over its curvature."""
    l, c, r = hist[k - 1], hist[k], hist[(k + 1) % 36]
    den = abs(l - 2 * c + r)
    return (2 * np.pi / 36) * (bound / den + abs(l - r) * 4 * bound / (2 * den * den)) + 8 * U


def ref_describe(L, xo, yo, sigma, ori, clip=True, transpose_cells=False, rootsift=False, e_level=E_LEVEL):
    """-> (descriptor [128], bound per entry)."""
    hw = 3.0 * sigma
    rad = int(np.round(hw * math.sqrt(2.0) * 2.5))
    cx, cy = int(np.round(xo)), int(np.round(yo))
    xs, ys, gx, gy = _window(L, cx, cy, rad)
    c, s = math.cos(ori), math.sin(ori)
    dx, dy = xs - xo, ys - yo
    rx, ry = (c * dx + s * dy) / hw, (-s * dx + c * dy) / hw
    cb, rb = rx + 1.5, ry + 1.5
    ins = (rb > -1) & (rb < 4) & (cb > -1) & (cb < 4)
    wgt = np.exp(-(rx * rx + ry * ry) / 8.0) * np.hypot(gx, gy) * ins
    ob = np.mod((np.arctan2(gy, gx) - ori) * 8 / (2 * np.pi), 8.0)
    d = np.zeros(128)
    for r in range(4):
        for cc in range(4):
            wrc = wgt * np.maximum(0, 1 - np.abs(rb - r)) * np.maximum(0, 1 - np.abs(cb - cc))
            for o in range(8):
                do = np.abs(ob - o)
                cell = cc * 4 + r if transpose_cells else r * 4 + cc
                d[cell * 8 + o] = np.sum(wrc * np.maximum(0, 1 - np.minimum(do, 8 - do)))
    raw_norm = np.linalg.norm(d)
    bound = (30 * e_level * float(np.sum(np.exp(-(rx * rx + ry * ry) / 8.0) * ins)) + 60 * U * raw_norm) / max(raw_norm, 1e-300) + 4 * U
    d = d / max(raw_norm, 1e-12)
    if clip:
        d = np.minimum(d, 0.2)
    n2 = max(np.linalg.norm(d), 1e-12)
    d = d / n2
    bound = 2 * bound / n2
    if rootsift:
        d = d / max(np.abs(d).sum(), 1e-6)
        d = np.sqrt(np.maximum(d, 1e-6))
        d = d / max(np.linalg.norm(d), 1e-6)
    return d, bound


def shift_recovered(a, b, shape, tol_xy, tol_desc):
    """(recovered, considered) keypoints of `a` in `b` = `a` moved by SHIFT."""
    h, w = shape
    ka, kb = a["keypoints"][0].double(), b["keypoints"][0].double()
    radius = a["scales"][0].double() * 3 * np.sqrt(2) * 2.5 + 1
    far = ((ka[:, 0] > radius) & (ka[:, 1] > radius) & (ka[:, 0] + SHIFT < w - radius) & (ka[:, 1] + SHIFT < h - radius))
    rec = 0
    for i in far.nonzero()[:, 0]:
        near = ((kb - (ka[i] + SHIFT)).abs().amax(1) <= tol_xy) & ((b["oris"][0] - a["oris"][0][i]).abs() <= max(tol_desc, 1e-6))
        rec += bool(near.any() and (b["descriptors"][0][near] - a["descriptors"][0][i]).abs().amax(1).min() <= tol_desc)
    return rec, int(far.sum())


def prefilter_stack():
    """A DoG stack built for the 0.8 prefilter, (D [5,12,14] float32-exact, cell (s, y, x)): around the cell a separable
    paraboloid whose sampled maximum 0.75 thr lies under the prefilter while the fitted one, 1.28 thr at offsets (0.46, 0.46, 0),
    passes the contrast test; curvatures equal in x and y (edge ratio 4).  With the prefilter the cell is no candidate;
    without it the cell is accepted.  Every margin of the cell is far outside its band."""
    D = np.zeros((5, 12, 14))
    s0, y0, x0 = 2, 6, 7
    side = {-1: 2.4 * THR, 0: 0.0, 1: 0.1 * THR}
    for ds in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                D[s0 + ds, y0 + dy, x0 + dx] = 0.75 * THR - side[dx] - side[dy] - 0.5 * THR * abs(ds)
    return D.astype(np.float32).astype(np.float64), (s0, y0, x0)


def edge_level():
    """A Gaussian-level stand-in with one soft vertical edge and a keypoint on it, (L [40,44], xo, yo, sigma, ori): nearly
    all gradient mass falls into a few bins, so entries exceed 0.2 before the clip (the smooth blobs above never do)."""
    yy, xx = np.meshgrid(np.arange(40.0), np.arange(44.0), indexing="ij")
    L = 0.25 + 0.2 / (1.0 + np.exp(-(xx - 20.3 + 0.05 * yy)))
    return L, 20.4, 19.7, 2.0, 0.3


# ------------------------------------------------------------------------------------------------ keypoints of one image
def ref_keypoints(img, first_octave=-1, num_octaves=4):
    """Every accepted candidate of an image with its orientations: dicts with octave, cell, offset, sigma (octave px), level,
    xy (input px, corner convention), scale, score, oris, margin (all decisions, detection and second peak)."""
    gauss, dog = ref_pyramid(img, first_octave, num_octaves)
    out = []
    for o, D in enumerate(dog):
        for cnd in ref_detect(D, e_dog=e_dog(o)):
            cnd["octave"] = o
            if cnd["accepted"]:
                s, y, x = cnd["cell"]
                so = s + cnd["offset"][2]
                cnd["sigma"] = SIGMA0 * 2.0 ** (so / LAYERS)
                cnd["level"] = int(min(max(np.round(so), 0), LEVELS - 1))
                step = 2.0 ** (o + first_octave)
                cnd["xy_oct"] = (x + cnd["offset"][0], y + cnd["offset"][1])
                cnd["xy"] = ((cnd["xy_oct"][0] * 2.0 ** o + 0.5) * 2.0 ** first_octave, (cnd["xy_oct"][1] * 2.0 ** o + 0.5) * 2.0 ** first_octave)
                cnd["scale"] = cnd["sigma"] * step
                cnd["score"] = abs(cnd["dhat"]) * cnd["scale"]
                oris, bound, m2, hist = ref_orient(gauss[o][cnd["level"]], x, y, cnd["sigma"], e_level=e_level(o))
                cnd.update(oris=oris, ori_bin_bound=bound, ori_margin=m2, hist=hist)
            out.append(cnd)
    return gauss, dog, out


def decisive(c):
    return c["margin"] > 1.0 and (not c["accepted"] or c.get("ori_margin") is None or c["ori_margin"] > 1.0)


# ------------------------------------------------------------------------------------------------ the reference's functions
def reference_functions(ref_root="/root/reference"):
    """(filter_dog_point, sift_to_rootsift) of the reference checkout, or None where it is absent.  Only the file
    gluefactory/models/extractors/sift.py is executed, inside an empty stand-in package, with tests/sift_stubs in front."""
    path = os.path.join(ref_root, "gluefactory", "models", "extractors", "sift.py")
    if not os.path.exists(path):
        return None
    import importlib.util
    stubs = os.path.join(ROOT, "tests", "sift_stubs")
    names = ("cv2", "kornia", "kornia.color", "pycolmap")
    saved = {name: sys.modules.pop(name) for name in names if name in sys.modules}      # (another test's stand-ins, put back below)
    sys.path.insert(0, stubs)
    try:
        pkg = "gf_sift_reference"
        for name in (pkg, pkg + ".models", pkg + ".models.extractors", pkg + ".models.utils"):
            mod = types.ModuleType(name)
            mod.__path__ = []
            sys.modules[name] = mod
        base = types.ModuleType(pkg + ".models.base_model")
        base.BaseModel = type("BaseModel", (), {})
        misc = types.ModuleType(pkg + ".models.utils.misc")
        misc.pad_to_length = None
        sys.modules[base.__name__], sys.modules[misc.__name__] = base, misc
        spec = importlib.util.spec_from_file_location(pkg + ".models.extractors.sift", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        return mod.filter_dog_point, mod.sift_to_rootsift
    finally:
        sys.path.remove(stubs)
        for name in names:
            sys.modules.pop(name, None)
        sys.modules.update(saved)


def post_lists():
    """Keypoint lists for filter_dog_point: duplicate pixels, equal scores, +-equal angles; (points, scales, angles,
    scores, (h, w)) float32 numpy, per list."""
    rng = np.random.RandomState(7)
    lists = []
    for h, w, n in ((24, 31, 120), (40, 33, 300)):
        pix = np.stack([rng.randint(0, w, n), rng.randint(0, h, n)], -1)
        pix[n // 2:] = pix[rng.randint(0, n // 2, n - n // 2)]                    # duplicate pixels
        pts = (pix + rng.uniform(0.05, 0.95, (n, 2))).astype(np.float32)
        scores = rng.uniform(0.01, 1.0, n).astype(np.float32)
        scores[n // 2::3] = scores[rng.randint(0, n // 2, len(scores[n // 2::3]))]  # equal scores, some on the same pixel
        angles = rng.uniform(0, 6.28, n).astype(np.float32)
        same = np.arange(n // 2, n, 4)
        src = rng.randint(0, n // 2, len(same))
        pts[same], scores[same], angles[same] = pts[src], scores[src], -angles[src]   # same pixel and score, opposite angle
        scales = rng.uniform(1.0, 8.0, n).astype(np.float32)
        lists.append((pts, scales, angles, scores, (h, w)))
    return lists
