"""Homography view synthesis on the GPU: the `homographies` dataset of the reference from "decoded image" to the collated batch.

The reference (gluefactory/datasets/homographies.py) samples a homography per view on a DataLoader worker, warps with
cv2.warpPerspective, runs an albumentations chain and reduces to gray, one view at a time.  Here the decoded images are one
padded NHWC uint8 (or fp32) stack in device memory; the homographies and the photometric parameters are sampled on the host
(a few hundred floats per view), uploaded as two small tables, and every view of the batch is produced by two launches
(ops.warp_views, ops.filter_views; one launch when the preset has no blur).  Image search, decoding, splits, cached features
and prefetching are not part of this module.

GEOMETRY.  ``sample_homography_corners`` and ``compute_homography`` restate gluefactory/geometry/homography.py:17-128.  They draw
from ``rng`` in the same order and evaluate the same numpy expressions, so that for the same generator state H, the warped
corners and the generator's next draw are bit-equal to the reference's (tests/test_homography_views_reference.py).

PHOTOMETRY.  Neither albumentations nor cv2 is a dependency of this project, so the photometric semantics are this project's
own: float throughout, no uint8 round trip, and a FIXED order of stages per view whatever the preset lists:
    gamma -> value shift -> (one) blur -> brightness / contrast -> gray.
``sample_photometric`` maps the reference's presets (gluefactory/datasets/augmentations.py:173-243) onto these stages with the
presets' probabilities and ranges:
    RandomGamma(gamma_limit=(15, 65))             v ** g, g ~ U(0.15, 0.65)
    HueSaturationValue(val_shift_limit=(-100,-40)) the VALUE shift only: max(r,g,b) moved by s ~ U(-100, -40) / 255, channels
                                                  scaled alike (the hue and saturation shifts of the same transform are skipped)
    Blur(blur_limit=(3, 9))                       k x k box, k odd, uniform
    MotionBlur(blur_limit=(3, 25), allow_shifted=False)  a normalised line through the centre of a k x k window, k odd, at a
                                                  uniform angle (albumentations draws two random end points instead)
    RandomBrightnessContrast((-0.4, 0), (-0.3, 0)) clamp(a v + b, 0, 1), a = 1 + U(-0.3, 0), b = U(-0.4, 0)
    OneOf([...], p)                               fires with p, then picks a child with its normalised probability
A view is blurred at most once: when several blurs of a preset fire, the first one in the preset's order is kept (two chained
blurs would need more than GF_HV_MAXTAPS taps).  `dark` lists its transforms in another order (brightness first); it runs in the
fixed order above.  Skipped, because there is no kernel for them: RandomRain, ISONoise, ImageCompression (JPEG), CLAHE,
Equalize, ToSepia, ToGray, the hue and saturation shifts.  A skipped child of a OneOf still takes its share of the
probability, so the supported children fire as often as in the reference.
"""
import math

import numpy as np
import torch

from .. import ops
from ..conf import Conf
from ._views_ops import MAXTAPS, NPARAM, RADIUS




# ---- geometry -------------------------------------------------------------------------------------------------------------------
def _centre_patch(shape, patch_shape=None):
    """The four corners (left-bottom, left-top, right-top, right-bottom; integers, truncated) of a centred patch."""
    w, h = shape
    pw, ph = shape if patch_shape is None else patch_shape
    lo_x, lo_y = int((w - pw) / 2), int((h - ph) / 2)
    hi_x, hi_y = int((w + pw) / 2), int((h + ph) / 2)
    return np.array([[lo_x, lo_y], [lo_x, hi_y], [hi_x, hi_y], [hi_x, lo_y]])


def _convex(quad, min_convexity):
    n = quad.shape[0]
    for i in range(n):
        (x1, y1), (x2, y2), (x3, y3) = quad[(i - 1) % n], quad[i], quad[(i + 1) % n]
        if (x2 - x1) * (y3 - y2) - (x3 - x2) * (y2 - y1) > -min_convexity:
            return False
    return True


def compute_homography(pts1, pts2, shape):
    """The homography taking the four points pts1 to pts2 (both [4,2], scaled by shape = (h, w) reversed), h22 = 1: the 8 x 8
    linear system of the four correspondences."""
    scale = np.expand_dims(np.array(shape[::-1], dtype=np.float32), axis=0)
    p, q = pts1 * scale, pts2 * scale
    rows = []
    for i in range(4):
        rows.append([p[i][0], p[i][1], 1, 0, 0, 0, -p[i][0] * q[i][0], -p[i][1] * q[i][0]])
        rows.append([0, 0, 0, p[i][0], p[i][1], 1, -p[i][0] * q[i][1], -p[i][1] * q[i][1]])
    a = np.stack(rows, axis=0)
    b = np.transpose(np.stack([[q[i][j] for i in range(4) for j in range(2)]], axis=0))
    h = np.transpose(np.linalg.solve(a, b))
    return np.reshape(np.concatenate([h, np.ones_like(h[:, :1])], axis=1), [3, 3])


def _project(points, H):
    """points [N,2] through H (forward), with the reference's guard on the homogeneous coordinate."""
    hom = np.concatenate([points, np.ones([points.shape[0], 1], dtype=np.float32)], -1)
    w = np.transpose(np.tensordot(hom, np.transpose(H[None]), axes=[[1], [0]]), [2, 0, 1])
    w[np.abs(w[:, :, 2]) < 1e-8, 2] = 1e-8
    return (w[:, :, :2] / w[:, :, 2:])[0]


def sample_homography_corners(shape, patch_shape, difficulty=1.0, translation=0.4, n_angles=10, max_angle=90,
                              min_convexity=0.05, rng=np.random):
    """A random homography from the image (shape = (w, h)) to a patch (patch_shape = (pw, ph)): the four image points that land
    on the patch corners are the frame's corners moved inwards by up to `difficulty`, re-centred, rotated by one of `n_angles`
    angles that keeps them inside the frame, and translated.  -> (H [3,3] fp64, frame corners [4,2], their images [4,2],
    patch_shape)."""
    max_angle = max_angle / 180.0 * math.pi
    width, height = shape
    inner = _centre_patch(shape, (width * (1 - difficulty), height * (1 - difficulty)))
    full = _centre_patch(shape)
    pts2 = _centre_patch(patch_shape)
    reach = inner - full
    while True:
        pts1 = full + rng.uniform(0.0, 1.0, size=(4, 2)) * reach
        if _convex(pts1 / np.array(shape), min_convexity):
            break
    pts1 = pts1 - np.mean(pts1, axis=0, keepdims=True)
    pts1 = pts1 + np.mean(inner, axis=0, keepdims=True)

    if n_angles > 0 and difficulty > 0:
        angles = np.linspace(-max_angle * difficulty, max_angle * difficulty, n_angles)
        rng.shuffle(angles)
        rng.shuffle(angles)
        angles = np.concatenate([[0.0], angles], axis=0)
        centre = np.mean(pts1, axis=0, keepdims=True)
        rot = np.reshape(np.stack([np.cos(angles), -np.sin(angles), np.sin(angles), np.cos(angles)], axis=1), [-1, 2, 2])
        rotated = np.matmul(np.tile(np.expand_dims(pts1 - centre, axis=0), [n_angles + 1, 1, 1]), rot) + centre
        for k in range(1, n_angles):                   # (the last angle is never tried, as in the reference)
            rel = rotated[k] / np.array(shape)
            if np.all((rel >= 0.0) & (rel < 1.0)):
                pts1 = rotated[k]
                break

    if translation > 0:
        lo = -np.min(pts1, axis=0)
        hi = shape - np.max(pts1, axis=0)
        pts1 += rng.uniform(lo, hi)[None] * translation * difficulty

    H = compute_homography(pts1, pts2, [1.0, 1.0])
    return H, full, _project(full, H), patch_shape


# ---- photometry -----------------------------------------------------------------------------------------------------------------
def identity_taps():
    return np.zeros((1, 2), np.int32), np.ones((1,), np.float32)


def box_taps(k):
    """k x k box, k odd: k^2 taps of weight 1 / k^2, row major."""
    r = k // 2
    off = np.array([(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)], np.int32)
    return off, np.full((k * k,), 1.0 / (k * k), np.float32)


def line_taps(k, angle):
    """A line through the centre of a k x k window (k odd) at `angle` (radians, image axes): one tap per step along the
    major axis, so at most k distinct taps of equal weight."""
    r = k // 2
    c, s = math.cos(angle), math.sin(angle)
    taps = []
    for i in range(-r, r + 1):
        if abs(c) >= abs(s):
            t = (i, int(round(i * s / c)))
        else:
            t = (int(round(i * c / s)), i)
        if t not in taps:
            taps.append(t)
    off = np.array(taps, np.int32)
    return off, np.full((len(taps),), 1.0 / len(taps), np.float32)


def _odd(rng, lo, hi):
    n = (hi - lo) // 2 + 1
    return lo + 2 * min(int(rng.uniform(0.0, 1.0) * n), n - 1)


_BLUR = {"box": (3, 9), "motion": (3, 25)}
# preset -> (p of the whole chain, [(stage, p, ...)]) in the preset's order; "oneof": (p, [(child or None, weight)])
PRESETS = {
    "identity": (1.0, []),
    "lg": (0.95, [("gamma", 0.1), ("vshift", 0.1),
                  ("oneof", 0.1, [("box", 0.5), ("motion", 0.5), (None, 0.5), (None, 0.5)]),
                  ("box", 0.1), ("motion", 0.1), ("bc", 0.5)]),
    "dark": (0.75, [("bc", 0.5),
                    ("oneof", 0.1, [("box", 0.1), ("motion", 0.2), (None, 0.5), (None, 0.5)]),
                    ("gamma", 0.1),
                    ("oneof", 0.5, [(None, 0.5), (None, 0.2), (None, 0.5), (None, 0.1), ("vshift", 0.1)])]),
}
GAMMA_RANGE, VSHIFT_RANGE = (0.15, 0.65), (-100.0 / 255.0, -40.0 / 255.0)
CONTRAST_RANGE, BRIGHTNESS_RANGE = (-0.3, 0.0), (-0.4, 0.0)


def preset_blurs(name):
    """Whether views of this preset can carry more than the identity tap (decides between one launch and two)."""
    def has(stages):
        return any(s[0] in _BLUR or (s[0] == "oneof" and any(c in _BLUR for c, _ in s[2])) for s in stages)
    return has(PRESETS[name][1])


def sample_photometric(name, p=None, rng=np.random, gray=False):
    """One view's photometric draw -> (params [4] fp32 = (gamma, value shift, a, b), (tap_off [n,2] int32, tap_w [n] fp32)).
    `p` overrides the preset's own probability of applying the chain at all.  The draws do not depend on `gray` (the stages
    are the same for 1 and 3 channels); it is accepted so that a caller can pass its view setting through."""
    if name not in PRESETS:
        raise ValueError(f"photometric preset {name!r} not in {sorted(PRESETS)}")
    chain_p, stages = PRESETS[name]
    chain_p = chain_p if p is None else p
    state = {"gamma": 1.0, "vshift": 0.0, "a": 1.0, "b": 0.0, "taps": None}

    def apply(stage):
        if stage == "gamma":
            state["gamma"] = rng.uniform(*GAMMA_RANGE)
        elif stage == "vshift":
            state["vshift"] = rng.uniform(*VSHIFT_RANGE)
        elif stage == "bc":
            state["a"] = 1.0 + rng.uniform(*CONTRAST_RANGE)
            state["b"] = rng.uniform(*BRIGHTNESS_RANGE)
        elif stage == "box":
            taps = box_taps(_odd(rng, *_BLUR["box"]))
            state["taps"] = state["taps"] or taps
        elif stage == "motion":
            k, angle = _odd(rng, *_BLUR["motion"]), rng.uniform(0.0, math.pi)
            state["taps"] = state["taps"] or line_taps(k, angle)

    if stages and rng.uniform(0.0, 1.0) < chain_p:
        for stage in stages:
            if not rng.uniform(0.0, 1.0) < stage[1]:
                continue
            if stage[0] == "oneof":
                pick = rng.uniform(0.0, 1.0) * sum(w for _, w in stage[2])
                for child, w in stage[2]:
                    if pick < w:
                        if child is not None:
                            apply(child)
                        break
                    pick -= w
            else:
                apply(stage[0])
    params = np.array([state["gamma"], state["vshift"], state["a"], state["b"]], np.float32)
    return params, (state["taps"] or identity_taps())


def check_tables(view_src, src_sizes, ntaps, tap_off, n_sources, padded):
    """The ranges the kernels clamp to (include/gf_amd.h), enforced where the tables are still host arrays."""
    wmax, hmax = padded
    if view_src.min() < 0 or view_src.max() >= n_sources:
        raise ValueError("view_src outside [0, S)")
    if src_sizes.min() < 1 or src_sizes[:, 0].max() > wmax or src_sizes[:, 1].max() > hmax:
        raise ValueError(f"a source size outside [1, {wmax}] x [1, {hmax}]")
    if ntaps.min() < 1 or ntaps.max() > MAXTAPS:
        raise ValueError(f"ntaps outside [1, {MAXTAPS}]")
    if np.abs(tap_off).max() > RADIUS:
        raise ValueError(f"a tap offset beyond {RADIUS}")


# ---- the stage ------------------------------------------------------------------------------------------------------------------
class HomographyViews:
    """conf -> callable: images [B,Hmax,Wmax,C] (or [B,Hmax,Wmax]) uint8 / fp32 on the GPU -> the reference's collated batch.

    ``tables(sizes)`` samples on the host and packs everything the device needs into two arrays (one int32, one fp32);
    ``upload(tables, into=None)`` copies them (in place when `into` is a previous upload: the tensors a captured graph reads
    keep their addresses); ``run(dev, images, out=None)`` makes the launches and returns the batch, with no host read."""
    default_conf = {
        "homography": {"difficulty": 0.8, "translation": 1.0, "max_angle": 60, "n_angles": 10, "patch_shape": [640, 480],
                       "min_convexity": 0.05},
        "photometric": {"name": "dark", "p": 0.75},
        "grayscale": False,
        "triplet": False,
        "right_only": False,    # view 0 is the whole image rescaled to the patch (difficulty 0), without photometric changes
        "seed": 0,
    }

    def __init__(self, conf=None):
        self.conf = Conf.merge(Conf.create(self.default_conf), Conf.create(conf or {}))
        if self.conf.photometric.name not in PRESETS:
            raise ValueError(f"photometric preset {self.conf.photometric.name!r} not in {sorted(PRESETS)}")
        self.rng = np.random.RandomState(self.conf.seed)
        self.n_views = 3 if self.conf.triplet else 2
        self.two_launches = preset_blurs(self.conf.photometric.name)
        self.patch = tuple(int(v) for v in self.conf.homography.patch_shape)        # (pw, ph)

    # -- host ---------------------------------------------------------------------------------------------------------------------
    def _segments(self, b, s):
        v = self.n_views * b
        n_pairs = 3 if self.conf.triplet else 1
        ints = [("src_sizes", (s, 2)), ("view_src", (v,)), ("ntaps", (v,)), ("tap_off", (v, MAXTAPS, 2)),
                ("original_image_size", (b, 2))]
        floats = [("Hinv", (v, 9)), ("params", (v, NPARAM)), ("tap_w", (v, MAXTAPS)), ("H_", (v, 3, 3)), ("coords", (v, 4, 2)),
                  ("image_size", (v, 2)), ("H_pairs", (n_pairs, b, 3, 3))]
        return ints, floats

    @staticmethod
    def _carve(buf, segments):
        out, at = {}, 0
        for name, shape in segments:
            n = int(np.prod(shape))
            out[name] = buf[at:at + n].reshape(shape)
            at += n
        assert at == buf.shape[0]
        return out

    def tables(self, sizes, padded=None):
        """sizes: [B,2] (w, h) of every source on the host.  -> {"int": int32 array, "float": fp32 array, "B": B}; view k of
        image b is row k * B + b of every per-view table."""
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        b = sizes.shape[0]
        c = self.conf
        ints, floats = self._segments(b, b)
        ibuf = np.zeros(sum(int(np.prod(s)) for _, s in ints), np.int32)
        fbuf = np.zeros(sum(int(np.prod(s)) for _, s in floats), np.float32)
        ti, tf = self._carve(ibuf, ints), self._carve(fbuf, floats)
        ti["src_sizes"][:] = sizes
        ti["original_image_size"][:] = sizes
        hconf = c.homography.to_container()
        hconf["patch_shape"] = list(self.patch)
        coords = np.zeros((self.n_views, b, 4, 2), np.float32)   # the pair homographies come from the fp32 corners
        for i in range(b):                                         # per image: view 0, view 1 (, view 2), as the reference reads
            shape = (int(sizes[i, 0]), int(sizes[i, 1]))
            for k in range(self.n_views):
                left = k == 0
                conf_k = dict(hconf, difficulty=0.0) if (left and c.right_only) else hconf
                H, _, warped, _ = sample_homography_corners(shape, rng=self.rng, **conf_k)
                if left and c.right_only:
                    par, (off, wgt) = sample_photometric("identity", rng=self.rng, gray=c.grayscale)
                else:
                    par, (off, wgt) = sample_photometric(c.photometric.name, c.photometric.p, self.rng, c.grayscale)
                row = k * b + i
                ti["view_src"][row] = i
                ti["ntaps"][row] = len(wgt)
                ti["tap_off"][row, :len(wgt)] = off
                tf["tap_w"][row, :len(wgt)] = wgt
                tf["Hinv"][row] = np.linalg.inv(H).reshape(9)     # fp64 inverse, rounded once
                tf["params"][row] = par
                tf["H_"][row] = H
                tf["coords"][row] = warped
                tf["image_size"][row] = self.patch
                coords[k, i] = warped.astype(np.float32)
            pairs = [(0, 1)] + ([(0, 2), (1, 2)] if c.triplet else [])
            for j, (k0, k1) in enumerate(pairs):
                tf["H_pairs"][j, i] = compute_homography(coords[k0, i], coords[k1, i], [1, 1])
        check_tables(ti["view_src"], ti["src_sizes"], ti["ntaps"], ti["tap_off"], b,
                     padded or (int(sizes[:, 0].max()), int(sizes[:, 1].max())))
        return {"int": ibuf, "float": fbuf, "B": b}

    def upload(self, tables, into=None, device="cuda"):
        """Two host-to-device copies.  `into`: a previous return value, refreshed in place."""
        if into is None:
            into = {"int": torch.empty(tables["int"].shape, dtype=torch.int32, device=device),
                    "float": torch.empty(tables["float"].shape, dtype=torch.float32, device=device), "B": tables["B"]}
            ints, floats = self._segments(tables["B"], tables["B"])
            into.update(self._carve(into["int"], ints))
            into.update(self._carve(into["float"], floats))
        if into["B"] != tables["B"]:
            raise ValueError("upload: the batch size of the device tables differs")
        into["int"].copy_(torch.from_numpy(tables["int"]), non_blocking=True)
        into["float"].copy_(torch.from_numpy(tables["float"]), non_blocking=True)
        return into

    # -- device -------------------------------------------------------------------------------------------------------------------
    def run(self, dev, images, out=None, scratch=None):
        """dev: upload()'s tables; images [B,Hmax,Wmax,C] or [B,Hmax,Wmax].  `out` [V,Cout,ph,pw] and, for presets with a blur,
        `scratch` [V,C,ph,pw] may be preallocated (graph capture)."""
        if images.dim() == 3:
            images = images[..., None]
        b, gray = dev["B"], bool(self.conf.grayscale)
        if images.shape[0] != b:
            raise ValueError(f"run: {images.shape[0]} images for tables of {b}")
        if self.two_launches:
            scratch = ops.warp_views(images, dev["src_sizes"], dev["view_src"], dev["Hinv"], dev["params"], self.patch,
                                     finish=False, gray=gray, out=scratch)
            out = ops.filter_views(scratch, dev["tap_off"], dev["tap_w"], dev["ntaps"], dev["params"], gray=gray, out=out)
        else:
            out = ops.warp_views(images, dev["src_sizes"], dev["view_src"], dev["Hinv"], dev["params"], self.patch,
                                 finish=True, gray=gray, out=out)
        v = self.n_views
        stack = out.view(v, b, *out.shape[1:])
        batch = {"original_image_size": dev["original_image_size"]}            # int32 (the reference collates int64)
        for k in range(v):
            rows = slice(k * b, (k + 1) * b)
            batch[f"view{k}"] = {"image": stack[k], "H_": dev["H_"][rows], "coords": dev["coords"][rows],
                                 "image_size": dev["image_size"][rows]}
        for j, key in enumerate(["H_0to1"] + (["H_0to2", "H_1to2"] if self.conf.triplet else [])):
            batch[key] = dev["H_pairs"][j]
        return batch

    def __call__(self, images, sizes=None):
        if not images.is_cuda:
            raise RuntimeError("HomographyViews needs the images on a HIP device (no CPU fallback)")
        hmax, wmax = images.shape[1], images.shape[2]
        if sizes is None:
            sizes = [(wmax, hmax)] * images.shape[0]
        tables = self.tables(sizes, padded=(wmax, hmax))
        return self.run(self.upload(tables, device=images.device), images)
