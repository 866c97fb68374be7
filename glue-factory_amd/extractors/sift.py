"""SIFT extractor (inference only) -- two paths, like aliked.py.

Interface and configuration keys are those of gluefactory/models/extractors/sift.py:
``{"image" [B,1|3,H,W] in [0,1], optional "image_size"} -> {"keypoints" [B,N,2], "scales" [B,N], "oris" [B,N],
"descriptors" [B,N,128], "keypoint_scores" [B,N]}``.  The reference runs cv2 or pycolmap on the CPU, one image at a
time; neither exists here, so the SEMANTICS are this module's own, fixed by the stock path below (Lowe's formulation
with COLMAP's parameter meanings, the ones the shipped yamls use).  All four ``backend`` strings select the same
implementation; an unknown one raises the reference's ValueError.

* Stock path (any device, fp32 or fp64 following the image): torch ops only; the statement of the semantics.
* Fused path (HIP device, fp32): csrc/sift.hip through extractors/sift_kernels.py -- gf_sift_blur (one launch per
  Gaussian level, row pass into LDS, column pass out of it, the 2x upsampling / octave subsampling folded into the
  read and the DoG level into the write), gf_sift_extrema (extremum test, refinement, thresholds, ordered list),
  gf_sift_orient and gf_sift_describe (one wave per keypoint, fixed accumulation order) and gf_sift_dedupe
  (filter_dog_point's per-pixel steps on packed keys).

Semantics
---------
Base image: gray with the kornia weights 0.299 / 0.587 / 0.114.  ``first_octave: -1``: 2x bilinear upsampling
(align_corners=False), assumed blur 0.5 of the input (1.0 after upsampling), blurred to sigma0 = 1.6.  ``first_octave: 0``:
no upsampling.  Other values raise.
Pyramid: ``num_octaves`` octaves (the pycolmap meaning; the opencv backend's wiring of num_octaves into nOctaveLayers is
NOT reproduced), S = 3 layers, 6 Gaussian levels sigma_i = sigma0 2^(i/3), each blurred from the one below by
sqrt(sigma_i^2 - sigma_{i-1}^2) with a separable normalised kernel of radius ceil(4 sigma) and reflect-101 borders; 5 DoG
levels; the next octave's base is level 3 with every second pixel taken; an octave whose shorter side would fall under
8 px ends the pyramid.
Detection: strict 26-neighbour extremum in DoG levels 1..3 with |D| > 0.8 detection_threshold, >= 1 px from the border;
up to 5 steps of the 3-D quadratic fit (offset = -H^-1 g by cofactors), moving one cell along each axis whose offset
exceeds 0.5 in magnitude; rejected when the fit leaves the volume, is singular or has not settled after 5 steps.  Kept when
|D^| >= detection_threshold, det > 0 and tr^2 r < (r + 1)^2 det with r = edge_threshold (2 x 2 spatial Hessian).
A consequence of that rule, as in Lowe's formulation: an extremum that lies half-way between two cells can make the fit
step back and forth between them and is then dropped after the 5 steps, however clean the blob; likewise a blob whose scale
falls on the seam between two octaves (refined layer near 0.5 / 3.5) can be seen by neither.
Orientation: on the Gaussian level nearest the refined scale, around the integer cell: window sigma_w = 1.5 sigma, radius
round(3 sigma_w), gradients by central differences (pixels 1 px from the border only), angle atan2(dy, dx) with y down;
36 bins with linear interpolation between the two nearest bin centres; six passes of the circular 3-tap box; peaks are
strict local maxima >= 0.8 max, refined by the parabola, reported in [0, 2 pi); at most 2 per keypoint, strongest first
(ties: lower bin first).
Descriptor: 4 x 4 cells x 8 bins around the refined position, cell width 3 sigma, window radius
round(3 sigma sqrt(2) 2.5), Gaussian window of 2 cells, trilinear interpolation, rotated by the orientation; bin index
(row 4 + col) 8 + o.  L2, clip at 0.2, L2.  NO uint8 quantisation (a deliberate difference: with rootsift it would be
scale noise only).  ``rootsift`` applies the reference's sift_to_rootsift.
Outputs: keypoints in input pixels, corner convention (centre of pixel (0, 0) = (0.5, 0.5)); scales = sigma in input
pixels; keypoint_scores = |D^| scale; points with keypoints + 0.5 >= (w, h) are dropped (per image from ``image_size``, a
device tensor; the pyramid itself is built on the whole tensor, where the reference crops first).
Post-processing: ``nms_radius`` not None -> the reference's filter_dog_point (per pixel the highest score, then the lowest
|angle|, then for radius > 0 the max-pool NMS); then the top ``max_num_keypoints`` by score.  Rows are ALWAYS delivered
by descending score (the reference keeps list order when nothing is cut).
Batching: ``force_num_keypoints: true`` pads every image to exactly max_num_keypoints rows (a deliberate difference: the
reference's min(max, len) makes its padding a no-op): keypoints uniform within the image's own keypoint range per
coordinate ((0, min(H, W)) when it has none), from a seeded device generator, drawn once per shape; zeros elsewhere.
That mode makes no host read and is capturable after one eager call (on a HIP device it takes max_num_keypoints <= 4096,
the limit of gf_topk_candidates, and raises above it); the candidate-list overflow flag is ``self.overflow``
[B].  Without it, overflow and unequal counts raise (the latter BatchedExtractionUnsupported).
"""
import math

import torch
import torch.nn.functional as F

from ..base_model import BaseModel, BatchedExtractionUnsupported

SIGMA0 = 1.6
N_LAYERS = 3
N_LEVELS = N_LAYERS + 3
N_ORI_BINS = 36
MAX_ORIS = 2
MAX_OCTAVES = 8
BACKENDS = {"opencv", "pycolmap", "pycolmap_cpu", "pycolmap_cuda"}


def level_sigma(i):
    return SIGMA0 * 2.0 ** (i / N_LAYERS)


def increment_sigma(i):
    """Blur that takes level i - 1 to level i."""
    return math.sqrt(level_sigma(i) ** 2 - level_sigma(i - 1) ** 2)


def base_sigma(first_octave):
    assumed = 0.5 * 2.0 ** (-first_octave)
    return math.sqrt(SIGMA0 ** 2 - assumed ** 2)


def gaussian_taps(sigma):
    """Normalised taps [2 r + 1] in float64, r = ceil(4 sigma)."""
    r = int(math.ceil(4.0 * sigma))
    i = torch.arange(-r, r + 1, dtype=torch.float64)
    k = torch.exp(-(i * i) / (2.0 * sigma * sigma))
    return k / k.sum()


def reflect101(idx, n):
    p = 2 * (n - 1)
    m = torch.remainder(idx, p)
    return torch.where(m < n, m, p - m)


def gaussian_blur(x, sigma):
    """x [B,h,w] -> blurred, reflect-101 borders for any radius."""
    k = gaussian_taps(sigma).to(x)
    r = (len(k) - 1) // 2
    h, w = x.shape[-2:]
    iy = reflect101(torch.arange(-r, h + r, device=x.device), h)
    ix = reflect101(torch.arange(-r, w + r, device=x.device), w)
    xp = x[:, iy][:, :, ix].unsqueeze(1)
    xp = F.conv2d(xp, k.view(1, 1, 1, -1))
    return F.conv2d(xp, k.view(1, 1, -1, 1))[:, 0]


def octave_shapes(h, w, first_octave, num_octaves):
    if first_octave == -1:
        h, w = 2 * h, 2 * w
    shapes = []
    for _ in range(num_octaves):
        if min(h, w) < 8:
            break
        shapes.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return shapes


def build_pyramid(img, first_octave, num_octaves):
    """img [B,H,W] -> (gauss, dog): per octave [B,6,h,w] and [B,5,h,w]."""
    shapes = octave_shapes(img.shape[-2], img.shape[-1], first_octave, num_octaves)
    if first_octave == -1:
        img = F.interpolate(img.unsqueeze(1), scale_factor=2, mode="bilinear", align_corners=False)[:, 0]
    base = gaussian_blur(img, base_sigma(first_octave))
    gauss, dog = [], []
    for _ in shapes:
        levels = [base]
        for i in range(1, N_LEVELS):
            levels.append(gaussian_blur(levels[-1], increment_sigma(i)))
        g = torch.stack(levels, 1)
        gauss.append(g)
        dog.append(g[:, 1:] - g[:, :-1])
        base = levels[N_LAYERS][:, ::2, ::2]
    return gauss, dog


# ---------------------------------------------------------------------------------------------- detection (stock)
def extrema_mask(D, thr):
    """D [B,5,h,w] -> bool [B,3,h-2,w-2]: strict 26-neighbour extrema with |D| > 0.8 thr."""
    h, w = D.shape[-2:]
    c = D[:, 1:4, 1:h - 1, 1:w - 1]
    nmax = nmin = None
    for ds in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if ds == 0 and dy == 0 and dx == 0:
                    continue
                n = D[:, 1 + ds:4 + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                nmax = n if nmax is None else torch.maximum(nmax, n)
                nmin = n if nmin is None else torch.minimum(nmin, n)
    return (c.abs() > 0.8 * thr) & ((c > nmax) | (c < nmin))


def _derivatives(D, b, s, y, x):
    def at(ds, dy, dx):
        return D[b, s + ds, y + dy, x + dx]
    v = at(0, 0, 0)
    g = torch.stack([0.5 * (at(0, 0, 1) - at(0, 0, -1)), 0.5 * (at(0, 1, 0) - at(0, -1, 0)), 0.5 * (at(1, 0, 0) - at(-1, 0, 0))], -1)
    dxx = at(0, 0, 1) + at(0, 0, -1) - 2 * v
    dyy = at(0, 1, 0) + at(0, -1, 0) - 2 * v
    dss = at(1, 0, 0) + at(-1, 0, 0) - 2 * v
    dxy = 0.25 * (at(0, 1, 1) - at(0, 1, -1) - at(0, -1, 1) + at(0, -1, -1))
    dxs = 0.25 * (at(1, 0, 1) - at(1, 0, -1) - at(-1, 0, 1) + at(-1, 0, -1))
    dys = 0.25 * (at(1, 1, 0) - at(1, -1, 0) - at(-1, 1, 0) + at(-1, -1, 0))
    return v, g, (dxx, dxy, dxs, dyy, dys, dss)


def _solve(hess, g):
    """offset = -H^-1 g by cofactors for the symmetric H = [[a,b,c],[b,e,f],[c,f,i]]; (offset [n,3], det != 0)."""
    a, b, c, e, f, i = hess
    c00, c01, c02 = e * i - f * f, c * f - b * i, b * f - c * e
    c11, c12, c22 = a * i - c * c, b * c - a * f, a * e - b * b
    det = a * c00 + b * c01 + c * c02
    ok = det != 0
    inv = 1.0 / torch.where(ok, det, torch.ones_like(det))
    gx, gy, gs = g.unbind(-1)
    off = torch.stack([-(c00 * gx + c01 * gy + c02 * gs) * inv, -(c01 * gx + c11 * gy + c12 * gs) * inv,
                       -(c02 * gx + c12 * gy + c22 * gs) * inv], -1)
    return off, ok


def refine_candidates(D, b, s, y, x, thr, edge_r):
    """Candidates (b, s, y, x) of one octave -> (keep, s, y, x, offset [n,3] (x, y, s), D^)."""
    h, w = D.shape[-2:]
    alive = torch.ones_like(b, dtype=torch.bool)
    done = torch.zeros_like(alive)
    for _ in range(5):
        _, g, hess = _derivatives(D, b, s, y, x)
        off, ok = _solve(hess, g)
        act = alive & ~done
        step = (off > 0.5).long() - (off < -0.5).long()
        settled = (step == 0).all(-1)
        done = done | (act & ok & settled)
        alive = alive & ~(act & ~ok)
        move = act & ok & ~settled
        x = torch.where(move, x + step[:, 0], x)
        y = torch.where(move, y + step[:, 1], y)
        s = torch.where(move, s + step[:, 2], s)
        inside = (s >= 1) & (s <= N_LAYERS) & (y >= 1) & (y <= h - 2) & (x >= 1) & (x <= w - 2)
        alive = alive & inside
        x, y, s = x.clamp(1, w - 2), y.clamp(1, h - 2), s.clamp(1, N_LAYERS)
    v, g, hess = _derivatives(D, b, s, y, x)
    off, ok = _solve(hess, g)
    dhat = v + 0.5 * (g * off).sum(-1)
    dxx, dxy, _, dyy, _, _ = hess
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    keep = alive & done & ok & (dhat.abs() >= thr) & (det > 0) & (tr * tr * edge_r < (edge_r + 1) ** 2 * det)
    return keep, s, y, x, off, dhat


# ---------------------------------------------------------------------------------------------- orientation (stock)
def _gradients(G, b, lvl, yy, xx):
    """Central differences of level `lvl` of G [B,6,h,w] at pixels (yy, xx) [M,P]; `ok` marks pixels >= 1 px inside."""
    h, w = G.shape[-2:]
    ok = (yy >= 1) & (yy <= h - 2) & (xx >= 1) & (xx <= w - 2)
    lin = ((b * N_LEVELS + lvl) * h).unsqueeze(1) * w + yy.clamp(1, h - 2) * w + xx.clamp(1, w - 2)
    flat = G.reshape(-1)
    return flat[lin + 1] - flat[lin - 1], flat[lin + w] - flat[lin - w], ok


def orientations(G, b, lvl, xi, yi, sigma, chunk=4096):
    """-> (ori [M,2] in [0, 2 pi), valid [M,2])."""
    outs = []
    for lo in range(0, len(b), chunk):
        sl = slice(lo, lo + chunk)
        outs.append(_orientations(G, b[sl], lvl[sl], xi[sl], yi[sl], sigma[sl]))
    if not outs:
        return sigma.new_zeros((0, MAX_ORIS)), torch.zeros((0, MAX_ORIS), dtype=torch.bool, device=sigma.device)
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


def _orientations(G, b, lvl, xi, yi, sigma):
    sw = 1.5 * sigma
    rad = torch.round(3.0 * sw).long()
    R = int(rad.max())
    d = torch.arange(-R, R + 1, device=G.device)
    jj, ii = d.view(-1, 1).expand(2 * R + 1, 2 * R + 1).reshape(1, -1), d.view(1, -1).expand(2 * R + 1, 2 * R + 1).reshape(1, -1)
    gx, gy, ok = _gradients(G, b, lvl, yi.unsqueeze(1) + jj, xi.unsqueeze(1) + ii)
    ok = ok & (jj.abs() <= rad.unsqueeze(1)) & (ii.abs() <= rad.unsqueeze(1))
    wgt = torch.exp(-(ii * ii + jj * jj).to(G.dtype) / (2.0 * sw * sw).unsqueeze(1)) * torch.sqrt(gx * gx + gy * gy) * ok
    fb = torch.atan2(gy, gx) * (N_ORI_BINS / (2.0 * math.pi))
    fb = torch.where(fb < 0, fb + N_ORI_BINS, fb)
    b0 = torch.floor(fb)
    fr = fb - b0
    b0 = b0.long() % N_ORI_BINS
    hist = G.new_zeros((len(b), N_ORI_BINS))
    hist.scatter_add_(1, b0, wgt * (1 - fr))
    hist.scatter_add_(1, (b0 + 1) % N_ORI_BINS, wgt * fr)
    for _ in range(6):
        hist = (hist.roll(1, 1) + hist + hist.roll(-1, 1)) / 3.0
    left, right = hist.roll(1, 1), hist.roll(-1, 1)
    peak = (hist > left) & (hist > right) & (hist >= 0.8 * hist.max(dim=1, keepdim=True).values)
    val = torch.where(peak, hist, torch.full_like(hist, -1.0))
    oris, valids = [], []
    for _ in range(MAX_ORIS):
        k = val.argmax(dim=1, keepdim=True)
        top = val.gather(1, k)
        valid = top[:, 0] > 0
        l, c, r = left.gather(1, k)[:, 0], hist.gather(1, k)[:, 0], right.gather(1, k)[:, 0]
        den = l - 2 * c + r
        dd = 0.5 * (l - r) / torch.where(valid, den, torch.ones_like(den))
        th = (k[:, 0].to(G.dtype) + dd) * (2.0 * math.pi / N_ORI_BINS)
        th = torch.where(th < 0, th + 2.0 * math.pi, th)
        th = torch.where(th >= 2.0 * math.pi, th - 2.0 * math.pi, th)
        oris.append(torch.where(valid, th, torch.zeros_like(th)))
        valids.append(valid)
        val = val.scatter(1, k, -1.0)
    return torch.stack(oris, 1), torch.stack(valids, 1)


# ---------------------------------------------------------------------------------------------- descriptor (stock)
def finish_descriptors(desc):
    """L2, clip at 0.2, L2 (rows of zeros stay zeros)."""
    desc = desc / desc.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    desc = desc.clamp(max=0.2)
    return desc / desc.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def sift_to_rootsift(x, eps=1e-6):
    x = F.normalize(x, p=1, dim=-1, eps=eps)
    x = x.clip(min=eps).sqrt()
    return F.normalize(x, p=2, dim=-1, eps=eps)


def descriptors(G, b, lvl, xo, yo, sigma, ori, chunk=512):
    """-> [M,128], finished (not RootSIFT)."""
    outs = [_descriptors(G, b[lo:lo + chunk], lvl[lo:lo + chunk], xo[lo:lo + chunk], yo[lo:lo + chunk], sigma[lo:lo + chunk],
                         ori[lo:lo + chunk]) for lo in range(0, len(b), chunk)]
    return torch.cat(outs) if outs else G.new_zeros((0, 128))


def _descriptors(G, b, lvl, xo, yo, sigma, ori):
    hw = 3.0 * sigma
    rad = torch.round(hw * (math.sqrt(2.0) * 2.5)).long()
    R = int(rad.max())
    d = torch.arange(-R, R + 1, device=G.device)
    jj, ii = d.view(-1, 1).expand(2 * R + 1, 2 * R + 1).reshape(1, -1), d.view(1, -1).expand(2 * R + 1, 2 * R + 1).reshape(1, -1)
    xi, yi = torch.round(xo).long(), torch.round(yo).long()
    yy, xx = yi.unsqueeze(1) + jj, xi.unsqueeze(1) + ii
    gx, gy, ok = _gradients(G, b, lvl, yy, xx)
    dxp, dyp = xx.to(G.dtype) - xo.unsqueeze(1), yy.to(G.dtype) - yo.unsqueeze(1)
    c, s = torch.cos(ori).unsqueeze(1), torch.sin(ori).unsqueeze(1)
    rx, ry = (c * dxp + s * dyp) / hw.unsqueeze(1), (-s * dxp + c * dyp) / hw.unsqueeze(1)
    cb, rb = rx + 1.5, ry + 1.5
    ok = ok & (jj.abs() <= rad.unsqueeze(1)) & (ii.abs() <= rad.unsqueeze(1)) & (rb > -1) & (rb < 4) & (cb > -1) & (cb < 4)
    wgt = torch.exp(-(rx * rx + ry * ry) / 8.0) * torch.sqrt(gx * gx + gy * gy) * ok
    ob = (torch.atan2(gy, gx) - ori.unsqueeze(1)) * (8.0 / (2.0 * math.pi))
    ob = ob - torch.floor(ob / 8.0) * 8.0
    r0, c0, o0 = torch.floor(rb), torch.floor(cb), torch.floor(ob)
    fr, fc, fo = rb - r0, cb - c0, ob - o0
    r0, c0, o0 = r0.long(), c0.long(), o0.long()
    desc = G.new_zeros((len(b), 128))
    for dr in (0, 1):
        for dc in (0, 1):
            for do in (0, 1):
                rr, cc, oo = r0 + dr, c0 + dc, (o0 + do) % 8
                inb = (rr >= 0) & (rr < 4) & (cc >= 0) & (cc < 4)
                wv = wgt * (fr if dr else 1 - fr) * (fc if dc else 1 - fc) * (fo if do else 1 - fo) * inb
                desc.scatter_add_(1, (rr.clamp(0, 3) * 4 + cc.clamp(0, 3)) * 8 + oo, wv)
    return finish_descriptors(desc)


# ---------------------------------------------------------------------------------------------- post-processing
def dedupe_keep(kpts, scores, angles, valid, h, w, nms_radius, fused=False):
    """The reference's filter_dog_point on padded batches: kpts [B,N,2], scores / angles / valid [B,N] -> keep [B,N].
    Scores are >= 0 (the buffers start at 0, as the reference's)."""
    b, n = scores.shape
    pix = torch.round(kpts - 0.5).long()
    ix, iy = pix[..., 0], pix[..., 1]
    valid = valid & (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    if fused:
        from . import sift_kernels
        keep, buf = sift_kernels.dedupe(ix, iy, scores, angles, valid, h, w)
    else:
        dummy = b * h * w
        lin = torch.arange(b, device=kpts.device).view(b, 1) * (h * w) + iy.clamp(0, h - 1) * w + ix.clamp(0, w - 1)

        def reduce(mask, vals, init, op):
            buf = torch.full((dummy + 1,), init, dtype=vals.dtype, device=vals.device)
            buf.scatter_reduce_(0, torch.where(mask, lin, torch.full_like(lin, dummy)).reshape(-1), vals.reshape(-1), op)
            return buf
        keep = valid & (reduce(valid, scores, 0.0, "amax")[lin] == scores)
        a = angles.abs()
        keep = keep & (reduce(keep, a, float("inf"), "amin")[lin] == a)
        buf = reduce(keep, scores, 0.0, "amax")[:dummy].view(b, h, w) if nms_radius > 0 else None
    if nms_radius > 0:
        pooled = F.max_pool2d(buf.unsqueeze(1), kernel_size=2 * nms_radius + 1, stride=1, padding=nms_radius)[:, 0]
        lin = torch.arange(b, device=kpts.device).view(b, 1) * (h * w) + iy.clamp(0, h - 1) * w + ix.clamp(0, w - 1)
        keep = keep & (buf.reshape(-1)[lin] == pooled.reshape(-1)[lin])
    return keep


def filter_dog_point(points, scales, angles, image_shape, nms_radius, scores=None):
    """The reference's signature on one list of torch tensors -> kept indices, ascending."""
    s = scales if scores is None else scores
    valid = torch.ones_like(s, dtype=torch.bool)
    keep = dedupe_keep(points[None], s[None], angles[None], valid[None], image_shape[0], image_shape[1], nms_radius)
    return keep[0].nonzero()[:, 0]


class SIFT(BaseModel):
    default_conf = {
        "rootsift": True,
        "nms_radius": 0,  # None to disable filtering entirely.
        "max_num_keypoints": 4096,
        "backend": "opencv",  # in {opencv, pycolmap, pycolmap_cpu, pycolmap_cuda}: all select this implementation
        "detection_threshold": 0.0066667,  # from COLMAP
        "edge_threshold": 10,
        "first_octave": -1,
        "num_octaves": 4,
        "force_num_keypoints": False,
        "candidate_cap": 16384,     # slots of the fused path's candidate list per image
        "padding_seed": 0,
    }
    required_data_keys = ["image"]
    batchable_views = True

    def _init(self, conf):
        if conf.backend not in BACKENDS:
            raise ValueError(f"Unknown backend: {conf.backend} not in " f"{{{','.join(BACKENDS)}}}.")
        if conf.first_octave not in (-1, 0):
            raise ValueError("SIFT: first_octave must be -1 or 0")
        if not 1 <= conf.num_octaves <= MAX_OCTAVES:
            raise ValueError(f"SIFT: num_octaves must be in 1..{MAX_OCTAVES}")
        if conf.force_num_keypoints and not conf.max_num_keypoints:
            raise ValueError("SIFT: force_num_keypoints needs max_num_keypoints")
        self.overflow = None
        self._pad_uniform = {}

    def _use_fused(self, image):
        return image.is_cuda and image.dtype == torch.float32

    # ------------------------------------------------------------------ candidates: padded [B,C] tensors
    def _detect_stock(self, dog):
        conf = self.conf
        rows = []
        for o, D in enumerate(dog):
            b, s, y, x = extrema_mask(D, conf.detection_threshold).nonzero(as_tuple=True)
            keep, s, y, x, off, dhat = refine_candidates(D, b, s + 1, y + 1, x + 1, conf.detection_threshold, float(conf.edge_threshold))
            rows.append((b[keep], torch.full_like(b[keep], o), s[keep], y[keep], x[keep], off[keep], dhat[keep]))
        b, o, s, y, x, off, dhat = (torch.cat(t) for t in zip(*rows))
        nb = dog[0].shape[0]
        order = torch.sort(b, stable=True).indices
        b, o, s, y, x, off, dhat = b[order], o[order], s[order], y[order], x[order], off[order], dhat[order]
        per_image = torch.bincount(b, minlength=nb)
        cmax = max(int(per_image.max()), 1)
        slot = torch.arange(len(b), device=b.device) - (per_image.cumsum(0) - per_image)[b]
        meta = torch.full((nb, cmax, 4), -1, dtype=torch.long, device=b.device)
        vals = dhat.new_zeros((nb, cmax, 4))
        meta[b, slot] = torch.stack([o, s, y, x], -1)
        vals[b, slot] = torch.cat([off, dhat[:, None]], -1)
        return meta, vals

    def _detect_fused(self, dog, force):
        from . import sift_kernels
        conf = self.conf
        meta, vals, count = sift_kernels.extrema(dog, conf.detection_threshold, float(conf.edge_threshold), conf.candidate_cap)
        self.overflow = count > conf.candidate_cap
        if not force:
            cmax = int(count.max())
            if cmax > conf.candidate_cap:
                raise RuntimeError(f"SIFT: {cmax} candidates exceed candidate_cap {conf.candidate_cap}")
            meta, vals = meta[:, :max(cmax, 1)], vals[:, :max(cmax, 1)]
        slot = torch.arange(meta.shape[1], device=meta.device).view(1, -1)
        meta = torch.where((slot < count.view(-1, 1)).unsqueeze(-1), meta.long(), torch.full_like(meta, -1, dtype=torch.long))
        return meta, vals

    # ------------------------------------------------------------------ per-keypoint stages on padded tensors
    def _orient(self, gauss, octv, lvl, xi, yi, sigma, fused):
        if fused:
            from . import sift_kernels
            return sift_kernels.orient(gauss, octv, lvl, xi, yi, sigma)
        ori = sigma.new_zeros(octv.shape + (MAX_ORIS,))
        valid = torch.zeros(octv.shape + (MAX_ORIS,), dtype=torch.bool, device=octv.device)
        for o, G in enumerate(gauss):
            b, n = (octv == o).nonzero(as_tuple=True)
            if len(b):
                ori[b, n], valid[b, n] = orientations(G, b, lvl[b, n], xi[b, n], yi[b, n], sigma[b, n])
        return ori, valid

    def _describe(self, gauss, octv, lvl, xo, yo, sigma, ori, fused):
        if fused:
            from . import sift_kernels
            return sift_kernels.describe(gauss, octv, lvl, xo, yo, sigma, ori, self.conf.rootsift)
        desc = sigma.new_zeros(octv.shape + (128,))
        for o, G in enumerate(gauss):
            b, n = (octv == o).nonzero(as_tuple=True)
            if len(b):
                d = descriptors(G, b, lvl[b, n], xo[b, n], yo[b, n], sigma[b, n], ori[b, n])
                desc[b, n] = sift_to_rootsift(d) if self.conf.rootsift else d
        return desc

    def _padding(self, b, k, device):
        key = (b, k, str(device))
        if key not in self._pad_uniform:
            gen = torch.Generator(device=device)
            gen.manual_seed(int(self.conf.padding_seed))
            self._pad_uniform[key] = torch.rand((b, k, 2), generator=gen, device=device, dtype=torch.float32)
        return self._pad_uniform[key]

    def _forward(self, data):
        conf = self.conf
        image = data["image"]
        if image.shape[1] == 3:
            image = 0.299 * image[:, 0:1] + 0.587 * image[:, 1:2] + 0.114 * image[:, 2:3]
        img = image[:, 0]
        nb, h, w = img.shape
        fused = self._use_fused(img)
        force = bool(conf.force_num_keypoints)
        dt = img.dtype
        if fused:
            from . import sift_kernels
            gauss, dog = sift_kernels.pyramid(img.contiguous(), conf.first_octave, conf.num_octaves)
            meta, vals = self._detect_fused(dog, force)
        else:
            gauss, dog = build_pyramid(img, conf.first_octave, conf.num_octaves)
            meta, vals = self._detect_stock(dog)
        octv, layer, yi, xi = meta.unbind(-1)
        cand = octv >= 0
        s_o = layer.to(dt) + vals[..., 2]
        sigma = SIGMA0 * torch.exp2(s_o / N_LAYERS)                      # octave pixels
        lvl = torch.round(s_o).long().clamp(0, N_LEVELS - 1)
        ori, ovalid = self._orient(gauss, octv, lvl, xi, yi, sigma, fused)
        # one row per (candidate, orientation)
        step = torch.exp2((octv.clamp(min=0) + conf.first_octave).to(dt))      # octave pixel in input pixels
        xo, yo = xi.to(dt) + vals[..., 0], yi.to(dt) + vals[..., 1]
        rep = lambda t: t.unsqueeze(2).expand(t.shape[:2] + (MAX_ORIS,) + t.shape[2:]).reshape((nb, -1) + t.shape[2:])   # noqa: E731
        valid = (cand.unsqueeze(2) & ovalid).reshape(nb, -1)
        base_step = 2.0 ** conf.first_octave
        kx, ky = (xo * (step / base_step) + 0.5) * base_step, (yo * (step / base_step) + 0.5) * base_step
        kpts = rep(torch.stack([kx, ky], -1))
        scales = rep(sigma * step)
        scores = rep(vals[..., 3].abs() * sigma * step)
        oris = ori.reshape(nb, -1)
        size = data.get("image_size")
        if size is None:
            lim = torch.cat([img.new_full((1,), w), img.new_full((1,), h)]).view(1, 1, 2)      # (no host copy: capturable)
        else:
            lim = size.to(img.device).to(dt).view(nb, 1, 2)
        valid = valid & (kpts + 0.5 < lim).all(-1)
        if conf.nms_radius is not None:
            valid = valid & dedupe_keep(kpts, scores, oris, valid, h, w, int(conf.nms_radius), fused)
        # selection by descending score
        masked = torch.where(valid, scores, torch.full_like(scores, -1.0))
        total = masked.shape[1]
        if force:
            k = int(conf.max_num_keypoints)
        else:
            counts = valid.sum(1)
            if int(counts.min()) != int(counts.max()) and not (conf.max_num_keypoints and int(counts.min()) >= conf.max_num_keypoints):
                raise BatchedExtractionUnsupported("images yield different keypoint counts: use force_num_keypoints")
            k = int(counts.min())
            if conf.max_num_keypoints:
                k = min(k, int(conf.max_num_keypoints))
        kk = min(k, total)
        if fused and force and kk > 4096:
            # the library top-k is not safe inside a captured graph on this runtime (see gf_topk_candidates in gf_amd.h)
            raise ValueError("SIFT: force_num_keypoints on a HIP device takes max_num_keypoints <= 4096 (gf_topk_candidates)")
        if fused and 0 < kk <= 4096:
            from . import sift_kernels
            sel = sift_kernels.topk(masked, kk)
        else:
            sel = torch.topk(masked, kk, dim=1).indices
        if kk < k:
            sel = torch.cat([sel, sel.new_zeros((nb, k - kk))], 1)
        take = lambda t: t.gather(1, sel if t.dim() == 2 else sel.unsqueeze(-1).expand(-1, -1, t.shape[-1]))   # noqa: E731
        svalid = take(valid)
        if kk < k:
            svalid = svalid & (torch.arange(k, device=sel.device).view(1, -1) < kk)
        kpts, scales, oris, scores = take(kpts), take(scales), take(oris), take(scores)
        s_octv = torch.where(svalid, take(rep(octv)), torch.full_like(sel, -1))
        desc = self._describe(gauss, s_octv, take(rep(lvl)), take(rep(xo)), take(rep(yo)), take(rep(sigma)), oris, fused)
        zero = lambda t: torch.where(svalid if t.dim() == 2 else svalid.unsqueeze(-1), t, torch.zeros_like(t))   # noqa: E731
        scales, oris, scores, desc = zero(scales), zero(oris), zero(scores), zero(desc)
        if force:
            big = torch.finfo(dt).max
            lo = torch.where(svalid.unsqueeze(-1), kpts, torch.full_like(kpts, big)).amin(1, keepdim=True)
            hi = torch.where(svalid.unsqueeze(-1), kpts, torch.full_like(kpts, -big)).amax(1, keepdim=True)
            none = ~svalid.any(1).view(nb, 1, 1)
            lo = torch.where(none, torch.zeros_like(lo), lo)
            hi = torch.where(none, torch.full_like(hi, float(min(h, w))), hi)
            pad = lo + (hi - lo) * self._padding(nb, k, img.device).to(dt)
            kpts = torch.where(svalid.unsqueeze(-1), kpts, pad)
        return {"keypoints": kpts, "scales": scales, "oris": oris, "descriptors": desc, "keypoint_scores": scores}

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = SIFT
