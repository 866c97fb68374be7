"""Seeded scenes for the wireframe extractor's tests (host and GPU) and for tools/gen_wireframe_golden.py.

Every scene keeps the two decisions of the extractor away from rounding: no keypoint-to-end-point distance within 1e-3 of
nms_radius and no end-point pair with |d^2 - eps^2| < 1e-3, except PLANTED integer-lattice cases whose distances are exact
in any precision (d^2 == eps^2: merged; d^2 == eps^2 + 1: not merged; d == r: kept; d == r - 1: suppressed).
``band_violations`` is the check; tests/test_wireframe_host.py asserts it on the CPU for every scene listed here, so the
GPU tests cannot hide a failure behind a borderline input.  Nothing here retries a seed: a scene that violates the band
fails that test and gets another seed by hand."""
import numpy as np
import torch

BAND = 1e-3


def band_violations(lines, kpts, eps, radius):
    """Number of (end point, end point) and (keypoint, end point) pairs inside the band that are not exact lattice cases.
    lines [B,L,2,2], kpts [B,N,2] or None; fp64 throughout."""
    bad = 0
    lines = np.asarray(lines, dtype=np.float64)
    for b in range(lines.shape[0]):
        e = lines[b].reshape(-1, 2)
        lat_e = np.all(e == np.round(e), axis=1)
        d2 = _d2(e, e)
        near = np.abs(d2 - eps * eps) < BAND
        exact = (lat_e[:, None] & lat_e[None]) & (d2 == eps * eps)
        bad += int((near & ~exact).sum())
        if kpts is not None:
            k = np.asarray(kpts, dtype=np.float64)[b]
            lat_k = np.all(k == np.round(k), axis=1)
            d = np.sqrt(_d2(k, e))
            near = np.abs(d - radius) < BAND
            exact = (lat_k[:, None] & lat_e[None]) & (d == radius)
            bad += int((near & ~exact).sum())
    return bad


def _d2(a, b):
    dx, dy = a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1]
    return dx * dx + dy * dy


def _nudge(lines, kp, eps, radius):
    """Moves a non-lattice point of every pair inside the band by 1/64 px (a few pairs per thousand points land there by
    chance); at most 8 passes, and the host test asserts the outcome."""
    e = lines.reshape(-1, 2)
    for _ in range(8):
        e64 = e.astype(np.float64)
        lat = np.all(e64 == np.round(e64), axis=1)
        d2 = _d2(e64, e64)
        bad = (np.abs(d2 - eps * eps) < BAND) & ~(lat[:, None] & lat[None] & (d2 == eps * eps))
        k64 = kp.astype(np.float64)
        latk = np.all(k64 == np.round(k64), axis=1)
        d = np.sqrt(_d2(k64, e64))
        badk = (np.abs(d - radius) < BAND) & ~(latk[:, None] & lat[None] & (d == radius))
        if not bad.any() and not badk.any():
            break
        for i in np.nonzero(bad.any(1) & ~lat)[0][::2]:
            e[i, 0] += np.float32(1 / 64)
        for i in np.nonzero(badk.any(1) & ~latk)[0]:
            kp[i, 0] += np.float32(1 / 64)


def _image_lines(rng, n_lines, n_pad, hw, eps, lattice):
    """n_lines segments whose end points are jittered copies of a few base points (chains and merges happen), the last n_pad
    zero segments; scores in (0, 1], 0 on the padding."""
    h, w = hw
    real = n_lines - n_pad
    lines = np.zeros((n_lines, 2, 2), np.float32)
    scores = np.zeros(n_lines, np.float32)
    if real > 0:
        nbase = max(2, real // 2 + 1)
        if lattice:
            base = np.stack([rng.randint(8, w - 8, nbase), rng.randint(8, h - 8, nbase)], 1).astype(np.float32)
            jit = rng.randint(-int(eps), int(eps) + 1, (real, 2, 2)).astype(np.float32)
        else:
            base = np.stack([rng.uniform(8, w - 8, nbase), rng.uniform(8, h - 8, nbase)], 1).astype(np.float32)
            ang, rad = rng.uniform(0, 2 * np.pi, (real, 2)), 0.8 * eps * np.sqrt(rng.uniform(0, 1, (real, 2)))
            jit = np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1).astype(np.float32)
        pick = np.stack([rng.permutation(nbase)[:2] if nbase > 2 else np.array([0, 1]) for _ in range(real)])
        pick = np.where(rng.uniform(size=(real, 1)) < 0.5, pick, rng.randint(0, nbase, (real, 2)))
        lines[:real] = base[pick] + jit
        scores[:real] = rng.uniform(0.05, 1.0, real).astype(np.float32)
    return lines, scores


def plant_lattice_pairs(lines, eps, at=(40, 30)):
    """Overwrites lines 0 and 1 (L >= 2): d^2 == eps^2 between their first end points (merged), d^2 == eps^2 + 1 between
    their second end points (not merged)."""
    x, y = at
    e = int(eps)
    lines[0] = [[x, y], [x + 40, y + 20]]
    lines[1] = [[x + e, y], [x + 40 + e, y + 21]]
    return lines


def make_scene(seed, batch, n_lines, n_kpts, hw=(128, 160), eps=3, n_pad=0, lattice=False, plant=True):
    """dict of numpy arrays: lines [B,L,2,2], line_scores [B,L], valid_lines [B,L], keypoints [B,N,2], keypoint_scores [B,N].
    Keypoints: uniform, a few next to end points (suppressed), and with ``plant`` two lattice keypoints at exactly r (kept)
    and exactly r - 1 (suppressed) from the first end point of line 0."""
    rng = np.random.RandomState(seed)
    h, w = hw
    radius = eps                                                 # the extractor uses nms_radius for both decisions
    out = {k: [] for k in ("lines", "line_scores", "valid_lines", "keypoints", "keypoint_scores")}
    for _ in range(batch):
        lines, scores = _image_lines(rng, n_lines, n_pad, hw, eps, lattice)
        planted = plant and n_lines - n_pad >= 2
        if planted:
            plant_lattice_pairs(lines, eps)
        kp = np.stack([rng.uniform(0, w - 1, n_kpts), rng.uniform(0, h - 1, n_kpts)], 1).astype(np.float32)
        ends = lines[: n_lines - n_pad].reshape(-1, 2)
        near = min(n_kpts // 4, len(ends))
        if near:
            sel = rng.choice(len(ends), near, replace=False)
            kp[:near] = ends[sel] + (0.5 * radius * rng.uniform(-0.7, 0.7, (near, 2))).astype(np.float32)
        if planted and n_kpts >= near + 2:
            kp[near] = lines[0, 0] + np.float32([0, -radius])
            kp[near + 1] = lines[0, 0] + np.float32([-(radius - 1), 0])
        _nudge(lines, kp, eps, radius)
        out["lines"].append(lines)
        out["line_scores"].append(scores)
        out["valid_lines"].append(np.arange(n_lines) < n_lines - n_pad)
        out["keypoints"].append(kp)
        out["keypoint_scores"].append(rng.uniform(0.01, 1.0, n_kpts).astype(np.float32))
    return {k: np.stack(v) for k, v in out.items()}


# ---- constructed end-point sets for the cluster entry: name -> lines [B,L,2,2], eps -----------------------------------
def _pairs(points):
    points = np.asarray(points, np.float32)
    assert len(points) % 2 == 0
    return points.reshape(1, -1, 2, 2)


def chain(eps=3, count=300, seed=5):
    """`count` lattice points spaced exactly eps apart in shuffled index order: one cluster, the longest propagation."""
    pts = np.stack([10 + eps * np.arange(count), np.full(count, 20)], 1).astype(np.float32)
    return _pairs(pts[np.random.RandomState(seed).permutation(count)])


def isolated(eps=3, count=128):
    pts = np.stack([(np.arange(count) % 16) * (2 * eps + 1) + 5, (np.arange(count) // 16) * (2 * eps + 1) + 5], 1)
    return _pairs(pts)


def clique(eps=3, count=128, seed=6):
    rng = np.random.RandomState(seed)
    ang, rad = rng.uniform(0, 2 * np.pi, count), 0.45 * eps * np.sqrt(rng.uniform(0, 1, count))
    return _pairs(np.stack([50 + rad * np.cos(ang), 60 + rad * np.sin(ang)], 1))


def padded_near_origin(eps=3):
    """Zero segments: their end points at (0,0) form one cluster with the real end point (1,2) (d^2 = 5 <= 9); (3,1) is out
    (d^2 = 10 from the origin) unless it chains through (1,2) (d^2 = 5): it does, so the cluster is {pads, (1,2), (3,1)}."""
    lines = np.zeros((1, 6, 2, 2), np.float32)
    lines[0, 0] = [[1, 2], [50, 50]]
    lines[0, 1] = [[3, 1], [80, 20]]
    lines[0, 2] = [[60, 90], [51, 52]]
    return lines


def duplicates():
    pts = [[10, 10], [30, 30], [10, 10], [30, 30], [10, 10], [70, 70], [70, 70], [90, 5]]
    return _pairs(pts)


def boundary_pairs(eps=3):
    lines = np.zeros((1, 2, 2, 2), np.float32)
    return plant_lattice_pairs(lines[0], eps)[None]


CONSTRUCTED = {"chain": chain, "isolated": isolated, "clique": clique, "padded_near_origin": padded_near_origin,
               "duplicates": duplicates, "boundary_pairs": boundary_pairs}

# ---- the random scenes of the GPU tests: (seed, batch, L, N, hw, eps, n_pad, lattice) ----------------------------------
CLUSTER_SCENES = {
    "L1": dict(seed=11, batch=3, n_lines=1, n_kpts=4, hw=(128, 160)),
    "L33": dict(seed=12, batch=3, n_lines=33, n_kpts=4, hw=(128, 160), n_pad=5),
    "L250": dict(seed=13, batch=3, n_lines=250, n_kpts=4, hw=(480, 640), n_pad=20),
    "L512": dict(seed=14, batch=3, n_lines=512, n_kpts=4, hw=(1024, 1024), eps=4),
    "L2048": dict(seed=15, batch=1, n_lines=2048, n_kpts=4, hw=(2048, 2048), n_pad=100),
    "L250_lattice": dict(seed=16, batch=3, n_lines=250, n_kpts=4, hw=(128, 160), eps=5, lattice=True),
}
SUPPRESS_SCENES = {
    "N1_n2": dict(seed=21, batch=2, n_lines=1, n_kpts=1, hw=(64, 64), plant=False),
    "N65_n2": dict(seed=22, batch=2, n_lines=1, n_kpts=65, hw=(64, 64), plant=False),
    "N65_n500": dict(seed=23, batch=2, n_lines=250, n_kpts=65, hw=(480, 640)),
    "N1000_n500": dict(seed=24, batch=2, n_lines=250, n_kpts=1000, hw=(480, 640)),
    "N1000_n2": dict(seed=25, batch=2, n_lines=1, n_kpts=1000, hw=(64, 64), plant=False),
}
# the three golden scenes (tools/gen_wireframe_golden.py): 128 x 160 image, s = 8, C = 64, N = 64, L = 24 of which 6 padded
GOLDEN_SCENES = {
    "forced": dict(seed=31, batch=2), "forced_nomerge": dict(seed=32, batch=2), "variable": dict(seed=33, batch=1),
}
GOLDEN_GEOMETRY = dict(n_lines=24, n_kpts=64, hw=(128, 160), n_pad=6)
GOLDEN_C, GOLDEN_S = 64, 8


def golden_inputs(name):
    """Scene + seeded descriptors / dense map of one golden scene (numpy)."""
    spec = GOLDEN_SCENES[name]
    sc = make_scene(**spec, **GOLDEN_GEOMETRY)
    g = torch.Generator().manual_seed(spec["seed"])
    b, (h, w) = spec["batch"], GOLDEN_GEOMETRY["hw"]
    desc = torch.nn.functional.normalize(torch.randn(b, GOLDEN_GEOMETRY["n_kpts"], GOLDEN_C, generator=g), dim=-1)
    dense = torch.nn.functional.normalize(torch.randn(b, GOLDEN_C, h // GOLDEN_S, w // GOLDEN_S, generator=g), dim=1)
    sc["descriptors"], sc["dense_descriptors"] = desc.numpy(), dense.numpy()
    return sc


def all_scenes():
    """(name, lines, keypoints or None, eps, radius) of every scene above, for the band check."""
    for name, fn in CONSTRUCTED.items():
        yield name, fn(), None, 3, 3
    for group in (CLUSTER_SCENES, SUPPRESS_SCENES):
        for name, spec in group.items():
            sc = make_scene(**spec)
            eps = spec.get("eps", 3)
            yield name, sc["lines"], sc["keypoints"], eps, eps
    for name in GOLDEN_SCENES:
        sc = golden_inputs(name)
        yield "golden_" + name, sc["lines"], sc["keypoints"], 3, 3


# ---- the golden scenes through this package's extractor, and the assertions both the host and the GPU test make ----------
GOLDEN_CONFS = {
    "forced": dict(force=True, merge_line_endpoints=True),
    "forced_nomerge": dict(force=True, merge_line_endpoints=False),
    "variable": dict(force=False, merge_line_endpoints=True),
}


def golden_extractor(tensors, force, merge_line_endpoints, fused=None):
    """WireframeExtractor whose two sub-extractors hand back copies of ``tensors`` (what the fixture's generator plugs into
    the reference)."""
    from glue_factory_amd.lines.wireframe import WireframeExtractor

    class Feed(torch.nn.Module):
        batchable_views = True

        def __init__(self, keys):
            super().__init__()
            self.keys = keys

        def forward(self, data):
            return {k: tensors[k] for k in self.keys}           # (never written to: no copies)

    class Fixture(WireframeExtractor):
        def _init(self, conf):
            self.point_extractor = Feed(("keypoints", "keypoint_scores", "descriptors", "dense_descriptors"))
            self.line_extractor = Feed(("lines", "line_scores", "valid_lines"))

    return Fixture({
        "point_extractor": {"name": "fixture", "max_num_keypoints": tensors["keypoints"].shape[1], "force_num_keypoints": force},
        "line_extractor": {"name": "fixture", "max_num_lines": tensors["lines"].shape[1], "force_num_lines": force},
        "wireframe_params": {"merge_points": True, "merge_line_endpoints": merge_line_endpoints, "nms_radius": 3},
        "fused": fused,
    })


def golden_tensors(z, name, device="cpu"):
    pre = name + ".in."
    return {k[len(pre):]: torch.from_numpy(v).to(device) for k, v in z.items() if k.startswith(pre)}


def run_golden(z, name, device="cpu", fused=None):
    t = golden_tensors(z, name, device)
    model = golden_extractor(t, fused=fused, **GOLDEN_CONFS[name])
    h, w = GOLDEN_GEOMETRY["hw"]
    return model({"image": torch.zeros(t["lines"].shape[0], 1, h, w, device=device)})


def assert_matches_golden(pred, z, name):
    """Bit for bit on every decision and on the true-junction rows; descriptors at rtol 1e-5 / atol 1e-6 (the bound of
    test_sample_descriptors_kernel for the same arithmetic); random-fill rows by property."""
    from glue_factory_amd.lines.wireframe import sample_descriptors_corner_conv
    ref = {k[len(name) + 5:]: v for k, v in z.items() if k.startswith(name + ".out.")}
    inp = {k: v.cpu().numpy() for k, v in golden_tensors(z, name).items()}
    sup = z[name + ".suppressed"]
    assert set(pred) == set(ref)
    got = {k: v.detach().cpu().numpy() for k, v in pred.items()}
    for k in ("lines_junc_idx", "num_junctions", "pl_associativity", "lines", "orig_lines", "valid_lines", "line_scores"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    for k in ("keypoints", "keypoint_scores", "descriptors"):
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float32, k
    (h, w), n = GOLDEN_GEOMETRY["hw"], 2 * inp["lines"].shape[1]
    dense = torch.from_numpy(inp["dense_descriptors"])
    tol = dict(rtol=1e-5, atol=1e-6)
    if not GOLDEN_CONFS[name]["force"]:
        np.testing.assert_array_equal(got["keypoints"], ref["keypoints"])
        np.testing.assert_array_equal(got["keypoint_scores"], ref["keypoint_scores"])
        np.testing.assert_allclose(got["descriptors"], ref["descriptors"], **tol)
        nc = int(ref["num_junctions"][0])
        np.testing.assert_array_equal(got["keypoints"][0, nc:], inp["keypoints"][0][~sup[0]])
        np.testing.assert_array_equal(got["descriptors"][0, nc:], inp["descriptors"][0][~sup[0]])
        return
    np.testing.assert_array_equal(got["keypoint_scores"][:, n:] == 0, sup)           # the suppressed-keypoint mask
    for b in range(sup.shape[0]):
        nc = int(ref["num_junctions"][b])
        det = np.concatenate([np.arange(nc), n + np.nonzero(~sup[b])[0]])
        fill = np.setdiff1d(np.arange(got["keypoints"].shape[1]), det)
        np.testing.assert_array_equal(got["keypoints"][b, det], ref["keypoints"][b, det])
        np.testing.assert_array_equal(got["keypoint_scores"][b, det], ref["keypoint_scores"][b, det])
        np.testing.assert_allclose(got["descriptors"][b, det], ref["descriptors"][b, det], **tol)
        np.testing.assert_array_equal(got["descriptors"][b, n:][~sup[b]], inp["descriptors"][b][~sup[b]])
        assert len(fill) == (n - nc) + int(sup[b].sum()) and len(fill) > 0
        pos = got["keypoints"][b, fill]
        assert (pos >= 0).all() and (pos[:, 0] <= w - 1).all() and (pos[:, 1] <= h - 1).all()
        assert len(np.unique(pos, axis=0)) == len(pos)                               # drawn, not a constant
        np.testing.assert_array_equal(got["keypoint_scores"][b, fill], 0)
        want = sample_descriptors_corner_conv(torch.from_numpy(pos)[None], dense[b:b + 1], GOLDEN_S).mT[0].numpy()
        np.testing.assert_allclose(got["descriptors"][b, fill], want, **tol)
