"""Wireframe extractor, host side (no GPU): the C ABI carries the four gf_wf_* entries (ABI still 20), the torch form equals
the reference's recorded outputs (tests/golden/wireframe.npz, written by tools/gen_wireframe_golden.py), `lines.given`
equals a numpy restatement of LSD's post-processing, asking for the kernels on CPU tensors is an error, and every generated
scene of tests/wireframe_cases.py keeps its decisions away from rounding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import wireframe_cases as wc
from conftest import ROOT, load_golden

ENTRIES = {"gf_wf_cluster": 14, "gf_wf_suppress": 14, "gf_wf_descriptors": 14, "gf_wf_associativity": 6}


@pytest.fixture(scope="module")
def z():
    return load_golden("wireframe")


def test_header_declares_and_library_exports_the_entries():
    from glue_factory_amd import lib
    text = open(os.path.join(ROOT, "include", "gf_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+GF_AMD_ABI_VERSION\s+20\b", code)
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(so, name), name
        assert len(lib.SIGNATURES[name]) == nargs, name
    assert lib.ABI_VERSION == 20 == lib.load().gf_abi_version()


def test_entries_reject_non_positive_sizes_without_a_launch():
    """-1 before anything is enqueued (no device is touched: the pointers are never read)."""
    from glue_factory_amd import lib
    L = lib.load()
    n8, n7, n5 = (None,) * 8, (None,) * 7, (None,) * 5
    for b, l, p in ((0, 1, 4), (1, 0, 4), (1, 1, 0), (-2, 1, 4), (1, -1, 4)):
        assert L.gf_wf_cluster(*n8, b, l, p, 3.0, 1, None) == -1
        assert L.gf_wf_associativity(None, None, b, l, p, None) == -1
    for b, n, p in ((0, 1, 3), (1, 0, 3), (1, 1, 0), (1, -5, 3)):
        assert L.gf_wf_suppress(*n7, b, n, 2, p, 2, 3.0, None) == -1
    for b, p, h, w, c, s in ((0, 4, 2, 2, 64, 8), (1, 0, 2, 2, 64, 8), (1, 4, 0, 2, 64, 8), (1, 4, 2, 0, 64, 8),
                             (1, 4, 2, 2, 0, 8), (1, 4, 2, 2, 64, 0), (1, 4, 2, 2, 64, -8)):
        assert L.gf_wf_descriptors(*n5, b, p, 2, h, w, c, s, 0, None) == -1
    assert L.gf_wf_cluster(*n8, 1, 2049, 5000, 3.0, 1, None) == -1         # GF_ERR_UNSUPPORTED past the LDS limit


def test_model_resolves_by_both_names():
    from glue_factory_amd.base_model import get_model
    from glue_factory_amd.lines import given, wireframe
    assert get_model("lines.wireframe") is wireframe.WireframeExtractor is wireframe.__main_model__
    assert get_model("glue_factory_amd.lines.wireframe") is wireframe.WireframeExtractor
    assert get_model("lines.given") is given.GivenLines
    conf = wireframe.WireframeExtractor.default_conf
    assert set(conf) == {"point_extractor", "line_extractor", "wireframe_params", "fused"}
    assert conf["wireframe_params"] == {"merge_points": True, "merge_line_endpoints": True, "nms_radius": 3}
    assert wireframe.WireframeExtractor.required_data_keys == ["image"]


@pytest.mark.parametrize("fused", [None, False])
@pytest.mark.parametrize("name", list(wc.GOLDEN_CONFS))
def test_torch_form_equals_the_reference_outputs(z, name, fused):
    torch.manual_seed(3)
    wc.assert_matches_golden(wc.run_golden(z, name, fused=fused), z, name)


def test_golden_scenes_do_merge_and_suppress(z):
    """The fixture reaches the non-trivial branches: merged junctions, suppressed keypoints, padding clustered at the origin."""
    for name in ("forced", "variable"):
        nc, idx = z[name + ".out.num_junctions"], z[name + ".out.lines_junc_idx"]
        assert (nc < 2 * idx.shape[1]).all() and z[name + ".suppressed"].any()
        assert (idx[:, -6:] == idx[:, -1:, -1:]).all()
    assert (z["forced_nomerge.out.num_junctions"] == 48).all()


def test_no_lines_and_merge_points_off(z):
    """No lines: the "independent lines" outputs with an empty junction block; merge_points off: keypoints pass through."""
    from glue_factory_amd.conf import Conf
    from glue_factory_amd.lines.wireframe import wireframe_from_parts
    t = wc.golden_tensors(z, "forced")
    params = Conf.create({"merge_points": True, "merge_line_endpoints": True, "nms_radius": 3})
    empty = dict(t, lines=t["lines"][:, :0], line_scores=t["line_scores"][:, :0])
    out = wireframe_from_parts(empty, (2, 1, 128, 160), params, True, True)
    assert out["lines_junc_idx"].shape == (2, 0, 2) and out["num_junctions"].tolist() == [0, 0]
    assert torch.equal(out["keypoints"], t["keypoints"]) and torch.equal(out["descriptors"], t["descriptors"])
    assert torch.equal(out["pl_associativity"], torch.eye(64, dtype=torch.bool)[None].repeat(2, 1, 1))
    params = Conf.create({"merge_points": False, "merge_line_endpoints": True, "nms_radius": 3})
    out = wireframe_from_parts(t, (2, 1, 128, 160), params, True, True)
    assert torch.equal(out["keypoints"][:, 48:], t["keypoints"]) and torch.equal(out["descriptors"][:, 48:], t["descriptors"])
    np.testing.assert_array_equal(out["lines_junc_idx"].numpy(), z["forced.out.lines_junc_idx"])


def test_fused_on_cpu_tensors_raises(z):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wc.run_golden(z, "forced", fused=True)


def test_variable_mode_needs_a_batch_of_one(z):
    t = wc.golden_tensors(z, "forced")
    model = wc.golden_extractor(t, force=False, merge_line_endpoints=True)
    with pytest.raises(AssertionError, match="batch size of 1"):
        model({"image": torch.zeros(2, 1, 128, 160)})


def test_every_generated_scene_keeps_its_decisions_away_from_rounding():
    names = []
    for name, lines, kpts, eps, radius in wc.all_scenes():
        assert wc.band_violations(lines, kpts, eps, radius) == 0, name
        names.append(name)
    assert len(names) == len(wc.CONSTRUCTED) + len(wc.CLUSTER_SCENES) + len(wc.SUPPRESS_SCENES) + 3


def test_planted_lattice_cases_decide_as_stated():
    """d^2 == eps^2 merges, d^2 == eps^2 + 1 does not; a keypoint at exactly r stays, at exactly r - 1 goes."""
    from glue_factory_amd.lines.wireframe import cluster_endpoints
    for eps in (3, 4, 5):
        lab = cluster_endpoints(torch.from_numpy(wc.boundary_pairs(eps)[0].reshape(-1, 2)), eps)
        assert lab.tolist() == [0, 1, 0, 2]
    sc = wc.make_scene(seed=12, batch=1, n_lines=33, n_kpts=40, n_pad=5)
    ends = torch.from_numpy(sc["lines"]).reshape(1, -1, 2)
    flag = (torch.norm(torch.from_numpy(sc["keypoints"])[:, :, None] - ends[:, None], dim=-1) < 3).any(2)[0]
    assert not flag[10] and flag[11] and flag[:10].all()


# ---- lines.given against a numpy restatement of gluefactory/models/lines/lsd.py:28-53 ---------------------------------
def _lsd_postprocess(segs, scores, min_length, max_num_lines, force):
    lengths = np.linalg.norm(segs[:, 1] - segs[:, 0], axis=1)
    to_keep = lengths >= min_length
    segs, scores = segs[to_keep], scores[to_keep]
    indices = np.argsort(-scores, kind="stable")
    if max_num_lines is not None:
        indices = indices[:max_num_lines]
    segs, scores = segs[indices], scores[indices]
    n = len(segs)
    valid = np.ones(n, dtype=bool)
    if force:
        pad = max_num_lines - n
        segs = np.concatenate([segs, np.zeros((pad, 2, 2), np.float32)], 0)
        scores = np.concatenate([scores, np.zeros(pad, np.float32)], 0)
        valid = np.concatenate([valid, np.zeros(pad, dtype=bool)], 0)
    return segs, scores, valid


def _segments(seed, m, min_length=15):
    rng = np.random.RandomState(seed)
    a = rng.uniform(0, 200, (m, 2)).astype(np.float32)
    ang, ln = rng.uniform(0, 2 * np.pi, m), rng.uniform(2, 40, m)
    ln = np.where(np.abs(ln - min_length) < 0.01, ln + 1, ln)
    segs = np.stack([a, a + np.stack([ln * np.cos(ang), ln * np.sin(ang)], 1).astype(np.float32)], 1)
    for i, d in enumerate(((9, 12), (12, 9), (15, 0), (0, 15), (9, 11), (14, 0))[: m]):      # length exactly 15 (kept) / just under
        segs[i] = [[20 + i, 30], [20 + i + d[0], 30 + d[1]]]
    return segs, rng.uniform(0.1, 5, m).astype(np.float32)


@pytest.mark.parametrize("m,max_num_lines,force", [(40, 16, True), (40, 16, False), (10, 16, True), (10, None, False),
                                                   (0, 8, True), (0, None, False), (40, 64, True)])
def test_given_lines_equal_the_lsd_postprocessing(m, max_num_lines, force):
    from glue_factory_amd.base_model import get_model
    model = get_model("lines.given")({"min_length": 15, "max_num_lines": max_num_lines, "force_num_lines": force})
    batch = 3 if force else 1
    segs, scores = zip(*[_segments(40 + i, m) for i in range(batch)])
    out = model({"lines": torch.from_numpy(np.stack(segs)), "line_scores": torch.from_numpy(np.stack(scores))})
    for i in range(batch):
        want = _lsd_postprocess(segs[i], scores[i], 15, max_num_lines, force)
        for k, w in zip(("lines", "line_scores", "valid_lines"), want):
            assert out[k][i].shape == w.shape, k
            np.testing.assert_array_equal(out[k][i].numpy(), w, err_msg=k)
    if m:
        kept = out["lines"][0][out["valid_lines"][0]]
        assert any(np.array_equal(s, segs[0][0]) for s in kept.numpy())            # the length == min_length segment stays
    with pytest.raises(AssertionError):
        get_model("lines.given")({"force_num_lines": True})
