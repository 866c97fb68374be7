"""CPU checks of the SIFT extractor: the stock path of glue_factory_amd/extractors/sift.py against the fp64 restatement
of tests/sift_cases.py (equal in fp64, agreeing on every decisive candidate in fp32), the named mutations, planted blobs,
the module's interface, and the post-processing against the reference's own filter_dog_point / sift_to_rootsift (live
where the reference checkout exists, and always against their recorded outputs in tests/golden/sift_post.npz)."""
import json
import os

import numpy as np
import pytest
import torch

import sift_cases as sc
from conftest import GOLDEN
from glue_factory_amd.base_model import BatchedExtractionUnsupported, get_model
from glue_factory_amd.extractors import sift as S
from glue_factory_amd.extractors.sift import SIFT

IMAGES = {"plain": 0, "odd": 1, "early": 2, "coarse": 3, "e2e": 4}
_cache = {}


def _image(name):
    i = IMAGES[name]
    return sc.case_images()[i] if i < 4 else sc.e2e_batch()[0][0, 0].numpy()


def _reference(name):
    if name not in _cache:
        _cache[name] = sc.ref_keypoints(_image(name))
    return _cache[name]


def _stock(name, dtype):
    """Stock stages on one image: pyramid, candidate list [(octave, layer, y, x)], values, orientations."""
    key = (name, dtype)
    if key not in _cache:
        img = torch.from_numpy(_image(name)).to(dtype)[None]
        gauss, dog = S.build_pyramid(img, -1, 4)
        m = SIFT({"nms_radius": None, "max_num_keypoints": None, "rootsift": False})
        meta, vals = m._detect_stock(dog)
        ok = meta[0, :, 0] >= 0
        _cache[key] = (gauss, dog, meta[0][ok], vals[0][ok])
    return _cache[key]


def _stage_inputs(meta, vals, dtype):
    octv, layer, yi, xi = meta.unbind(-1)
    s_o = layer.to(dtype) + vals[:, 2]
    sigma = S.SIGMA0 * torch.exp2(s_o / 3)
    lvl = torch.round(s_o).long().clamp(0, 5)
    return octv, lvl, xi, yi, sigma, xi.to(dtype) + vals[:, 0], yi.to(dtype) + vals[:, 1]


def _stock_orientations(gauss, meta, vals, dtype):
    octv, lvl, xi, yi, sigma, _, _ = _stage_inputs(meta, vals, dtype)
    oris = []
    for i in range(len(meta)):
        o, v = S.orientations(gauss[int(octv[i])], torch.zeros(1, dtype=torch.long), lvl[i:i + 1], xi[i:i + 1], yi[i:i + 1], sigma[i:i + 1])
        oris.append([float(a) for a, ok in zip(o[0], v[0]) if ok])
    return oris


@pytest.mark.parametrize("name", list(IMAGES))
def test_stock_fp64_equals_restatement(name):
    gauss_r, dog_r, cands = _reference(name)
    gauss, dog, meta, vals = _stock(name, torch.float64)
    assert len(gauss) == len(gauss_r) == 4
    for o in range(len(gauss_r)):
        assert gauss[o].shape[1:] == gauss_r[o].shape
        np.testing.assert_allclose(gauss[o][0].numpy(), gauss_r[o], rtol=0, atol=1e-13)
        np.testing.assert_allclose(dog[o][0].numpy(), dog_r[o], rtol=0, atol=1e-13)
    acc = sc.accepted(cands)
    assert [tuple(int(v) for v in row) for row in meta] == [(c["octave"],) + tuple(int(v) for v in c["cell"]) for c in acc]
    assert len(acc) >= 3
    oris = _stock_orientations(gauss, meta, vals, torch.float64)
    octv, lvl, xi, yi, sigma, xo, yo = _stage_inputs(meta, vals, torch.float64)
    for i, c in enumerate(acc):
        np.testing.assert_allclose(vals[i, :3].numpy(), c["offset"], rtol=0, atol=1e-9)
        assert abs(float(vals[i, 3]) - c["dhat"]) < 1e-12 and int(lvl[i]) == c["level"] and abs(float(sigma[i]) - c["sigma"]) < 1e-12
        np.testing.assert_allclose(oris[i], c["oris"], rtol=0, atol=1e-9)
        for th in c["oris"]:
            for rootsift in (False, True):
                d = S.descriptors(gauss[c["octave"]], torch.zeros(1, dtype=torch.long), lvl[i:i + 1], xo[i:i + 1], yo[i:i + 1], sigma[i:i + 1],
                                  torch.tensor([th], dtype=torch.float64))
                d = S.sift_to_rootsift(d) if rootsift else d
                ref, _ = sc.ref_describe(gauss_r[c["octave"]][c["level"]], c["xy_oct"][0], c["xy_oct"][1], c["sigma"], th, rootsift=rootsift)
                np.testing.assert_allclose(d[0].numpy(), ref, rtol=0, atol=1e-9)


def test_early_ending_pyramid():
    assert S.octave_shapes(33, 40, -1, 8) == [(66, 80), (33, 40), (17, 20), (9, 10)]
    assert S.octave_shapes(33, 40, 0, 4) == [(33, 40), (17, 20), (9, 10)]
    assert len(_reference("early")[0]) == 4 and len(sc.ref_pyramid(_image("early"), -1, 8)[0]) == 4


@pytest.mark.parametrize("name", list(IMAGES))
def test_stock_fp32_agrees_on_decisive_candidates(name):
    gauss_r, dog_r, cands = _reference(name)
    gauss, dog, meta, vals = _stock(name, torch.float32)
    for o in range(len(gauss_r)):
        assert np.abs(gauss[o][0].double().numpy() - gauss_r[o]).max() <= sc.e_level(o)
        assert np.abs(dog[o][0].double().numpy() - dog_r[o]).max() <= sc.e_dog(o)
    mine = {tuple(int(v) for v in row): i for i, row in enumerate(meta)}
    by_cell = {(c["octave"],) + tuple(int(v) for v in c["cell"]): c for c in sc.accepted(cands)}
    undecided = {(c["octave"],) + tuple(int(v) for v in c.get("cell", c["cell0"])) for c in cands if not sc.decisive(c)}
    undecided |= {(c["octave"],) + tuple(int(v) for v in c["cell0"]) for c in cands if not sc.decisive(c)}
    oris = _stock_orientations(gauss, meta, vals, torch.float32)
    octv, lvl, xi, yi, sigma, xo, yo = _stage_inputs(meta, vals, torch.float32)
    for cell, c in by_cell.items():
        if sc.decisive(c):
            assert cell in mine, cell
    for cell, i in mine.items():
        assert cell in by_cell or cell in undecided, cell
        c = by_cell.get(cell)
        if c is None or not sc.decisive(c):
            continue
        assert np.all(np.abs(vals[i, :3].double().numpy() - c["offset"]) <= c["offset_band"] + 4 * sc.U)
        assert abs(float(vals[i, 3]) - c["dhat"]) <= 3 * sc.e_dog(c["octave"])
        assert len(oris[i]) == len(c["oris"])
        ks = [int(np.round(th * 36 / (2 * np.pi))) % 36 for th in c["oris"]]
        for th, ref, k in zip(oris[i], c["oris"], ks):
            assert abs(th - ref) <= sc.ori_bound(c["hist"], k, c["ori_bin_bound"]), (th, ref)
        d = S.descriptors(gauss[c["octave"]], torch.zeros(1, dtype=torch.long), lvl[i:i + 1], xo[i:i + 1], yo[i:i + 1], sigma[i:i + 1],
                          torch.tensor([c["oris"][0]], dtype=torch.float32))
        # the restatement at the fp32 path's own inputs: the bound covers the rounding of this stage
        ref, bound = sc.ref_describe(gauss[c["octave"]][0, c["level"]].double().numpy(), float(xo[i]), float(yo[i]), float(sigma[i]),
                                     float(np.float32(c["oris"][0])), e_level=sc.e_level(c["octave"]))
        assert np.abs(d[0].double().numpy() - ref).max() <= bound


def test_nondecisive_share_is_at_most_ten_percent():
    images = sc.case_images() + [im[0].numpy() for im in sc.e2e_batch()[0]] + sc.shift_pair()[0]
    coarse = [c for c in sc.ref_keypoints(sc.coarse_image())[2] if c["accepted"]]
    assert sum(c["octave"] == 2 for c in coarse) >= 1 and sum(c["octave"] >= 2 for c in coarse) >= 3     # the small octaves are used
    for img in images:
        assert img.max() <= sc.VMAX and img.min() >= 0
        cands = sc.ref_keypoints(img)[2]
        n_bad = sum(not sc.decisive(c) for c in cands)
        assert len(cands) >= 3 and n_bad <= 0.1 * len(cands), (img.shape, len(cands), n_bad)


def test_mutations_are_caught():
    img = _image("odd")
    gauss_r, dog_r, cands = _reference("odd")
    for mut in ({"radius_delta": -1}, {"border": "zero"}):
        g, _ = sc.ref_pyramid(img, **mut)
        assert any(np.abs(a - b).max() > 4 * sc.e_level(o) for o, (a, b) in enumerate(zip(g, gauss_r))), mut
    caught = {"clip": False, "cells": False, "window": False}
    for c in sc.accepted(cands):
        L = gauss_r[c["octave"]][c["level"]]
        s, y, x = c["cell"]
        oris_m = sc.ref_orient(L, x, y, c["sigma"], window=1.0)[0]
        k = int(np.round(c["oris"][0] * 36 / (2 * np.pi))) % 36
        caught["window"] |= bool(abs(oris_m[0] - c["oris"][0]) > sc.ori_bound(c["hist"], k, c["ori_bin_bound"]))
        d, bound = sc.ref_describe(L, c["xy_oct"][0], c["xy_oct"][1], c["sigma"], c["oris"][0])
        caught["cells"] |= np.abs(sc.ref_describe(L, c["xy_oct"][0], c["xy_oct"][1], c["sigma"], c["oris"][0], transpose_cells=True)[0] - d).max() > bound
    L, xo, yo, sigma, ori = sc.edge_level()
    d, bound = sc.ref_describe(L, xo, yo, sigma, ori)
    caught["clip"] = bool(np.abs(sc.ref_describe(L, xo, yo, sigma, ori, clip=False)[0] - d).max() > bound)
    stock = S.descriptors(torch.from_numpy(L)[None, None].expand(1, 6, -1, -1).contiguous(), torch.zeros(1, dtype=torch.long),
                          torch.tensor([2]), torch.tensor([xo], dtype=torch.float64), torch.tensor([yo], dtype=torch.float64),
                          torch.tensor([sigma], dtype=torch.float64), torch.tensor([ori], dtype=torch.float64))
    np.testing.assert_allclose(stock[0].numpy(), d, rtol=0, atol=1e-9)
    assert caught == {"clip": True, "cells": True, "window": True}


def test_the_prefilter_mutation_is_caught_on_a_stack_built_for_it():
    """sift_cases.prefilter_stack(): the restatement accepts the cell only without the 0.8 prefilter, decisively, and the stock
    path's ACCEPTED list equals the restatement's with the prefilter (the cell absent), in fp64 and in fp32."""
    D, cell = sc.prefilter_stack()
    with_pf, without = sc.ref_detect(D), sc.ref_detect(D, prefilter=0.0)
    acc = lambda cands: [tuple(int(v) for v in c["cell"]) for c in cands if c["accepted"]]   # noqa: E731
    assert cell not in acc(with_pf) and cell in acc(without) and set(acc(without)) - set(acc(with_pf)) == {cell}
    hit = next(c for c in without if c["accepted"] and tuple(c["cell"]) == cell)
    assert hit["margin"] > 10 and abs(hit["dhat"]) >= sc.THR and abs(D[cell]) < 0.8 * sc.THR - 10 * sc.E_DOG
    assert all(c["margin"] > 10 for c in with_pf if c["accepted"])
    for dtype in (torch.float64, torch.float32):
        Dt = torch.from_numpy(D).to(dtype)[None]
        b, s, y, x = S.extrema_mask(Dt, sc.THR).nonzero(as_tuple=True)
        keep, s, y, x, _, _ = S.refine_candidates(Dt, b, s + 1, y + 1, x + 1, sc.THR, sc.EDGE)
        assert [(int(i), int(j), int(k)) for i, j, k in zip(s[keep], y[keep], x[keep])] == acc(with_pf)


def test_planted_blobs_are_found():
    """Position within 0.5 px; scale within one layer (a factor 2^(1/3)) of sigma_blob.  For a 2-D Gaussian blob of
    standard deviation sigma_blob the scale-normalised Laplacian peaks at sigma = sigma_blob, and a DoG level labelled with
    its lower sigma at sigma_blob / sqrt(2^(1/3)) = 0.89 sigma_blob; measured here: 0.877 .. 0.886 sigma_blob.  (A centre of
    sigma_blob sqrt(2), the figure for a 1-D profile, would need 1.12 .. 1.78 sigma_blob and is missed by every blob.)
    Blobs on the seam between two octaves (sift_cases.OCTAVE_SEAM) are not planted, and the image is one where no blob sits
    half-way between two cells of its octave: there the stated refinement rule (one cell per step, rejected when it has not
    settled after 5) can oscillate and drop the blob, as in Lowe's formulation."""
    img, blobs = sc.make_image(96, 128, 3, n_blobs=12, asym=0.0, texture=False, avoid_seams=True)
    out = SIFT({"nms_radius": None, "max_num_keypoints": None})({"image": torch.from_numpy(img)[None, None]})
    kp, scales = out["keypoints"][0].numpy(), out["scales"][0].numpy()
    assert len(blobs) >= 8
    for x, y, s, _ in blobs:
        d = np.hypot(kp[:, 0] - x, kp[:, 1] - y)
        i = int(d.argmin())
        assert d[i] <= 0.5, (x, y, s, d[i])
        assert 2.0 ** (-1 / 3) <= scales[i] / s <= 2.0 ** (1 / 3), (s, scales[i])


def test_interface_and_batching():
    imgs, sizes = sc.e2e_batch()
    rgb = imgs.float().repeat(1, 3, 1, 1)
    conf = {"max_num_keypoints": 40, "force_num_keypoints": True, "nms_radius": 3}
    out = SIFT(conf)({"image": rgb, "image_size": sizes})
    assert {k: tuple(v.shape) for k, v in out.items()} == {"keypoints": (3, 40, 2), "scales": (3, 40), "oris": (3, 40),
                                                           "descriptors": (3, 40, 128), "keypoint_scores": (3, 40)}
    real = out["scales"] > 0
    assert real.sum(1).min() >= 5 and (~real).any()                 # some rows are padding
    norms = out["descriptors"].norm(dim=-1)
    torch.testing.assert_close(norms[real], torch.ones_like(norms[real]), rtol=0, atol=1e-5)
    assert (out["descriptors"][~real] == 0).all() and (out["oris"][~real] == 0).all() and (out["keypoint_scores"][~real] == 0).all()
    assert ((out["oris"] >= 0) & (out["oris"] < 2 * np.pi)).all()
    for b in range(3):
        k = out["keypoints"][b]
        assert (k[real[b]] + 0.5 < sizes[b]).all()
        lo, hi = k[real[b]].amin(0), k[real[b]].amax(0)
        assert ((k[~real[b]] >= lo) & (k[~real[b]] <= hi)).all()     # padding inside the image's own keypoint range
    assert (out["keypoint_scores"][:, :-1] >= out["keypoint_scores"][:, 1:]).all()
    again = SIFT(conf)({"image": rgb, "image_size": sizes})
    assert all(torch.equal(out[k], again[k]) for k in out)           # seeded padding
    gray = SIFT(conf)({"image": (0.299 * rgb[:, 0:1] + 0.587 * rgb[:, 1:2] + 0.114 * rgb[:, 2:3]), "image_size": sizes})
    assert torch.equal(gray["keypoints"], out["keypoints"])
    empty = SIFT(conf)({"image": torch.full((1, 1, 32, 32), 0.5)})
    assert (empty["scales"] == 0).all() and ((empty["keypoints"] >= 0) & (empty["keypoints"] <= 32)).all()
    with pytest.raises(BatchedExtractionUnsupported):
        SIFT({"max_num_keypoints": None, "nms_radius": 0})({"image": rgb, "image_size": sizes})
    for backend in ("opencv", "pycolmap", "pycolmap_cpu", "pycolmap_cuda"):
        SIFT({"backend": backend})
    with pytest.raises(ValueError, match="Unknown backend"):
        SIFT({"backend": "vlfeat"})
    with pytest.raises(ValueError):
        SIFT({"first_octave": 1})
    with pytest.raises(NotImplementedError):
        SIFT({}).loss({}, {})
    o0 = SIFT({"first_octave": 0, "nms_radius": None})({"image": imgs[:1].float()})
    assert o0["keypoints"].shape[1] >= 5
    assert get_model("extractors.sift") is SIFT and get_model("glue_factory_amd.extractors.sift") is SIFT


def test_yaml_extractor_blocks_construct_this_module():
    blocks = json.load(open(os.path.join(GOLDEN, "sift_extractor_blocks.json")))
    assert set(blocks) == {"sift+lightglue_homography.yaml", "sift+lightglue_megadepth.yaml", "sift+lightglue-official.yaml", "sift+NN.yaml"}
    for name, block in blocks.items():
        model = get_model(block["name"])(block)
        assert isinstance(model, SIFT) and model.conf.max_num_keypoints == block["max_num_keypoints"], name
    img = sc.e2e_batch()[0][:1].float()
    out = get_model("extractors.sift")(blocks["sift+NN.yaml"])({"image": img})          # nms_radius -1: dedupe, no NMS
    assert out["descriptors"].shape[-1] == 128 and out["keypoints"].shape[1] >= 5


def test_fp32_stock_stays_within_two_percent_of_fp64_on_the_e2e_images():
    """The share that test_gpu_sift.py's 5 % bound of fused against stock rests on."""
    imgs, sizes = sc.e2e_batch()
    conf = {"max_num_keypoints": None, "nms_radius": None}
    for b in range(3):
        a = SIFT(conf)({"image": imgs[b:b + 1]})
        c = SIFT(conf)({"image": imgs[b:b + 1].float()})
        ka, kc = a["keypoints"][0], c["keypoints"][0].double()
        d = torch.cdist(ka, kc)
        d = d + 1e3 * ((a["scales"][0][:, None] / c["scales"][0][None].double()).log2().abs() > 0.01)
        lost = (d.min(1).values > 0.01).sum().item() + (d.min(0).values > 0.01).sum().item()
        assert lost <= 0.02 * (len(ka) + len(kc)), (b, lost, len(ka), len(kc))


def test_integer_shift_fp64():
    """sift_cases.SHIFT_RECOVERED_FP64: every keypoint farther than the largest descriptor radius from the border is found
    again at the shifted position, with an equal descriptor."""
    pair, _ = sc.shift_pair()
    conf = {"max_num_keypoints": None, "nms_radius": None}
    a, b = (SIFT(conf)({"image": torch.from_numpy(p)[None, None]}) for p in pair)
    rec, n = sc.shift_recovered(a, b, pair[0].shape, 1e-9, 1e-9)
    assert n >= 10 and rec / n == sc.SHIFT_RECOVERED_FP64


# ------------------------------------------------------------------------------------------------ post-processing
def _ours(pts, scales, angles, scores, shape, radius):
    keep = S.filter_dog_point(torch.from_numpy(pts), torch.from_numpy(scales), torch.from_numpy(angles), shape, radius,
                              torch.from_numpy(scores))
    return keep.numpy()


def test_post_processing_equals_the_reference_bit_for_bit():
    z = np.load(os.path.join(GOLDEN, "sift_post.npz"))
    live = sc.reference_functions()
    for i, (pts, scales, angles, scores, shape) in enumerate(sc.post_lists()):
        for radius in (0, 3):
            ours = _ours(pts, scales, angles, scores, shape, radius)
            assert np.array_equal(ours, z[f"keep_{i}_r{radius}"]), (i, radius)
            assert 0 < len(ours) < len(pts)
            if live is not None:
                assert np.array_equal(np.sort(live[0](pts, scales, angles, shape, radius, scores)), ours)
    x = torch.from_numpy(z["rootsift_in"])
    assert torch.equal(S.sift_to_rootsift(x), torch.from_numpy(z["rootsift_out"]))
    if live is not None:
        assert torch.equal(live[1](x.clone()), torch.from_numpy(z["rootsift_out"]))
    # lists hold what they claim: a pixel shared by entries of equal score and opposite angle keeps both
    pts, scales, angles, scores, shape = sc.post_lists()[0]
    kept = set(_ours(pts, scales, angles, scores, shape, 0).tolist())
    pix = np.round(pts - 0.5).astype(int)
    twins = [(i, j) for i in kept for j in kept if i < j and (pix[i] == pix[j]).all() and scores[i] == scores[j] and angles[i] == -angles[j]]
    assert twins
