"""Junction clustering against the REFERENCE ITSELF over a sweep of seeded scenes (build container only: skipped where
/root/reference is absent).  tests/test_wireframe_host.py pins three scenes to committed vectors; here the reference's
``lines_to_wireframe`` (sklearn DBSCAN on the host + scatter_reduce_) runs side by side with the torch form of this package
on fresh scenes -- several seeds, eps in {3, 4, 5}, random and integer-lattice end points (many distances exactly eps) --
and labels, counts, junctions, junction scores, merged lines and connectivity must be equal on every scene.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

import wireframe_cases as wc

REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "gluefactory")),
                                reason="reference checkout not present (GPU box)")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref_lines_to_wireframe():
    stubs = os.path.join(ROOT, "oracle", "stubs")
    added = [p for p in (stubs, REF) if p not in sys.path]
    sys.path[:0] = [stubs]
    sys.path.append(REF)
    from gluefactory.models.lines.wireframe import lines_to_wireframe
    yield lines_to_wireframe
    for p in added:
        if p in sys.path:
            sys.path.remove(p)


@pytest.mark.parametrize("lattice", [False, True])
@pytest.mark.parametrize("eps", [3, 4, 5])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_clusters_and_junctions_equal_the_reference(ref_lines_to_wireframe, seed, eps, lattice):
    from glue_factory_amd.lines.wireframe import _stage_torch, associativity_torch
    n_lines, n_kpts, hw, s, ch = (40, 8, (96, 128), 8, 64) if seed % 2 else (97, 8, (128, 160), 8, 64)
    sc = wc.make_scene(seed=100 + seed, batch=2, n_lines=n_lines, n_kpts=n_kpts, hw=hw, eps=eps, n_pad=7 * (seed % 3),
                       lattice=lattice)
    assert wc.band_violations(sc["lines"], None, eps, eps) == 0
    g = torch.Generator().manual_seed(seed)
    lines, scores = torch.from_numpy(sc["lines"]), torch.from_numpy(sc["line_scores"])
    dense = torch.randn(2, ch, hw[0] // s, hw[1] // s, generator=g)
    junc, jscores, jdesc, conn, new_lines, idx, ntrue = ref_lines_to_wireframe(
        lines.clone(), scores.clone(), dense, s, eps, True, n_lines)
    kp = torch.from_numpy(sc["keypoints"])
    fill = torch.rand(2, 2 * n_lines, 2, generator=g) * 50
    points, pscores, descs, flag, our_idx, nc, our_lines = _stage_torch(
        lines, scores, kp, torch.ones(2, n_kpts), torch.zeros(2, n_kpts, ch), dense, s, eps, -1.0, True, fill, kp)
    assert nc.tolist() == list(ntrue)
    np.testing.assert_array_equal(our_idx.numpy(), idx.numpy())
    np.testing.assert_array_equal(our_lines.numpy(), new_lines.numpy())
    assoc = associativity_torch(our_idx, 2 * n_lines)
    for b in range(2):
        c = ntrue[b]
        assert c < 2 * n_lines                                              # something merged
        np.testing.assert_array_equal(points[b, :c].numpy(), junc[b, :c].numpy())
        np.testing.assert_array_equal(pscores[b, :c].numpy(), jscores[b][:c].numpy())
        np.testing.assert_array_equal(points[b, c:2 * n_lines].numpy(), fill[b, c:].numpy())
        np.testing.assert_allclose(descs[b, :c].numpy(), jdesc[b, :c].numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_array_equal(assoc[b].numpy(), conn[b].numpy())
    assert not flag.any()
