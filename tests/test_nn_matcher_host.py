"""Nearest-neighbour matcher, host side (no GPU): plugin registry, configuration surface, the loud CPU error, and the
reference fixture's own consistency (gluefactory/models/matchers/nearest_neighbor_matcher.py)."""
import numpy as np
import pytest
import torch

import nn_matcher_cases as cases
from conftest import load_golden


def test_registry_resolves_every_spelling():
    from glue_factory_amd.base_model import get_model
    NN = get_model("glue_factory_amd.matchers.nearest_neighbor_matcher")
    assert NN.__name__ == "NearestNeighborMatcher"
    assert get_model("matchers.nearest_neighbor_matcher") is NN and get_model("nearest_neighbor_matcher") is NN


def test_default_conf_and_temperature_parameter():
    from glue_factory_amd.matchers.nearest_neighbor_matcher import NearestNeighborMatcher as NN
    conf = NN({}).conf
    assert conf.ratio_thresh is None and conf.distance_thresh is None and conf.mutual_check is True and conf.loss is None
    assert conf.dense_outputs is True
    assert NN.required_data_keys == ["descriptors0", "descriptors1"]
    assert not list(NN({}).parameters())
    m = NN({"loss": "N_pair"})
    assert [n for n, _ in m.named_parameters()] == ["temperature"]
    assert m.temperature.shape == () and m.temperature.item() == 1.0 and m.temperature.requires_grad
    with pytest.raises(ValueError, match="dense_outputs"):
        NN({"loss": "N_pair", "dense_outputs": False})
    with pytest.raises(NotImplementedError):
        NN({}).loss({}, {})


def test_reference_superpoint_nn_blocks_construct():
    """The matcher blocks of the reference's superpoint+NN, superpoint-open+NN (and sift / disk / aliked +NN) configs."""
    from glue_factory_amd.base_model import get_model
    for block in ({"name": "matchers.nearest_neighbor_matcher"},
                  {"name": "matchers.nearest_neighbor_matcher", "ratio_thresh": 0.8, "mutual_check": True}):
        m = get_model(block["name"])(block)
        assert m.conf.name == block["name"] and m.conf.mutual_check is True


def test_cpu_tensors_raise():
    from glue_factory_amd.matchers.nearest_neighbor_matcher import NearestNeighborMatcher as NN
    data = {"descriptors0": torch.rand(1, 8, 64), "descriptors1": torch.rand(1, 9, 64)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NN({})(data)
    from glue_factory_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rows_top2(data["descriptors0"], data["descriptors1"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.n_pair_loss(torch.rand(1, 8, 9), torch.tensor(1.0), (torch.zeros(1, dtype=torch.long),) * 3)


def test_fixture_loads_and_is_consistent():
    z = load_golden("nn_matcher")
    d0, d1, sim = z["descriptors0"], z["descriptors1"], z["similarity"]
    B, M, D = d0.shape
    N = d1.shape[1]
    assert (B, M, N, D) == (2, 150, 201, 64)
    np.testing.assert_allclose(np.linalg.norm(d0, axis=-1), 1.0, atol=1e-6)
    np.testing.assert_allclose(np.linalg.norm(d1, axis=-1), 1.0, atol=1e-6)
    sim64 = np.einsum("bmd,bnd->bmn", d0.astype(np.float64), d1.astype(np.float64))
    np.testing.assert_allclose(sim, sim64, atol=1e-5)
    la = z["log_assignment"]
    assert la.shape == (B, M + 1, N + 1) and not la[:, -1].any() and not la[:, :, -1].any()
    for name, conf in cases.CASES.items():
        m0, m1 = z[f"{name}.matches0"], z[f"{name}.matches1"]
        assert m0.shape == (B, M) and m1.shape == (B, N) and m0.dtype == np.int64
        np.testing.assert_array_equal(z[f"{name}.matching_scores0"], (m0 > -1).astype(np.float32))
        np.testing.assert_array_equal(z[f"{name}.matching_scores1"], (m1 > -1).astype(np.float32))
        cases.check_mutual_invariant(sim, m0, m1, **conf)
        # the float64 restatement agrees with the reference wherever the decisions have a margin; few rows have none
        r0, r1 = cases.ref_matches(sim, **conf)
        s0, s1 = cases.safe_rows(sim, **conf)
        assert cases.excluded_share(s0, s1) <= cases.MAX_EXCLUDED
        np.testing.assert_array_equal(m0[s0], r0[s0])
        np.testing.assert_array_equal(m1[s1], r1[s1])
    assert (z["b.matches0"] > -1).sum() < (z["a.matches0"] > -1).sum()          # the thresholds cut
    assert not np.array_equal(z["b.matches1"], z["c.matches1"]) or not np.array_equal(z["b.matches0"], z["c.matches0"])
    assert z["gt_assignment"].sum() == 2 * (N // 2) and z["d.loss.total"].shape == (B,)
    assert z["d.grad.descriptors0"].shape == d0.shape and z["d.grad.descriptors1"].shape == d1.shape
    assert z["d.grad.temperature"].shape == () and z["d.loss.n_pair_temperature"] == np.float32(cases.TEMPERATURE_D)


def test_kernel_case_seeds_keep_the_float64_reference_within_the_cap():
    """The GPU test of rows_top2 excludes rows whose float64 top-1 / top-2 gap is within the tolerance and caps their share:
    the seeded inputs satisfy that cap by themselves, whatever the kernel does."""
    for shape in cases.TOP2_SHAPES:
        for dim in cases.TOP2_DIMS:
            for bf16 in (False, True):
                a, b, (best, arg, second) = cases.top2_inputs(shape, dim, bf16)
                assert a.shape == (shape[0], shape[1], dim) and b.shape == (shape[0], shape[2], dim)
                assert ((best - second) <= cases.TOL).mean() <= cases.MAX_EXCLUDED
    # bf16-rounded fixture descriptors (the module's bf16 test): the same cap
    z = load_golden("nn_matcher")
    d0, d1 = (torch.from_numpy(z[k]).bfloat16().double().numpy() for k in ("descriptors0", "descriptors1"))
    sim = np.einsum("bmd,bnd->bmn", d0, d1)
    for conf in cases.CASES.values():
        assert cases.excluded_share(*cases.safe_rows(sim, **conf)) <= cases.MAX_EXCLUDED
