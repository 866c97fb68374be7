"""matcher_metrics (gluefactory/models/utils/metrics.py) side by side with the reference over random predictions -- matched,
unmatched (-1) and ignored (-2) ground truth, empty rows, tied scores, the `line_` prefixes GlueStick uses.  The reference's
outputs for every case are stored in tests/golden/metrics_sweep.npz (oracle/gen_golden.py metrics_sweep); where the reference
checkout is present, the test also calls it live and checks the stored vectors against it."""
import os
import sys

import numpy as np
import pytest
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics_sweep.npz")

SHAPES = [(1, 3, 40, 50), (2, 1, 7, 3), (3, 4, 128, 128), (4, 2, 1, 1)]
PREFIXES = [("", None), ("line_", None), ("line_0_", "line_")]
CASES = [s + p for p in PREFIXES for s in SHAPES]


def case_key(seed, batch, m, n, prefix, prefix_gt):
    return f"s{seed}_b{batch}_m{m}_n{n}_p{prefix}_g{prefix_gt}"


def case_inputs(seed, batch, m, n, prefix, prefix_gt):
    """(pred, data) of one case: seeded matches / scores / ground truth."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(-2, n, (batch, m), generator=g)
    pred_m = torch.where(torch.rand(batch, m, generator=g) < 0.6, gt, torch.randint(-1, n, (batch, m), generator=g))
    scores = torch.rand(batch, m, generator=g)
    scores = torch.where(torch.rand(batch, m, generator=g) < 0.2, torch.full_like(scores, 0.5), scores)      # ties
    scores = torch.where(pred_m > -1, scores, torch.zeros_like(scores))
    if batch > 1:
        gt[0] = -2                     # a pair without any usable ground truth
        pred_m[-1] = -1                # a pair without any prediction
    pred = {f"{prefix}matches0": pred_m, f"{prefix}matching_scores0": scores}
    data = {f"gt_{prefix if prefix_gt is None else prefix_gt}matches0": gt}
    return pred, data


@pytest.fixture(scope="module")
def ref_fn():
    """The reference's matcher_metrics where the checkout is present, else None."""
    if not os.path.isdir(os.path.join(REF, "gluefactory")):
        yield None
        return
    stubs = os.path.join(ROOT, "oracle", "stubs")
    added = [p for p in (stubs, REF) if p not in sys.path]
    sys.path[:0] = [stubs]
    sys.path.append(REF)
    from gluefactory.models.utils.metrics import matcher_metrics
    yield matcher_metrics
    for p in added:
        if p in sys.path:
            sys.path.remove(p)


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("seed,batch,m,n", SHAPES)
@pytest.mark.parametrize("prefix,prefix_gt", PREFIXES)
def test_matcher_metrics_equal_the_reference(ref_fn, golden, seed, batch, m, n, prefix, prefix_gt):
    from glue_factory_amd.metrics import matcher_metrics
    pred, data = case_inputs(seed, batch, m, n, prefix, prefix_gt)
    head = case_key(seed, batch, m, n, prefix, prefix_gt) + "."
    ref = {k[len(head):]: torch.from_numpy(v) for k, v in golden.items() if k.startswith(head)}
    assert ref, f"no stored reference outputs for {head[:-1]}"
    if ref_fn is not None:             # the stored vectors are the reference's own outputs
        live = ref_fn(pred, data, prefix=prefix, prefix_gt=prefix_gt)
        assert set(live) == set(ref)
        for k in live:
            torch.testing.assert_close(ref[k], live[k], rtol=0, atol=0, msg=lambda s: f"stored {k}: {s}")
    out = matcher_metrics(pred, data, prefix=prefix, prefix_gt=prefix_gt)
    assert set(out) == set(ref)
    for k in ref:
        torch.testing.assert_close(out[k], ref[k], rtol=1e-6, atol=1e-7, msg=lambda s: f"{k}: {s}")
