"""Writes tests/golden/nn_matcher.npz from the UNMODIFIED reference nearest_neighbor_matcher (build machine only).

The reference module is imported the way oracle/gen_golden.py imports its models: the omegaconf / kornia stand-ins of
oracle/stubs first on the path, the reference checkout appended.  CPU fp32.  Cases (tests/nn_matcher_cases.py): B=2,
M=150, N=201, D=64, L2-normalised descriptors where about half of descriptors1 are noisy copies of rows of descriptors0;
(a) default configuration, (b) ratio 0.8 + distance 0.9 + mutual check, (c) the same without the mutual check,
(d) loss N_pair at temperature 1.7 with a seeded gt_assignment: loss entries and the gradients of total.sum() with respect
to the temperature and both descriptor tensors.  `similarity` and `log_assignment` do not depend on the configuration and
are stored once.  The generator asserts that the rows whose decisions sit within the fp32 tolerance of a boundary stay
under the cap the tests use.

    python tools/gen_golden_nn_matcher.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "stubs"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.append("/root/reference")

import nn_matcher_cases as cases  # noqa: E402

B, M, N, D = 2, 150, 201, 64
SEED = 0


def make_inputs(seed=SEED):
    g = torch.Generator().manual_seed(seed)
    d0 = torch.nn.functional.normalize(torch.randn(B, M, D, generator=g), dim=-1)
    d1 = torch.nn.functional.normalize(torch.randn(B, N, D, generator=g), dim=-1)
    gt = torch.zeros(B, M, N, dtype=torch.bool)
    k = N // 2
    for b in range(B):
        src = torch.randperm(M, generator=g)[:k]                   # distinct rows of descriptors0 ...
        dst = torch.randperm(N, generator=g)[:k]                   # ... copied to distinct rows of descriptors1
        sigma = 0.02 + 0.18 * torch.rand(k, 1, generator=g)       # per-copy noise: some pass the thresholds, some do not
        d1[b, dst] = torch.nn.functional.normalize(d0[b, src] + sigma * torch.randn(k, D, generator=g), dim=-1)
        gt[b, src, dst] = True
    return d0, d1, gt


def main():
    from gluefactory.models.matchers.nearest_neighbor_matcher import NearestNeighborMatcher
    d0, d1, gt = make_inputs()
    out = {"descriptors0": d0.numpy(), "descriptors1": d1.numpy(), "gt_assignment": gt.numpy()}
    shared = None
    for name, conf in cases.CASES.items():
        model = NearestNeighborMatcher(dict(conf))
        a = d0.clone().requires_grad_(name == "d")
        b = d1.clone().requires_grad_(name == "d")
        pred = model({"descriptors0": a, "descriptors1": b})
        dense = (pred["similarity"].detach().numpy(), pred["log_assignment"].detach().numpy())
        if shared is None:
            shared = dense
            out["similarity"], out["log_assignment"] = dense
        assert all(np.array_equal(x, y) for x, y in zip(shared, dense))
        for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
            out[f"{name}.{k}"] = pred[k].numpy()
        s0, s1 = cases.safe_rows(shared[0], **conf)
        share = cases.excluded_share(s0, s1)
        assert share <= cases.MAX_EXCLUDED, (name, share)
        print(f"case {name}: matched {int((pred['matches0'] > -1).sum())} rows, excluded share {share:.4f}")
        if name == "d":
            with torch.no_grad():
                model.temperature.fill_(cases.TEMPERATURE_D)
            pred = model({"descriptors0": a, "descriptors1": b})
            losses, _ = model.loss(pred, {"gt_assignment": gt})
            losses["total"].sum().backward()
            for k, v in losses.items():
                out[f"d.loss.{k}"] = v.detach().numpy()
            out["d.grad.temperature"] = model.temperature.grad.numpy()
            out["d.grad.descriptors0"] = a.grad.numpy()
            out["d.grad.descriptors1"] = b.grad.numpy()
    path = os.path.join(ROOT, "tests", "golden", "nn_matcher.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
