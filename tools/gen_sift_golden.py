#!/usr/bin/env python
"""Records tests/golden/sift_post.npz: the outputs of the REFERENCE's filter_dog_point and sift_to_rootsift on the lists of
tests/sift_cases.post_lists(), for machines without the reference checkout.

    python tools/gen_sift_golden.py [reference root]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sift_cases as sc  # noqa: E402


def main():
    fns = sc.reference_functions(*sys.argv[1:2])
    if fns is None:
        raise SystemExit("reference checkout not found")
    filter_dog_point, sift_to_rootsift = fns
    out = {}
    for i, (pts, scales, angles, scores, shape) in enumerate(sc.post_lists()):
        for radius in (0, 3):
            out[f"keep_{i}_r{radius}"] = np.sort(filter_dog_point(pts, scales, angles, shape, radius, scores)).astype(np.int64)
    x = torch.rand((64, 128), generator=torch.Generator().manual_seed(3)) ** 3
    x[0] = 0
    x = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    out["rootsift_in"] = x.numpy()
    out["rootsift_out"] = sift_to_rootsift(x.clone()).numpy()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "sift_post.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
