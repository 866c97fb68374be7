"""Writes tests/golden/homography_eval.npz: the REFERENCE's sym_homography_error and homography_corner_error
(gluefactory/geometry/homography.py:314-323, :336-342) on the seeded inputs of tests/h_solver_cases.py: eval_inputs().

Runs where the reference checkout is present (python tools/gen_homography_eval_golden.py [reference root]).  The file holds
results only: ``sym_error`` [3,50] and ``corner_error`` [3], evaluated by the reference on the fp32 inputs CAST TO fp64: its
fp32 evaluation inverts through torch.pinverse, whose fp32 SVD moves these errors by up to 0.02 px from its own fp64 values
(measured on these inputs), so the fp64 evaluation is the reference's answer that a tolerance can be stated against."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "stubs")]
sys.path.append(REF)

import h_solver_cases as hc  # noqa: E402
from gluefactory.geometry.homography import homography_corner_error, sym_homography_error  # noqa: E402


def main():
    z = {k: torch.from_numpy(v).double() for k, v in hc.eval_inputs().items()}
    sym = torch.stack([sym_homography_error(z["kpts0"][i], z["kpts1"][i], z["H_gt"][i]) for i in range(3)])
    corner = torch.stack([homography_corner_error(z["T"][i], z["H_gt"][i], z["image_size"][i]) for i in range(3)])
    out = os.path.join(ROOT, "tests", "golden", "homography_eval.npz")
    np.savez(out, sym_error=sym.numpy(), corner_error=corner.numpy())
    print("wrote", out, sym.shape, corner.tolist())


if __name__ == "__main__":
    main()
