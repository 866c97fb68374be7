"""Writes tests/golden/relative_pose_eval.npz: the REFERENCE's relative_pose_error and sym_epipolar_distance
(gluefactory/geometry/epipolar.py:32-56, :139-155) and cal_error_auc (gluefactory/utils/tools.py:137-149) on the seeded
inputs of tests/e_solver_cases.py: eval_inputs().

Runs where the reference checkout is present (python tools/gen_relative_pose_eval_golden.py [reference root]).  The file
holds results only, evaluated by the reference in fp64: ``t_err`` [4], ``r_err`` [4], ``epi`` [4,40] (the non-squared
symmetric epipolar distance to the ground-truth E, which eval_matches_epipolar thresholds), ``epi_prec`` [4,3] at
1e-4 / 5e-4 / 1e-3 and ``auc_a``, ``auc_b`` [3] at 5 / 10 / 20 degrees."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "stubs")]
sys.path.append(REF)

import e_solver_cases as ec  # noqa: E402
from gluefactory.geometry.epipolar import T_to_E, relative_pose_error, sym_epipolar_distance  # noqa: E402
from gluefactory.geometry.wrappers import Pose  # noqa: E402
from gluefactory.utils.tools import cal_error_auc  # noqa: E402


def main():
    if not hasattr(np, "trapz"):
        np.trapz = np.trapezoid
    z = ec.eval_inputs()
    t_err, r_err, epi = [], [], []
    for i in range(4):
        T = Pose.from_Rt(torch.from_numpy(z["R_gt"][i]), torch.from_numpy(z["t_gt"][i]))
        te, re_ = relative_pose_error(T, torch.from_numpy(z["R"][i]), torch.from_numpy(z["t"][i]))
        t_err.append(float(te))
        r_err.append(float(re_))
        epi.append(sym_epipolar_distance(torch.from_numpy(z["p0"][i]).double(), torch.from_numpy(z["p1"][i]).double(),
                                         T_to_E(T), squared=False).numpy())
    epi = np.array(epi)
    prec = np.stack([(epi < th).mean(1) for th in (1e-4, 5e-4, 1e-3)], 1)
    out = os.path.join(ROOT, "tests", "golden", "relative_pose_eval.npz")
    np.savez(out, t_err=np.array(t_err), r_err=np.array(r_err), epi=epi, epi_prec=prec,
             auc_a=np.array(cal_error_auc(z["errors_a"], [5, 10, 20])), auc_b=np.array(cal_error_auc(z["errors_b"], [5, 10, 20])))
    print("wrote", out, t_err, r_err, prec.tolist())


if __name__ == "__main__":
    main()
