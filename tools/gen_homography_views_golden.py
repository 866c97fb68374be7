"""Writes tests/golden/homography_views.npz: what the REFERENCE's sample_homography_corners and compute_homography
(gluefactory/geometry/homography.py:40-128) return on the seeded settings of tests/homography_views_cases.py: SAMPLER_SETTINGS.

Runs where the reference checkout is present (python tools/gen_homography_views_golden.py [reference root]).  The file holds
results only; this script calls nothing but the reference's two functions."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle", "stubs")]
sys.path.append(REF)

import homography_views_cases as vc  # noqa: E402
from gluefactory.geometry.homography import compute_homography, sample_homography_corners  # noqa: E402


def main():
    out = os.path.join(ROOT, "tests", "golden", "homography_views.npz")
    res = vc.run_sampler(sample_homography_corners, compute_homography)
    np.savez(out, **res)
    print("wrote", out, len(res), "arrays")


if __name__ == "__main__":
    main()
