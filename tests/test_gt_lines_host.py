"""Fused close-point counts of the line ground truth, host side (no GPU): the C ABI carries gf_line_close_counts (ABI 20),
the torch form stays what the CPU goldens pin, and asking for the kernel on CPU tensors is an error."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def _homography_inputs():
    z = load_golden("gt_lines")
    t = lambda k: torch.from_numpy(z[k])
    h, w = (int(v) for v in z["hw"])
    args = (t("lines0"), t("lines1"), t("valid0"), t("valid1"), (2, 1, h, w), (2, 1, h, w), t("H"))
    return z, args, dict(npts=50, dist_th=5, overlap_th=0.2, min_visibility_th=0.5)


def test_header_declares_and_library_exports_the_entry():
    from glue_factory_amd import lib
    text = open(os.path.join(ROOT, "include", "gf_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+gf_line_close_counts\s*\(", code)
    assert re.search(r"#define\s+GF_AMD_ABI_VERSION\s+20\b", code)
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "gf_line_close_counts")
    assert len(lib.SIGNATURES["gf_line_close_counts"]) == 13
    assert lib.ABI_VERSION == 20 == lib.load().gf_abi_version()


def test_entry_rejects_non_positive_sizes_without_a_launch():
    """-1 before anything is enqueued (no device is touched: the pointers are never read)."""
    from glue_factory_amd import lib
    fn = lib.load().gf_line_close_counts
    for b, a, c, p in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, -3, 1, 1)):
        assert fn(None, None, None, None, None, None, b, a, c, p, 5.0, 0, None) == -1


def test_torch_form_still_equals_the_cpu_golden():
    from glue_factory_amd.gt import gt_line_matches_from_homography
    z, args, kw = _homography_inputs()
    for fused in (False, None):                      # None on CPU tensors is the torch form
        pos, m0, m1 = gt_line_matches_from_homography(*args, **kw, fused=fused)
        np.testing.assert_array_equal(pos.numpy(), z["assignment"])
        np.testing.assert_array_equal(m0.numpy(), z["matches0"])
        np.testing.assert_array_equal(m1.numpy(), z["matches1"])


def test_fused_on_cpu_tensors_raises():
    from glue_factory_amd.gt import _close_point_counts_fused, gt_line_matches_from_homography, gt_line_matches_from_pose_depth
    from test_gt_golden import _line_depth_data
    _, args, kw = _homography_inputs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gt_line_matches_from_homography(*args, **kw, fused=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gt_line_matches_from_pose_depth(*_line_depth_data(load_golden("gt_lines_depth")), fused=True)
    with pytest.raises(AssertionError):
        _close_point_counts_fused(torch.rand(1, 3, 4), torch.rand(1, 2, 5, 2), 5)


def test_empty_view_takes_the_torch_form_on_cpu():
    from glue_factory_amd.gt import gt_line_matches_from_homography
    _, args, kw = _homography_inputs()
    l0, l1, v0, v1 = args[:4]
    pos, m0, m1 = gt_line_matches_from_homography(l0[:, :0], l1, v0[:, :0], v1, *args[4:], **kw)
    assert pos.shape == (2, 0, l1.shape[1]) and pos.dtype == torch.bool and m0.shape == (2, 0)
