"""Batched homography RANSAC on the GPU (csrc/h_solver.hip: gf_h_ransac) behind the plugin surface.

``HomographyRansac`` fills the `solver` slot of TwoViewPipeline (gluefactory/models/two_view_pipeline.py:29,54-55,84-85):
``solver: {name: glue_factory_amd.solvers.homography_ransac}``.  ``HomographyEstimator`` has the shape of the reference's
robust estimators (gluefactory/robust_estimators/base_estimator.py, homography/opencv.py:27-53): one pair, dict in / dict
out, so code written like eval_homography_robust (gluefactory/eval/utils.py:197-238) calls it unchanged.

All ``max_iters`` hypotheses are always evaluated: there is no early exit, which is why ``confidence`` is accepted (yaml
compatibility) and unused.  The result is a pure function of the inputs and ``seed``."""
import torch

from .. import lib as _lib
from ..base_model import BaseModel
from ..conf import Conf
from .dlt import _prep, workspace


@torch.no_grad()
def homography_ransac(kpts0, kpts1, matches0, ransac_th=3.0, max_iters=3000, lo_iters=2, seed=0, debug=False):
    """-> dict(M_0to1 [B,3,3] fp32, inliers [B,M] bool, num_inliers [B] int32, success [B] bool); with ``debug`` also
    samples [B,T,4] int32 and hyp_counts [B,T] int32.  No host read: capturable on one stream."""
    with torch.autocast(device_type="cuda", enabled=False):
        kp0, kp1, m0, b, m, n = _prep(kpts0, kpts1, matches0)
        dev = kp0.device
        t = int(max_iters)
        H = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
        inl = torch.empty((b, m), dtype=torch.bool, device=dev)
        num = torch.empty((b,), dtype=torch.int32, device=dev)
        success = torch.empty((b,), dtype=torch.bool, device=dev)
        out = {"M_0to1": H, "inliers": inl, "num_inliers": num, "success": success}
        if m == 0 or n == 0:
            H.copy_(torch.eye(3, device=dev))
            inl.zero_(), num.zero_(), success.zero_()
            return out
        samples = torch.empty((b, t, 4), dtype=torch.int32, device=dev) if debug else None
        counts = torch.empty((b, t), dtype=torch.int32, device=dev) if debug else None
        ws, nbytes = workspace("gf_h_ws_bytes", b, m, t, dev)
        _lib.check(_lib.load().gf_h_ransac(
            kp0.data_ptr(), kp1.data_ptr(), m0.data_ptr(), b, m, n, t, float(ransac_th), int(lo_iters), int(seed) & 0xFFFFFFFF,
            ws.data_ptr(), nbytes, H.data_ptr(), inl.data_ptr(), num.data_ptr(), success.data_ptr(),
            None if samples is None else samples.data_ptr(), None if counts is None else counts.data_ptr(),
            torch.cuda.current_stream().cuda_stream), "gf_h_ransac")
        if debug:
            out.update(samples=samples, hyp_counts=counts)
    return out


class HomographyRansac(BaseModel):
    default_conf = {
        "ransac_th": 3.0,       # pixels, forward transfer error (opencv.py:9)
        "max_iters": 3000,      # number of hypotheses; all of them are always evaluated
        "confidence": 0.995,    # accepted for yaml compatibility; unused (no early exit)
        "lo_iters": 2,          # rounds of {refit on the inliers, rescore}
        "seed": 0,
    }
    required_data_keys = ["keypoints0", "keypoints1", "matches0"]

    def _init(self, conf):
        pass

    def _forward(self, data):
        c = self.conf
        out = homography_ransac(data["keypoints0"], data["keypoints1"], data["matches0"], c.ransac_th, c.max_iters,
                                c.lo_iters, c.seed)
        return out

    def loss(self, pred, data):
        raise NotImplementedError


class HomographyEstimator:
    """One pair, the reference's estimator shape: {"m_kpts0": [K,2], "m_kpts1": [K,2]} -> {"success": bool, "M_0to1": [3,3],
    "inliers": [K] bool}.  ``success`` as a Python bool is the one host read of this module."""
    default_conf = {"ransac_th": 3.0, "options": {"method": "ransac", "max_iters": 3000, "confidence": 0.995},
                    "lo_iters": 2, "seed": 0}
    required_data_keys = ["m_kpts0", "m_kpts1"]

    def __init__(self, conf=None):
        self.conf = Conf.merge(Conf.create(self.default_conf), Conf.create(conf or {}))
        if self.conf.options.method != "ransac":
            raise ValueError(f"HomographyEstimator: method {self.conf.options.method!r} is not implemented (ransac only)")

    def __call__(self, data):
        for key in self.required_data_keys:
            assert key in data, f"Missing key {key} in data"
        pts0, pts1 = data["m_kpts0"], data["m_kpts1"]
        k = pts0.shape[0]
        if k == 0:
            return {"success": False, "M_0to1": torch.eye(3, device=pts0.device, dtype=pts0.dtype),
                    "inliers": torch.zeros(0, dtype=torch.bool, device=pts0.device)}
        c = self.conf
        m0 = torch.arange(k, device=pts0.device)[None]
        out = homography_ransac(pts0[None], pts1[None], m0, c.ransac_th, c.options.max_iters, c.lo_iters, c.seed)
        return {"success": bool(out["success"][0].item()), "M_0to1": out["M_0to1"][0].to(pts0.dtype),
                "inliers": out["inliers"][0]}


__main_model__ = HomographyRansac
