"""Batched relative-pose RANSAC on the GPU (csrc/e_solver.hip: gf_e_ransac, gf_e_pose) behind the plugin surface.

``RelativePoseRansac`` fills the `solver` slot of TwoViewPipeline: ``solver: {name: glue_factory_amd.solvers.relative_pose_ransac}``.
``RelativePoseEstimator`` has the shape of the reference's robust estimators
(gluefactory/robust_estimators/relative_pose/opencv.py:10-64): one pair, dict in / dict out, so code written like
eval_relative_pose_robust (gluefactory/eval/utils.py:159-194) calls it unchanged.

The C ABI is camera-agnostic: keypoints are normalised here with the cameras' own ``image2cam`` (any distortion model of the
reference's wrapper passes through) and the pixel threshold becomes ``ransac_th / mean(f0x, f0y, f1x, f1y)`` per pair, on
the device (opencv.py:30-34).  All ``max_iters`` hypotheses are always evaluated: there is no early exit, which is why
``confidence`` is accepted (yaml compatibility) and unused.  The result is a pure function of the inputs and ``seed``."""
import torch

from .. import lib as _lib
from ..base_model import BaseModel
from ..conf import Conf
from ..geometry import Pose
from .dlt import _prep, workspace


def _normalised(kpts, camera):
    return camera.image2cam(kpts.float())[..., :2]


def _threshold(camera0, camera1, ransac_th, b):
    f = torch.cat([camera0.f, camera1.f], -1).float()
    return (float(ransac_th) / f.mean(-1)).reshape(-1).expand(b).contiguous()


@torch.no_grad()
def relative_pose_ransac(kpts0, kpts1, matches0, camera0, camera1, ransac_th=0.5, max_iters=2048, lo_iters=2, seed=0,
                         debug=False):
    """kpts0 [B,M,2], kpts1 [B,N,2] pixels, matches0 [B,M], cameras batched [B] (or one for all pairs) -> dict(M_0to1 Pose
    [B,12] fp32 with |t| = 1, E [B,3,3] fp32 with ||E||_F = 1 in normalised coordinates, inliers [B,M] bool, num_inliers [B]
    int32, success [B] bool); with ``debug`` also samples [B,T,5], cand [B,T,10,3,3], ncand [B,T], cand_counts [B,T,10].
    A pair without a model has R = I, t = 0, E = 0 and no inliers.  No host read: capturable on one stream."""
    with torch.autocast(device_type="cuda", enabled=False):
        kp0, kp1, m0, b, m, n = _prep(kpts0, kpts1, matches0)
        dev = kp0.device
        t = int(max_iters)
        E = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
        Rt = torch.empty((b, 12), dtype=torch.float32, device=dev)
        inl = torch.empty((b, m), dtype=torch.bool, device=dev)
        num = torch.empty((b,), dtype=torch.int32, device=dev)
        success = torch.empty((b,), dtype=torch.bool, device=dev)
        out = {"M_0to1": Pose(Rt), "E": E, "inliers": inl, "num_inliers": num, "success": success}
        if m == 0 or n == 0:
            Rt.copy_(torch.cat([torch.eye(3, device=dev).flatten(), torch.zeros(3, device=dev)]))
            E.zero_(), inl.zero_(), num.zero_(), success.zero_()
            return out
        p0 = _normalised(kp0, camera0).expand(b, m, 2).contiguous()
        p1 = _normalised(kp1, camera1).expand(b, n, 2).contiguous()
        th = _threshold(camera0, camera1, ransac_th, b)
        R = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
        tv = torch.empty((b, 3), dtype=torch.float32, device=dev)
        dbg = {}
        if debug:
            dbg = {"samples": torch.empty((b, t, 5), dtype=torch.int32, device=dev),
                   "cand": torch.empty((b, t, 10, 3, 3), dtype=torch.float32, device=dev),
                   "ncand": torch.empty((b, t), dtype=torch.int32, device=dev),
                   "cand_counts": torch.empty((b, t, 10), dtype=torch.int32, device=dev)}
        ws, nbytes = workspace("gf_e_ws_bytes", b, m, t, dev)
        _lib.check(_lib.load().gf_e_ransac(
            p0.data_ptr(), p1.data_ptr(), m0.data_ptr(), th.data_ptr(), b, m, n, t, int(lo_iters), int(seed) & 0xFFFFFFFF,
            ws.data_ptr(), nbytes, E.data_ptr(), R.data_ptr(), tv.data_ptr(), inl.data_ptr(), num.data_ptr(),
            success.data_ptr(), *[dbg[k].data_ptr() if debug else None for k in ("samples", "cand", "ncand", "cand_counts")],
            torch.cuda.current_stream().cuda_stream), "gf_e_ransac")
        Rt[:, :9] = R.flatten(1)
        Rt[:, 9:] = tv
        out.update(dbg)
    return out


@torch.no_grad()
def recover_pose(pts0n, pts1n, matches0, inliers, E):
    """gf_e_pose alone: normalised points [B,M,2], [B,N,2], matches0 [B,M], inliers [B,M] bool, E [B,3,3] -> (R [B,3,3],
    t [B,3], num_front [B] int32): the decomposition of E with the most flagged correspondences in front of both cameras."""
    with torch.autocast(device_type="cuda", enabled=False):
        p0, p1, m0, b, m, n = _prep(pts0n, pts1n, matches0)
        dev = p0.device
        assert inliers.shape == (b, m) and E.shape == (b, 3, 3) and m > 0 and n > 0
        flags = inliers.to(torch.uint8).contiguous()
        Ec = E.float().contiguous()
        R = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
        t = torch.empty((b, 3), dtype=torch.float32, device=dev)
        nf = torch.empty((b,), dtype=torch.int32, device=dev)
        ws, nbytes = workspace("gf_e_ws_bytes", b, m, 1, dev)
        _lib.check(_lib.load().gf_e_pose(p0.data_ptr(), p1.data_ptr(), m0.data_ptr(), flags.data_ptr(), Ec.data_ptr(), b, m, n,
                                         ws.data_ptr(), nbytes, R.data_ptr(), t.data_ptr(), nf.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "gf_e_pose")
    return R, t, nf


class RelativePoseRansac(BaseModel):
    default_conf = {
        "ransac_th": 0.5,        # pixels; divided by the mean focal length of the pair (opencv.py:12,30-31)
        "max_iters": 2048,       # number of hypotheses; all of them are always evaluated
        "confidence": 0.99999,   # accepted for yaml compatibility; unused (no early exit)
        "lo_iters": 2,           # rounds of {refit on the inliers, rescore}
        "seed": 0,
    }
    required_data_keys = ["keypoints0", "keypoints1", "matches0", "view0", "view1"]

    def _init(self, conf):
        pass

    def _forward(self, data):
        c = self.conf
        return relative_pose_ransac(data["keypoints0"], data["keypoints1"], data["matches0"], data["view0"]["camera"],
                                    data["view1"]["camera"], c.ransac_th, c.max_iters, c.lo_iters, c.seed)

    def loss(self, pred, data):
        raise NotImplementedError


class RelativePoseEstimator:
    """One pair, the reference's estimator shape: {"m_kpts0": [K,2], "m_kpts1": [K,2], "camera0", "camera1"} ->
    {"success": bool, "M_0to1": Pose, "inliers": [K] bool}.  ``success`` as a Python bool is the one host read of this
    module."""
    default_conf = {"ransac_th": 0.5, "options": {"confidence": 0.99999, "method": "ransac"}, "max_iters": 2048,
                    "lo_iters": 2, "seed": 0}
    required_data_keys = ["m_kpts0", "m_kpts1", "camera0", "camera1"]

    def __init__(self, conf=None):
        self.conf = Conf.merge(Conf.create(self.default_conf), Conf.create(conf or {}))
        if self.conf.options.method != "ransac":
            raise ValueError(f"RelativePoseEstimator: method {self.conf.options.method!r} is not implemented (ransac only)")

    def __call__(self, data):
        for key in self.required_data_keys:
            assert key in data, f"Missing key {key} in data"
        pts0, pts1 = data["m_kpts0"], data["m_kpts1"]
        k = pts0.shape[0]
        if k == 0:
            eye = torch.cat([torch.eye(3, device=pts0.device, dtype=pts0.dtype).flatten(), pts0.new_zeros(3)])
            return {"success": False, "M_0to1": Pose(eye), "inliers": torch.zeros(0, dtype=torch.bool, device=pts0.device)}
        c = self.conf
        m0 = torch.arange(k, device=pts0.device)[None]
        out = relative_pose_ransac(pts0[None], pts1[None], m0, data["camera0"], data["camera1"], c.ransac_th, c.max_iters,
                                   c.lo_iters, c.seed)
        return {"success": bool(out["success"][0].item()), "M_0to1": Pose(out["M_0to1"]._data[0].to(pts0.dtype)),
                "inliers": out["inliers"][0]}


__main_model__ = RelativePoseRansac
