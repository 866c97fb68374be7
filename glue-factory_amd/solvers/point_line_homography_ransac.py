"""Batched point-and-line homography RANSAC on the GPU (csrc/hl_solver.hip: gf_hl_ransac) behind the plugin surface.

It fills the place of the reference's hybrid estimator, gluefactory/robust_estimators/homography/homography_est.py
(``estimator: homography_est`` of configs/superpoint+lsd+gluestick.yaml, the "Hest" column of its README), which evaluates
GlueStick's line matches together with its point matches.  That estimator is a CPU package this project cannot install, so
nothing was compared against it: the semantics are this solver's own, stated in the header comments of csrc/hl_solver.hip
and csrc/hl_fit.h (hypotheses from four features, each a point match or a line match; a line match constrains the two
view-0 endpoints to fall on the view-1 line, wherever along it).

``PointLineHomographyRansac`` fills the `solver` slot of TwoViewPipeline:
``solver: {name: glue_factory_amd.solvers.point_line_homography_ransac}``.  ``PointLineHomographyEstimator`` has the shape of
the reference's robust estimators: one pair, dict in / dict out, so code written like eval_homography_robust
(gluefactory/eval/utils.py:197-238) calls it unchanged.

All ``max_iters`` hypotheses are always evaluated (no early exit); the result is a pure function of the inputs and ``seed``."""
import torch

from .. import lib as _lib
from ..base_model import BaseModel
from ..conf import Conf


def _empty(like, *shape, dtype):
    return torch.empty(shape, dtype=dtype, device=like.device)


@torch.no_grad()
def point_line_homography_ransac(kpts0, kpts1, matches0, lines0, lines1, line_matches0, ransac_th=2.0, max_iters=3000,
                                 lo_iters=2, seed=0, debug=False):
    """kpts0 [B,M,2], kpts1 [B,N,2], matches0 [B,M]; lines0 [B,L,2,2], lines1 [B,L1,2,2], line_matches0 [B,L] (-1 = no
    match).  Either list may be empty (M == 0 or L == 0) or None.
    -> dict(M_0to1 [B,3,3] fp32, inliers [B,M] bool, line_inliers [B,L] bool, num_inliers [B] int32, num_line_inliers [B]
    int32, success [B] bool); with ``debug`` also samples [B,T,4] int32, hyp_H [B,T,3,3] fp32 and hyp_counts [B,T,2] int32.
    No host read: capturable on one stream."""
    ref = kpts0 if kpts0 is not None else lines0
    if ref is None:
        raise ValueError("point_line_homography_ransac: neither points nor lines were given")
    if not ref.is_cuda:
        raise RuntimeError("point-and-line homography solver: tensors must be on a HIP device (hl_solver.hip has no CPU fallback)")
    with torch.autocast(device_type="cuda", enabled=False):
        b = ref.shape[0]
        if kpts0 is None:
            kpts0, kpts1, matches0 = ref.new_zeros(b, 0, 2), ref.new_zeros(b, 0, 2), ref.new_zeros(b, 0, dtype=torch.long)
        if lines0 is None:
            lines0, lines1 = ref.new_zeros(b, 0, 2, 2), ref.new_zeros(b, 0, 2, 2)
            line_matches0 = ref.new_zeros(b, 0, dtype=torch.long)
        m, n, l, l1 = kpts0.shape[1], kpts1.shape[1], lines0.shape[1], lines1.shape[1]
        assert kpts0.shape == (b, m, 2) and kpts1.shape == (b, n, 2) and matches0.shape == (b, m)
        assert lines0.shape == (b, l, 2, 2) and lines1.shape == (b, l1, 2, 2) and line_matches0.shape == (b, l)
        kp0, kp1, m0 = kpts0.float().contiguous(), kpts1.float().contiguous(), matches0.long().contiguous()
        ln0, ln1, lm0 = lines0.float().contiguous(), lines1.float().contiguous(), line_matches0.long().contiguous()
        t = int(max_iters)
        H = _empty(ref, b, 3, 3, dtype=torch.float32)
        inl = _empty(ref, b, m, dtype=torch.bool)
        linl = _empty(ref, b, l, dtype=torch.bool)
        num = _empty(ref, b, 2, dtype=torch.int32)
        success = _empty(ref, b, dtype=torch.bool)
        # a list that cannot hold a match is passed as empty (the inputs of an empty list are not read)
        mm, ll = (m if n > 0 else 0), (l if l1 > 0 else 0)
        if mm == 0:
            inl.zero_()
        if ll == 0:
            linl.zero_()
        if b == 0 or mm + ll == 0:                       # nothing to launch
            H.copy_(torch.eye(3, device=ref.device))
            num.zero_(), success.zero_()
        else:
            samples = _empty(ref, b, t, 4, dtype=torch.int32) if debug else None
            hyp_h = _empty(ref, b, t, 9, dtype=torch.float32) if debug else None
            counts = _empty(ref, b, t, 2, dtype=torch.int32) if debug else None
            L = _lib.load()
            nbytes = int(L.gf_hl_ws_bytes(b, mm, ll, t))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=ref.device)
            ptr = lambda x, used=True: x.data_ptr() if (x is not None and used) else None
            _lib.check(L.gf_hl_ransac(
                ptr(kp0, mm), ptr(kp1, mm), ptr(m0, mm), ptr(ln0, ll), ptr(ln1, ll), ptr(lm0, ll), b, mm, n, ll, l1, t,
                float(ransac_th), int(lo_iters), int(seed) & 0xFFFFFFFF, ws.data_ptr(), nbytes, H.data_ptr(), ptr(inl, mm),
                ptr(linl, ll), num.data_ptr(), success.data_ptr(), ptr(samples), ptr(hyp_h), ptr(counts),
                torch.cuda.current_stream().cuda_stream), "gf_hl_ransac")
        out = {"M_0to1": H, "inliers": inl, "line_inliers": linl, "num_inliers": num[:, 0], "num_line_inliers": num[:, 1],
               "success": success}
        if debug and b > 0 and mm + ll > 0:
            out.update(samples=samples, hyp_H=hyp_h.view(b, t, 3, 3), hyp_counts=counts)
    return out


def _line_inputs(data):
    """(lines0, lines1, line_matches0) of a prediction, or three Nones without line keys.  The detector's ``orig_lines`` are
    preferred over the junction-snapped ``lines`` where both exist, as gluefactory/eval/utils.py:211-217 does."""
    if "line_matches0" not in data or "lines0" not in data or "lines1" not in data:
        return None, None, None
    if "orig_lines0" in data and "orig_lines1" in data:
        return data["orig_lines0"], data["orig_lines1"], data["line_matches0"]
    return data["lines0"], data["lines1"], data["line_matches0"]


class PointLineHomographyRansac(BaseModel):
    default_conf = {
        "ransac_th": 2.0,       # pixels (homography_est.py:46): transfer error of a point, endpoint-to-line distance of a line
        "max_iters": 3000,      # number of hypotheses; all of them are always evaluated
        "confidence": 0.995,    # accepted for yaml compatibility; unused (no early exit)
        "lo_iters": 2,          # rounds of {refit on the inliers of both kinds, rescore}
        "seed": 0,
    }
    required_data_keys = ["keypoints0", "keypoints1", "matches0"]

    def _init(self, conf):
        pass

    def _forward(self, data):
        c = self.conf
        lines0, lines1, lm0 = _line_inputs(data)                    # points alone when the prediction has no line keys
        return point_line_homography_ransac(data["keypoints0"], data["keypoints1"], data["matches0"], lines0, lines1, lm0,
                                            c.ransac_th, c.max_iters, c.lo_iters, c.seed)

    def loss(self, pred, data):
        raise NotImplementedError


class PointLineHomographyEstimator:
    """One pair, the reference's estimator shape: any of {"m_kpts0": [K,2], "m_kpts1": [K,2]} and {"m_lines0": [Kl,2,2],
    "m_lines1": [Kl,2,2]} -> {"success": bool, "M_0to1": [3,3], "inliers": [K] bool, "line_inliers": [Kl] bool}.
    It fails, returning the identity, with fewer than 4 matched FEATURES (K + Kl < 4).  This deviates from the reference,
    whose test adds the feature counts of both views (homography_est.py:18-25: n = 2 K + 2 Kl).  ``success`` as a Python
    bool is the one host read of this module."""
    default_conf = {"ransac_th": 2.0, "options": {"max_iters": 3000, "confidence": 0.995}, "lo_iters": 2, "seed": 0}
    required_data_keys = []

    def __init__(self, conf=None):
        self.conf = Conf.merge(Conf.create(self.default_conf), Conf.create(conf or {}))

    def __call__(self, data):
        pts0, pts1 = data.get("m_kpts0"), data.get("m_kpts1")
        ln0, ln1 = data.get("m_lines0"), data.get("m_lines1")
        assert (pts0 is None) == (pts1 is None) and (ln0 is None) == (ln1 is None), "a list needs both of its views"
        ref = pts0 if pts0 is not None else ln0
        assert ref is not None, "PointLineHomographyEstimator: none of m_kpts0/1, m_lines0/1 in data"
        k = 0 if pts0 is None else pts0.shape[0]
        kl = 0 if ln0 is None else ln0.shape[0]
        if k + kl < 4:
            return {"success": False, "M_0to1": torch.eye(3, device=ref.device, dtype=ref.dtype),
                    "inliers": torch.zeros(k, dtype=torch.bool, device=ref.device),
                    "line_inliers": torch.zeros(kl, dtype=torch.bool, device=ref.device)}
        c = self.conf
        ar = lambda n: torch.arange(n, device=ref.device)[None]
        out = point_line_homography_ransac(
            None if pts0 is None else pts0[None], None if pts1 is None else pts1[None], None if pts0 is None else ar(k),
            None if ln0 is None else ln0.reshape(1, kl, 2, 2), None if ln1 is None else ln1.reshape(1, kl, 2, 2),
            None if ln0 is None else ar(kl), c.ransac_th, c.options.max_iters, c.lo_iters, c.seed)
        return {"success": bool(out["success"][0].item()), "M_0to1": out["M_0to1"][0].to(ref.dtype),
                "inliers": out["inliers"][0], "line_inliers": out["line_inliers"][0]}


__main_model__ = PointLineHomographyRansac
