"""No-grad matcher metrics on the [B,N] match vectors (eval mode only).

Restates gluefactory/models/utils/metrics.py:4-50 (recall, precision, accuracy and the
ranking average precision of matches0 against gt_matches0); tiny tensors, stock torch ops.

Homography evaluation (gluefactory/geometry/homography.py:314-342, gluefactory/eval/utils.py:137-156, 197-261), batched:
sym_homography_error, homography_corner_error and homography_metrics, the last on top of the GPU solvers of ``solvers/``;
point_line_homography_metrics adds the line inliers of the point-and-line solver.

Relative-pose evaluation (gluefactory/geometry/epipolar.py:127-155, gluefactory/utils/tools.py:137-149,
gluefactory/eval/utils.py:41-70, 159-194), batched: relative_pose_error, pose_auc and relative_pose_metrics."""
import torch


@torch.no_grad()
def matcher_metrics(pred, data, prefix="", prefix_gt=None):
    prefix_gt = prefix if prefix_gt is None else prefix_gt
    m = pred[f"{prefix}matches0"]
    gt = data[f"gt_{prefix_gt}matches0"]
    scores = pred[f"{prefix}matching_scores0"]
    hit = (m == gt)

    def ratio(mask):
        mask = mask.float()
        return (hit * mask).sum(1) / (1e-8 + mask.sum(1))

    has_gt = gt > -1
    labelled = gt >= -1
    predicted = (m > -1) & labelled
    order = torch.argsort(-scores)
    p_mask = predicted.float().gather(-1, order)
    r_mask = has_gt.float().gather(-1, order)
    tp = hit.gather(-1, order)
    p_pts = torch.cumsum(tp * p_mask, -1) / (1e-8 + torch.cumsum(p_mask, -1))
    r_pts = torch.cumsum(tp * r_mask, -1) / (1e-8 + r_mask.sum(-1)[:, None])
    r_diff = r_pts[..., 1:] - r_pts[..., :-1]
    ap = torch.sum(r_diff * p_pts[:, None, -1], dim=-1)
    return {
        f"{prefix}match_recall": ratio(has_gt),
        f"{prefix}match_precision": ratio(predicted),
        f"{prefix}accuracy": ratio(labelled),
        f"{prefix}average_precision": ap,
    }


# ------------------------------------------------------------------------------------------------ homography evaluation
def _batched(*ts):
    """Add the batch axis the 3x3 helpers of gt expect where the caller passes one pair."""
    single = ts[-1].dim() == 2
    return single, [t[None] if single else t for t in ts]


@torch.no_grad()
def sym_homography_error(kpts0, kpts1, T_0to1):
    """gluefactory/geometry/homography.py:314-323: mean of the forward and the backward transfer distance.  kpts [B,N,2] and
    T_0to1 [B,3,3] -> [B,N] (or one pair without the batch axis).  The reference inverts with torch.pinverse; here the
    adjugate of gt.inv3x3 (the same matrix for an invertible homography, and capturable)."""
    from .gt import warp_points
    single, (kpts0, kpts1, T) = _batched(kpts0, kpts1, T_0to1)
    d01 = ((warp_points(kpts0, T, eps=0.0) - kpts1) ** 2).sum(-1).sqrt()
    d10 = ((warp_points(kpts1, T, inverse=True, eps=0.0) - kpts0) ** 2).sum(-1).sqrt()
    err = (d01 + d10) / 2.0
    return err[0] if single else err


@torch.no_grad()
def homography_corner_error(T, T_gt, image_size):
    """gluefactory/geometry/homography.py:336-342: mean distance of the four image corners under T and T_gt.  T, T_gt
    [B,3,3], image_size [B,2] = (W, H) -> [B] (or one pair without the batch axis -> a scalar tensor)."""
    from .gt import warp_points
    single, (T, T_gt) = _batched(T, T_gt)
    size = image_size.to(T).reshape(-1, 2).expand(T.shape[0], 2)
    W, Hh = size[:, 0], size[:, 1]
    zero = torch.zeros_like(W)
    corners = torch.stack([torch.stack([zero, zero], -1), torch.stack([W, zero], -1), torch.stack([W, Hh], -1),
                           torch.stack([zero, Hh], -1)], -2)
    d = ((warp_points(corners, T, eps=0.0) - warp_points(corners, T_gt, eps=0.0)) ** 2).sum(-1).sqrt().mean(-1)
    return d[0] if single else d


@torch.no_grad()
def homography_metrics(pred, data):
    """Batched restatement of gluefactory/eval/utils.py:137-156 (eval_matches_homography), :241-261 (eval_homography_dlt)
    and, when ``pred`` carries a solver's output (``M_0to1``, ``inliers``, ``success``), :197-238 (eval_homography_robust).
    Every value is a [B] tensor.  A pair without matches has precision 0 (the reference's nan_to_num) and infinite errors;
    a pair whose DLT or RANSAC finds no model has an infinite error."""
    from .solvers.dlt import homography_dlt
    kp0, kp1, m0 = pred["keypoints0"], pred["keypoints1"], pred["matches0"]
    H_gt = data["H_0to1"].float()
    size = data["view0"]["image_size"].float()
    valid = m0 > -1
    nm = valid.sum(1)
    pts1 = kp1.float().gather(1, m0.clamp(min=0)[..., None].expand(-1, -1, 2))
    err = sym_homography_error(kp0.float(), pts1, H_gt)
    inf = torch.full_like(size[:, 0], float("inf"))

    def prec(th):
        return ((err < th) & valid).float().sum(1) / nm.clamp(min=1)

    out = {"prec@1px": prec(1), "prec@3px": prec(3), "num_matches": nm}
    H_dlt, ok = homography_dlt(kp0, kp1, m0, pred.get("matching_scores0"))
    out["H_error_dlt"] = torch.where(ok, homography_corner_error(H_dlt, H_gt, size), inf)
    if "M_0to1" in pred and "success" in pred:
        ok_r = pred["success"]
        out["H_error_ransac"] = torch.where(ok_r, homography_corner_error(pred["M_0to1"].float(), H_gt, size), inf)
        if "inliers" in pred:
            ninl = pred["inliers"].float().sum(1)
            out["ransac_inl"] = ninl
            out["ransac_inl%"] = ninl / nm.clamp(min=1)
    return out


@torch.no_grad()
def point_line_homography_metrics(pred, data):
    """homography_metrics for a prediction that carries the point-and-line solver's output (solvers.
    point_line_homography_ransac): the same values, plus ``ransac_line_inl`` (the line inliers of the model) and
    ``ransac_line_inl%`` (their share of the line matches; 0 without line matches), where ``pred`` has ``line_inliers``.
    Every value is a [B] tensor."""
    return {**homography_metrics(pred, data), **line_inlier_metrics(pred)}


@torch.no_grad()
def line_inlier_metrics(pred):
    """The line part of point_line_homography_metrics (plain tensor arithmetic on any device): {} without ``line_inliers``."""
    if "line_inliers" not in pred:
        return {}
    ninl = pred["line_inliers"].float().sum(1)
    if "line_matches0" in pred and pred["line_matches0"].shape == pred["line_inliers"].shape:
        nlm = (pred["line_matches0"] > -1).sum(1)
    else:
        nlm = torch.zeros_like(ninl, dtype=torch.long)
    return {"ransac_line_inl": ninl, "ransac_line_inl%": ninl / nlm.clamp(min=1)}


# ---------------------------------------------------------------------------------------------- relative-pose evaluation
@torch.no_grad()
def relative_pose_error(T_gt, R, t, ignore_gt_t_thr=0.0, eps=1e-10):
    """gluefactory/geometry/epipolar.py:127-155, batched on the device: (t_err, r_err) in degrees, each [B] (or scalars for
    one pair).  T_gt: a Pose (or anything with .R [B,3,3] and .t [B,3]).  The translation angle folds at 90 degrees (the
    sign of t is not observable from E); where |t_gt| < ignore_gt_t_thr it is 0, as in the reference."""
    R_gt, t_gt = T_gt.R.to(R), T_gt.t.to(t)
    n = (t.norm(dim=-1) * t_gt.norm(dim=-1)).clamp(min=eps)
    t_err = torch.rad2deg(torch.arccos(((t * t_gt).sum(-1) / n).clamp(-1.0, 1.0)))
    t_err = torch.minimum(t_err, 180 - t_err)
    t_err = torch.where(t_gt.norm(dim=-1) < ignore_gt_t_thr, torch.zeros_like(t_err), t_err)
    cos = ((R.transpose(-1, -2) @ R_gt).diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2
    r_err = torch.rad2deg(torch.arccos(cos.clamp(-1.0, 1.0)).abs())
    return t_err, r_err


def pose_auc(errors, thresholds):
    """cal_error_auc of gluefactory/utils/tools.py:137-149, rounding to 4 places included: the area under the recall curve
    of ``errors`` (a tensor or a sequence; inf = failure) up to every threshold, divided by the threshold."""
    import numpy as np
    if torch.is_tensor(errors):
        errors = errors.detach().double().cpu().numpy()
    e = np.sort(np.asarray(errors, np.float64).reshape(-1))
    recall = np.r_[0.0, (np.arange(len(e)) + 1) / len(e)]
    e = np.r_[0.0, e]
    aucs = []
    for th in thresholds:
        last = np.searchsorted(e, th)
        r = np.r_[recall[:last], recall[last - 1]]
        x = np.r_[e[:last], th]
        aucs.append(float(np.round(np.sum((x[1:] - x[:-1]) * (r[1:] + r[:-1]) / 2) / th, 4)))
    return aucs


@torch.no_grad()
def relative_pose_metrics(pred, data):
    """Batched restatement of gluefactory/eval/utils.py:41-70 (eval_matches_epipolar) and, when ``pred`` carries a solver's
    output (``M_0to1``, ``inliers``, ``success``), :159-194 (eval_relative_pose_robust).  Every value is a [B] tensor.  A pair
    without matches has precision 0 (the reference's nan_to_num); a pair without a model has an infinite pose error."""
    from .geometry import T_to_E, sym_epipolar_distance
    kp0, kp1, m0 = pred["keypoints0"], pred["keypoints1"], pred["matches0"]
    cam0, cam1, T_gt = data["view0"]["camera"], data["view1"]["camera"], data["T_0to1"]
    valid = m0 > -1
    nm = valid.sum(1)
    pts1 = kp1.float().gather(1, m0.clamp(min=0)[..., None].expand(-1, -1, 2))
    p0 = cam0.image2cam(kp0.float())
    err = sym_epipolar_distance(p0, cam1.image2cam(pts1).to(p0.dtype), T_to_E(T_gt).to(p0.dtype), squared=False)

    def prec(th):
        return ((err < th) & valid).float().sum(1) / nm.clamp(min=1)

    out = {"epi_prec@1e-4": prec(1e-4), "epi_prec@5e-4": prec(5e-4), "epi_prec@1e-3": prec(1e-3), "num_matches": nm}
    if "M_0to1" in pred and "success" in pred:
        M = pred["M_0to1"]
        t_err, r_err = relative_pose_error(T_gt, M.R.float(), M.t.float())
        out["rel_pose_error"] = torch.where(pred["success"], torch.maximum(t_err, r_err), torch.full_like(t_err, float("inf")))
        if "inliers" in pred:
            ninl = pred["inliers"].float().sum(1)
            out["ransac_inl"] = ninl
            out["ransac_inl%"] = ninl / nm.clamp(min=1)
    return out
