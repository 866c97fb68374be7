"""Wireframe extractor: a point extractor's output plus line segments -> what GlueStick consumes.

Behavioural mirror of gluefactory/models/lines/wireframe.py:22-128 (lines_to_wireframe) and :131-312 (WireframeExtractor):
``keypoints = [junctions; keypoints]``, ``keypoint_scores``, ``descriptors``, ``lines`` (end points moved onto their
junctions), ``lines_junc_idx``, ``line_scores``, ``pl_associativity``, ``num_junctions``, ``orig_lines``; ``valid_lines`` and
whatever else the two sub-extractors return pass through, ``dense_descriptors`` is removed.

On HIP tensors the work is five kernel launches for the whole batch (csrc/wireframe.hip: gf_wf_cluster, gf_wf_suppress,
gf_wf_descriptors, gf_wf_associativity), where the reference loops over the batch in Python, clusters on the host with
sklearn, reads a count back and re-samples descriptors image by image.  With ``force_num_keypoints`` and ``force_num_lines``
there is no host synchronisation and no data-dependent shape, so the stage runs inside a captured step: both random fills
are drawn for every row with fixed shapes ([B,2L,2] and ``rand_like(keypoints)``) and the kernels select between the fill
and the real value.  Without them (batch of one, as in the reference) rows are dropped with torch indexing around the same
kernels, at the price of one host read.

``fused``: None = the kernels on HIP tensors and the torch form below on CPU tensors; False = the torch form; True = the
kernels, and an error on CPU tensors (there is no CPU fallback).  The torch form restates the reference without sklearn:
DBSCAN(eps, min_samples=1) makes every point a core point, so its clusters are the connected components of the graph
``dx^2 + dy^2 <= eps^2`` (fp64 on the fp32 coordinates, inclusive) numbered by their lowest end-point index; it finds them
by label propagation on the fp64 adjacency.

Two deviations from the reference, both deliberate:
  * the random fill VALUES do not follow the reference's generator stream (it draws one of the two fills on the CPU and its
    draw counts are data dependent); their distribution, uniform on [0, w-1] x [0, h-1], is the same;
  * ``num_junctions`` is an int64 tensor [B] on the inputs' device (the reference returns a CPU tensor built from a Python
    list), so that every output is a batched tensor and a two-view pipeline can split a concatenated call.
"""
import torch

from .. import lib as _lib
from ..base_model import BaseModel, get_model
from ..conf import to_container


def sample_descriptors_corner_conv(keypoints, descriptors, s: int = 8):
    """wireframe.py:8-19: bilinear sample at pixel x / s - 0.5 (zero padding), L2-normalised; [B,C,n]."""
    b, c, h, w = descriptors.shape
    keypoints = keypoints / (keypoints.new_tensor([w, h]) * s)
    keypoints = keypoints * 2 - 1
    descriptors = torch.nn.functional.grid_sample(descriptors, keypoints.view(b, 1, -1, 2), mode="bilinear", align_corners=False)
    return torch.nn.functional.normalize(descriptors.reshape(b, c, -1), p=2, dim=1)


def cluster_endpoints(ends, eps):
    """ends [n,2] fp32 -> labels [n] int64 = DBSCAN(eps, min_samples=1).labels_: connected components of the graph with an
    edge where fp64 dx*dx + dy*dy <= eps*eps, ids in the order of each component's lowest index."""
    n = ends.shape[0]
    p = ends.double()
    d = p[:, None] - p[None]
    adj = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] <= float(eps) * float(eps)
    lab = torch.arange(n, device=ends.device)
    big = torch.full((), n, device=ends.device, dtype=lab.dtype)
    for _ in range(n):                                           # labels only decrease: at most n sweeps
        new = torch.where(adj, lab[None], big).min(1).values
        new = torch.minimum(new, lab)                            # (a NaN point is not adjacent to itself)
        new = new[new]
        if torch.equal(new, lab):
            break
        lab = new
    roots = lab == torch.arange(n, device=ends.device)
    return (torch.cumsum(roots, 0) - 1)[lab]


def _stage_torch(lines, line_scores, kpts, kscores, kdesc, dense, s, eps, radius, merge, fill_j, fill_k):
    """The torch form of the four kernels, with their output layout (see _stage_fused)."""
    b, nl = lines.shape[:2]
    n, nk = 2 * nl, kpts.shape[1]
    p = n + nk
    dev = lines.device
    ends = lines.reshape(b, n, 2)
    if radius > 0 and n > 0 and nk > 0:
        flag = (torch.norm(kpts[:, :, None] - ends[:, None], dim=-1) < radius).any(2)
    else:
        flag = torch.zeros(b, nk, dtype=torch.bool, device=dev)
    points = torch.empty(b, p, 2, device=dev)
    scores = torch.empty(b, p, device=dev)
    points[:, n:] = torch.where(flag[..., None], fill_k, kpts)
    scores[:, n:] = torch.where(flag, torch.zeros_like(kscores), kscores)
    idx = torch.empty(b, nl, 2, dtype=torch.long, device=dev)
    nc = torch.empty(b, dtype=torch.long, device=dev)
    new_lines = torch.empty_like(lines)
    for i in range(b):
        lab = cluster_endpoints(ends[i], eps) if merge else torch.arange(n, device=dev)
        c = int(lab.max()) + 1 if n else 0
        junc = torch.zeros(c, 2, device=dev).scatter_reduce_(0, lab[:, None].repeat(1, 2), ends[i], reduce="mean", include_self=False)
        js = torch.zeros(c, device=dev).scatter_reduce_(0, lab, torch.repeat_interleave(line_scores[i], 2), reduce="mean",
                                                       include_self=False)
        points[i, :c], points[i, c:n] = junc, fill_j[i, c:]
        scores[i, :c], scores[i, c:n] = js, 0
        new_lines[i] = junc[lab].reshape(-1, 2, 2)
        idx[i] = lab.reshape(-1, 2)
        nc[i] = c
    ch = dense.shape[1]
    sampled = sample_descriptors_corner_conv(points, dense.float(), s).mT
    take = torch.cat([torch.ones(b, n, dtype=torch.bool, device=dev), flag], 1)
    descs = torch.where(take[..., None], sampled, torch.cat([kdesc.new_zeros(b, n, ch), kdesc], 1))
    return points, scores, descs, flag, idx, nc, new_lines


def associativity_torch(idx, p):
    """pl_associativity [B,P,P]: identity plus both orientations of every line's junction pair (:100-104, :256-262)."""
    b = idx.shape[0]
    out = torch.eye(p, dtype=torch.bool, device=idx.device)[None].repeat(b, 1, 1)
    bi = torch.arange(b, device=idx.device)[:, None].expand(b, idx.shape[1])
    out[bi, idx[..., 0], idx[..., 1]] = True
    out[bi, idx[..., 1], idx[..., 0]] = True
    return out


def associativity_fused(idx, p):
    b, nl = idx.shape[:2]
    assert idx.is_cuda and idx.dtype == torch.long and idx.is_contiguous()
    out = torch.empty(b, p, p, dtype=torch.bool, device=idx.device)
    _lib.check(_lib.load().gf_wf_associativity(idx.data_ptr(), out.data_ptr(), b, nl, p,
                                               torch.cuda.current_stream().cuda_stream), "gf_wf_associativity")
    return out


def _map_nhwc(dense):
    """The dense map as a contiguous [B,h,w,C] fp32 / bf16 tensor (a view of a channels-last map)."""
    if dense.dtype not in (torch.float32, torch.bfloat16):
        dense = dense.float()
    return dense.permute(0, 2, 3, 1).contiguous()


def _stage_fused(lines, line_scores, kpts, kscores, kdesc, dense, s, eps, radius, merge, fill_j, fill_k):
    """Junction block, suppressed keypoints and the concatenated descriptors through the kernels.  Returns points [B,P,2],
    scores [B,P], descs [B,P,C] with P = 2L + N, flag [B,N] (suppressed keypoints), lines_junc_idx [B,L,2],
    num_junctions [B], merged lines [B,L,2,2]."""
    b, nl = lines.shape[:2]
    n, nk = 2 * nl, kpts.shape[1]
    p = n + nk
    dev = lines.device
    f32 = lambda t: t.float().contiguous()
    lines, line_scores, kpts, kscores, kdesc, fill_j, fill_k = (f32(t) for t in (lines, line_scores, kpts, kscores, kdesc, fill_j, fill_k))
    assert all(t.is_cuda for t in (lines, line_scores, kpts, kscores, kdesc, dense, fill_j, fill_k))
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    points = torch.empty(b, p, 2, device=dev)
    scores = torch.empty(b, p, device=dev)
    flag = torch.empty(b, nk, dtype=torch.bool, device=dev)
    idx = torch.empty(b, nl, 2, dtype=torch.long, device=dev)
    nc = torch.zeros(b, dtype=torch.long, device=dev)
    new_lines = torch.empty_like(lines)
    if nl > 0:
        if nl > 2048:
            raise RuntimeError(f"gf_wf_cluster: {nl} lines per image, at most 2048 are supported")
        _lib.check(L.gf_wf_cluster(lines.data_ptr(), line_scores.data_ptr(), fill_j.data_ptr(), idx.data_ptr(), nc.data_ptr(),
                                   new_lines.data_ptr(), points.data_ptr(), scores.data_ptr(), b, nl, p, float(eps),
                                   int(bool(merge)), st), "gf_wf_cluster")
    if nk > 0:
        _lib.check(L.gf_wf_suppress(kpts.data_ptr(), kscores.data_ptr(), lines.data_ptr(), fill_k.data_ptr(), flag.data_ptr(),
                                    points.data_ptr(), scores.data_ptr(), b, nk, n, p, n, float(radius), st), "gf_wf_suppress")
    cmap = _map_nhwc(dense)
    _, h, w, ch = cmap.shape
    descs = torch.empty(b, p, ch, device=dev)
    if p > 0:
        _lib.check(L.gf_wf_descriptors(cmap.data_ptr(), points.data_ptr(), kdesc.data_ptr(), flag.data_ptr(), descs.data_ptr(),
                                       b, p, n, h, w, ch, int(s), 1 if cmap.dtype == torch.bfloat16 else 0, st),
                   "gf_wf_descriptors")
    return points, scores, descs, flag, idx, nc, new_lines


class WireframeExtractor(BaseModel):
    default_conf = {
        "point_extractor": {
            "name": None,
            "trainable": False,
            "dense_outputs": True,
            "max_num_keypoints": None,
            "force_num_keypoints": False,
        },
        "line_extractor": {
            "name": None,
            "trainable": False,
            "max_num_lines": None,
            "force_num_lines": False,
            "min_length": 15,
        },
        "wireframe_params": {
            "merge_points": True,
            "merge_line_endpoints": True,
            "nms_radius": 3,
        },
        "fused": None,      # None: HIP kernels on HIP tensors, torch form on CPU tensors; False: torch form; True: kernels only
    }
    required_data_keys = ["image"]

    def _init(self, conf):
        self.point_extractor = get_model(conf.point_extractor.name)(to_container(conf.point_extractor))
        self.line_extractor = get_model(conf.line_extractor.name)(to_container(conf.line_extractor))
        # a frozen instance may see both views of a pair in one call when both parts can
        self.batchable_views = bool(getattr(self.point_extractor, "batchable_views", False)
                                    and getattr(self.line_extractor, "batchable_views", False))

    def _forward(self, data):
        pred = self.line_extractor(data)
        if pred["line_scores"].shape[-1] != 0:
            pred["line_scores"] = pred["line_scores"] / (pred["line_scores"].max(dim=1)[0][:, None] + 1e-8)
        pred = {**pred, **self.point_extractor(data)}
        assert "dense_descriptors" in pred, "The KP extractor should return dense descriptors"
        out = wireframe_from_parts(pred, data["image"].shape, self.conf.wireframe_params,
                                   bool(self.conf.point_extractor.force_num_keypoints),
                                   bool(self.conf.line_extractor.force_num_lines), self.conf.fused)
        del pred["dense_descriptors"]
        return {**pred, **out}

    def loss(self, pred, data):
        raise NotImplementedError

    def metrics(self, _pred, _data):
        return {}


@torch.no_grad()
def wireframe_from_parts(pred, image_shape, params, force_kpts, force_lines, fused=None, fills=None):
    """wireframe.py:163-306 after the two sub-extractors: ``pred`` holds lines / line_scores (normalised) / keypoints /
    keypoint_scores / descriptors / dense_descriptors.  ``fills`` = (junction fill [B,2L,2], keypoint fill [B,N,2]) replaces the
    random draws (tests)."""
    lines, line_scores = pred["lines"], pred["line_scores"]
    kpts, kscores, kdesc, dense = pred["keypoints"], pred["keypoint_scores"], pred["descriptors"], pred["dense_descriptors"]
    b_size, _, h, w = image_shape
    if fused and not lines.is_cuda:
        raise RuntimeError("wireframe: fused=True needs tensors on a HIP device (the gf_wf_* kernels have no CPU fallback)")
    if fused is None:
        fused = lines.is_cuda
    if not force_kpts or not force_lines:
        assert b_size == 1, "Only batch size of 1 accepted for non padded inputs"
    s_desc = h // dense.shape[2]
    nl, nk = lines.shape[1], kpts.shape[1]
    n = 2 * nl
    merge = bool(params.merge_line_endpoints) and nl > 0
    radius = float(params.nms_radius) if params.merge_points else -1.0
    if fills is None:
        fill_j = torch.rand(b_size, n, 2, device=lines.device)
        fill_k = torch.rand_like(kpts, dtype=torch.float32)
        for f in (fill_j, fill_k):                               # (in place, column by column: no host tensor in a captured step)
            f[..., 0].mul_(w - 1)
            f[..., 1].mul_(h - 1)
    else:
        fill_j, fill_k = fills
    stage = _stage_fused if fused else _stage_torch
    points, scores, descs, flag, idx, nc, new_lines = stage(
        lines.float(), line_scores.float(), kpts.float(), kscores.float(), kdesc.float(), dense, s_desc, params.nms_radius,
        radius, merge, fill_j, fill_k)
    p = n + nk
    if not (force_kpts and force_lines):
        # drop what the padded form fills: junction rows behind the true ones, suppressed keypoints (one host read)
        keep_j = torch.arange(n, device=lines.device) < nc[0] if not force_lines else torch.ones(n, dtype=torch.bool, device=lines.device)
        keep_k = ~flag[0] if not force_kpts else torch.ones(nk, dtype=torch.bool, device=lines.device)
        rows = torch.cat([keep_j, keep_k]).nonzero()[:, 0]
        points, scores, descs = points[:, rows], scores[:, rows], descs[:, rows]
        p = rows.shape[0]
    if not merge:                                                # independent lines: the reference leaves the identity (:287-289)
        assoc = torch.eye(p, dtype=torch.bool, device=lines.device)[None].repeat(b_size, 1, 1)
    else:
        assoc = (associativity_fused if fused else associativity_torch)(idx, p)
    return {"keypoints": points, "keypoint_scores": scores, "descriptors": descs, "pl_associativity": assoc,
            "num_junctions": nc, "orig_lines": lines, "lines": new_lines, "lines_junc_idx": idx}


__main_model__ = WireframeExtractor
