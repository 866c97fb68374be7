"""Generate golden vectors under tests/golden/ by RUNNING THE REFERENCE ITSELF.

Build-container only: imports the unmodified reference modules from /root/reference
(through the omegaconf/kornia stand-ins in oracle/stubs) on CPU fp32, feeds them seeded
inputs and seeded weights (shared with the oracle through the reference's own
state_dict names) and stores inputs, outputs, losses and gradients as small .npz
fixtures.  /root/reference does not exist on the GPU box; tests only read the .npz.

    python oracle/gen_golden.py            # rewrites tests/golden/*.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "stubs"))
sys.path.append("/root/reference")

from glue_factory_amd.synthetic import make_pairs  # noqa: E402
from oracle import lightglue_oracle as lgo  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def _np(d, prefix=""):
    out = {}
    for k, v in d.items():
        if torch.is_tensor(v):
            out[prefix + k] = v.detach().cpu().numpy()
    return out


def ref_lightglue(n_layers, dim, heads, params, filter_threshold=0.0):
    from gluefactory.models.matchers.lightglue import LightGlue

    model = LightGlue({"n_layers": n_layers, "descriptor_dim": dim, "input_dim": dim,
                       "num_heads": heads, "weights": None, "flash": False,
                       "checkpointed": False, "filter_threshold": filter_threshold})
    missing = model.load_state_dict(params, strict=True)  # asserts the state_dict contract
    assert not missing.missing_keys and not missing.unexpected_keys
    return model


def gen_lightglue(name, batch, n0, n1, n_layers, dim, heads, seed, size, store_params):
    torch.manual_seed(seed)
    params = lgo.init_params(n_layers, dim, heads, seed=seed)
    data = make_pairs(batch, n0, n1, dim=dim, size=size, seed=seed + 1)
    model = ref_lightglue(n_layers, dim, heads, params, filter_threshold=0.0)
    out = {}
    # ---- eval forward (plain path: no early stop / pruning)
    model.eval()
    with torch.no_grad():
        pe = model(data)
    out.update(_np({k: pe[k] for k in ("matches0", "matches1", "matching_scores0",
                                       "matching_scores1", "log_assignment")}, "eval."))
    # ---- train step: forward + loss + backward
    model.train()
    pred = model(data)
    losses, _ = model.loss(pred, {**pred, **data})
    losses["total"].mean().backward()
    out.update(_np({k: pred[k] for k in ("matches0", "matches1", "matching_scores0",
                                         "matching_scores1", "log_assignment",
                                         "ref_descriptors0", "ref_descriptors1")}, "train."))
    out.update(_np({k: v for k, v in losses.items() if torch.is_tensor(v)}, "loss."))
    grads = {k: p.grad for k, p in model.named_parameters()}
    if store_params:
        out.update(_np(params, "param."))
        out.update(_np(grads, "grad."))
    else:
        # parameters are regenerated from the seed by the test; keep checksums + small grads
        out["param_checksum"] = np.array([float(sum(v.double().abs().sum() for v in params.values()))])
        for k, g in grads.items():
            out["gradnorm." + k] = np.array([float(g.double().norm())])
            if g.numel() <= 1024:
                out["grad." + k] = g.numpy()
    out.update(_np({k: v for k, v in data.items() if torch.is_tensor(v)}, "data."))
    out["data.image_size0"] = data["view0"]["image_size"].numpy()
    out["data.image_size1"] = data["view1"]["image_size"].numpy()
    out["meta"] = np.array([batch, n0, n1, n_layers, dim, heads, seed, size[0], size[1]])
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, "total loss", losses["total"].tolist(),
          "matches", (pred["matches0"] > -1).sum(1).tolist())


def gen_lightglue_sift(name, batch, n0, n1, n_layers, seed):
    """The reference LightGlue as `configs/sift+lightglue_*.yaml` set it up: 128-d input descriptors through `input_proj`
    (lightglue.py:343-346) and `add_scale_ori: true` -- keypoint scale and orientation join the positional encoding
    (lightglue.py:348-350, 426-443).  Inputs stored; weights regenerated from the seed (checksum)."""
    params = lgo.init_params(n_layers, 256, 4, input_dim=128, seed=seed, pos_dim=4)
    data = make_pairs(batch, n0, n1, dim=128, size=(640, 480), seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    for i, n in (("0", n0), ("1", n1)):
        data["scales" + i] = torch.rand(batch, n, generator=g) * 4 + 1          # SIFT-like scales (pixels) ...
        data["oris" + i] = (torch.rand(batch, n, generator=g) * 2 - 1) * 3.14159  # ... and orientations (radians)
    model = ref_lightglue_conf({"n_layers": n_layers, "descriptor_dim": 256, "input_dim": 128, "num_heads": 4,
                                "add_scale_ori": True, "weights": None, "flash": False, "checkpointed": False,
                                "filter_threshold": 0.0}, params)
    out = {}
    model.eval()
    with torch.no_grad():
        pe = model(data)
    out.update(_np({k: pe[k] for k in ("matches0", "matches1", "matching_scores0", "log_assignment")}, "eval."))
    model.train()
    pred = model(data)
    losses, _ = model.loss(pred, {**pred, **data})
    losses["total"].mean().backward()
    out.update(_np({k: pred[k] for k in ("matches0", "matches1", "matching_scores0", "log_assignment")}, "train."))
    out.update(_np({k: v for k, v in losses.items() if torch.is_tensor(v)}, "loss."))
    for k, prm in model.named_parameters():
        out["gradnorm." + k] = np.array([float(prm.grad.double().norm())])
        if prm.grad.numel() <= 2048:
            out["grad." + k] = prm.grad.numpy()
    out["param_checksum"] = np.array([float(sum(v.double().abs().sum() for v in params.values()))])
    out.update(_np({k: v for k, v in data.items() if torch.is_tensor(v)}, "data."))
    out["data.image_size0"] = data["view0"]["image_size"].numpy()
    out["data.image_size1"] = data["view1"]["image_size"].numpy()
    out["meta"] = np.array([batch, n0, n1, n_layers, seed])
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, "total loss", losses["total"].tolist(), "matches", (pred["matches0"] > -1).sum(1).tolist())


# ---------------------------------------------------------------------------------------------------------------
# Configuration options and edge cases of SuperGlue / GlueStick that no other fixture touches (tests/golden/matcher_options.npz)
def gen_matcher_options(name="matcher_options"):
    from gluefactory.models.matchers.gluestick import GlueStick
    from gluefactory_nonfree.superglue import SuperGlue
    out = {}
    from oracle.option_cases import option_cases
    for cname, (kind, conf, params, data) in option_cases().items():
        from gluefactory.models.matchers.lightglue import LightGlue
        model = {"superglue": SuperGlue, "gluestick": GlueStick, "lightglue": LightGlue}[kind](conf)
        res = model.load_state_dict(params, strict=True)
        assert not res.missing_keys and not res.unexpected_keys, (cname, res)
        out[f"{cname}.param_checksum"] = np.array([float(sum(v.double().abs().sum() for v in params.values()))])
        model.eval()
        with torch.no_grad():
            pe = model(data)
        for k, v in pe.items():
            if torch.is_tensor(v):
                out[f"{cname}.eval.{k}"] = v.numpy()
        if cname.endswith("_empty"):
            continue
        model.train()
        pred = model(data)
        losses = model.loss(pred, {**pred, **data})
        losses = losses[0] if isinstance(losses, tuple) else losses
        losses["total"].mean().backward()
        for k in ("log_assignment", "line_log_assignment"):
            if k in pred:
                out[f"{cname}.train.{k}"] = pred[k].detach().numpy()
        for k, v in losses.items():
            if torch.is_tensor(v):
                out[f"{cname}.loss.{k}"] = v.detach().numpy()
        for k, prm in model.named_parameters():
            if prm.grad is not None:
                out[f"{cname}.gradnorm.{k}"] = np.array([float(prm.grad.double().norm())])
        # BatchNorm buffers AFTER the step (forward + backward): the reference's activation checkpointing re-runs the GNN
        # layers' forward during the backward, so their running statistics have been updated twice per call by now
        for k, buf in model.named_buffers():
            out[f"{cname}.buffer.{k}"] = buf.detach().numpy().copy()
        print(name, cname, "loss", losses["total"].tolist())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)


def ref_lightglue_conf(conf, params):
    from gluefactory.models.matchers.lightglue import LightGlue
    model = LightGlue(conf)
    res = model.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model


def gen_superglue(name, batch, n0, n1, gnn, iters, seed):
    """Reference SuperGlue (weights=None, seeded state_dict shared with the oracle): eval and
    train-mode forward, loss values and gradient norms; plus a bare log_optimal_transport case."""
    from gluefactory_nonfree.superglue import SuperGlue, log_optimal_transport
    from oracle import superglue_oracle as sgo

    params = sgo.init_params(256, gnn_layers=len(gnn), seed=seed)
    data = make_pairs(batch, n0, n1, dim=256, size=(640, 480), seed=seed + 1)
    data["view0"]["image"] = torch.zeros(batch, 1, 480, 640)
    data["view1"]["image"] = torch.zeros(batch, 1, 480, 640)
    model = SuperGlue({"weights": None, "GNN_layers": gnn, "num_sinkhorn_iterations": iters})
    res = model.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    out = {}
    model.eval()
    with torch.no_grad():
        pe = model(data)
    out.update(_np({k: pe[k] for k in ("log_assignment", "matches0", "matches1", "matching_scores0")}, "eval."))
    model.train()
    pred = model(data)
    losses = model.loss(pred, {**pred, **data})      # the reference returns a bare dict here
    losses["total"].mean().backward()
    out.update(_np({k: pred[k] for k in ("log_assignment", "matches0", "sinkhorn_cost")}, "train."))
    out.update(_np({k: v for k, v in losses.items() if torch.is_tensor(v)}, "loss."))
    for k, prm in model.named_parameters():
        out["gradnorm." + k] = np.array([float(prm.grad.double().norm())])
        if prm.grad.numel() <= 512:
            out["grad." + k] = prm.grad.numpy()
    out["param_checksum"] = np.array([float(sum(v.double().abs().sum() for v in params.values()))])
    out.update(_np({k: v for k, v in data.items() if torch.is_tensor(v)}, "data."))
    out["data.image_size0"] = data["view0"]["image_size"].numpy()
    out["data.image_size1"] = data["view1"]["image_size"].numpy()
    out["meta"] = np.array([batch, n0, n1, len(gnn), iters, seed])
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, "loss", losses["total"].tolist(), "matches", (pred["matches0"] > -1).sum(1).tolist())
    # bare optimal transport, with gradients w.r.t. scores and alpha
    g = torch.Generator().manual_seed(seed)
    scores = (torch.randn(2, 37, 45, generator=g) * 2).requires_grad_(True)
    alpha = torch.tensor(0.8, requires_grad=True)
    Z = log_optimal_transport(scores, alpha, 25)
    G = torch.randn(Z.shape, generator=g)
    (Z * G).sum().backward()
    np.savez_compressed(os.path.join(GOLD, "superglue_ot.npz"), scores=scores.detach().numpy(),
                        alpha=alpha.detach().numpy(), iters=np.array(25), out=Z.detach().numpy(),
                        G=G.numpy(), gscores=scores.grad.numpy(), galpha=alpha.grad.numpy())


def gen_gluestick(name, batch, n_kpts, n_lines, gnn, inter, seed, line_attention=False):
    """Reference GlueStick (weights=None) on a synthetic point+line batch: eval + train forward,
    every loss entry and all gradient norms."""
    from gluefactory.models.matchers.gluestick import GlueStick
    from glue_factory_amd.synthetic import make_point_line_pairs
    from oracle import gluestick_oracle as gso

    params = gso.init_params(256, gnn_layers=len(gnn), inter=inter, seed=seed)
    data = make_point_line_pairs(batch, n_kpts, n_lines, dim=256, size=(640, 480), seed=seed + 1)
    if line_attention:
        gso.add_line_attention_params(params, seed=seed + 2)
    model = GlueStick({"weights": None, "GNN_layers": gnn, "inter_supervision": inter, "line_attention": line_attention})
    res = model.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    out = {}
    keys = ("log_assignment", "matches0", "matching_scores0", "line_log_assignment", "line_matches0",
            "raw_line_scores")
    model.eval()
    with torch.no_grad():
        pe = model(data)
    out.update(_np({k: pe[k] for k in keys}, "eval."))
    model.train()
    pred = model(data)
    losses, _ = model.loss(pred, {**pred, **data})
    losses["total"].mean().backward()
    out.update(_np({k: pred[k] for k in keys}, "train."))
    for layer in inter or []:
        out[f"train.line_{layer}_log_assignment"] = pred[f"line_{layer}_log_assignment"].detach().numpy()
    out.update(_np({k: v for k, v in losses.items() if torch.is_tensor(v)}, "loss."))
    for k, prm in model.named_parameters():
        out["gradnorm." + k] = np.array([float(prm.grad.double().norm())])
    out["param_checksum"] = np.array([float(sum(v.double().abs().sum() for v in params.values()))])
    out.update(_np({k: v for k, v in data.items() if torch.is_tensor(v)}, "data."))
    out["data.image_size0"] = data["view0"]["image_size"].numpy()
    out["data.image_size1"] = data["view1"]["image_size"].numpy()
    out["meta"] = np.array([batch, n_kpts, n_lines, len(gnn), seed] + list(inter or []))
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, "loss", losses["total"].tolist(), "line matches", (pred["line_matches0"] > -1).sum(1).tolist())


def gen_superpoint(name, seed):
    """Reference superpoint_open on seeded random weights (shared through a temp state_dict file)
    and seeded images; eval-mode and train-mode (batch-statistics BatchNorm) outputs."""
    import tempfile
    from gluefactory.models.extractors.superpoint_open import SuperPoint as RefSP
    from glue_factory_amd.extractors.superpoint_open import SuperPoint

    conf = {"max_num_keypoints": 100, "force_num_keypoints": True, "detection_threshold": 0.0, "nms_radius": 3}
    torch.manual_seed(seed)
    ours = SuperPoint(conf)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sp.pth")
        torch.save(ours.state_dict(), path)
        ref = RefSP({**conf, "weights": path})
    g = torch.Generator().manual_seed(seed + 1)
    image = torch.rand(2, 3, 120, 160, generator=g)
    out = {"image": image.numpy(), "seed": np.array(seed)}
    for mode in ("eval", "train"):
        getattr(ref, mode)()
        with torch.no_grad():
            pr = ref({"image": image})
        out.update(_np(pr, mode + "."))
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, "keypoints", tuple(pr["keypoints"].shape))


def gen_superpoint_options(name, seed):
    """Reference superpoint_open under the configurations of superpoint_option_cases(), seeded weights shared through a temp
    state_dict file; the detector's last convolution is scaled so that the scores spread (random weights give 1/65 everywhere)."""
    import tempfile
    from gluefactory.models.extractors.superpoint_open import SuperPoint as RefSP
    from glue_factory_amd.extractors.superpoint_open import SuperPoint
    out = {"seed": np.array(seed)}
    from oracle.option_cases import superpoint_option_cases
    for cname, (conf, shape) in superpoint_option_cases().items():
        torch.manual_seed(seed)
        ours = SuperPoint(conf)
        for prm in ours.detector[1].parameters():
            if prm.ndim == 4:
                prm.data.mul_(40.0)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "sp.pth")
            torch.save(ours.state_dict(), path)
            ref = RefSP({**conf, "weights": path}).eval()
        g = torch.Generator().manual_seed(seed + 1)
        image = torch.rand(*shape, generator=g)
        with torch.no_grad():
            pr = ref({"image": image})
        out[f"{cname}.image"] = image.numpy()
        out.update(_np(pr, cname + "."))
        print(name, cname, {k: tuple(v.shape) for k, v in pr.items()})
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)


def gen_superpoint_nonfree(name, seed):
    """Reference gluefactory_nonfree.superpoint (the MagicLeap-layout extractor the N=2048 LightGlue yaml names) on seeded
    random weights: the reference constructor downloads superpoint_v1.pth, so torch.hub is pointed at the state_dict of OUR
    module's seeded initialisation (same names / shapes: that is the drop-in claim); eval-mode outputs for three
    configurations (legacy sampling, corrected sampling, soft-argmax refinement), with and without `image_size`."""
    from gluefactory_nonfree.superpoint import SuperPoint as RefSP
    from glue_factory_amd.extractors.superpoint import SuperPoint
    g = torch.Generator().manual_seed(seed + 1)
    image = torch.rand(2, 1, 120, 160, generator=g)
    size = torch.tensor([[160, 120], [131, 97]])
    out = {"image": image.numpy(), "image_size": size.numpy(), "seed": np.array(seed)}
    cases = {"legacy": {"nms_radius": 3}, "fixed": {"nms_radius": 4, "legacy_sampling": False},
             "refine": {"nms_radius": 3, "refinement_radius": 2}}
    for cname, extra in cases.items():
        conf = {"max_num_keypoints": 100, "force_num_keypoints": True, "detection_threshold": 0.0, **extra}
        torch.manual_seed(seed)
        ours = SuperPoint(conf)
        ours.convPb.weight.data.mul_(40.0)      # spread the detector logits: random weights give 1/65 everywhere (all scores tied)
        sd = ours.state_dict()
        torch.hub.load_state_dict_from_url = lambda *a, **k: sd
        ref = RefSP(conf).eval()
        assert set(ref.state_dict()) == set(sd)
        for tag, data in (("plain", {"image": image}), ("sized", {"image": image, "image_size": size})):
            with torch.no_grad():
                pr = ref(dict(data))
            out.update(_np(pr, f"{cname}.{tag}."))
        print(name, cname, "keypoints", tuple(pr["keypoints"].shape))
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)


def gen_gt(name, batch, n0, n1, seed):
    from gluefactory.geometry.gt_generation import gt_matches_from_homography

    data = make_pairs(batch, n0, n1, dim=8, size=(640, 480), seed=seed, with_gt=False)
    ref = gt_matches_from_homography(data["keypoints0"], data["keypoints1"], data["H_0to1"],
                                     pos_th=3.0, neg_th=3.0)
    out = _np({k: data[k] for k in ("keypoints0", "keypoints1", "H_0to1")}, "data.")
    out.update(_np(ref, "gt."))
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, "positives", ref["assignment"].sum((1, 2)).tolist())


def depth_scene(batch, n0, n1, seed, hw=(96, 128)):
    """Seeded synthetic two-view scene: smooth positive depth maps with holes, pinhole cameras, a small relative
    pose; kp1 = reprojections of a subset of kp0 (+ noise) followed by uniform points.  Plain tensors only."""
    g = torch.Generator().manual_seed(seed)
    h, w = hw
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    depth = []
    for v in range(2):
        d = 4.0 + 0.6 * torch.sin(xs / 17.0 + v) + 0.4 * torch.cos(ys / 11.0 - v) + 0.05 * torch.rand(batch, h, w, generator=g)
        d[:, 20:30, 40:60] = 0.0                       # a hole (invalid depth)
        d[torch.rand(batch, h, w, generator=g) < 0.03] = 0.0
        depth.append(d)
    f = 100.0
    cam = torch.tensor([w, h, f, f, w / 2.0, h / 2.0]).repeat(batch, 1)
    ang = 0.05 * (torch.rand(batch, 3, generator=g) - 0.5)
    K = torch.zeros(batch, 3, 3)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -ang[:, 2], ang[:, 1], -ang[:, 0]
    K = K - K.transpose(1, 2)
    R = torch.linalg.matrix_exp(K)
    t = 0.3 * (torch.rand(batch, 3, generator=g) - 0.5)
    kp0 = torch.rand(batch, n0, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0])
    return {"depth0": depth[0], "depth1": depth[1], "camera0": cam, "camera1": cam.clone(), "R": R, "t": t,
            "keypoints0": kp0, "n1": n1, "seed": seed}


def gen_gt_depth(name, batch, n0, n1, seed):
    from gluefactory.geometry.depth import project, sample_depth
    from gluefactory.geometry.gt_generation import gt_matches_from_pose_depth
    from gluefactory.geometry.wrappers import Camera, Pose

    sc = depth_scene(batch, n0, n1, seed)
    cam0, cam1 = Camera(sc["camera0"]), Camera(sc["camera1"])
    T = Pose.from_Rt(sc["R"], sc["t"])
    kp0 = sc["keypoints0"]
    d0, v0 = sample_depth(kp0, sc["depth0"])
    proj, vis = project(kp0, d0, sc["depth1"], cam0, cam1, T, v0)
    g = torch.Generator().manual_seed(seed + 1)
    nm = (2 * n1) // 3
    kp1 = torch.rand(batch, n1, 2, generator=g) * torch.tensor([127.0, 95.0])
    src = torch.nan_to_num(proj[:, :nm], nan=5.0) + 0.7 * torch.randn(batch, nm, 2, generator=g)
    kp1[:, :nm] = torch.where(vis[:, :nm, None], src, kp1[:, :nm])
    kp1 = kp1[:, torch.randperm(n1, generator=g)]
    data = {"view0": {"camera": cam0, "depth": sc["depth0"]}, "view1": {"camera": cam1, "depth": sc["depth1"]},
            "T_0to1": T}
    out = {"data.depth0": sc["depth0"].numpy(), "data.depth1": sc["depth1"].numpy(), "data.camera0": sc["camera0"].numpy(),
           "data.camera1": sc["camera1"].numpy(), "data.R": sc["R"].numpy(), "data.t": sc["t"].numpy(),
           "data.keypoints0": kp0.numpy(), "data.keypoints1": kp1.numpy()}
    for tag, kwargs in (("plain", {}), ("cc", {"cc_th": 4.0}), ("epi", {"epi_th": 1.0, "cc_th": 4.0})):
        ref = gt_matches_from_pose_depth(kp0, kp1, data, pos_th=3.0, neg_th=5.0, **kwargs)
        out.update(_np(ref, f"{tag}."))
        print(name, tag, "positives", ref["assignment"].sum((1, 2)).tolist(),
              "unmatched0", (ref["matches0"] == -1).sum(1).tolist(), "ignored0", (ref["matches0"] == -2).sum(1).tolist())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)


def gen_gt_lines_depth(name, batch, n0, n1, seed):
    """Reference gt_line_matches_from_pose_depth (gt_generation.py:207-407) on the seeded depth scene: segments of view 0,
    view-1 segments = reprojected endpoints of a subset (+ noise) followed by random ones, a few lines flagged invalid, some
    reaching over the depth hole (ignored) and some leaving the image (unmatched)."""
    from gluefactory.geometry.depth import project, sample_depth
    from gluefactory.geometry.gt_generation import gt_line_matches_from_pose_depth
    from gluefactory.geometry.wrappers import Camera, Pose

    sc = depth_scene(batch, 4, 4, seed)
    h, w = sc["depth0"].shape[-2:]
    cam0, cam1 = Camera(sc["camera0"]), Camera(sc["camera1"])
    T = Pose.from_Rt(sc["R"], sc["t"])
    g = torch.Generator().manual_seed(seed + 1)
    wh = torch.tensor([w - 1.0, h - 1.0])
    p = torch.rand(batch, n0, 2, generator=g) * (wh - 10) + 5
    ang = torch.rand(batch, n0, generator=g) * 6.2832
    ln = 8 + torch.rand(batch, n0, generator=g) * 30
    q = p + ln[..., None] * torch.stack([torch.cos(ang), torch.sin(ang)], -1)
    lines0 = torch.stack([p, q], 2)                                        # [B,L0,2,2] (may leave the image: clamped inside)
    ends = lines0.reshape(batch, n0 * 2, 2).clamp(min=torch.zeros(2), max=wh)
    d, v = sample_depth(ends, sc["depth0"])
    proj, vis = project(ends, d, sc["depth1"], cam0, cam1, T, v)
    proj = torch.nan_to_num(proj, nan=7.0).reshape(batch, n0, 2, 2)
    nm = (2 * n1) // 3
    lines1 = torch.rand(batch, n1, 2, 2, generator=g) * wh
    lines1[:, :nm] = proj[:, :nm] + 0.8 * torch.randn(batch, nm, 2, 2, generator=g)
    lines1 = lines1[:, torch.randperm(n1, generator=g)]
    valid0 = torch.rand(batch, n0, generator=g) > 0.1
    valid1 = torch.rand(batch, n1, generator=g) > 0.1
    image = torch.zeros(batch, 1, h, w)
    data = {"view0": {"camera": cam0, "depth": sc["depth0"], "image": image},
            "view1": {"camera": cam1, "depth": sc["depth1"], "image": image}, "T_0to1": T, "T_1to0": T.inv()}
    out = {"data.depth0": sc["depth0"].numpy(), "data.depth1": sc["depth1"].numpy(), "data.camera0": sc["camera0"].numpy(),
           "data.camera1": sc["camera1"].numpy(), "data.R": sc["R"].numpy(), "data.t": sc["t"].numpy(),
           "data.lines0": lines0.numpy(), "data.lines1": lines1.numpy(), "data.valid0": valid0.numpy(), "data.valid1": valid1.numpy()}
    for tag, kw in (("default", {}), ("loose", {"npts": 30, "dist_th": 3, "overlap_th": 0.4, "min_visibility_th": 0.3})):
        pos, m0, m1 = gt_line_matches_from_pose_depth(lines0, lines1, valid0, valid1, data, **kw)
        out.update({f"{tag}.assignment": pos.numpy(), f"{tag}.matches0": m0.numpy(), f"{tag}.matches1": m1.numpy()})
        print(name, tag, "positives", pos.sum((1, 2)).tolist(), "unmatched0", (m0 == -1).sum(1).tolist(),
              "ignored0", (m0 == -2).sum(1).tolist(), "ignored1", (m1 == -2).sum(1).tolist())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)


def gen_gt_lines(name, batch, n0, n1, seed):
    from gluefactory.geometry.gt_generation import gt_line_matches_from_homography
    from gluefactory.geometry.homography import warp_points_torch

    g = torch.Generator().manual_seed(seed)
    w, h = 320, 240
    ang = 0.08
    H = torch.tensor([[1.02 * np.cos(ang), -np.sin(ang), 6.0], [np.sin(ang), 0.98 * np.cos(ang), -4.0],
                      [1e-5, -2e-5, 1.0]], dtype=torch.float32).repeat(batch, 1, 1)
    wh = torch.tensor([w - 1.0, h - 1.0])
    lines0 = torch.rand(batch, n0, 2, 2, generator=g) * wh
    nm = (2 * n1) // 3                                     # images of some lines of view 0 (+ noise), then random ones
    warped = warp_points_torch(lines0[:, :nm].reshape(batch, nm * 2, 2), H, inverse=False).reshape(batch, nm, 2, 2)
    lines1 = torch.rand(batch, n1, 2, 2, generator=g) * wh
    lines1[:, :nm] = warped + 1.5 * torch.randn(batch, nm, 2, 2, generator=g)
    lines1 = lines1[:, torch.randperm(n1, generator=g)]
    valid0 = torch.rand(batch, n0, generator=g) > 0.1
    valid1 = torch.rand(batch, n1, generator=g) > 0.1
    pos, m0, m1 = gt_line_matches_from_homography(lines0, lines1, valid0, valid1, (batch, 1, h, w), (batch, 1, h, w), H,
                                                  npts=50, dist_th=5, overlap_th=0.2, min_visibility_th=0.5)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), lines0=lines0.numpy(), lines1=lines1.numpy(),
                        valid0=valid0.numpy(), valid1=valid1.numpy(), H=H.numpy(), hw=np.array([h, w]),
                        assignment=pos.numpy(), matches0=m0.numpy(), matches1=m1.numpy())
    print(name, "positives", pos.sum((1, 2)).tolist(), "unmatched0", (m0 == -1).sum(1).tolist(),
          "ignored0", (m0 == -2).sum(1).tolist())


def _data_checksum(data):
    return np.array([float(sum(v.double().abs().sum() for v in data.values() if torch.is_tensor(v) and v.is_floating_point()))])


def gen_lightglue_config(name, batch, n, n_layers, seed, size, stride=61, sharp=None):
    """Compact golden of a BASELINE.json configuration run through the REFERENCE LightGlue itself (config 1:
    B=4, N=512, L=4; config 2 shape at B=1: N=2048, L=9).  Inputs and weights are regenerated from the seed by
    the test (checksums stored); stored are every loss entry, the eval-mode matcher metrics, the match
    vectors, a strided sample of the (N+1)^2 log-assignment plus its row sums, and the gradient norm of every
    parameter (full gradients for the small tensors).
    sharp=(damp, sharp, noise): the decisive case of lgo.sharp_case instead (every row / column arg-max of the reference's
    own output is separated from the runner-up by the stored margin, so the tests compare matches0/1 bit for bit on
    100 % of the rows)."""
    if sharp is None:
        params = lgo.init_params(n_layers, 256, 4, seed=seed)
        data = make_pairs(batch, n, dim=256, size=size, seed=seed + 1)
    else:
        params, data = lgo.sharp_case(batch, n, n_layers, seed, size, *sharp)
    model = ref_lightglue(n_layers, 256, 4, params, filter_threshold=0.0)
    out = {}
    model.eval()
    with torch.no_grad():
        pe = model(data)
        le, me = model.loss(pe, {**pe, **data})
    out.update(_np({k: pe[k] for k in ("matches0", "matches1", "matching_scores0", "matching_scores1")}, "eval."))
    out.update(_np(me, "metric."))
    out.update(_np({k: v for k, v in le.items() if torch.is_tensor(v)}, "evalloss."))
    model.train()
    pred = model(data)
    losses, _ = model.loss(pred, {**pred, **data})
    losses["total"].mean().backward()
    la = pred["log_assignment"].detach()
    out["train.la_sample"] = la.flatten(1)[:, ::stride].numpy()
    out["train.la_rowsum"] = la.double().sum(2).float().numpy()
    out["train.la_colsum"] = la.double().sum(1).float().numpy()
    out["train.rowmax"] = la[:, :-1, :-1].max(2).values.numpy()
    out.update(_np({k: pred[k] for k in ("matches0", "matches1", "matching_scores0")}, "train."))
    out.update(_np({k: v for k, v in losses.items() if torch.is_tensor(v)}, "loss."))
    for k, prm in model.named_parameters():
        out["gradnorm." + k] = np.array([float(prm.grad.double().norm())])
        if prm.grad.numel() <= 1024:
            out["grad." + k] = prm.grad.numpy()
    out["param_checksum"] = np.array([float(sum(v.double().abs().sum() for v in params.values()))])
    out["data_checksum"] = _data_checksum(data)
    out["meta"] = np.array([batch, n, n_layers, seed, size[0], size[1], stride])
    if sharp is not None:
        out["sharp"] = np.array(sharp, dtype=np.float64)
        out["margins"] = np.array(lgo.decision_margins(la) + lgo.decision_margins(pe["log_assignment"]))
        assert out["margins"].min() > 1.0, out["margins"]          # decisive in train AND eval mode
        assert (pred["matches0"] > -1).all() and (pe["matches0"] == pred["matches0"]).all()
        print(name, "decision margins (train rows, cols, eval rows, cols)", out["margins"].tolist())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, "total loss", losses["total"].tolist(), "matches", (pred["matches0"] > -1).sum(1).tolist(),
          "metrics", {k: v.tolist() for k, v in me.items()})


def _grad_digest(out, named_grads, sample=2048):
    """norm of every parameter gradient + a strided sample of <= `sample` entries (the bf16 tests bound the relative
    error of the sample, the fp32 tests hold the norm and the sample to the reference)."""
    for k, g in named_grads:
        out["gradnorm." + k] = np.array([float(g.double().norm())])
        flat = g.detach().flatten()
        st = max(1, flat.numel() // sample)
        out["gradsample." + k] = flat[::st][:sample].numpy()


def _la_digest(out, la, stride, prefix="train."):
    la = la.detach()
    out[prefix + "la_sample"] = la.flatten(1)[:, ::stride].numpy()
    out[prefix + "la_rowsum"] = la.double().sum(2).float().numpy()
    out[prefix + "la_colsum"] = la.double().sum(1).float().numpy()
    out[prefix + "rowmax"] = la[:, :-1, :-1].max(2).values.numpy()


def gen_superglue_config(name, batch, n, iters, seed, stride=997, sharp=None):
    """BASELINE configs[3] through the REFERENCE SuperGlue itself: N=2048 keypoints per image, the full 18-layer
    GNN, 100 Sinkhorn iterations (B=1: the reference keeps ~10 GB of autograd state for the unrolled Sinkhorn).
    Compact storage as for lightglue_n2048_l9: inputs / weights regenerated from the seed by the test.
    sharp=(damp, sharp, noise, unmatched): the decisive case of sgo.sharp_case (B=2, so the train-mode BatchNorm
    statistics run over several pairs): every mutual-NN decision of the reference's own output -- matched or -1 -- is
    taken by the stored margin, so the tests compare matches0/1 bit for bit, in fp32 and bf16."""
    from gluefactory_nonfree.superglue import SuperGlue
    from oracle import superglue_oracle as sgo

    if sharp is None:
        params = sgo.init_params(256, gnn_layers=18, seed=seed)
        data = make_pairs(batch, n, dim=256, size=(1024, 1024), seed=seed + 1)
    else:
        params, data = sgo.sharp_case(batch, n, 18, seed, (1024, 1024), *sharp)
    data["view0"]["image"] = torch.zeros(batch, 1, 1024, 1024)
    data["view1"]["image"] = torch.zeros(batch, 1, 1024, 1024)
    model = SuperGlue({"weights": None, "num_sinkhorn_iterations": iters})
    res = model.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    out = {}
    model.eval()
    with torch.no_grad():
        pe = model(data)
    out.update(_np({k: pe[k] for k in ("matches0", "matches1", "matching_scores0")}, "eval."))
    _la_digest(out, pe["log_assignment"], stride, "eval.")
    model.train()
    pred = model(data)
    losses = model.loss(pred, {**pred, **data})
    losses["total"].mean().backward()
    _la_digest(out, pred["log_assignment"], stride)
    out["train.cost_sample"] = pred["sinkhorn_cost"].detach().flatten(1)[:, ::stride].numpy()
    out.update(_np({k: pred[k] for k in ("matches0", "matches1", "matching_scores0")}, "train."))
    out.update(_np({k: v for k, v in losses.items() if torch.is_tensor(v)}, "loss."))
    _grad_digest(out, [(k, p.grad) for k, p in model.named_parameters()])
    out["param_checksum"] = np.array([float(sum(v.double().abs().sum() for v in params.values()))])
    out["data_checksum"] = _data_checksum(data)
    out["meta"] = np.array([batch, n, 18, iters, seed, stride])
    if sharp is not None:
        out["sharp"] = np.array(sharp, dtype=np.float64)
        out["margins"] = np.array([sgo.decisiveness(pred["log_assignment"].detach(), 0.2), sgo.decisiveness(pe["log_assignment"], 0.2)])
        assert out["margins"].min() > 1.0, out["margins"]          # decisive in train AND eval mode
        for m in (pred, pe):                                        # ... and the decisions are the constructed ones
            assert (m["matches0"] == data["gt_matches0"]).all() and (m["matches1"] == data["gt_matches1"]).all()
        print(name, "decision margins (train, eval)", out["margins"].tolist())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, "loss", losses["total"].tolist(), "matches", (pred["matches0"] > -1).sum(1).tolist())


def gen_gluestick_config(name, batch, n_kpts, n_lines, seed, stride=997, sharp=None):
    """BASELINE configs[4] through the REFERENCE GlueStick: 2048 keypoints + 512 lines (1024 junctions -> 3072 tokens
    per image), default 9 x (self, cross) GNN with the line layers, B=1.  Compact storage.
    sharp=(damp, sharp, noise, unmatched): the decisive case of gso.sharp_case (B=2: train-mode BatchNorm over several
    pairs) -- points AND lines, matched and -1 -- for bit-exact matches0/1 and line_matches0/1 in fp32 and bf16."""
    from gluefactory.models.matchers.gluestick import GlueStick
    from glue_factory_amd.synthetic import make_point_line_pairs
    from oracle import gluestick_oracle as gso
    from oracle import superglue_oracle as sgo

    gnn = ["self", "cross"] * 9
    if sharp is None:
        params = gso.init_params(256, gnn_layers=len(gnn), inter=None, seed=seed)
        data = make_point_line_pairs(batch, n_kpts, n_lines, dim=256, size=(1024, 1024), seed=seed + 1)
    else:
        params, data = gso.sharp_case(batch, n_kpts, n_lines, len(gnn), seed, (1024, 1024), *sharp)
    model = GlueStick({"weights": None})
    res = model.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    out = {}
    model.eval()
    with torch.no_grad():
        pe = model(data)
    mkeys = ("matches0", "matches1", "matching_scores0", "line_matches0", "line_matches1", "line_matching_scores0")
    out.update(_np({k: pe[k] for k in mkeys}, "eval."))
    model.train()
    pred = model(data)
    losses, _ = model.loss(pred, {**pred, **data})
    losses["total"].mean().backward()
    _la_digest(out, pred["log_assignment"], stride)
    _la_digest(out, pred["line_log_assignment"], 97, "train.line_")
    out["train.raw_line_scores_sample"] = pred["raw_line_scores"].detach().flatten(1)[:, ::97].numpy()
    out.update(_np({k: pred[k] for k in mkeys}, "train."))
    out.update(_np({k: v for k, v in losses.items() if torch.is_tensor(v)}, "loss."))
    _grad_digest(out, [(k, p.grad) for k, p in model.named_parameters() if p.grad is not None])
    out["param_checksum"] = np.array([float(sum(v.double().abs().sum() for v in params.values()))])
    out["data_checksum"] = _data_checksum(data)
    out["meta"] = np.array([batch, n_kpts, n_lines, len(gnn), seed, stride])
    if sharp is not None:
        out["sharp"] = np.array(sharp, dtype=np.float64)
        out["margins"] = np.array([sgo.decisiveness(m[k].detach(), 0.2) for m in (pred, pe)
                                   for k in ("log_assignment", "line_log_assignment")])
        assert out["margins"].min() > 1.0, out["margins"]          # decisive in train AND eval mode, points and lines
        for m in (pred, pe):
            for k in ("matches0", "matches1", "line_matches0", "line_matches1"):
                assert (m[k] == data["gt_" + k]).all(), k
        print(name, "decision margins (train points, lines, eval points, lines)", out["margins"].tolist())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, "loss", losses["total"].tolist(), "matches", (pred["matches0"] > -1).sum(1).tolist(),
          "line matches", (pred["line_matches0"] > -1).sum(1).tolist())


def gen_metrics(name, seed):
    """matcher_metrics of the reference (models/utils/metrics.py:4-50) on seeded match / ground-truth vectors
    with every label class present: correct and wrong matches, unmatched (-1) and ignored (-2) ground truth."""
    from gluefactory.models.utils.metrics import matcher_metrics
    g = torch.Generator().manual_seed(seed)
    B, M, N = 3, 200, 180
    gt = torch.randint(0, N, (B, M), generator=g)
    r = torch.rand(B, M, generator=g)
    gt = torch.where(r < 0.3, torch.full_like(gt, -1), gt)
    gt = torch.where(r > 0.9, torch.full_like(gt, -2), gt)
    m = gt.clone()
    r2 = torch.rand(B, M, generator=g)
    m = torch.where(r2 < 0.25, torch.randint(0, N, (B, M), generator=g), m)      # wrong matches
    m = torch.where((r2 > 0.8), torch.full_like(m, -1), m)                        # missed
    scores = torch.rand(B, M, generator=g) * (m > -1)
    pred = {"matches0": m, "matching_scores0": scores}
    data = {"gt_matches0": gt}
    out = {"matches0": m.numpy(), "matching_scores0": scores.numpy(), "gt_matches0": gt.numpy()}
    out.update(_np(matcher_metrics(pred, data), "metric."))
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, {k: v.tolist() for k, v in matcher_metrics(pred, data).items()})


def gen_metrics_sweep(name):
    """matcher_metrics of the reference on every case of tests/test_reference_metrics_sweep.py (inputs rebuilt there from
    their seeds; only the outputs are stored, as "<case>.<metric>")."""
    from gluefactory.models.utils.metrics import matcher_metrics
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_reference_metrics_sweep as sweep
    out = {}
    for case in sweep.CASES:
        pred, data = sweep.case_inputs(*case)
        out.update(_np(matcher_metrics(pred, data, prefix=case[4], prefix_gt=case[5]), sweep.case_key(*case) + "."))
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, len(sweep.CASES), "cases")


def gen_lightglue_adaptive(name, n0, n1, n_layers, seed):
    """Eval-only adaptive depth / width (lightglue.py:461-529, b == 1) of the REFERENCE on seeded weights whose
    token-confidence / matchability biases are shifted so that the stop and the pruning actually trigger."""
    base = lgo.init_params(n_layers, 256, 4, seed=seed)
    data = make_pairs(1, n0, n1, dim=256, size=(640, 480), seed=seed + 1)
    cases = {
        # name: (param edits, depth_confidence, width_confidence)
        "neutral": ({}, 0.95, 0.99),
        # (an early stop before the last layer cannot be generated: the reference itself raises there --
        #  `torch.stack(all_desc0)` of an empty list, lightglue.py:536 -- so only non-stopping cases exist)
        "prune": ({}, -1, 0.5),
        "prune_tok": ({"token_confidence.0.token.0.bias": 1.5, "token_confidence.1.token.0.bias": 2.0}, 0.999, 0.55),
    }
    out = {}
    for cname, (edits, dc, wc) in cases.items():
        params = {k: v.clone() for k, v in base.items()}
        for k, val in edits.items():
            params[k] = torch.full_like(params[k], val)
        from gluefactory.models.matchers.lightglue import LightGlue
        model = LightGlue({"n_layers": n_layers, "descriptor_dim": 256, "input_dim": 256, "num_heads": 4,
                           "weights": None, "flash": False, "filter_threshold": 0.0,
                           "depth_confidence": dc, "width_confidence": wc})
        model.load_state_dict(params, strict=True)
        model.eval()
        with torch.no_grad():
            pe = model(data)
        for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "prune0", "prune1", "log_assignment"):
            out[f"{cname}.{k}"] = pe[k].numpy()
        out[f"{cname}.conf"] = np.array([dc, wc])
        for k, val in edits.items():
            out[f"{cname}.edit.{k}"] = np.array([val])
        print(name, cname, "la", tuple(pe["log_assignment"].shape), "matches", int((pe["matches0"] > -1).sum()),
              "prune0 hist", torch.bincount(pe["prune0"].long().flatten()).tolist())
    out["meta"] = np.array([n0, n1, n_layers, seed])
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)



def gen_trained_state(name, kind, state_path, stride=101):
    """Parity AT A TRAINED STATE (round-5 review, item 1a): every other golden pins the kernels at random-init weights; this one
    takes the state a 300-step run of tests/learning_cases.py ENDS in -- sharp attention, BatchNorm statistics far from their
    initial values, a grown bin_score -- and records the REFERENCE module's eval forward and train step (outputs, losses, every
    gradient) on a held-out batch of that run.  `state_path`: a state_dict saved by tools/probe/ref_learning_curve.py (the
    reference's own training run on the CPU) or tools/probe/learn_save_state.py (the HIP path's run on the MI355X).  The fixture
    keeps the state as the seeded initial state + its drift rounded to bf16 (2 bytes per parameter), and the golden is generated AT
    that reconstructed state, so both sides start from bit-identical parameters."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import learning_cases as lc
    if kind == "superglue":
        from gluefactory_nonfree.superglue import SuperGlue as Model
    else:
        from gluefactory.models.matchers.gluestick import GlueStick as Model
    init = lc.initial_params(kind)
    trained = torch.load(state_path, map_location="cpu")
    out = {}
    for k, v in init.items():
        if v.is_floating_point():
            out["delta." + k] = (trained[k].float() - v).to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint16)
        else:
            out["state." + k] = trained[k].numpy()
    state = lc.trained_state_from_delta(init, out)
    data = lc.batch(kind, lc.HELD_OUT[0])
    model = Model({**lc.conf(kind), "weights": None})
    res = model.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    lines = kind == "gluestick"
    mkeys = ("matches0", "matches1", "matching_scores0") + (("line_matches0", "line_matches1", "line_matching_scores0") if lines else ())
    model.eval()
    with torch.no_grad():
        pe = model(data)
        le = model.loss(pe, {**pe, **data})
        le = le[0] if isinstance(le, tuple) else le
    out.update(_np({k: pe[k] for k in mkeys}, "eval."))
    _la_digest(out, pe["log_assignment"], stride, "eval.")
    out["eval.loss_total"] = le["total"].numpy()
    if lines:
        _la_digest(out, pe["line_log_assignment"], 7, "eval.line_")
    model.train()
    pred = model(data)
    losses = model.loss(pred, {**pred, **data})
    losses = losses[0] if isinstance(losses, tuple) else losses
    losses["total"].mean().backward()
    _la_digest(out, pred["log_assignment"], stride)
    if lines:
        _la_digest(out, pred["line_log_assignment"], 7, "train.line_")
    out.update(_np({k: pred[k] for k in mkeys}, "train."))
    out.update(_np({k: v for k, v in losses.items() if torch.is_tensor(v)}, "loss."))
    _grad_digest(out, [(k, p.grad) for k, p in model.named_parameters() if p.grad is not None])
    post = model.state_dict()           # BatchNorm buffers after the step (incl. the second update under the reference's checkpointing)
    for k in post:
        if "running_" in k:
            out["post." + k] = post[k].numpy()
    out["data_checksum"] = _data_checksum(data)
    out["meta"] = np.array([lc.HELD_OUT[0], stride])
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    sharp = float((pred["log_assignment"].detach()[:, :-1, :-1].max(2).values).exp().mean())
    print(name, "eval loss", float(le["total"].mean()), "train-mode loss", float(losses["total"].mean()), "bin_score",
          float(state["bin_score"]), "mean row-max probability", round(sharp, 3), "file MB",
          round(os.path.getsize(os.path.join(GOLD, name + ".npz")) / 1e6, 2))


def main():
    os.makedirs(GOLD, exist_ok=True)
    only = set(sys.argv[1:])
    if only:      # python oracle/gen_golden.py lightglue_config1 ...: regenerate the named fixtures only
        todo = {
            "lightglue_config1": lambda: gen_lightglue_config("lightglue_config1", 4, 512, 4, seed=101, size=(640, 480)),
            "lightglue_n2048_l9": lambda: gen_lightglue_config("lightglue_n2048_l9", 1, 2048, 9, seed=103,
                                                                size=(1024, 1024), stride=997),
            "lightglue_sharp": lambda: gen_lightglue_config("lightglue_sharp", 1, 2048, 9, seed=131, size=(1024, 1024),
                                                             stride=997, sharp=(0.04, 11.0, 0.06)),
            "lightglue_adaptive": lambda: gen_lightglue_adaptive("lightglue_adaptive", 160, 200, 3, seed=107),
            "superpoint_options": lambda: gen_superpoint_options("superpoint_options", seed=57),
            "superpoint_nonfree": lambda: gen_superpoint_nonfree("superpoint_nonfree", seed=53),
            "metrics": lambda: gen_metrics("metrics", seed=109),
            "metrics_sweep": lambda: gen_metrics_sweep("metrics_sweep"),
            "superglue_config4": lambda: gen_superglue_config("superglue_config4", 1, 2048, 100, seed=113),
            "gluestick_config5": lambda: gen_gluestick_config("gluestick_config5", 1, 2048, 512, seed=127),
            "matcher_options": lambda: gen_matcher_options(),
            "gt_lines_depth": lambda: gen_gt_lines_depth("gt_lines_depth", batch=2, n0=40, n1=36, seed=73),
            "lightglue_sift": lambda: gen_lightglue_sift("lightglue_sift", 2, 150, 121, 2, seed=191),
            "superglue_sharp": lambda: gen_superglue_config("superglue_sharp", 2, 2048, 100, seed=151,
                                                             sharp=(0.01, 16.0, 0.03, 0.125)),
            "gluestick_sharp": lambda: gen_gluestick_config("gluestick_sharp", 2, 2048, 512, seed=157,
                                                             sharp=(0.01, 16.0, 0.03, 0.125)),
            "superglue_trained_ref": lambda: gen_trained_state("superglue_trained_ref", "superglue", "gpurun_out/learn_ref/ref_sg_t3.pt"),
            "superglue_trained_hip": lambda: gen_trained_state("superglue_trained_hip", "superglue", "gpurun_out/learn/sg_hip_fp32.pt"),
            "gluestick_trained_hip": lambda: gen_trained_state("gluestick_trained_hip", "gluestick", "gpurun_out/learn/gs_hip_fp32.pt"),
            "gluestick_lineattn": lambda: gen_gluestick("gluestick_lineattn", batch=2, n_kpts=36, n_lines=14,
                                                        gnn=["self", "cross"] * 2, inter=[0], seed=43, line_attention=True),
        }
        for k in only:
            todo[k]()
        return
    gen_lightglue("lightglue_small", batch=2, n0=40, n1=48, n_layers=2, dim=64, heads=4,
                  seed=11, size=(640, 480), store_params=True)
    gen_lightglue("lightglue_d256", batch=1, n0=72, n1=64, n_layers=2, dim=256, heads=4,
                  seed=23, size=(1024, 1024), store_params=False)
    gen_gt("gt_homography", batch=2, n0=96, n1=80, seed=5)
    gen_gt_depth("gt_depth", batch=2, n0=120, n1=100, seed=61)
    gen_gt_lines("gt_lines", batch=2, n0=40, n1=36, seed=71)
    gen_gt_lines_depth("gt_lines_depth", batch=2, n0=40, n1=36, seed=73)
    gen_superpoint("superpoint_open", seed=51)
    gen_superpoint_nonfree("superpoint_nonfree", seed=53)
    gen_superpoint_options("superpoint_options", seed=57)
    gen_gluestick("gluestick_d256", batch=2, n_kpts=40, n_lines=12, gnn=["self", "cross"] * 2, inter=[0], seed=41)
    gen_superglue("superglue_d256", batch=2, n0=60, n1=52, gnn=["self", "cross"] * 2, iters=20, seed=31)
    gen_lightglue_config("lightglue_config1", 4, 512, 4, seed=101, size=(640, 480))
    gen_lightglue_config("lightglue_n2048_l9", 1, 2048, 9, seed=103, size=(1024, 1024), stride=997)
    gen_lightglue_config("lightglue_sharp", 1, 2048, 9, seed=131, size=(1024, 1024), stride=997, sharp=(0.04, 11.0, 0.06))
    gen_lightglue_adaptive("lightglue_adaptive", 160, 200, 3, seed=107)
    gen_metrics("metrics", seed=109)
    gen_metrics_sweep("metrics_sweep")
    gen_superglue_config("superglue_config4", 1, 2048, 100, seed=113)
    gen_gluestick_config("gluestick_config5", 1, 2048, 512, seed=127)
    gen_gluestick("gluestick_lineattn", batch=2, n_kpts=36, n_lines=14, gnn=["self", "cross"] * 2, inter=[0], seed=43,
                  line_attention=True)
    gen_lightglue_sift("lightglue_sift", 2, 150, 121, 2, seed=191)
    gen_matcher_options()
    gen_superglue_config("superglue_sharp", 2, 2048, 100, seed=151, sharp=(0.01, 16.0, 0.03, 0.125))
    gen_gluestick_config("gluestick_sharp", 2, 2048, 512, seed=157, sharp=(0.01, 16.0, 0.03, 0.125))


if __name__ == "__main__":
    main()
