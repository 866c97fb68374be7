"""ALIKED extractor (frozen, inference only) -- two paths, like superpoint_open.py.

Interface, defaults, the four layouts and the ``state_dict`` names / shapes are those of
gluefactory/models/extractors/aliked.py, so the published ``aliked-*.pth`` files load with ``strict=True``:
``{"image"} -> {"keypoints" (pixels, wh (k + 1) / 2, no +0.5), "descriptors", "keypoint_scores", "score_dispersity",
"score_map"}``.

* Stock path (any device): library convolutions and torch ops, the reference's formulation op for op, with the per-image
  python loops of DKD batched.  ``deform_cols`` below restates torchvision's ``deform_conv2d`` sampling (groups 1, stride
  1, dilation 1, no mask); this module never imports torchvision.
* Fused path (HIP device, eval BatchNorm, no gradient wanted): csrc/aliked.hip through extractors/aliked_kernels.py --
  gf_ak_deform_cols (blocks 3 and 4), gf_ak_aggregate (feature aggregation, normalisation and the score head's first
  layer in one pass: no upsampled map, concatenation or un-normalised copy is written), gf_ak_dkd_refine (25 score
  values per KEYPOINT instead of an unfold of the map) and gf_ak_sddh (patch gather, offsets, M samples, sf_conv and the
  agg_weights contraction on fp32 MFMA tiles, per tile of keypoints).  NMS + top-k reuse the SuperPoint path's
  gf_nms_candidates / gf_topk_candidates where their contracts fit (radius 1..4, k <= min(4096, cap)), else torch ops.
  The values that decide an integer (the keypoint position p = (k / 2 + 0.5) (w - 1, h - 1) that SDDH truncates) are
  computed here in torch, in the reference's operation order, and passed to the kernel.

Differences in HOW: top-k mode (``detection_threshold <= 0`` and ``max_num_keypoints > 0``) is batched without a host read;
``image_size`` zeroes the border through a device tensor of limits.  Threshold mode keeps the stock selection (with the
``masks.sum() == 0`` fallback and the n_limit sort) and raises BatchedExtractionUnsupported when the images of a batch yield
different counts.  One deliberate difference in WHAT: with ``image_size`` the reference decodes the flat indices of every
image with the LAST image's width; here they are decoded with the width of the map, which is the same whenever the
last image fills the tensor.  The module never downloads: ``pretrained: true`` needs ``weights: <path>``.
"""
from pathlib import Path

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..base_model import BaseModel, BatchedExtractionUnsupported
from .superpoint_open import batched_nms


def deform_cols(x, offset, pad=1):
    """Column matrix [B, C * 9, H * W] of a 3 x 3 deformable convolution: for tap k = ky * 3 + kx the sample point is
    (y - pad + ky + offset[2k], x - pad + kx + offset[2k + 1]); 0 at py <= -1, py >= H, px <= -1 or px >= W, else bilinear
    on the floor corners, each corner counted only if it lies inside the map."""
    b, c, h, w = x.shape
    k = torch.arange(9, device=x.device)
    ys = torch.arange(h, device=x.device, dtype=x.dtype).view(1, 1, h, 1) - pad + (k // 3).to(x.dtype).view(1, 9, 1, 1)
    xs = torch.arange(w, device=x.device, dtype=x.dtype).view(1, 1, 1, w) - pad + (k % 3).to(x.dtype).view(1, 9, 1, 1)
    off = offset.reshape(b, 9, 2, h, w)
    py, px = ys + off[:, :, 0], xs + off[:, :, 1]
    inside = (py > -1) & (py < h) & (px > -1) & (px < w)
    fy, fx = py.floor(), px.floor()
    ly, lx = py - fy, px - fx
    y0, x0 = fy.long(), fx.long()
    flat = x.reshape(b, c, h * w)

    def corner(yy, xx, wgt):
        ok = inside & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(b, 1, -1).expand(b, c, -1)
        return flat.gather(2, idx).view(b, c, 9, h, w) * (wgt * ok).unsqueeze(1)

    cols = (corner(y0, x0, (1 - ly) * (1 - lx)) + corner(y0, x0 + 1, (1 - ly) * lx)
            + corner(y0 + 1, x0, ly * (1 - lx)) + corner(y0 + 1, x0 + 1, ly * lx))
    return cols.reshape(b, c * 9, h * w)


def _scale_xy(t, sx, sy):
    """t [..., 2] * (sx, sy) without a host -> device copy of the pair (a captured graph cannot hold one)."""
    return torch.stack([t[..., 0] * sx, t[..., 1] * sy], dim=-1)


class DeformableConv2d(nn.Module):
    """3 x 3 deformable convolution without mask: offsets from a plain convolution, clamped to +-max(h, w) / 4."""

    def __init__(self, c_in, c_out):
        super().__init__()
        self.offset_conv = nn.Conv2d(c_in, 18, 3, padding=1, bias=True)
        self.regular_conv = nn.Conv2d(c_in, c_out, 3, padding=1, bias=False)

    def forward(self, x, fused=False):
        b, _, h, w = x.shape
        lim = max(h, w) / 4.0
        offset = self.offset_conv(x).clamp(-lim, lim)
        if fused:
            from . import aliked_kernels
            cols = aliked_kernels.deform_cols(x, offset)
        else:
            cols = deform_cols(x, offset)
        wgt = self.regular_conv.weight
        return torch.matmul(wgt.reshape(wgt.shape[0], -1), cols).view(b, -1, h, w)


def _conv3(c_in, c_out, dcn):
    return DeformableConv2d(c_in, c_out) if dcn else nn.Conv2d(c_in, c_out, 3, padding=1, bias=False)


def _run(conv, x, fused):
    return conv(x, fused) if isinstance(conv, DeformableConv2d) else conv(x)


class ConvBlock(nn.Module):
    def __init__(self, c_in, c_out):
        super().__init__()
        self.conv1, self.bn1 = _conv3(c_in, c_out, False), nn.BatchNorm2d(c_out)
        self.conv2, self.bn2 = _conv3(c_out, c_out, False), nn.BatchNorm2d(c_out)

    def forward(self, x, fused=False):
        x = F.selu(self.bn1(self.conv1(x)))
        return F.selu(self.bn2(self.conv2(x)))


class ResBlock(nn.Module):
    def __init__(self, c_in, c_out, dcn):
        super().__init__()
        self.conv1, self.bn1 = _conv3(c_in, c_out, dcn), nn.BatchNorm2d(c_out)
        self.conv2, self.bn2 = _conv3(c_out, c_out, dcn), nn.BatchNorm2d(c_out)
        self.downsample = nn.Conv2d(c_in, c_out, 1)

    def forward(self, x, fused=False):
        out = F.selu(self.bn1(_run(self.conv1, x, fused)))
        out = self.bn2(_run(self.conv2, out, fused))
        return F.selu(out + self.downsample(x))


class SDDH(nn.Module):
    """Sparse deformable descriptor head: parameters only; the arithmetic is ALIKED._describe_* below."""

    def __init__(self, dim, K, M):
        super().__init__()
        self.kernel_size, self.n_pos = K, M
        self.offset_conv = nn.Sequential(nn.Conv2d(dim, 2 * M, K, bias=True), nn.SELU(), nn.Conv2d(2 * M, 2 * M, 1, bias=True))
        self.sf_conv = nn.Conv2d(dim, dim, 1, bias=False)
        self.agg_weights = nn.Parameter(torch.rand(M, dim, dim))


class ALIKED(BaseModel):
    default_conf = {
        "model_name": "aliked-n16",
        "max_num_keypoints": -1,
        "detection_threshold": 0.2,
        "force_num_keypoints": False,
        "pretrained": True,
        "nms_radius": 2,
        "weights": None,        # local path of an aliked-*.pth file (pretrained: true never downloads)
    }
    n_limit_max = 20000
    temperature = 0.1
    cfgs = {
        "aliked-t16": {"c1": 8, "c2": 16, "c3": 32, "c4": 64, "dim": 64, "K": 3, "M": 16},
        "aliked-n16": {"c1": 16, "c2": 32, "c3": 64, "c4": 128, "dim": 128, "K": 3, "M": 16},
        "aliked-n16rot": {"c1": 16, "c2": 32, "c3": 64, "c4": 128, "dim": 128, "K": 3, "M": 16},
        "aliked-n32": {"c1": 16, "c2": 32, "c3": 64, "c4": 128, "dim": 128, "K": 3, "M": 32},
    }
    required_data_keys = ["image"]
    batchable_views = True

    def _init(self, conf):
        if conf.force_num_keypoints:
            assert conf.detection_threshold <= 0 and conf.max_num_keypoints > 0
        if conf.get("mask") or conf.get("conv2D"):
            raise ValueError("ALIKED: the mask / conv2D arms are used by no layout and are not built")
        cfg = self.cfgs[conf.model_name]
        c1, c2, c3, c4, dim = cfg["c1"], cfg["c2"], cfg["c3"], cfg["c4"], cfg["dim"]
        self.dim, self.K, self.M = dim, cfg["K"], cfg["M"]
        self.block1 = ConvBlock(3, c1)
        self.block2 = ResBlock(c1, c2, False)
        self.block3 = ResBlock(c2, c3, True)
        self.block4 = ResBlock(c3, c4, True)
        self.conv1 = nn.Conv2d(c1, dim // 4, 1, bias=False)
        self.conv2 = nn.Conv2d(c2, dim // 4, 1, bias=False)
        self.conv3 = nn.Conv2d(c3, dim // 4, 1, bias=False)
        self.conv4 = nn.Conv2d(dim, dim // 4, 1, bias=False)
        self.score_head = nn.Sequential(
            nn.Conv2d(dim, 8, 1, bias=False), nn.SELU(),
            nn.Conv2d(8, 4, 3, padding=1, bias=False), nn.SELU(),
            nn.Conv2d(4, 4, 3, padding=1, bias=False), nn.SELU(),
            nn.Conv2d(4, 1, 3, padding=1, bias=False))
        self.desc_head = SDDH(dim, self.K, self.M)
        self.top_k = -1 if conf.detection_threshold > 0 else conf.max_num_keypoints
        self.n_limit = conf.max_num_keypoints if conf.max_num_keypoints > 0 else self.n_limit_max
        if conf.pretrained:
            if not conf.weights:
                raise ValueError("ALIKED: `pretrained: true` needs `weights: <path of aliked-*.pth>`; nothing is downloaded")
            path = Path(conf.weights)
            if not path.exists():
                raise FileNotFoundError(f"ALIKED weights '{conf.weights}' not found locally")
            self.load_state_dict(torch.load(str(path), map_location="cpu"), strict=True)

    # ------------------------------------------------------------------ dense maps
    def _use_fused(self, image):
        if not image.is_cuda or image.dtype != torch.float32 or not 1 <= self.conf.nms_radius <= 4:
            return False
        if any(m.training for m in self.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)):
            return False
        return not (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()))

    def _dense(self, image, fused):
        """(feature map, score map [B,1,H,W]); the feature map is [B,dim,H,W] (stock) or channels-last [B,H,W,dim] (fused)."""
        h, w = image.shape[-2:]
        ph, pw = (-h) % 32, (-w) % 32
        left, top = pw // 2, ph // 2
        x = F.pad(image, [left, pw - left, top, ph - top], mode="replicate")
        x1 = self.block1(x)
        x2 = self.block2(F.avg_pool2d(x1, 2, 2))
        x3 = self.block3(F.avg_pool2d(x2, 4, 4), fused)
        x4 = self.block4(F.avg_pool2d(x3, 4, 4), fused)
        g2, g3, g4 = F.selu(self.conv2(x2)), F.selu(self.conv3(x3)), F.selu(self.conv4(x4))
        if fused:
            from . import aliked_kernels
            feat, s8 = aliked_kernels.aggregate(x1, g2, g3, g4, self.conv1.weight, self.score_head[0].weight, top, left, h, w)
            score = torch.sigmoid(self.score_head[2:](s8))
        else:
            def up(t, s):
                return F.interpolate(t, scale_factor=s, mode="bilinear", align_corners=True)
            x1234 = torch.cat([F.selu(self.conv1(x1)), up(g2, 2), up(g3, 8), up(g4, 32)], dim=1)
            score = torch.sigmoid(self.score_head(x1234))
            feat = F.normalize(x1234, p=2, dim=1)[..., top:top + h, left:left + w]
        return feat, score[..., top:top + h, left:left + w].contiguous()

    # ------------------------------------------------------------------ detection
    def _limits(self, data, b, h, w, device):
        size = data.get("image_size")
        if size is None:
            return w, h
        size = size.to(device).long()
        return size[:, 0].view(b, 1, 1), size[:, 1].view(b, 1, 1)

    def _border(self, b, h, w, wl, hl, device):
        r = self.conf.nms_radius
        ys = torch.arange(h, device=device).view(1, h, 1)
        xs = torch.arange(w, device=device).view(1, 1, w)
        return (ys < r) | (xs < r) | (ys >= hl - r) | (xs >= wl - r)

    def _select(self, score, data, fused):
        """Flat pixel indices [B, N] of the selected NMS maxima."""
        conf = self.conf
        b, _, h, w = score.shape
        r = conf.nms_radius
        wl, hl = self._limits(data, b, h, w, score.device)
        sized = data.get("image_size") is not None
        if self.top_k > 0 and fused and h * w < 2 ** 31:
            from .. import lib as _lib
            L = _lib.load()
            cap = L.gf_nms_candidates_cap(h, w, r)
            if self.top_k <= min(4096, cap):
                st = torch.cuda.current_stream().cuda_stream
                cand_s = torch.full((b, cap), -1.0, dtype=torch.float32, device=score.device)
                cand_i = torch.zeros((b, cap), dtype=torch.int32, device=score.device)
                _lib.check(L.gf_nms_candidates(score.data_ptr(), cand_s.data_ptr(), cand_i.data_ptr(), b, h, w, r, r, st),
                           "gf_nms_candidates")
                if sized:
                    ci = cand_i.long()
                    out = (ci % w >= wl.view(b, 1) - r) | (ci // w >= hl.view(b, 1) - r)
                    cand_s = torch.where(out, torch.full_like(cand_s, -1.0), cand_s)
                ind = torch.empty((b, self.top_k), dtype=torch.int64, device=score.device)
                ksc = torch.empty((b, self.top_k), dtype=torch.float32, device=score.device)
                _lib.check(L.gf_topk_candidates(cand_s.data_ptr(), cand_i.data_ptr(), ksc.data_ptr(), ind.data_ptr(), b, cap,
                                                self.top_k, st), "gf_topk_candidates")
                return ind
        nms = batched_nms(score.detach(), r)[:, 0]
        nms = nms.masked_fill(self._border(b, h, w, wl, hl, score.device), 0.0)
        if self.top_k > 0:
            return torch.topk(nms.reshape(b, -1), self.top_k).indices
        flat = score.detach().reshape(b, -1)
        if conf.detection_threshold > 0:
            masks = nms > conf.detection_threshold
            if masks.sum() == 0:
                masks = nms > flat.mean(dim=1).view(b, 1, 1)
        else:
            masks = nms > flat.mean(dim=1).view(b, 1, 1)
        picked = []
        for mask, sc in zip(masks.reshape(b, -1), flat):
            ind = mask.nonzero()[:, 0]
            if len(ind) > self.n_limit:
                ind = ind[sc[ind].sort(descending=True)[1][:self.n_limit]]
            picked.append(ind)
        if len({len(i) for i in picked}) != 1:
            raise BatchedExtractionUnsupported("images yield different keypoint counts: use top-k mode "
                                               "(detection_threshold <= 0 with max_num_keypoints)")
        return torch.stack(picked)

    def _refine_stock(self, score, ind):
        """Soft-argmax refinement, dispersity and the bilinear score of keypoints `ind` [B, N] -> normalised xy in [-1, 1]."""
        b, _, h, w = score.shape
        r = self.conf.nms_radius
        ks = 2 * r + 1
        d = torch.arange(ks, device=score.device)
        x0, y0 = ind % w, torch.div(ind, w, rounding_mode="trunc")
        yy = y0[..., None, None] + d.view(1, 1, ks, 1)
        xx = x0[..., None, None] + d.view(1, 1, 1, ks)
        padded = F.pad(score[:, 0], (r, r, r, r)).reshape(b, -1)
        patch = padded.gather(1, (yy * (w + 2 * r) + xx).reshape(b, -1)).view(b, -1, ks * ks)
        grid = torch.stack([(d - r).view(1, ks).expand(ks, ks), (d - r).view(ks, 1).expand(ks, ks)], -1).reshape(-1, 2).to(score)
        x_exp = ((patch - patch.max(dim=-1, keepdim=True).values) / self.temperature).exp()
        total = x_exp.sum(dim=-1, keepdim=True)
        residual = x_exp @ grid / total
        dist2 = torch.norm((grid[None, None] - residual[:, :, None]) / r, dim=-1) ** 2
        dispersity = (x_exp * dist2).sum(dim=-1) / total[..., 0]
        wh = torch.tensor([w - 1, h - 1], device=score.device)
        kxy = (torch.stack([x0, y0], dim=-1) + residual) / wh * 2 - 1
        kscore = F.grid_sample(score, kxy.view(b, 1, -1, 2), mode="bilinear", align_corners=True)[:, 0, 0]
        return kxy, kscore, dispersity

    # ------------------------------------------------------------------ description
    def _describe_stock(self, feat, kxy):
        head = self.desc_head
        b, c, h, w = feat.shape
        K, M = self.K, self.M
        wh = torch.tensor([[w - 1, h - 1]], device=feat.device)
        lim = max(h, w) / 4.0
        d = torch.arange(K, device=feat.device)
        out = []
        for xi, ki in zip(feat, kxy):
            n = len(ki)
            p = (ki / 2 + 0.5) * wh
            pl = p.long()
            if K > 1:
                corner = (pl - K / 2 + 1).long()
                cx = corner[:, 0].clamp(min=0, max=w - 1 - K)
                cy = corner[:, 1].clamp(min=0, max=h - 1 - K)
                patch = xi[:, (cy[:, None, None] + d.view(1, K, 1)), (cx[:, None, None] + d.view(1, 1, K))].permute(1, 0, 2, 3)
            else:
                patch = xi[:, pl[:, 1], pl[:, 0]].permute(1, 0).reshape(n, c, 1, 1)
            offset = head.offset_conv(patch).clamp(-lim, lim)[:, :, 0, 0].view(n, 2, M).permute(0, 2, 1)
            pos = 2.0 * (p.unsqueeze(1) + offset) / wh[None] - 1
            sampled = F.grid_sample(xi.unsqueeze(0), pos.reshape(1, n * M, 1, 2), mode="bilinear", align_corners=True)
            sampled = sampled.reshape(c, n, M, 1).permute(1, 0, 2, 3)
            sampled = F.selu(head.sf_conv(sampled)).squeeze(-1)
            out.append(F.normalize(torch.einsum("ncp,pcd->nd", sampled, head.agg_weights), p=2.0, dim=1))
        return torch.stack(out)

    def _forward(self, data):
        image = data["image"]
        fused = self._use_fused(image)
        feat, score = self._dense(image.contiguous() if fused else image, fused)
        ind = self._select(score, data, fused)
        if fused:
            from . import aliked_kernels
            kxy, kscore, dispersity = aliked_kernels.dkd_refine(score, ind, self.conf.nms_radius, self.temperature)
            h, w = score.shape[-2:]
            p = _scale_xy(kxy / 2 + 0.5, w - 1, h - 1)       # the reference's order: SDDH truncates it
            descriptors = aliked_kernels.sddh(feat, p, self._sddh_weights(), self.K, self.M)
        else:
            kxy, kscore, dispersity = self._refine_stock(score, ind)
            descriptors = self._describe_stock(feat, kxy)
        h, w = image.shape[-2:]
        return {"keypoints": _scale_xy(kxy + 1, w - 1, h - 1) / 2.0, "descriptors": descriptors, "keypoint_scores": kscore,
                "score_dispersity": dispersity, "score_map": score}

    def _sddh_weights(self):
        """The head's weights in the kernel's layouts, rebuilt when a parameter changed: offset_conv.0 as [2M][tap][c]
        (the patch is read channels-last), agg_weights as [m][d][c] (8 consecutive c per MFMA operand lane)."""
        head = self.desc_head
        tensors = list(head.parameters())
        key = (tuple(t._version for t in tensors), tuple(t.data_ptr() for t in tensors))
        cache = self.__dict__.get("_sddh_cache")
        if cache is not None and cache[0] == key:
            return cache[1]
        c0, c2 = head.offset_conv[0], head.offset_conv[2]
        w = {"w1": c0.weight.detach().permute(0, 2, 3, 1).reshape(c0.out_channels, -1).contiguous(),
             "b1": c0.bias.detach().contiguous(),
             "w2": c2.weight.detach().reshape(c2.out_channels, -1).contiguous(), "b2": c2.bias.detach().contiguous(),
             "sf": head.sf_conv.weight.detach().reshape(self.dim, self.dim).contiguous(),
             "agg": head.agg_weights.detach().permute(0, 2, 1).contiguous()}
        self.__dict__["_sddh_cache"] = (key, w)
        return w

    def loss(self, pred, data):
        raise NotImplementedError


__main_model__ = ALIKED
