"""A torch restatement of the published ``deform_conv2d`` (groups 1, stride 1, dilation 1), written independently of
glue_factory_amd.extractors.aliked.deform_cols: every tap is one ``grid_sample`` with zero padding and
``align_corners=True`` at pixel coordinates, which is the same rule -- a corner outside the map contributes nothing, and a
point at or beyond -1 / H / W has no corner inside."""
import torch
import torch.nn.functional as F


def deform_conv2d(input, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None):
    pad = padding if isinstance(padding, int) else padding[0]
    b, c, h, w = input.shape
    c_out, _, kh, kw = weight.shape
    assert offset.shape == (b, 2 * kh * kw, h + 2 * pad - kh + 1, w + 2 * pad - kw + 1)
    ho, wo = offset.shape[-2:]
    ys = torch.arange(ho, dtype=input.dtype, device=input.device).view(1, ho, 1)
    xs = torch.arange(wo, dtype=input.dtype, device=input.device).view(1, 1, wo)
    out = input.new_zeros(b, c_out, ho, wo)
    for k in range(kh * kw):
        py = ys - pad + k // kw + offset[:, 2 * k]
        px = xs - pad + k % kw + offset[:, 2 * k + 1]
        grid = torch.stack([2 * px / max(w - 1, 1) - 1, 2 * py / max(h - 1, 1) - 1], dim=-1)
        tap = F.grid_sample(input, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        if mask is not None:
            tap = tap * mask[:, k:k + 1]
        out = out + torch.einsum("oc,bchw->bohw", weight[:, :, k // kw, k % kw], tap)
    return out if bias is None else out + bias.view(1, -1, 1, 1)
