"""Parity of the frozen SuperPoint extractor AT THE BENCHMARKED GEOMETRY (bench.py scope P: bf16 autocast, 64 images of
1024 x 1024 = 32 uniform-noise images + their 32 homography-warped views, max_num_keypoints 2048, force_num_keypoints,
detection_threshold 0, nms_radius 3, borders 4): the shapes, tile orders and index ranges that only this geometry reaches.

  A. the HIP kernels at the benchmarked shapes against fp64 on the kernels' own bf16 inputs, elementwise bounds derived
     from where each kernel rounds; the 32-tile-row column skew of gf_conv3x3_c64 (csrc/conv3x3.hip, W % 1024 == 0), the
     largest image it accepts (32-bit byte offsets), and batch consistency of the B = 64 launch chain (images on either
     side of the 2^31-element mark bit-identical to B = 1 launches);
  B. block-by-block parity through SuperPoint._fused_features itself (the real dispatch, teacher-forced: every block
     against fp64 of that block on its own recorded bf16 input), open and non-free variants;
  C. NMS candidates + top-k + descriptor sampling on the fused path's own score / descriptor maps against the stock chain
     of the module's non-fused branch, and one end-to-end check of the bf16 fused module against the fp32 stock modules.

Rounding model used by every bound below.  fp32 unit roundoff u = 2^-24; bf16 keeps 8 significand bits, so rounding a
value v to bf16 (round to nearest even) moves it by at most 2^-8 |v| (half of the 2^-7 relative spacing; bf16 has the
fp32 exponent range, ATOL covers flushed subnormals).  A sum of n terms accumulated in fp32 in ANY order is within
(n - 1) u sum|terms| (+ O(u^2)) of the exact sum; bf16 x bf16 products are exact in fp32 (16 significand bits).  For a
block  out = bf16( relu(sum_k x_k w_k + b) s + h )  computed in fp32 that gives

    |out - ref| <= 2^-8 |ref| + (1 + 2^-8) ( |s| n u (sum_k |x_k w_k| + |b|) + 2 u (|relu(.) s| + |h|) )

with n = taps * c_in + 1 (the tail's add and fma round once each).  A 2x2 max-pool of bf16 values is exact, and
|max a' - max a| <= max |a' - a|: the pooled bound is the max-pool of the bound.  Where the library convolution writes a
bf16 intermediate before the tail, its rounding (2^-8 |conv|) enters scaled by |s| as well; its internal reduction order
and precision are not ours (measured: up to 1.5x the single-rounding bound), so library blocks also allow one bf16
rounding of the sum of |terms| (2^-8 sum |x w|).
"""
import time

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                  # fp32 unit roundoff
UB = 2.0 ** -8                  # bf16 unit roundoff
ATOL = 2.0 ** -126              # flushed subnormals
IMG = 1024
KPTS = 2048
BENCH_CONF = {"max_num_keypoints": KPTS, "force_num_keypoints": True, "detection_threshold": 0.0, "nms_radius": 3,
              "remove_borders": 4}


@pytest.fixture(scope="module", autouse=True)
def _report_time_and_memory():
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"\n  {__name__}: {time.time() - t0:.1f} s, peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from glue_factory_amd import lib
    return lib


def _ratio(err, bound):
    """max(err / bound), NaN (an unwritten output) counted as infinite."""
    r = err / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def _check(tag, out, ref, bound):
    err = (out.double() - ref).abs()
    q = _ratio(err, bound)
    print(f"  {tag}: max err / bound = {q:.3f}  (max err {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e})")
    assert q <= 1.0, f"{tag}: error exceeds its bound by {q:.3f}x"
    return q


# ------------------------------------------------------------------------------------------------ inputs (bench.py recipe)
def bench_images(batch, seed=7, img=IMG):
    """bench.py scope_p_inputs: `batch` images ~U(0,1) and their homography-warped views (bilinear, zeros outside the
    warp), as [2 batch, 1, img, img] fp32: the uniform images first."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    img0 = torch.rand(batch, 1, img, img, device="cuda", generator=g)
    side = float(img)
    src = torch.tensor([[0.0, 0.0], [side, 0.0], [side, side], [0.0, side]], device="cuda")[None].repeat(batch, 1, 1)
    dst = src + (torch.rand(batch, 4, 2, device="cuda", generator=g) - 0.5) * 0.24 * side
    x, y, u, v = src[..., 0].double(), src[..., 1].double(), dst[..., 0].double(), dst[..., 1].double()
    z, o = torch.zeros_like(x), torch.ones_like(x)
    A = torch.cat([torch.stack([x, y, o, z, z, z, -u * x, -u * y], -1), torch.stack([z, z, z, x, y, o, -v * x, -v * y], -1)], 1)
    h = torch.linalg.solve(A, torch.cat([u, v], 1)[..., None])[..., 0]
    H = torch.cat([h, torch.ones(batch, 1, device="cuda", dtype=torch.float64)], 1).reshape(batch, 3, 3)
    ys, xs = torch.meshgrid(torch.arange(img, device="cuda", dtype=torch.float64) + 0.5,
                            torch.arange(img, device="cuda", dtype=torch.float64) + 0.5, indexing="ij")
    p1 = torch.stack([xs, ys, torch.ones_like(xs)], -1).reshape(1, -1, 3)
    p0 = p1 @ torch.linalg.inv(H).transpose(1, 2)
    p0 = p0[..., :2] / p0[..., 2:]
    grid = (p0 / side * 2 - 1).reshape(batch, img, img, 2).float()
    img1 = F.grid_sample(img0, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return torch.cat([img0, img1], 0).contiguous()


def _bn_eval_stats(model, seed):
    """Non-trivial eval BatchNorm: running statistics of one bench-style image (train mode, momentum=None = the plain
    average), then random affine weights around 1 and biases around 0 -- scale != 1 and shift != 0 in every fused tail."""
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    if not bns:
        return
    for m in bns:
        m.momentum = None
        m.reset_running_stats()
    model.train()
    with torch.no_grad():
        model._dense_unfused(bench_images(1, seed=seed)[:1])
        g = torch.Generator(device="cuda").manual_seed(seed)
        for m in bns:
            m.weight.copy_(1 + 0.3 * torch.randn(m.weight.shape, device="cuda", generator=g))
            m.bias.copy_(0.2 * torch.randn(m.bias.shape, device="cuda", generator=g))
    model.eval()


def make_model(kind, seed=0, **conf):
    if kind == "open":
        from glue_factory_amd.extractors.superpoint_open import SuperPoint
    else:
        from glue_factory_amd.extractors.superpoint import SuperPoint
    torch.manual_seed(seed)
    model = SuperPoint({**BENCH_CONF, "weights": None, **conf}).cuda().eval()
    for p in model.parameters():
        p.requires_grad_(False)
    _bn_eval_stats(model, seed + 11)
    return model


# ------------------------------------------------------------------------------------------------ fp64 references
def conv_fp64(x, w, rows=None):
    """Zero-padded stride-1 convolution in fp64 on channels-last activations: x [B, H, W, Cin] (any dtype, converted
    exactly), w [Cout, Cin, k, k] -> (sum, sum of |terms|) [B, r1 - r0, W, Cout] for output rows rows = (r0, r1)."""
    B, H, W, C = x.shape
    k = w.shape[-1]
    p = k // 2
    r0, r1 = rows if rows is not None else (0, H)
    lo, hi = max(r0 - p, 0), min(r1 + p, H)
    xp = torch.zeros(B, r1 - r0 + 2 * p, W + 2 * p, C, dtype=torch.float64, device=x.device)
    xp[:, lo - (r0 - p):hi - (r0 - p), p:p + W] = x[:, lo:hi].double()
    wd = w.double()
    acc = torch.zeros(B, r1 - r0, W, w.shape[0], dtype=torch.float64, device=x.device)
    aab = torch.zeros_like(acc)
    for dy in range(k):
        for dx in range(k):
            sl = xp[:, dy:dy + r1 - r0, dx:dx + W]
            wt = wd[:, :, dy, dx].t()
            acc += sl @ wt
            aab += sl.abs() @ wt.abs()
    return acc, aab


def tail_fp64(acc, aab, bias, scale, shift, relu, n, pre_bf16=False, bn=None):
    """(ref, bound) of  [bf16](relu(acc + bias) * scale + shift)  per the rounding model of the module docstring.
    pre_bf16: the convolution output was rounded to bf16 before the tail (library convolution).  bn: the BatchNorm the
    fp32 scale / shift were folded from (the fold's own rounding, a few u, is added)."""
    b = bias.double()
    a = acc + b
    pre = torch.relu(a) if relu else a
    s, h = scale.double(), shift.double()
    ref = pre * s + h
    e_acc = n * U * (aab + b.abs())
    if pre_bf16:        # the library may round to bf16 inside its reduction as well: up to 2^-8 sum |terms| more
        e_acc = e_acc + UB * (acc.abs() + e_acc) + UB * aab
    d = s.abs() * e_acc + 2 * U * ((pre * s).abs() + h.abs())
    if bn is not None:
        d = d + 4 * U * ((pre * s).abs() + (bn.running_mean.double() * s).abs() + bn.bias.double().abs())
    return ref, UB * ref.abs() + (1 + UB) * d + ATOL


def bn_affine(blk):
    if blk.bn is None:
        return torch.ones(blk.conv.out_channels, dtype=torch.float64, device="cuda"), \
            torch.zeros(blk.conv.out_channels, dtype=torch.float64, device="cuda")
    bn = blk.bn
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return s, bn.bias.double() - bn.running_mean.double() * s


def pool_fp64(t):
    """2x2 max-pool of a [B, H, W, C] fp64 tensor."""
    return F.max_pool2d(t.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)


def softmax_scores_fp64(z, rel_z):
    """Score map of the detector tail from the fp64 logits z [B, h, w, 65] and a per-logit error bound rel_z (absolute,
    same shape): p = softmax(z)[..., :64] unfolded to [B, 8h, 8w] and its bound.  An error d_j in logit j moves
    p_i by a factor within exp(d_i - max_j d_j) .. exp(d_i + max_j d_j): |dp_i| <= p_i (2 max_j d_j) (1 + 2 max d);
    fp32 itself adds the subtraction of the max (u |z - m|, into d), expf (<= 2 ulp = 2^-22 relative, numerator and
    denominator), the 65-term sum (64 u) and the division (u)."""
    B, h, w, _ = z.shape
    m = z.max(-1, keepdim=True).values
    p = torch.softmax(z, -1)[..., :64]
    d = (rel_z + U * (z - m).abs()).amax(-1, keepdim=True)
    rel = 2 * d * (1 + 2 * d) + 2 * 2.0 ** -22 + 66 * U
    bound = p * rel + ATOL
    unfold = lambda t: t.reshape(B, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, h * 8, w * 8)     # noqa: E731
    return unfold(p), unfold(bound)


def sample_fp64(kp, dmap):
    """Descriptors at integer pixel keypoints kp [B, N, 2] (x, y) of the channels-last map dmap [B, h, w, C] (stride 8):
    the per-pixel-normalised map sampled bilinearly at (kp + 0.5) / 8 - 0.5 (zero padding), normalised again -- in fp64,
    with the bound of the fp32 kernel: its two normalisations (a 256-term sum of squares, sqrt, divide) and the
    4-neighbour weighted sum each err by a few tens of u relative to the vectors they act on; relative to the output
    that is amplified by K = (sum of in-range weights) / |unnormalised sample| when the neighbours cancel."""
    from glue_factory_amd.extractors.superpoint_open import sample_descriptors
    m = dmap.permute(0, 3, 1, 2).double()
    mn = F.normalize(m, p=2, dim=1)
    kpd = kp.double()
    ref = sample_descriptors(kpd, mn, 8).transpose(-1, -2)                         # [B, N, C]
    b, c, h, w = mn.shape
    g = ((kpd + 0.5) / (kpd.new_tensor([w, h]) * 8) * 2 - 1).view(b, 1, -1, 2)
    raw = F.grid_sample(mn, g, mode="bilinear", align_corners=False).reshape(b, c, -1)
    mag = F.grid_sample(mn.abs(), g, mode="bilinear", align_corners=False).reshape(b, c, -1)
    wsum = F.grid_sample(torch.ones_like(mn[:, :1]), g, mode="bilinear", align_corners=False).reshape(b, 1, -1)
    nr = raw.norm(dim=1, keepdim=True)
    K = (wsum / nr).transpose(-1, -2)
    bound = 64 * U * (K * ref.abs() + (mag / nr).transpose(-1, -2) + K / c ** 0.5) + ATOL
    return ref, bound


# ------------------------------------------------------------------------------------------------ kernel launches
def launch_c64(x, taps, bias, scale, shift, out_ptr, ldy, pool, relu=1):
    B, H, W, _ = x.shape
    return _lib().load().gf_conv3x3_c64_ld(x.data_ptr(), taps.data_ptr(), bias.data_ptr(), scale.data_ptr(),
                                           shift.data_ptr(), out_ptr, ldy, B, H, W, relu, int(pool), 1, _stream())


def c64_operands(c_out, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(c_out, 64, 3, 3, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(c_out, device="cuda", generator=g) * 0.5
    scale = 1 + 0.5 * torch.randn(c_out, device="cuda", generator=g)
    shift = 0.5 * torch.randn(c_out, device="cuda", generator=g)
    return w, bias, scale, shift


def c64_reference(x, w, bias, scale, shift, pool, rows=None):
    """fp64 (ref, bound) of gf_conv3x3_c64 on x [B, H, W, 64], one image at a time (memory)."""
    refs, bounds = [], []
    for b in range(x.shape[0]):
        acc, aab = conv_fp64(x[b:b + 1], w, rows)
        r, bd = tail_fp64(acc, aab, bias, scale, shift, True, n=9 * 64 + 1)
        del acc, aab
        if pool:
            r, bd = pool_fp64(r), pool_fp64(bd)
        refs.append(r)
        bounds.append(bd)
    return torch.cat(refs), torch.cat(bounds)


# ================================================================================================ A. kernels vs fp64
@pytest.mark.parametrize("shape,pool", [
    ((2, 1024, 1024), False), ((2, 1024, 1024), True),     # backbone.0.1 geometry: 32-tile rows, skew taken
    ((2, 512, 512), False), ((2, 512, 512), True),         # backbone.1.0 / 1.1: 16-tile rows
    ((1, 64, 2048), False),                                # 64-tile rows: skew * ty wraps modulo the row
    ((1, 64, 1056), True),                                 # 33-tile rows: no skew; 264 tiles, not a multiple of 256 workgroups
    ((3, 40, 1024), False),                                # skew restarts per image (5 tile rows per image)
])
def test_conv3x3_c64_bench_shapes_vs_fp64(shape, pool):
    """gf_conv3x3_c64 (csrc/conv3x3.hip: implicit GEMM, persistent 256 workgroups, 8 x 32 tiles whose columns are skewed by
    the tile row on rows of a multiple of 32 tiles) at the benchmark's shapes against fp64 of conv + bias + ReLU +
    BatchNorm affine [+ 2x2 max-pool] on the kernel's own bf16 inputs; NaN-filled output (an unwritten pixel fails)."""
    B, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(H + W + B)
    x = torch.randn(B, H, W, 64, device="cuda", generator=g).to(torch.bfloat16)
    w, bias, scale, shift = c64_operands(64, H * 3 + W)
    taps = w.permute(2, 3, 0, 1).contiguous()
    out = torch.full((B, H // 2, W // 2, 64) if pool else (B, H, W, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert launch_c64(x, taps, bias, scale, shift, out.data_ptr(), 64, pool) == 0
    ref, bound = c64_reference(x, w, bias, scale, shift, pool)
    _check(f"gf_conv3x3_c64 {shape} pool={pool}", out, ref, bound)


@pytest.mark.parametrize("shape", [(2, 256, 256), (1, 64, 1024)])
def test_conv3x3_c64_ld_bench_shapes_vs_fp64(shape):
    """gf_conv3x3_c64_ld (the 64 -> 128 block backbone.2.0 as one launch per half of the output channels, pixel stride
    ldy = 128): the benchmark's 256^2 shape, and a 32-tile row (skew) with the wide output; each launch leaves the other
    half of every pixel untouched (NaN)."""
    B, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(H * 2 + W)
    x = torch.randn(B, H, W, 64, device="cuda", generator=g).to(torch.bfloat16)
    w, bias, scale, shift = c64_operands(128, H + 5 * W)
    out = torch.full((B, H, W, 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    for half in range(2):
        sl = slice(64 * half, 64 * half + 64)
        taps = w[sl].permute(2, 3, 0, 1).contiguous()
        assert launch_c64(x, taps, bias[sl].contiguous(), scale[sl].contiguous(), shift[sl].contiguous(),
                          out.data_ptr() + 128 * half, 128, False) == 0
        if half == 0:
            assert bool(torch.isnan(out[..., 64:]).all())
    ref, bound = c64_reference(x, w, bias, scale, shift, False)
    _check(f"gf_conv3x3_c64_ld {shape}", out, ref, bound)


def test_conv3x3_c64_largest_image_32bit_offsets():
    """gf_conv3x3_c64 on the largest image it accepts (H W 128 < 2^31 bytes): H = 30840, W = 544 -- the bottom halo
    row of the last tile row lies beyond byte offset 2^31 of the image (buffer loads with 32-bit offsets must read it as
    zeros); top and bottom tile rows against fp64 on crops.  The first size past the guard is refused."""
    H, W = 30840, 544
    assert H * W * 128 < 2 ** 31 <= (H * W + W - 33) * 128        # halo row H, column W - 33 of the last tile: past 2^31
    w, bias, scale, shift = c64_operands(64, 99)
    taps = w.permute(2, 3, 0, 1).contiguous()
    small = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    for hh, ww in ((H + 8, W), (H, W + 32)):
        assert hh * ww * 128 >= 2 ** 31
        assert _lib().load().gf_conv3x3_c64(small.data_ptr(), taps.data_ptr(), bias.data_ptr(), scale.data_ptr(),
                                            shift.data_ptr(), small.data_ptr(), 1, hh, ww, 1, 0, 1, None) == -1
    g = torch.Generator(device="cuda").manual_seed(31)
    x = torch.randn(1, H, W, 64, device="cuda", generator=g, dtype=torch.bfloat16)
    out = torch.full((1, H, W, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert launch_c64(x, taps, bias, scale, shift, out.data_ptr(), 64, False) == 0
    for r0, r1 in ((0, 16), (H - 16, H)):
        acc, aab = conv_fp64(x, w, (r0, r1))
        ref, bound = tail_fp64(acc, aab, bias, scale, shift, True, n=9 * 64 + 1)
        _check(f"gf_conv3x3_c64 (1, {H}, {W}) rows {r0}:{r1}", out[:, r0:r1], ref, bound)
    assert not bool(torch.isnan(out).any())
    del x, out
    torch.cuda.empty_cache()


def conv1_reference(img, w, bias, scale, shift, dtype):
    """fp64 (ref, bound) of gf_conv1_bias_act_bn on img [B, H, W] (bf16: exact products, 9 + 1 fp32 additions;
    fp32: the 9 products round as well)."""
    refs, bounds = [], []
    for b in range(img.shape[0]):
        acc, aab = conv_fp64(img[b:b + 1, :, :, None], w)
        r, bd = tail_fp64(acc, aab, bias, scale, shift, True, n=10 if dtype == torch.bfloat16 else 19)
        if dtype == torch.float32:         # fp32 output: no final bf16 rounding (the bound's 2^-8 |ref| term removed)
            bd = bd - UB * r.abs()
        refs.append(r)
        bounds.append(bd)
    return torch.cat(refs), torch.cat(bounds)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_conv1_bias_act_bn_bench_shape_vs_fp64(dtype):
    """gf_conv1_bias_act_bn (backbone.0.0: Conv2d(1, 64, 3) + bias + ReLU + BatchNorm(eval), channels-last out) on
    4 bench-style 1024^2 images (2 uniform, 2 warped with zero regions) against fp64."""
    img = bench_images(2, seed=3)[:, 0].to(dtype).contiguous()
    g = torch.Generator(device="cuda").manual_seed(17)
    w = (torch.randn(64, 1, 3, 3, device="cuda", generator=g) * 0.3).to(dtype)
    bias = torch.randn(64, device="cuda", generator=g) * 0.2
    scale = 1 + 0.5 * torch.randn(64, device="cuda", generator=g)
    shift = 0.5 * torch.randn(64, device="cuda", generator=g)
    B = img.shape[0]
    out = torch.full((B, IMG, IMG, 64), float("nan"), dtype=dtype, device="cuda")
    assert _lib().load().gf_conv1_bias_act_bn(img.data_ptr(), w.data_ptr(), bias.data_ptr(), scale.data_ptr(),
                                              shift.data_ptr(), out.data_ptr(), B, IMG, IMG, 64, 1,
                                              1 if dtype == torch.bfloat16 else 0, _stream()) == 0
    ref, bound = conv1_reference(img, w, bias, scale, shift, dtype)
    _check(f"gf_conv1_bias_act_bn {dtype}", out, ref, bound)


def detector_reference(y, bias, scale, shift, relu):
    """fp64 (scores, bound) of gf_detector_scores on y [B, h, w, 65]: logits z = act(y + b) s + h; fp32 rounds the add
    and the fma (2 u |.| each)."""
    a = y.double() + bias.double()
    if relu:
        a = torch.relu(a)
    z = a * scale.double() + shift.double()
    dz = 2 * U * ((a * scale.double()).abs() + z.abs())
    return softmax_scores_fp64(z, dz)


def test_detector_scores_bench_shape_vs_fp64():
    """gf_detector_scores (detector.1 tail: bias + BatchNorm, softmax over 65 channels, 8 x 8 cells unfolded) at
    [4, 65, 128, 128] -> [4, 1024, 1024] against the fp64 softmax."""
    g = torch.Generator(device="cuda").manual_seed(65)
    y = (torch.randn(4, 128, 128, 65, device="cuda", generator=g) * 3).to(torch.bfloat16)
    bias, scale, shift = (torch.randn(65, device="cuda", generator=g) for _ in range(3))
    out = torch.full((4, IMG, IMG), float("nan"), device="cuda")
    assert _lib().load().gf_detector_scores(y.data_ptr(), bias.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                            out.data_ptr(), 4, 128, 128, 0, 1, _stream()) == 0
    ref, bound = detector_reference(y, bias, scale, shift, False)
    _check("gf_detector_scores [4, 65, 128, 128]", out, ref, bound)


def test_sample_descriptors_bench_shape_vs_fp64():
    """gf_sample_descriptors on a [2, 256, 128, 128] bf16 map at N = 2048 integer pixel keypoints (what the top-k hands
    it), incl. the four extreme pixel centres (0, 0), (1023, 1023), (0, 1023), (1023, 0)."""
    g = torch.Generator(device="cuda").manual_seed(256)
    B, N = 2, KPTS
    m = torch.randn(B, 128, 128, 256, device="cuda", generator=g).to(torch.bfloat16)
    kp = torch.randint(0, IMG, (B, N, 2), device="cuda", generator=g).float()
    kp[:, :4] = torch.tensor([[0.0, 0.0], [1023.0, 1023.0], [0.0, 1023.0], [1023.0, 0.0]], device="cuda")
    out = torch.full((B, N, 256), float("nan"), device="cuda")
    assert _lib().load().gf_sample_descriptors(m.data_ptr(), kp.data_ptr(), out.data_ptr(), B, N, 128, 128, 256, 8, 1,
                                               _stream()) == 0
    ref, bound = sample_fp64(kp, m)
    _check("gf_sample_descriptors [2, 256, 128, 128] N=2048", out, ref, bound)


def _chain(img, ops_):
    """conv1 -> c64 (pool) -> detector scores -> NMS candidates -> top-k -> descriptor sampling on a batch of images
    [B, H, W] bf16, every launch of the batch as a whole; the detector / descriptor inputs are exact (batch-independent)
    re-arrangements of the pooled activation.  Returns every intermediate."""
    lib = _lib().load()
    w1, b1, s1, h1, w2, b2, s2, h2, bd, sd, hd = ops_
    B, H, W = img.shape
    a1 = torch.empty(B, H, W, 64, dtype=torch.bfloat16, device="cuda")
    assert lib.gf_conv1_bias_act_bn(img.data_ptr(), w1.data_ptr(), b1.data_ptr(), s1.data_ptr(), h1.data_ptr(),
                                    a1.data_ptr(), B, H, W, 64, 1, 1, _stream()) == 0
    a2 = torch.empty(B, H // 2, W // 2, 64, dtype=torch.bfloat16, device="cuda")
    assert launch_c64(a1, w2, b2, s2, h2, a2.data_ptr(), 64, True) == 0
    sub = a2[:, ::4, ::4]                                                     # [B, H / 8, W / 8, 64]
    ydet = torch.cat([sub, sub[..., :1]], -1).contiguous()
    scores = torch.empty(B, H, W, device="cuda")
    assert lib.gf_detector_scores(ydet.data_ptr(), bd.data_ptr(), sd.data_ptr(), hd.data_ptr(), scores.data_ptr(),
                                  B, H // 8, W // 8, 0, 1, _stream()) == 0
    cap = lib.gf_nms_candidates_cap(H, W, 3)
    cs = torch.full((B, cap), -1.0, device="cuda")
    ci = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    assert lib.gf_nms_candidates(scores.data_ptr(), cs.data_ptr(), ci.data_ptr(), B, H, W, 3, 4, _stream()) == 0
    ks = torch.empty(B, KPTS, device="cuda")
    ki = torch.empty(B, KPTS, dtype=torch.int64, device="cuda")
    assert lib.gf_topk_candidates(cs.data_ptr(), ci.data_ptr(), ks.data_ptr(), ki.data_ptr(), B, cap, KPTS, _stream()) == 0
    kp = torch.stack([ki % W, ki // W], -1).float().contiguous()
    dmap = torch.cat([sub, -sub, sub * 2, sub * 0.5], -1).contiguous()       # [B, H / 8, W / 8, 256], exact in bf16
    desc = torch.empty(B, KPTS, 256, device="cuda")
    assert lib.gf_sample_descriptors(dmap.data_ptr(), kp.data_ptr(), desc.data_ptr(), B, KPTS, H // 8, W // 8, 256, 8, 1,
                                     _stream()) == 0
    return {"conv1": a1, "c64": a2, "scores": scores, "cand_s": cs, "cand_i": ci, "topk_s": ks, "topk_i": ki, "desc": desc}


def test_extractor_kernels_batch_consistency_at_b64():
    """The benchmark's launch geometry B = 64 x 1024^2 (64-channel activation = 2^32 elements: images >= 32 lie beyond
    the 2^31-element mark): gf_conv1_bias_act_bn -> gf_conv3x3_c64 (pool) -> gf_detector_scores -> gf_nms_candidates ->
    gf_topk_candidates -> gf_sample_descriptors.  Images 0, 31, 32, 63 of the batch are BIT-identical to B = 1 launches
    of the same images (fixed per-tile summation order: no batch dependence is tolerated)."""
    img = bench_images(32, seed=7)[:, 0].to(torch.bfloat16).contiguous()
    assert img.shape[0] == 64 and 64 * IMG * IMG * 64 == 2 ** 32
    g = torch.Generator(device="cuda").manual_seed(64)
    w1 = (torch.randn(64, 1, 3, 3, device="cuda", generator=g) * 0.3).to(torch.bfloat16)
    w2 = (torch.randn(64, 64, 3, 3, device="cuda", generator=g) * 0.05).to(torch.bfloat16).permute(2, 3, 0, 1).contiguous()
    vec = lambda n, s0, sc: (s0 + sc * torch.randn(n, device="cuda", generator=g))   # noqa: E731
    ops_ = (w1, vec(64, 0, 0.2), vec(64, 1, 0.3), vec(64, 0, 0.3), w2, vec(64, 0, 0.2), vec(64, 1, 0.3), vec(64, 0, 0.3),
            vec(65, 0, 0.5), vec(65, 1, 1.0), vec(65, 0, 0.5))
    big = _chain(img, ops_)
    for b in (0, 31, 32, 63):
        one = _chain(img[b:b + 1].contiguous(), ops_)
        for k, v in one.items():
            assert torch.equal(big[k][b:b + 1], v), f"image {b}: {k} of the B = 64 launch differs from the B = 1 launch"
        assert bool((one["topk_s"] > 0).all())                   # 2048 real maxima per image (no padding)
    del big
    torch.cuda.empty_cache()


# ================================================================================================ B. block by block
EXPECTED_PATH = {"backbone.0.0": "conv1", "backbone.0.1": "c64", "backbone.1.0": "c64", "backbone.1.1": "c64",
                 "backbone.2.0": "c64_ld", "backbone.2.1": "lib", "backbone.3.0": "lib", "backbone.3.1": "lib",
                 "detector.0": "lib", "detector.1": "scores", "descriptor.0": "lib", "descriptor.1": "gemm"}


def record_blocks(model, monkeypatch):
    """Wrap the block methods _fused_features dispatches to: every call appends (name, path, input, output, pool)."""
    rec = []
    paths = {"_first_block": "conv1", "_conv64_block": "c64", "_conv64_wide_block": "c64_ld", "_fused_block": "lib",
             "_detector_scores": "scores"}
    for meth, path in paths.items():
        orig = getattr(model, meth)

        def wrapper(name, blk, x, params, *a, _orig=orig, _path=path, **kw):
            y = _orig(name, blk, x, params, *a, **kw)
            pool = bool(kw.get("pool", a[0] if a else False))
            rec.append((name, _path, x, y, pool))
            return y
        monkeypatch.setattr(model, meth, wrapper)
    orig_ff = model._fused_features
    out = {}

    def ff(image):
        det, desc = orig_ff(image)
        out["det"], out["desc"] = det, desc
        return det, desc
    monkeypatch.setattr(model, "_fused_features", ff)
    return rec, out


def block_reference(model, name, blk, x, path, pool):
    """fp64 (ref, bound) of one block on its recorded bf16 input x (NCHW view of a channels-last tensor)."""
    xl = x.permute(0, 2, 3, 1)                                               # [B, H, W, C]
    # the weights the kernels read: bf16 copies -- except the folded GEMM, compared with the UNFOLDED fp32 block
    w = blk.conv.weight.detach().float() if path == "gemm" else blk.conv.weight.detach().to(torch.bfloat16)
    s, h = bn_affine(blk)
    b0 = blk.conv.bias.detach().double()
    relu = isinstance(blk.activation, torch.nn.ReLU)
    n = w[0].numel() + 1
    refs, bounds = [], []
    for b in range(xl.shape[0]):
        acc, aab = conv_fp64(xl[b:b + 1], w)
        if path == "scores":          # library 1x1 convolution rounded to bf16, then bias / BN / softmax in fp32
            assert not relu
            e = n * U * aab
            a = acc + b0
            z = a * s + h
            dz = s.abs() * (UB * (acc.abs() + aab + e) + e) + 2 * U * ((a * s).abs() + z.abs())
            if blk.bn is not None:
                dz = dz + 4 * U * ((a * s).abs() + (blk.bn.running_mean.double() * s).abs() + blk.bn.bias.double().abs())
            r, bd = softmax_scores_fp64(z, dz)
        else:
            r, bd = tail_fp64(acc, aab, blk.conv.bias.detach(), s, h, relu, n, pre_bf16=(path == "lib"), bn=blk.bn)
            if path == "gemm":          # s w folded in fp32 and rounded to bf16: (2^-8 + u) |s w x| per term; s b + h in fp32
                bd = bd + (1 + UB) * ((UB + 2 * U) * s.abs() * aab + 2 * U * (s * b0).abs())
            if pool:
                r, bd = pool_fp64(r), pool_fp64(bd)
            r, bd = r.permute(0, 3, 1, 2), bd.permute(0, 3, 1, 2)
        refs.append(r)
        bounds.append(bd)
        del acc, aab
    return torch.cat(refs), torch.cat(bounds)


def run_block_parity(kind, monkeypatch):
    model = make_model(kind, seed=5)
    images = bench_images(2, seed=9)                                       # 2 uniform + 2 warped, [4, 1, 1024, 1024]
    rec, out = record_blocks(model, monkeypatch)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert model._use_fused(images)
        model({"image": images})
    blocks = dict(model._named_blocks())
    got = {r[0]: r for r in rec}
    # descriptor.1 went through the folded GEMM (no block call): its input = descriptor.0's output, its output = the map
    assert "descriptor.1" not in got
    got["descriptor.1"] = ("descriptor.1", "gemm", got["descriptor.0"][3], out["desc"], False)
    assert {k: v[1] for k, v in got.items()} == EXPECTED_PATH, f"{kind}: dispatch at 1024^2 changed"
    worst = {}
    for name in EXPECTED_PATH:
        _, path, x, y, pool = got[name]
        if name != "backbone.0.0":
            assert x.dtype == torch.bfloat16
        ref, bound = block_reference(model, name, blocks[name], x if x.dim() == 4 else x[:, None], path, pool)
        worst[name] = _check(f"{kind} {name} [{path}]", y, ref, bound)
    return model, worst


@pytest.mark.parametrize("kind", ["open", "nonfree"])
def test_fused_extractor_blocks_vs_fp64_at_1024(kind, monkeypatch):
    """SuperPoint._fused_features at 1024^2 under bf16 autocast (B = 4 bench-style images): the dispatch picks conv1 /
    c64 / c64_ld / library + tail / detector scores / folded descriptor GEMM per block as expected, and every block's
    output is within its fp64 bound, computed on that block's own recorded bf16 input (teacher forcing)."""
    run_block_parity(kind, monkeypatch)


# ================================================================================================ C. post-processing
def stock_topk(scores, r=3, border=4, k=KPTS):
    """The module's non-fused branch on a given score map: batched_nms, the border writes, torch.topk."""
    from glue_factory_amd.extractors.superpoint_open import batched_nms
    nms = batched_nms(scores.float(), r)
    nms[:, :border] = -1
    nms[:, :, :border] = -1
    nms[:, -border:] = -1
    nms[:, :, -border:] = -1
    ks, ki = torch.topk(nms.reshape(nms.shape[0], -1), k, dim=1, sorted=True)
    return nms, ks, ki


def test_postprocessing_on_fused_maps_at_bench_config(monkeypatch):
    """gf_nms_candidates -> gf_topk_candidates -> gf_sample_descriptors as the module runs them at the bench config
    (B = 64 bench-style images, K = 2048, radius 3, borders 4) against batched_nms + border writes + torch.topk on the
    SAME fused score map: identical scores, identical positions except inside the group tied at the K-th score (compared
    as a subset of that tie group), no positive lost to candidate-segment overflow that could enter the top-k, and the
    descriptors within the fp64 bound of normalise -> bilinear at keypoints / 8 -> normalise."""
    model = make_model("open", seed=1)
    images = bench_images(32, seed=7)
    rec, maps = record_blocks(model, monkeypatch)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        pred = model({"image": images})
    rec.clear()                 # (the recorded B = 64 activations: freed)
    del images
    scores, dmap = maps["det"], maps["desc"]
    B, H, W = scores.shape
    assert (B, H, W) == (64, IMG, IMG)
    lib = _lib().load()
    cap = lib.gf_nms_candidates_cap(H, W, 3)
    cs = torch.full((B, cap), -1.0, device="cuda")
    ci = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    assert lib.gf_nms_candidates(scores.data_ptr(), cs.data_ptr(), ci.data_ptr(), B, H, W, 3, 4, _stream()) == 0
    kp = pred["keypoints"] - 0.5
    ks = pred["keypoint_scores"]
    lost, ties = [], 0
    for b in range(B):
        nms, rs, ri = stock_topk(scores[b:b + 1])
        rs, ri, nms = rs[0], ri[0], nms[0].flatten()
        assert bool((rs > 0).all())
        assert torch.equal(ks[b], rs), f"image {b}: keypoint scores differ from torch.topk on the same map"
        idx = (kp[b, :, 1] * W + kp[b, :, 0]).long()
        kth = rs[-1]
        above = rs > kth
        assert torch.equal(torch.sort(idx[above]).values, torch.sort(ri[above]).values), f"image {b}: positions"
        at = ~above
        assert bool((nms[idx[at]] == kth).all()), f"image {b}: a keypoint of the K-th score group is not such a maximum"
        assert idx[at].unique().numel() == int(at.sum())
        ties += int((nms == kth).sum()) - int(at.sum())
        pos = torch.nonzero(nms > 0).flatten()
        got = ci[b][cs[b] > -1].long()
        missing = pos[~torch.isin(pos, got)]
        lost.append(int(missing.numel()))
        if missing.numel():
            assert float(nms[missing].max()) < float(kth), f"image {b}: a dropped candidate would enter the top-k"
    print(f"  bench config, B=64: {sum(lost)} positives lost to candidate-segment overflow (per image max {max(lost)}), "
          f"{ties} maxima tied at the K-th score left out by both")
    ref, bound = sample_fp64(kp, dmap.permute(0, 2, 3, 1))
    _check("_sample (gf_sample_descriptors) at the bench config", pred["descriptors"], ref, bound)


def test_fused_bf16_module_vs_fp32_stock_end_to_end(monkeypatch):
    """End-to-end at 1024^2, B = 4: the bf16 fused module against the fp32 stock modules (_use_fused false) of the same
    model -- a guard on the glue (grayscale, +0.5, force_num_keypoints padding).  Keypoints are compared only where the
    fp32 keypoint's margin exceeds twice the measured score-map difference: to the K-th score the largest difference
    anywhere, to every other score in its 7 x 7 NMS window the largest difference in that window; descriptors at the
    common keypoints."""
    model = make_model("open", seed=2)
    images = bench_images(2, seed=13).expand(-1, 3, -1, -1).contiguous()        # RGB: the module's grayscale conversion
    with torch.no_grad():       # a random network saturates the softmax (scores ~1.0, no margins): unit logit spread instead
        bn = model.detector[1].bn
        z = model._dense_unfused(images[:, :1])[0]
        sd = float(z.std(1).mean())
        bn.weight.div_(sd)
        bn.bias.div_(sd)
    rec, maps = record_blocks(model, monkeypatch)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        pred = model({"image": images})
    fused_scores = maps["det"].float()
    monkeypatch.setattr(model, "_use_fused", lambda image: False)
    dense = {}
    orig_dense = model._dense_unfused

    def dense_rec(image):
        det, desc = orig_dense(image)
        dense["det"] = det
        return det, desc
    monkeypatch.setattr(model, "_dense_unfused", dense_rec)
    with torch.no_grad():
        stock = model({"image": images})
    p = F.softmax(dense["det"].float(), 1)[:, :-1]
    b, _, h, w = p.shape
    stock_scores = p.permute(0, 2, 3, 1).reshape(b, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, h * 8, w * 8)
    diff = (fused_scores - stock_scores).abs()
    eps = float(diff.max())
    ewin = F.max_pool2d(diff[:, None], 7, 1, 3)[:, 0]                  # the largest difference in each NMS window
    matched = total = 0
    cos = []
    for i in range(b):
        kth = stock["keypoint_scores"][i, -1]
        sk = stock["keypoints"][i] - 0.5
        s = stock["keypoint_scores"][i]
        # second largest in the window: the window max with the point itself masked out
        ss = stock_scores[i].clone()
        ix, iy = sk[:, 0].long(), sk[:, 1].long()
        ss[iy, ix] = -1
        nb2 = F.max_pool2d(ss[None, None], 7, 1, 3)[0, 0][iy, ix]
        safe = ((s - kth) > 2 * eps) & ((s - nb2) > 2 * ewin[i][iy, ix])
        ours = {tuple(k): j for j, k in enumerate((pred["keypoints"][i] - 0.5).long().tolist())}
        for j in torch.nonzero(safe).flatten().tolist():
            total += 1
            key = (int(ix[j]), int(iy[j]))
            if key in ours:
                matched += 1
                cos.append(float((pred["descriptors"][i][ours[key]] * stock["descriptors"][i][j]).sum()))
    cos = torch.tensor(cos or [0.0])
    print(f"  end to end: score-map |bf16 fused - fp32 stock| max {eps:.3e} mean {float(diff.mean()):.3e}; "
          f"{matched} / {total} safe fp32 keypoints re-detected; descriptor cosine min {float(cos.min()):.4f} "
          f"mean {float(cos.mean()):.5f}")
    # measured on one MI355X: 3185 / 3185 re-detected, cosine min 0.9994, mean 0.99983 -- bounds with ~8x headroom on 1 - cos
    assert total >= 1000
    assert matched >= 0.99 * total
    assert float(cos.min()) > 0.995 and float(cos.mean()) > 0.9985
    assert torch.equal(pred["keypoints"] - torch.floor(pred["keypoints"]), torch.full_like(pred["keypoints"], 0.5))


