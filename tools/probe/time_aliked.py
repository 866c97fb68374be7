"""Timing record of the ALIKED extractor (extractors/aliked.py) at the benchmark's image geometry: 64 images of 1024 x 1024,
aliked-n16, 2048 keypoints, top-k mode.  The fused path (csrc/aliked.hip) eager and as a hipGraph replay against the stock
path of the same module in the same process (the reference's formulation op for op: upsampled maps, concatenation,
normalised copy, per-image description).  The stock path materialises > 1.5 GB per image, so it runs in chunks of 8
images; its figure is the sum over the 8 chunks.  Random weights and random images; every shape is warmed up first; the
variants alternate; each figure is the best / median of `rounds` windows between device events.  Per-stage times of the
fused path (one eager pass, events around each stage) follow.
    python tools/probe/time_aliked.py [out.txt]"""
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from glue_factory_amd.extractors import aliked as ak  # noqa: E402
from glue_factory_amd.extractors import aliked_kernels  # noqa: E402

B, IMG, K, CHUNK = 64, 1024, 2048, 8


def window(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, iters, rounds):
    for fn in fns.values():
        fn()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return times


def main():
    out_file = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    torch.manual_seed(0)
    model = ak.ALIKED({"model_name": "aliked-n16", "max_num_keypoints": K, "detection_threshold": -1.0, "force_num_keypoints": True,
                       "pretrained": False}).cuda().eval()
    model.score_head[6].weight.data.mul_(30.0)
    for p in model.parameters():
        p.requires_grad_(False)
    g = torch.Generator(device="cuda").manual_seed(1)
    images = torch.rand(B, 3, IMG, IMG, device="cuda", generator=g)
    say(f"ALIKED timing, {B} images {IMG}x{IMG}, aliked-n16, {K} keypoints, top-k mode, fp32, {torch.cuda.get_device_name(0)}")

    def fused():
        with torch.no_grad():
            return model({"image": images})

    def stock():
        model._use_fused = lambda image: False
        try:
            with torch.no_grad():
                for i in range(0, B, CHUNK):
                    model({"image": images[i:i + CHUNK]})
        finally:
            del model._use_fused

    fused()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fused()
        with torch.cuda.graph(graph, stream=side):
            fused()
    torch.cuda.current_stream().wait_stream(side)
    t = alternate({"fused eager": fused, "fused graph": graph.replay, "stock": stock}, iters=2, rounds=3)
    best = {}
    for key, ts in t.items():
        ts = sorted(ts)
        best[key] = ts[0]
        say(f"  {key:12s} best {ts[0]:9.2f} ms  median {ts[len(ts) // 2]:9.2f} ms per {B} images = {B / (ts[0] * 1e-3):7.1f} images/s")
    say(f"  stock / fused graph: {best['stock'] / best['fused graph']:.2f}x; stock / fused eager: {best['stock'] / best['fused eager']:.2f}x")

    # per-stage times of the fused path
    marks = []

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))

    with torch.no_grad():
        for _ in range(2):
            marks.clear()
            mark("start")
            h = w = IMG
            x1 = model.block1(images)
            x2 = model.block2(torch.nn.functional.avg_pool2d(x1, 2, 2))
            x3 = model.block3(torch.nn.functional.avg_pool2d(x2, 4, 4), True)
            x4 = model.block4(torch.nn.functional.avg_pool2d(x3, 4, 4), True)
            g2, g3, g4 = (torch.nn.functional.selu(c(x)) for c, x in ((model.conv2, x2), (model.conv3, x3), (model.conv4, x4)))
            mark("backbone (library convolutions, gf_ak_deform_cols + matmul in blocks 3, 4)")
            feat, s8 = aliked_kernels.aggregate(x1, g2, g3, g4, model.conv1.weight, model.score_head[0].weight, 0, 0, h, w)
            mark("gf_ak_aggregate")
            score = torch.sigmoid(model.score_head[2:](s8))
            mark("score head tail (three 3x3 library convolutions, sigmoid)")
            ind = model._select(score, {}, True)
            mark("NMS + top-k (gf_nms_candidates, gf_topk_candidates)")
            kxy, ksc, disp = aliked_kernels.dkd_refine(score, ind, 2, 0.1)
            mark("gf_ak_dkd_refine")
            p = ak._scale_xy(kxy / 2 + 0.5, w - 1, h - 1)
            desc = aliked_kernels.sddh(feat, p, model._sddh_weights(), model.K, model.M)
            mark("gf_ak_sddh")
            torch.cuda.synchronize()
    say("  fused path by stage (one eager pass after a warm-up pass; a stage pays the allocations of its outputs: compare the sum with the whole call):")
    for (_, a), (name, b) in zip(marks[:-1], marks[1:]):
        say(f"    {a.elapsed_time(b):9.2f} ms  {name}")
    nbytes = feat.numel() * 4 + s8.numel() * 4 + x1.numel() * 4
    say(f"  gf_ak_aggregate moves {nbytes / 2 ** 30:.1f} GiB algorithmically (x1 read, feature map and 8-channel map written)")


if __name__ == "__main__":
    main()
