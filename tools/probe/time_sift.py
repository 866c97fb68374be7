"""Timing record of the SIFT extractor (extractors/sift.py) at the benchmark's image geometry: 64 gray images of
1024 x 1024, 2048 keypoints, forced count, nms_radius 3 (the extractor block of sift+lightglue_megadepth.yaml).  The fused
path (csrc/sift.hip) eager and as a hipGraph replay against the stock path of the same module on the device, in the same
process.  The stock path gathers whole windows per keypoint and reads counts back, so it runs in chunks of 8 images; its
figure is the sum over the 8 chunks.  Images are smoothed noise (a few thousand candidates each); every shape is warmed up
first, so all outputs and intermediates come out of the caching allocator's warm blocks and no window times an allocation;
the variants alternate; each figure is the best / median of `rounds` windows between device events.  Per-stage times of
the fused path (one eager pass after the warm-up passes, events around each stage) follow.
    python tools/probe/time_sift.py [out.txt]"""
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from glue_factory_amd.extractors import sift as sf  # noqa: E402
from glue_factory_amd.extractors import sift_kernels  # noqa: E402

B, IMG, K, CHUNK, CAP = 64, 1024, 2048, 8, 32768


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

    conf = {"max_num_keypoints": K, "force_num_keypoints": True, "nms_radius": 3, "backend": "pycolmap_cuda", "candidate_cap": CAP}
    model = sf.SIFT(conf)
    g = torch.Generator(device="cuda").manual_seed(1)
    images = torch.rand(B, 1, IMG, IMG, device="cuda", generator=g)
    images = torch.nn.functional.avg_pool2d(images, 9, 1, 4) * 3 - 1
    images = images.clamp(0, 1).contiguous()
    say(f"SIFT timing, {B} gray images {IMG}x{IMG}, {K} keypoints forced, nms_radius 3, fp32, {torch.cuda.get_device_name(0)}")

    def fused():
        return model({"image": images})

    def stock():
        model._use_fused = lambda image: False
        try:
            for i in range(0, B, CHUNK):
                model({"image": images[i:i + CHUNK]})
        finally:
            del model._use_fused

    out = fused()
    say(f"  real keypoints per image: min {int((out['scales'] > 0).sum(1).min())}, max {int((out['scales'] > 0).sum(1).max())}; "
        f"candidate list overflow ({CAP} slots): {bool(model.overflow.any())}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fused()
        with torch.cuda.graph(graph, stream=side):
            fused()
    torch.cuda.current_stream().wait_stream(side)
    t = alternate({"fused eager": fused, "fused graph": graph.replay, "stock": stock}, iters=1, rounds=3)
    best = {}
    for key, ts in t.items():
        ts = sorted(ts)
        best[key] = ts[0]
        say(f"  {key:12s} best {ts[0]:9.2f} ms  median {ts[len(ts) // 2]:9.2f} ms per {B} images = {B / (ts[0] * 1e-3):7.1f} images/s")
    say(f"  stock / fused graph: {best['stock'] / best['fused graph']:.2f}x; stock / fused eager: {best['stock'] / best['fused eager']:.2f}x")

    # per-stage times of the fused path: the pass runs three times and its tensors die in between, so the measured (last)
    # pass finds every block it asks for in the caching allocator and times no allocation
    img = images[:, 0].contiguous()

    def stages():
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

        mark("start")
        gauss, dog = sift_kernels.pyramid(img, -1, 4)
        mark("pyramid (gf_sift_blur, 6 launches per octave)")
        meta, vals, count = sift_kernels.extrema(dog, model.conf.detection_threshold, float(model.conf.edge_threshold), CAP)
        mark("gf_sift_extrema (count, scan, write per octave)")
        octv, layer, yi, xi = meta.long().unbind(-1)
        octv = torch.where(torch.arange(CAP, device="cuda").view(1, -1) < count.view(-1, 1), octv, torch.full_like(octv, -1))
        s_o = layer.float() + vals[..., 2]
        sigma = sf.SIGMA0 * torch.exp2(s_o / 3)
        lvl = torch.round(s_o).long().clamp(0, 5)
        ori, valid = sift_kernels.orient(gauss, octv, lvl, xi, yi, sigma)
        mark(f"gf_sift_orient ({CAP} slots per image) + its torch glue")
        sel = slice(0, K)
        sift_kernels.describe(gauss, octv[:, sel], lvl[:, sel], xi[:, sel].float(), yi[:, sel].float(), sigma[:, sel], ori[:, sel, 0], True)
        mark(f"gf_sift_describe ({K} keypoints per image)")
        torch.cuda.synchronize()
        nbytes = sum(t.numel() * 4 for t in gauss) * 2 + sum(t.numel() * 4 for t in dog)
        return marks, nbytes, int(count.min()), int(count.max())

    for _ in range(3):
        marks, nbytes, cmin, cmax = stages()
    say(f"  candidates per image: min {cmin}, max {cmax}")
    say("  fused path by stage (third eager pass, warm blocks; the rest of the call is the torch glue of the selection: dedupe, "
        "max-pool NMS, top-k, gathers, padding):")
    for (_, a), (name, b) in zip(marks[:-1], marks[1:]):
        say(f"    {a.elapsed_time(b):9.2f} ms  {name}")
    say(f"  the pyramid moves {nbytes / 2 ** 30:.1f} GiB algorithmically (every level read once and written once, every DoG level written)")


if __name__ == "__main__":
    main()
