"""Timing record of the homography view synthesis (csrc/hviews.hip through data.homography_views) at the benchmark's geometry:
32 uint8 1024 x 1024 sources -> 64 gray views of 1024 x 1024 (two per source), preset `lg`, eager and as a hipGraph replay,
against the torch formulation bench.py builds its second view with today (a [B,H,W,2] fp32 grid from the inverse homography +
grid_sample, bilinear, zeros padding; restated here on fp32 one-channel sources, which is what grid_sample can read).
Every shape is warmed up first; the variants alternate inside one process; each figure is the best / median of `rounds`
windows of `iters` calls between device events.  Algorithmic bytes = the source bytes read once + the output bytes written
once; the fraction is of the 8.0 TB/s HBM3E peak (a float4 copy reaches 6.29 TB/s on this part).  The host sampling time per
batch (tables(): 64 homographies, 64 photometric draws) is reported next to it:
    python tools/probe/time_homography_views.py [out.txt]"""
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from glue_factory_amd.data.homography_views import HomographyViews  # noqa: E402

S, IMG, HBM_PEAK = 32, 1024, 8.0e12


def window(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, iters, rounds=7):
    for fn in fns.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return times


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def stage(preset, channels, images):
    views = HomographyViews({"homography": {"patch_shape": [IMG, IMG]}, "photometric": {"name": preset, "p": 0.95},
                             "grayscale": True, "seed": 0})
    sizes = [(IMG, IMG)] * S
    t0 = time.perf_counter()
    host = views.tables(sizes)
    host_ms = (time.perf_counter() - t0) * 1e3
    dev = views.upload(host)
    out = torch.empty(2 * S, 1, IMG, IMG, device="cuda")
    scratch = torch.empty(2 * S, channels, IMG, IMG, device="cuda") if views.two_launches else None
    return views, host, dev, (lambda: views.run(dev, images, out=out, scratch=scratch)), out, host_ms


def main():
    out_file = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    g = torch.Generator(device="cuda").manual_seed(0)
    src3 = torch.randint(0, 256, (S, IMG, IMG, 3), device="cuda", dtype=torch.uint8, generator=g)
    src1 = src3[..., :1].contiguous()
    say(f"homography view synthesis timing, {S} uint8 {IMG}x{IMG} sources -> {2 * S} gray views {IMG}x{IMG}, {torch.cuda.get_device_name(0)}")
    say("each figure: best / median of 7 alternating windows of 20 calls, ms per call (= per batch of 64 views)")

    views1, host1, dev1, run1, out1, host_ms = stage("lg", 1, src1)
    views3, _, _, run3, out3, _ = stage("lg", 3, src3)
    views_id, _, dev_id, run_id, out_id, _ = stage("identity", 1, src1)
    ints, floats = views1._segments(S, S)
    ntaps = views1._carve(host1["int"], ints)["ntaps"]
    say(f"  preset lg: {int((ntaps > 1).sum())} of {2 * S} views blurred, {int(ntaps.max())} taps at most; two launches "
        f"(gf_hv_warp, gf_hv_filter); preset identity: one launch")
    host_times = []
    for _ in range(5):
        t0 = time.perf_counter()
        views1.tables([(IMG, IMG)] * S)
        host_times.append((time.perf_counter() - t0) * 1e3)
    say(f"  host sampling (tables(): {2 * S} homographies + photometric draws, fp64 inverses, packing): first {host_ms:.2f} ms, "
        f"then best {min(host_times):.2f} / median {sorted(host_times)[2]:.2f} ms per batch = {min(host_times) / (2 * S):.3f} ms per view")

    # the torch formulation: grid build + grid_sample, fp32 one-channel sources, on the identity preset's homographies (the
    # presets consume the generator differently, so each stage has its own)
    Hinv = dev_id["Hinv"].view(2, S, 3, 3)
    srcf = src1.permute(0, 3, 1, 2).float().div(255.0).contiguous()
    ys, xs = torch.meshgrid(torch.arange(IMG, device="cuda", dtype=torch.float32),
                            torch.arange(IMG, device="cuda", dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1).reshape(1, -1, 3)
    tout = torch.empty(2, S, 1, IMG, IMG, device="cuda")

    def run_torch():
        for k in range(2):
            p = pix @ Hinv[k].transpose(1, 2)
            p = p[..., :2] / p[..., 2:]
            grid = (p * (2.0 / (IMG - 1)) - 1).reshape(S, IMG, IMG, 2)
            tout[k] = torch.nn.functional.grid_sample(srcf, grid, mode="bilinear", padding_mode="zeros", align_corners=True)

    # same picture: the identity preset (warp only) against grid_sample, away from the rounding of two fp32 formulations
    run_id()
    run_torch()
    torch.cuda.synchronize()
    diff = (out_id.view(2, S, 1, IMG, IMG) - tout).abs()
    say(f"  identity preset against the torch formulation: median |difference| {diff.median().item():.2e}, "
        f"{100 * (diff > 1e-2).float().mean().item():.3f} % of the pixels differ by more than 0.01 "
        f"(fp32 coordinates on both sides, random-noise sources)")

    g1, g3, gid, gt = capture(run1), capture(run3), capture(run_id), capture(run_torch)
    t = alternate({"ours eager C=1": run1, "ours graph C=1": g1.replay, "ours graph C=3": g3.replay, "ours graph identity": gid.replay,
                   "torch eager": run_torch, "torch graph": gt.replay}, iters=20)
    out_bytes = 2 * S * IMG * IMG * 4
    rows = [("ours eager C=1", "lg, uint8 gray sources, eager (2 launches)", S * IMG * IMG + out_bytes),
            ("ours graph C=1", "lg, uint8 gray sources, graph replay", S * IMG * IMG + out_bytes),
            ("ours graph C=3", "lg, uint8 RGB sources -> gray, graph replay", 3 * S * IMG * IMG + out_bytes),
            ("ours graph identity", "identity, uint8 gray sources, graph replay (1 launch)", S * IMG * IMG + out_bytes),
            ("torch eager", "torch grid build + grid_sample, fp32 sources, eager", 4 * S * IMG * IMG + out_bytes),
            ("torch graph", "torch grid build + grid_sample, fp32 sources, graph replay", 4 * S * IMG * IMG + out_bytes)]
    best = {}
    for key, name, nbytes in rows:
        ts = sorted(t[key])
        best[key] = ts[0]
        rate = nbytes / (ts[0] * 1e-3)
        say(f"  {name:62s} best {ts[0]:8.4f}  median {ts[len(ts) // 2]:8.4f}  algorithmic {nbytes / 2 ** 20:6.0f} MiB "
            f"-> {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of the HBM peak")
    say(f"  torch graph / ours graph (C=1, lg): {best['torch graph'] / best['ours graph C=1']:.2f}x; "
        f"{2 * S / (best['ours graph C=1'] * 1e-3):.0f} views/s on one GPU; the torch side has no photometric stage, no blur and "
        f"reads fp32 sources")


if __name__ == "__main__":
    main()
