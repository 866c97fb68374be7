"""Timing record of one homography solver call (csrc/h_solver.hip through solvers.homography_ransac) at B=32, M=N=2048,
T=3000 hypotheses, lo_iters=2: eager and as a hipGraph replay, and the weighted DLT (solvers.dlt) on the same matches.
Every shape is warmed up first; the variants alternate inside one process; each figure is the best / median of `rounds`
windows of `iters` calls between device events (a window lasts a few tenths of a second).  Prints the launch count too:
    python tools/probe/time_h_solver.py [out.txt]"""
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from glue_factory_amd.gt import warp_points  # noqa: E402
from glue_factory_amd.solvers.dlt import homography_dlt  # noqa: E402
from glue_factory_amd.solvers.homography_ransac import homography_ransac  # noqa: E402
from glue_factory_amd.synthetic import similarity_homography  # noqa: E402

B, M, T, LO = 32, 2048, 3000, 2


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


def scene():
    """80 % of the keypoints matched, 70 % of those on the homography with 0.5 px noise, the rest anywhere."""
    g = torch.Generator(device="cuda").manual_seed(0)
    wh = torch.tensor([1024.0, 1024.0], device="cuda")
    kp0 = torch.rand(B, M, 2, device="cuda", generator=g) * wh
    H = similarity_homography(1024, 1024).cuda()[None].repeat(B, 1, 1)
    kp1 = warp_points(kp0, H) + 0.5 * torch.randn(B, M, 2, device="cuda", generator=g)
    wrong = torch.rand(B, M, device="cuda", generator=g) < 0.3
    kp1 = torch.where(wrong[..., None], torch.rand(B, M, 2, device="cuda", generator=g) * wh, kp1)
    perm = torch.stack([torch.randperm(M, device="cuda", generator=g) for _ in range(B)])
    kp1p = torch.empty_like(kp1).scatter_(1, perm[..., None].expand(-1, -1, 2), kp1)
    m0 = torch.where(torch.rand(B, M, device="cuda", generator=g) < 0.8, perm, torch.full_like(perm, -1))
    return kp0.contiguous(), kp1p.contiguous(), m0.contiguous(), H, wrong


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    kp0, kp1, m0, H, wrong = scene()
    scores = torch.rand(B, M, device="cuda")
    say(f"homography solver timing, B={B} M=N={M} T={T} lo_iters={LO}, {torch.cuda.get_device_name(0)}")
    say(f"launches per call: gf_h_ransac {4 + 2 * LO} (compact, score, select, {LO} x (refit, rescore), outputs); gf_h_dlt 3")
    say("each figure: best / median of 7 alternating windows, ms per call")

    run = lambda: homography_ransac(kp0, kp1, m0, 3.0, T, LO, 0)
    res = run()
    planted = (m0 > -1) & ~wrong
    agree = (res["inliers"] == planted).float().mean().item()
    say(f"  success on {int(res['success'].sum())} of {B} pairs; inlier mask equals the planted set on {100 * agree:.2f} % of the keypoints "
        f"(0.5 px noise: a few planted points fall outside 3 px, a few wrong ones inside)")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        run()
        with torch.cuda.graph(graph, stream=side):
            captured = run()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(captured[k], res[k]) for k in res), "graph replay differs from the eager call"

    t = alternate({"eager": run, "graph": graph.replay, "dlt": lambda: homography_dlt(kp0, kp1, m0, scores),
                   "lo0": lambda: homography_ransac(kp0, kp1, m0, 3.0, T, 0, 0)}, iters=100)

    def report(name, ts):
        ts = sorted(ts)
        say(f"  {name:44s} best {ts[0]:8.4f}  median {ts[len(ts) // 2]:8.4f}")
        return ts[0]

    te = report("gf_h_ransac eager (8 launches + allocations)", t["eager"])
    tg = report("gf_h_ransac graph replay", t["graph"])
    t0 = report("gf_h_ransac eager, lo_iters = 0 (4 launches)", t["lo0"])
    report("gf_h_dlt eager (3 launches)", t["dlt"])
    k = float((m0 > -1).sum(1).float().mean())
    say(f"  mean matches per pair {k:.0f}: {B * T * k * 17 / (tg * 1e-3) / 1e12:.2f} TFLOP/s of the scoring loop's 17 flops per "
        f"(hypothesis, correspondence) if the whole replay were scoring")
    say(f"  local optimisation (2 refits + 2 rescores): {te - t0:.4f} ms of the eager call")
    say(f"  one replay = {100 * tg / 45.0:.2f} % of a 45 ms matcher step")


if __name__ == "__main__":
    main()
