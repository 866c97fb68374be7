"""Timing record of one point-and-line homography solver call (csrc/hl_solver.hip through
solvers.point_line_homography_ransac) at B=32, M=N=2048, L=L1=512, T=3000 hypotheses, lo_iters=2: eager and as a hipGraph
replay, and gf_h_ransac (solvers.homography_ransac) on the same points, for orientation.  Every shape is warmed up first; the
variants alternate inside one process; each figure is the best / median of `rounds` windows of `iters` calls between device
events.  Prints the launch count too:
    python tools/probe/time_hl_solver.py [out.txt]"""
import math
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from glue_factory_amd.gt import warp_points  # noqa: E402
from glue_factory_amd.solvers.homography_ransac import homography_ransac  # noqa: E402
from glue_factory_amd.solvers.point_line_homography_ransac import point_line_homography_ransac  # noqa: E402
from glue_factory_amd.synthetic import similarity_homography  # noqa: E402

B, M, L, T, LO, TH = 32, 2048, 512, 3000, 2, 2.0


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
    """80 % of the keypoints and of the segments matched, 70 % of those on the homography (points with 0.5 px noise; segments
    with their view-1 endpoints slid along the line and 0.5 px noise), the rest anywhere."""
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=g)
    randn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    wh = torch.tensor([1024.0, 1024.0], device="cuda")
    H = similarity_homography(1024, 1024).cuda()[None].repeat(B, 1, 1)

    def scatter(x1, n):
        perm = torch.stack([torch.randperm(n, device="cuda", generator=g) for _ in range(B)])
        idx = perm.reshape(B, n, *([1] * (x1.dim() - 2))).expand_as(x1)
        m0 = torch.where(rand(B, n) < 0.8, perm, torch.full_like(perm, -1))
        return torch.empty_like(x1).scatter_(1, idx, x1).contiguous(), m0.contiguous()

    kp0 = rand(B, M, 2) * wh
    kp1 = warp_points(kp0, H) + 0.5 * randn(B, M, 2)
    wrong = rand(B, M) < 0.3
    kp1, m0 = scatter(torch.where(wrong[..., None], rand(B, M, 2) * wh, kp1), M)
    p = rand(B, L, 2) * (wh - 200) + 100
    ang, length = rand(B, L) * 2 * math.pi, 20 + rand(B, L) * 80
    l0 = torch.stack([p, p + length[..., None] * torch.stack([torch.cos(ang), torch.sin(ang)], -1)], 2)
    w = warp_points(l0.reshape(B, -1, 2), H).reshape(B, L, 2, 2)
    d = w[:, :, 1] - w[:, :, 0]
    slid = torch.stack([w[:, :, 0] + (rand(B, L, 1) - 0.5) * d, w[:, :, 1] + (rand(B, L, 1) - 0.5) * 0.8 * d], 2)
    lwrong = rand(B, L) < 0.3
    l1, lm0 = scatter(torch.where(lwrong[..., None, None], rand(B, L, 2, 2) * wh, slid + 0.5 * randn(B, L, 2, 2)), L)
    return kp0.contiguous(), kp1, m0, l0.contiguous(), l1, lm0, wrong, lwrong


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    kp0, kp1, m0, l0, l1, lm0, wrong, lwrong = scene()
    say(f"point-and-line homography solver timing, B={B} M=N={M} L=L1={L} T={T} lo_iters={LO} th={TH}, {torch.cuda.get_device_name(0)}")
    say(f"launches per call: gf_hl_ransac {4 + 2 * LO} (compact, score, select, {LO} x (refit, rescore), outputs); gf_h_ransac {4 + 2 * LO}")
    say("each figure: best / median of 7 alternating windows, ms per call")

    run = lambda: point_line_homography_ransac(kp0, kp1, m0, l0, l1, lm0, TH, T, LO, 0)
    res = run()
    agree = (res["inliers"] == ((m0 > -1) & ~wrong)).float().mean().item()
    lagree = (res["line_inliers"] == ((lm0 > -1) & ~lwrong)).float().mean().item()
    say(f"  success on {int(res['success'].sum())} of {B} pairs; inlier masks equal the planted sets on {100 * agree:.2f} % of the "
        f"keypoints and {100 * lagree:.2f} % of the segments (0.5 px noise against a {TH} px threshold)")

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

    t = alternate({"eager": run, "graph": graph.replay,
                   "lo0": lambda: point_line_homography_ransac(kp0, kp1, m0, l0, l1, lm0, TH, T, 0, 0),
                   "points": lambda: point_line_homography_ransac(kp0, kp1, m0, None, None, None, TH, T, LO, 0),
                   "h": lambda: homography_ransac(kp0, kp1, m0, TH, T, LO, 0)}, iters=20)

    def report(name, ts):
        ts = sorted(ts)
        say(f"  {name:60s} best {ts[0]:8.4f}  median {ts[len(ts) // 2]:8.4f}")
        return ts[0]

    te = report("gf_hl_ransac eager (8 launches + allocations)", t["eager"])
    tg = report("gf_hl_ransac graph replay", t["graph"])
    t0 = report("gf_hl_ransac eager, lo_iters = 0 (4 launches)", t["lo0"])
    report("gf_hl_ransac eager, the points alone (L = 0)", t["points"])
    th = report("gf_h_ransac eager on the same points (for orientation)", t["h"])
    kp, kl = float((m0 > -1).sum(1).float().mean()), float((lm0 > -1).sum(1).float().mean())
    say(f"  mean matches per pair: {kp:.0f} points, {kl:.0f} lines; {B * T * (kp + kl) / (tg * 1e-3) / 1e9:.1f} G (hypothesis, feature) "
        f"inlier tests per second if the whole replay were scoring")
    say(f"  local optimisation (2 refits + 2 rescores): {te - t0:.4f} ms of the eager call; gf_hl_ransac / gf_h_ransac = {te / th:.2f}")


if __name__ == "__main__":
    main()
