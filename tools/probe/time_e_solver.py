"""Timing record of one relative-pose solver call (csrc/e_solver.hip through solvers.relative_pose_ransac) at B=32,
M=N=2048, T=2048 hypotheses, lo_iters=2: eager and as a hipGraph replay, with lo_iters=0 and T=1 for the split of the
call, and gf_h_ransac at the same B, M, T for scale.  Every shape is warmed up first; the variants alternate inside one
process; each figure is the best / median of `rounds` windows of `iters` calls between device events.
    python tools/probe/time_e_solver.py [out.txt]"""
import math
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from glue_factory_amd.geometry import Camera, Pose  # noqa: E402
from glue_factory_amd.metrics import relative_pose_error  # noqa: E402
from glue_factory_amd.solvers.homography_ransac import homography_ransac  # noqa: E402
from glue_factory_amd.solvers.relative_pose_ransac import relative_pose_ransac  # noqa: E402

B, M, T, LO = 32, 2048, 2048, 2


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
    """80 % of the keypoints matched, 70 % of those projections of 3-D points at depths 2-10 with 0.5 px noise, the rest
    anywhere; a rotation of 15 degrees about (1, 2, 0.5), a sideways unit translation, two pinhole cameras."""
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=g)
    wh = torch.tensor([1024.0, 768.0], device="cuda")
    cam0 = Camera(torch.tensor([1024.0, 768.0, 800.0, 810.0, 500.0, 390.0], device="cuda").repeat(B, 1))
    cam1 = Camera(torch.tensor([1024.0, 768.0, 1000.0, 990.0, 520.0, 380.0], device="cuda").repeat(B, 1))
    ax = torch.tensor([1.0, 2.0, 0.5], device="cuda")
    ax = ax / ax.norm()
    Kx = torch.tensor([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], device="cuda")
    a = math.radians(15.0)
    R = torch.eye(3, device="cuda") + math.sin(a) * Kx + (1 - math.cos(a)) * Kx @ Kx
    t = torch.tensor([0.9, 0.3, 0.1], device="cuda")
    T01 = Pose.from_Rt(R[None].repeat(B, 1, 1), (t / t.norm())[None].repeat(B, 1))
    kp0 = rand(B, M, 2) * wh
    X = cam0.image2cam(kp0) * (2 + 8 * rand(B, M, 1))
    kp1 = cam1.cam2image(T01.transform(X))[0] + 0.5 * torch.randn(B, M, 2, device="cuda", generator=g)
    wrong = rand(B, M) < 0.3
    kp1 = torch.where(wrong[..., None], rand(B, M, 2) * wh, kp1)
    perm = torch.stack([torch.randperm(M, device="cuda", generator=g) for _ in range(B)])
    kp1p = torch.empty_like(kp1).scatter_(1, perm[..., None].expand(-1, -1, 2), kp1)
    m0 = torch.where(rand(B, M) < 0.8, perm, torch.full_like(perm, -1))
    return kp0.contiguous(), kp1p.contiguous(), m0.contiguous(), cam0, cam1, T01


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    kp0, kp1, m0, cam0, cam1, T01 = scene()
    say(f"relative-pose solver timing, B={B} M=N={M} T={T} lo_iters={LO}, {torch.cuda.get_device_name(0)}")
    say(f"launches per call: gf_e_ransac {5 + 2 * LO} (compact, solve, score, select, {LO} x (refit, rescore), pose)")
    say("each figure: best / median of 7 alternating windows, ms per call")

    run = lambda t=T, lo=LO: relative_pose_ransac(kp0, kp1, m0, cam0, cam1, 0.5, t, lo, 0)
    res = run()
    t_err, r_err = relative_pose_error(T01, res["M_0to1"].R, res["M_0to1"].t)
    say(f"  success on {int(res['success'].sum())} of {B} pairs; mean inliers {res['num_inliers'].float().mean().item():.0f} of "
        f"{(m0 > -1).sum(1).float().mean().item():.0f} matches; worst pose error {torch.maximum(t_err, r_err).max().item():.3f} degrees "
        f"(0.5 px noise against a 0.5 px threshold)")

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
    assert torch.equal(captured["M_0to1"]._data, res["M_0to1"]._data) and torch.equal(captured["inliers"], res["inliers"]), \
        "graph replay differs from the eager call"

    t = alternate({"eager": run, "graph": graph.replay, "lo0": lambda: run(T, 0), "t1": lambda: run(1, 0),
                   "h": lambda: homography_ransac(kp0, kp1, m0, 3.0, T, LO, 0)}, iters=20)

    def report(name, ts):
        ts = sorted(ts)
        say(f"  {name:58s} best {ts[0]:8.4f}  median {ts[len(ts) // 2]:8.4f}")
        return ts[0]

    te = report(f"gf_e_ransac eager ({5 + 2 * LO} launches + normalisation + allocations)", t["eager"])
    tg = report("gf_e_ransac graph replay", t["graph"])
    t0 = report("gf_e_ransac eager, lo_iters = 0 (5 launches)", t["lo0"])
    t1 = report("gf_e_ransac eager, T = 1, lo_iters = 0 (the fixed part)", t["t1"])
    th = report(f"gf_h_ransac eager at the same B, M, T (lo_iters = {LO})", t["h"])
    say(f"  solve + score of {T} hypotheses: {t0 - t1:.4f} ms; local optimisation (2 refits + 2 rescores): {te - t0:.4f} ms")
    say(f"  one replay = {tg / th:.1f} x the homography solver's call, {100 * tg / 45.0:.2f} % of a 45 ms matcher step")


if __name__ == "__main__":
    main()
