"""Timing record of the depth ground truth at the reference's MegaDepth configuration (`th_epi: 5`), B=32, M=N=2048, on a
synthetic depth scene: the dense torch form (gt.gt_matches_from_pose_depth: what the plugin ran before gt_epi.hip, still the
CPU path and the tests' reference) against the fused form (gt.gt_matches_from_pose_depth_fused: gf_gt_nn + gf_gt_epi_min
[+ gf_gt_depth_reward]), with and without the dense reward.  The two forms alternate inside one process; both are warmed up
first; each figure is the median (and the best) of `rounds` windows of `iters` calls between device events.  Also prints the
peak allocation of one call of each form.
    python tools/probe/time_gt_depth.py [out.txt]"""
import math
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from glue_factory_amd.geometry import Camera, Pose  # noqa: E402
from glue_factory_amd.gt import gt_matches_from_pose_depth, gt_matches_from_pose_depth_fused  # noqa: E402

B, N, H, W = 32, 2048, 480, 640


def scene(seed=0):
    """Two views of a smooth surface 4-6 m away, the second camera moved 0.3 m sideways and turned by 3 degrees; 5 % of the
    depth pixels are holes (points without depth: the ones the epipolar extension labels)."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    phase = torch.rand(B, 2, 1, 1, generator=g) * 6.28
    depth = 5.0 + torch.sin(xs / 90.0 + phase[:, 0]) * 0.6 + torch.cos(ys / 70.0 + phase[:, 1]) * 0.4

    def holes():
        return depth * (torch.rand(B, H, W, generator=g) > 0.05)
    cam = torch.tensor([[W, H, 500.0, 500.0, W / 2, H / 2]]).repeat(B, 1)
    a = math.radians(3.0)
    R = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]]).repeat(B, 1, 1)
    t = torch.tensor([[0.3, 0.02, 0.05]]).repeat(B, 1)
    scale = torch.tensor([W - 1.0, H - 1.0])
    kp0, kp1 = torch.rand(B, N, 2, generator=g) * scale, torch.rand(B, N, 2, generator=g) * scale
    data = {"view0": {"camera": Camera(cam.cuda()), "depth": holes().cuda()},
            "view1": {"camera": Camera(cam.cuda()), "depth": holes().cuda()},
            "T_0to1": Pose.from_Rt(R.cuda(), t.cuda())}
    return kp0.cuda(), kp1.cuda(), data


def window(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    kp0, kp1, data = scene()
    kw = dict(pos_th=3.0, neg_th=5.0, epi_th=5.0)
    say(f"depth ground truth timing, B={B} M=N={N}, th_epi=5, {torch.cuda.get_device_name(0)}")
    dense = lambda: gt_matches_from_pose_depth(kp0, kp1, data, **kw)            # always builds the reward
    ref = dense()
    labels = ref["matches0"]
    say(f"scene: {int((labels >= 0).sum())} positives, {int((labels == -1).sum())} negatives, {int((labels == -2).sum())} ignored "
        f"of {labels.numel()} view-0 points")
    for with_reward in (False, True):
        fused = lambda: gt_matches_from_pose_depth_fused(kp0, kp1, data, with_reward=with_reward, **kw)
        got = fused()
        same = all(torch.equal(got[k], ref[k]) for k in ("assignment", "matches0", "matches1"))
        line = f"with_reward={with_reward}: labels equal to the dense form: {same}"
        if with_reward:
            line += f"; reward entries that differ: {int((got['reward'] != ref['reward']).sum())} of {ref['reward'].numel()}"
        say(line)
        del got
        fns = {"dense": dense, "fused": fused}
        for fn in fns.values():
            for _ in range(3):
                fn()
        times = {k: [] for k in fns}
        for _ in range(7):
            for k, fn in fns.items():
                times[k].append(window(fn, 5))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for k, v in times.items():
            say(f"  {k}: median {med[k]:.3f} ms, best {min(v):.3f} ms, worst {max(v):.3f} ms per call; "
                f"peak allocation {peak_of(fns[k]) / 2 ** 20:.0f} MiB")
        say(f"  dense / fused = {med['dense'] / med['fused']:.2f}x")


if __name__ == "__main__":
    main()
