"""Timing record of the line ground truth's close-point counts at GlueStick's training shape, B=32, 512 lines per view, 50
samples per line: the torch form (gt._close_point_counts, what both line ground truths ran before gt_lines.hip, still the CPU
path and the tests' yardstick) against the kernel (gt._close_point_counts_fused -> gf_line_close_counts), for BOTH calls of
one step (the second one transposed), without `keep` (homography ground truth) and with it (depth ground truth).  Lines are
uniform in a 1024^2 image and at least 15 px long; each view's samples lie within a few pixels of the other view's lines (in
another order), so that every line has a close partner.  5 warm-ups, then 20 timed runs of each form between device events, the two
forms alternating; also the peak allocation of one step's two calls, and whether the counts are equal.
    python tools/probe/time_gt_lines.py [out.txt]          (default: profiles/gt_lines_timing.txt)"""
import os
import sys

import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from glue_factory_amd.gt import _close_point_counts, _close_point_counts_fused, _line_samples  # noqa: E402

B, L, P, DIST_TH = 32, 512, 50, 5
WARMUP, RUNS = 5, 20


def lines(g):
    seg = torch.rand(B, L, 4, generator=g) * 1024
    while True:
        short = (seg[..., 2:] - seg[..., :2]).norm(dim=-1) < 15
        if not bool(short.any()):
            return seg
        seg[short] = torch.rand(int(short.sum()), 4, generator=g) * 1024


def scene(seed=0):
    g = torch.Generator().manual_seed(seed)
    l0, l1 = lines(g), lines(g)
    # the samples of view 0's lines land (under some warp) on view 1's lines in another order, and the other way round
    p0_in1 = _line_samples(l1[:, torch.randperm(L, generator=g)], P) + torch.randn(B, L, P, 2, generator=g)
    p1_in0 = _line_samples(l0[:, torch.randperm(L, generator=g)], P) + torch.randn(B, L, P, 2, generator=g)
    keep0, keep1 = torch.rand(B, L, P, generator=g) < 0.7, torch.rand(B, L, P, generator=g) < 0.7
    return [t.cuda().contiguous() for t in (l0, l1, p0_in1, p1_in0, keep0, keep1)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gt_lines_timing.txt")
    out = open(path, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    l0, l1, p0_in1, p1_in0, keep0, keep1 = scene()
    say(f"line ground truth close-point counts, B={B} A=C={L} P={P} dist_th={DIST_TH}, {torch.cuda.get_device_name(0)}")
    say(f"both calls of one step per run; {WARMUP} warm-ups, {RUNS} timed runs per form, alternating")
    for with_keep in (False, True):
        k0, k1 = (keep0, keep1) if with_keep else (None, None)
        torch_form = lambda: (_close_point_counts(l0, p1_in0, DIST_TH, k1),
                              _close_point_counts(l1, p0_in1, DIST_TH, k0).transpose(-1, -2))
        kernel = lambda: (_close_point_counts_fused(l0, p1_in0, DIST_TH, k1),
                          _close_point_counts_fused(l1, p0_in1, DIST_TH, k0, transposed=True))
        ref, got = torch_form(), kernel()
        same = all(torch.equal(g.long(), r) for g, r in zip(got, ref))
        say(f"keep={with_keep}: counts equal: {same}; pairs with a non-zero count: {int((ref[0] > 0).sum())} of {ref[0].numel()}, "
            f"sum {int(ref[0].sum())}")
        del ref, got
        fns = {"torch form": torch_form, "kernel": kernel}
        for fn in fns.values():
            for _ in range(WARMUP):
                fn()
        times = {k: [] for k in fns}
        for _ in range(RUNS):
            for k, fn in fns.items():
                times[k].append(timed(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for k, v in times.items():
            say(f"  {k}: median {med[k]:.3f} ms, best {min(v):.3f} ms, worst {max(v):.3f} ms per step (two calls); "
                f"peak allocation {peak_of(fns[k]) / 2 ** 20:.1f} MiB")
        say(f"  torch form / kernel = {med['torch form'] / med['kernel']:.1f}x")
    out.close()


if __name__ == "__main__":
    main()
