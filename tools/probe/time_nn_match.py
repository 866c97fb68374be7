"""Timing record of the nearest-neighbour matcher at B=32, M=N=2048, D=256, bf16:
  (1) gf_rows_top2 against gf_rows_argmax (same MFMA work; the device code of gf_rows_argmax is the parent commit's),
  (2) the whole matcher forward against a composition of stock torch ops (bmm, two topk, gathers, two logsumexp) on the same device.
The two sides of each comparison alternate inside one process; every shape is warmed up first; each figure is the best of
`rounds` windows of `iters` calls between device events.  Prints the raw times and both ratios:
    python tools/probe/time_nn_match.py [out.txt]"""
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from glue_factory_amd import ops  # noqa: E402
from glue_factory_amd.matchers.nearest_neighbor_matcher import NearestNeighborMatcher  # noqa: E402

B, N, D = 32, 2048, 256


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


def torch_baseline(d0, d1, ratio, dist, mutual=True):
    """The same six outputs from stock torch ops (the baseline only): one batched product, a top-k per direction, the two
    thresholds on squared distances, the mutual check through one gather per side, two log-sum-exp passes."""
    scores = torch.bmm(d0, d1.transpose(1, 2))
    k = 2 if ratio else 1

    def one_side(s):
        vals, idx = s.topk(k)
        sq = 2.0 - 2.0 * vals                                   # squared distance of two unit vectors
        drop = torch.zeros_like(idx[:, :, 0], dtype=torch.bool)
        if ratio:
            drop |= sq[:, :, 0] > ratio * ratio * sq[:, :, 1]
        if dist:
            drop |= sq[:, :, 0] > dist * dist
        return idx[:, :, 0].masked_fill(drop, -1)

    m0, m1 = one_side(scores), one_side(scores.transpose(1, 2))
    if mutual:
        back0 = m1.gather(1, m0.clamp(min=0)) != torch.arange(m0.shape[1], device=m0.device)
        back1 = m0.gather(1, m1.clamp(min=0)) != torch.arange(m1.shape[1], device=m1.device)
        m0, m1 = m0.masked_fill(back0, -1), m1.masked_fill(back1, -1)
    B, M, N = scores.shape
    la = torch.zeros((B, M + 1, N + 1), dtype=torch.float32, device=scores.device)
    wide = scores.float()
    la[:, :M, :N].copy_(wide).mul_(2.0).sub_(wide.logsumexp(2, keepdim=True)).sub_(wide.logsumexp(1, keepdim=True))
    return m0, m1, (m0 >= 0).float(), (m1 >= 0).float(), scores, la


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    g = torch.Generator(device="cuda").manual_seed(0)
    d0 = torch.nn.functional.normalize(torch.randn(B, N, D, device="cuda", generator=g), dim=-1).bfloat16()
    d1 = torch.nn.functional.normalize(torch.randn(B, N, D, device="cuda", generator=g), dim=-1).bfloat16()
    say(f"nearest-neighbour matcher timing, B={B} M=N={N} D={D} bf16, {torch.cuda.get_device_name(0)}")
    say("each figure: best / median of 7 alternating windows, ms per call")

    def report(name, ts):
        ts = sorted(ts)
        say(f"  {name:34s} best {ts[0]:8.4f}  median {ts[len(ts) // 2]:8.4f}")
        return ts[0]

    # same answers first (the arg-max of both kernels; top-1 of torch's topk wherever the top-2 gap is not a bf16 tie)
    best, arg, second = ops.rows_top2(d0, d1)
    vmax, amax = ops.rows_argmax(d0, d1)
    assert torch.equal(arg, amax) and torch.equal(best, vmax) and bool((second <= best).all())

    t = alternate({"top2": lambda: ops.rows_top2(d0, d1), "argmax": lambda: ops.rows_argmax(d0, d1)}, iters=50)
    t2, t1 = report("gf_rows_top2", t["top2"]), report("gf_rows_argmax", t["argmax"])
    say(f"  ratio rows_top2 / rows_argmax (best) = {t2 / t1:.3f}")
    flops = 2.0 * B * N * N * D
    say(f"  rows_top2: {flops / (t2 * 1e-3) / 1e12:.1f} TFLOP/s of the 2 B M N D product")

    for label, conf in (("default", {}), ("ratio 0.8 + distance 0.9", {"ratio_thresh": 0.8, "distance_thresh": 0.9})):
        dense = NearestNeighborMatcher(conf).cuda().eval()
        sparse = NearestNeighborMatcher({**conf, "dense_outputs": False}).cuda().eval()
        data = {"descriptors0": d0, "descriptors1": d1}
        ratio, dist = conf.get("ratio_thresh"), conf.get("distance_thresh")
        with torch.no_grad():
            t = alternate({"hip": lambda: dense(data), "hip_nodense": lambda: sparse(data),
                           "torch": lambda: torch_baseline(d0, d1, ratio, dist)}, iters=5)
        say(f"matcher forward, {label}:")
        th = report("this matcher (dense outputs)", t["hip"])
        tn = report("this matcher (dense_outputs: False)", t["hip_nodense"])
        tt = report("stock torch composition", t["torch"])
        say(f"  ratio torch / this matcher (best) = {tt / th:.2f}; without the dense outputs = {tt / tn:.2f}")
        with torch.no_grad():
            same = (dense(data)["matches0"] == torch_baseline(d0, d1, ratio, dist)[0]).float().mean().item()
        say(f"  matches0 equal on {100 * same:.2f} % of the keypoints (torch decides on the bf16-ROUNDED similarity)")


if __name__ == "__main__":
    main()
