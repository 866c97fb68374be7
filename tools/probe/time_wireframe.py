"""Timing record of the wireframe stage alone (lines/wireframe.py: wireframe_from_parts, the sub-extractors' outputs resident
on the device) at GlueStick's benchmark geometry: 64 images of 1024^2, 2048 keypoints, 512 lines, C = 256, dense map
128 x 128, forced-count mode.  Random data: line end points are jittered copies of shared base points (so that junctions
merge and chain), a quarter of the keypoints lie next to end points (so that they are suppressed).  5 warm-ups, then 20
timed calls between device events, of
  * the kernels (gf_wf_cluster / _suppress / _descriptors / _associativity: 5 kernel launches for the whole batch, plus the
    6 elementwise torch kernels that draw and scale the two random fills), and
  * "torch form + sklearn": the torch form with its clustering replaced by sklearn's DBSCAN on a host copy of each image's
    end points -- the reference's arrangement (wireframe.py:53-56) on the same box; its time is dominated by the host.
Also whether the two agree on every decision.
    python tools/probe/time_wireframe.py [out.txt]          (default: profiles/wireframe_timing.txt)"""
import os
import sys

import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
from glue_factory_amd.conf import Conf  # noqa: E402
from glue_factory_amd.lines import wireframe as wf  # noqa: E402

B, HW, N, L, C, S, EPS = 64, 1024, 2048, 512, 256, 8, 3
WARMUP, RUNS = 5, 20


def scene(seed=0):
    g = torch.Generator().manual_seed(seed)
    base = 8 + torch.rand(B, L // 2 + 1, 2, generator=g) * (HW - 16)
    pick = torch.randint(0, L // 2 + 1, (B, 2 * L), generator=g)
    ang, rad = torch.rand(B, 2 * L, generator=g) * 6.2831853, 0.8 * EPS * torch.rand(B, 2 * L, generator=g).sqrt()
    ends = base.gather(1, pick[..., None].expand(B, 2 * L, 2)) + torch.stack([rad * ang.cos(), rad * ang.sin()], -1)
    kp = torch.rand(B, N, 2, generator=g) * (HW - 1)
    kp[:, :N // 4] = ends[:, :N // 4] + (torch.rand(B, N // 4, 2, generator=g) - 0.5) * 2
    pred = {"lines": ends.reshape(B, L, 2, 2), "line_scores": torch.rand(B, L, generator=g), "keypoints": kp,
            "keypoint_scores": torch.rand(B, N, generator=g) + 0.01,
            "descriptors": torch.nn.functional.normalize(torch.randn(B, N, C, generator=g), dim=-1),
            "dense_descriptors": torch.nn.functional.normalize(torch.randn(B, C, HW // S, HW // S, generator=g), dim=1)}
    pred = {k: v.cuda() for k, v in pred.items()}
    pred["dense_descriptors"] = pred["dense_descriptors"].contiguous(memory_format=torch.channels_last)
    return pred


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def sklearn_clusters(ends, eps):
    from sklearn.cluster import DBSCAN
    labels = DBSCAN(eps=eps, min_samples=1).fit(ends.cpu().numpy()).labels_
    return torch.tensor(labels, dtype=torch.long, device=ends.device)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "wireframe_timing.txt")
    out = open(path, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    pred = scene()
    params = Conf.create({"merge_points": True, "merge_line_endpoints": True, "nms_radius": EPS})
    shape = (B, 1, HW, HW)
    say(f"wireframe stage, B={B} image {HW}^2 N={N} L={L} C={C} map {HW // S}^2, forced counts, {torch.cuda.get_device_name(0)}")
    say(f"{WARMUP} warm-ups, {RUNS} timed calls per form")
    kernels = lambda: wf.wireframe_from_parts(pred, shape, params, True, True, fused=True)
    forms = {"kernels (5 launches + 6 fill kernels)": kernels}
    try:
        import sklearn  # noqa: F401
        wf.cluster_endpoints = sklearn_clusters          # the torch form's clustering, as the reference arranges it
        forms["torch form + sklearn DBSCAN on the host"] = lambda: wf.wireframe_from_parts(pred, shape, params, True, True, fused=False)
    except ImportError:
        say("sklearn is not installed: the torch form is not timed")
    results = {k: fn() for k, fn in forms.items()}
    got = results["kernels (5 launches + 6 fill kernels)"]
    say(f"junctions per image: min {int(got['num_junctions'].min())}, max {int(got['num_junctions'].max())} of {2 * L}; "
        f"suppressed keypoints per image: mean {float((got['keypoint_scores'][:, 2 * L:] == 0).sum(1).float().mean()):.0f}")
    if len(results) == 2:
        ref = list(results.values())[1]
        same = all(torch.equal(got[k], ref[k]) for k in ("lines_junc_idx", "num_junctions", "pl_associativity")) and \
            torch.equal(got["keypoint_scores"] == 0, ref["keypoint_scores"] == 0)
        say(f"decisions equal (junction ids, counts, associativity, suppressed mask): {same}")
    del results, got
    for k, fn in forms.items():
        for _ in range(WARMUP):
            fn()
        t = sorted(timed(fn) for _ in range(RUNS))
        say(f"  {k}: median {t[len(t) // 2]:.3f} ms, best {t[0]:.3f} ms, worst {t[-1]:.3f} ms per call")
    out.close()


if __name__ == "__main__":
    main()
