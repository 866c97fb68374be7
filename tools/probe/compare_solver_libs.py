"""Bit comparison of the two-view solvers of two builds of libgf_amd.so (say a parent commit's and this tree's), both loaded
into one process: every output tensor of gf_h_ransac, gf_h_dlt, gf_e_ransac, gf_e_pose and gf_hl_ransac, debug outputs
included, on the small scenes of tests/h_solver_cases.py, e_solver_cases.py and hl_solver_cases.py, and the three workspace
sizes.  Every buffer starts from the same fill in both runs, so bytes a kernel leaves alone compare equal.  Exit status 1 when
anything differs:
    python tools/probe/compare_solver_libs.py OTHER/libgf_amd.so glue-factory_amd/libgf_amd.so [out.txt]"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import e_solver_cases as ec  # noqa: E402
import h_solver_cases as hc  # noqa: E402
import hl_solver_cases as hl  # noqa: E402
from glue_factory_amd import lib as gl  # noqa: E402

ENTRIES = ("gf_h_ws_bytes", "gf_h_ransac", "gf_h_dlt", "gf_e_ws_bytes", "gf_e_ransac", "gf_e_pose", "gf_hl_ws_bytes", "gf_hl_ransac")


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ENTRIES:
        fn = getattr(L, name)
        fn.argtypes, fn.restype = gl.SIGNATURES[name], gl._RESTYPE.get(name, ctypes.c_int)
    return L


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()


def call(L, entry, ws_entry, ws_shape, spec, args):
    """One call into buffers of a fixed fill: spec {name: (shape, dtype, fill)} in the order of the entry's output pointers,
    args(ws pointer, bytes, output pointers) -> the arguments without the stream.  A zero-sized output is passed as NULL."""
    nbytes = int(getattr(L, ws_entry)(*ws_shape))
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    out = {k: torch.full(shape, fill, dtype=dtype, device="cuda") for k, (shape, dtype, fill) in spec.items()}
    ptrs = [v.data_ptr() if v.numel() else None for v in out.values()]
    gl.check(getattr(L, entry)(*args(ws.data_ptr(), nbytes, ptrs), torch.cuda.current_stream().cuda_stream), entry)
    torch.cuda.synchronize()
    return out


def h_ransac(L, kp0, kp1, m0, T, lo):
    (B, M), N = m0.shape, kp1.shape[1]
    spec = {"H": ((B, 3, 3), torch.float32, -7.0), "inliers": ((B, M), torch.uint8, 0xAB), "num_inliers": ((B,), torch.int32, -77),
            "success": ((B,), torch.uint8, 0xAB), "samples": ((B, T, 4), torch.int32, -77), "hyp_counts": ((B, T), torch.int32, -77)}
    return call(L, "gf_h_ransac", "gf_h_ws_bytes", (B, M, T), spec, lambda ws, n, o: (
        kp0.data_ptr(), kp1.data_ptr(), m0.data_ptr(), B, M, N, T, hc.TH, lo, hc.SEED, ws, n, *o))


def h_dlt(L, kp0, kp1, m0, wt):
    (B, M), N = m0.shape, kp1.shape[1]
    spec = {"H": ((B, 3, 3), torch.float32, -7.0), "success": ((B,), torch.uint8, 0xAB)}
    return call(L, "gf_h_dlt", "gf_h_ws_bytes", (B, M, 1), spec, lambda ws, n, o: (
        kp0.data_ptr(), kp1.data_ptr(), m0.data_ptr(), None if wt is None else wt.data_ptr(), B, M, N, ws, n, *o))


def e_ransac(L, p0, p1, m0, th, T, lo):
    (B, M), N, S = m0.shape, p1.shape[1], ec.MAXSOL
    spec = {"E": ((B, 3, 3), torch.float32, -7.0), "R": ((B, 3, 3), torch.float32, -7.0), "t": ((B, 3), torch.float32, -7.0),
            "inliers": ((B, M), torch.uint8, 0xAB), "num_inliers": ((B,), torch.int32, -77), "success": ((B,), torch.uint8, 0xAB),
            "samples": ((B, T, 5), torch.int32, -77), "cand": ((B, T, S, 9), torch.float32, -7.0),
            "ncand": ((B, T), torch.int32, -77), "cand_counts": ((B, T, S), torch.int32, -77)}
    return call(L, "gf_e_ransac", "gf_e_ws_bytes", (B, M, T), spec, lambda ws, n, o: (
        p0.data_ptr(), p1.data_ptr(), m0.data_ptr(), th.data_ptr(), B, M, N, T, lo, ec.SEED, ws, n, *o))


def e_pose(L, p0, p1, m0, inliers, E):
    (B, M), N = m0.shape, p1.shape[1]
    spec = {"R": ((B, 3, 3), torch.float32, -7.0), "t": ((B, 3), torch.float32, -7.0), "num_front": ((B,), torch.int32, -77)}
    return call(L, "gf_e_pose", "gf_e_ws_bytes", (B, M, 1), spec, lambda ws, n, o: (
        p0.data_ptr(), p1.data_ptr(), m0.data_ptr(), inliers.data_ptr(), E.data_ptr(), B, M, N, ws, n, *o))


def hl_ransac(L, a, T, lo):
    kp0, kp1, m0, l0, l1, lm0 = a
    (B, M), N, Ln, L1 = m0.shape, kp1.shape[1], lm0.shape[1], l1.shape[1]
    p = lambda t, n: t.data_ptr() if n > 0 else None              # an empty list is passed with NULL pointers
    spec = {"H": ((B, 3, 3), torch.float32, -7.0), "inliers": ((B, M), torch.uint8, 0xAB), "line_inliers": ((B, Ln), torch.uint8, 0xAB),
            "num_inliers": ((B, 2), torch.int32, -77), "success": ((B,), torch.uint8, 0xAB), "samples": ((B, T, 4), torch.int32, -77),
            "hyp_H": ((B, T, 9), torch.float32, -7.0), "hyp_counts": ((B, T, 2), torch.int32, -77)}
    return call(L, "gf_hl_ransac", "gf_hl_ws_bytes", (B, M, Ln, T), spec, lambda ws, n, o: (
        p(kp0, M), p(kp1, M), p(m0, M), p(l0, Ln), p(l1, Ln), p(lm0, Ln), B, M, N, Ln, L1, T, hl.TH, lo, hl.SEED, ws, n, *o))


def stack(scenes, keys, dtypes):
    return [dev(np.stack([np.asarray(s[k]) for s in scenes]), d) for k, d in zip(keys, dtypes)]


H_KEYS = (("kpts0", "kpts1", "matches0"), (torch.float32, torch.float32, torch.int64))
E_KEYS = (("p0n", "p1n", "matches0", "th"), (torch.float32, torch.float32, torch.int64, torch.float32))
HL_KEYS = (("kpts0", "kpts1", "matches0", "lines0", "lines1", "line_matches0"),
           (torch.float32, torch.float32, torch.int64, torch.float32, torch.float32, torch.int64))


def cases():
    """(label, run) pairs: run(L) -> {name: tensor} of one library."""
    out = []
    T = 2 * hc.HYPS + 5
    h_inputs = [(f"planted {spec}", [hc.planted_scene(*spec, 0)]) for spec in hc.PLANTED]
    model, K, M, N = hc.PLANTED[0]
    h_inputs.append(("batch with 0, 4 and K matches", [hc.small_scene(model, 0, M, N), hc.small_scene(model, 4, M, N),
                                                       hc.planted_scene(model, K, M, N, 2)]))
    for label, scenes in h_inputs:
        a = stack(scenes, *H_KEYS)
        for lo in (0, 2):
            out.append((f"gf_h_ransac {label} lo_iters={lo}", lambda L, a=a, lo=lo: h_ransac(L, *a, T, lo)))
        wt = dev(np.random.RandomState(5).uniform(0.1, 1, size=tuple(a[2].shape)), torch.float32)
        out.append((f"gf_h_dlt {label}", lambda L, a=a: h_dlt(L, *a, None)))
        out.append((f"gf_h_dlt {label} weighted", lambda L, a=a, wt=wt: h_dlt(L, *a, wt)))

    def e_case(a, T, lo):
        def run(L):
            r = e_ransac(L, *a, T, lo)
            pose = e_pose(L, *a[:3], r["inliers"], r["E"].contiguous())
            return {**r, **{"pose_" + k: v for k, v in pose.items()}}
        return run

    for noise in (0.0, 0.5):
        a = stack([ec.scene(*spec, noise=noise) for spec in ec.PLANTED], *E_KEYS)
        for lo in (0, 2):
            out.append((f"gf_e_ransac + gf_e_pose planted noise={noise} lo_iters={lo}", e_case(a, ec.PLANTED_T, lo)))
    a = stack([ec.scene(80 + K, K, 0, 40, 36) for K in (0, 4, 5, 12)], *E_KEYS)
    out.append(("gf_e_ransac + gf_e_pose batch with 0, 4, 5 and 12 matches", e_case(a, ec.HYPS + 1, 2)))

    hl_inputs = [(f"planted {name}", [hl.planted_scene(name)], hl.T_FULL) for name in ("points", "lines", "mixed")]
    _, _, _, M, N, Ln, L1, _, _ = hl.PLANTED["mixed"]
    hl_inputs.append(("batch with unequal counts", [hl.build_scene("proj", 0, 0, M, N, Ln, L1, seed=1),
                                                   hl.four_feature_scene(M, N, Ln, L1, 1), hl.planted_scene("mixed", 2)], hl.T_FULL))
    for Kp, Kl in ((hl.TILE - 1, hl.TILE + 1), (hl.TILE, hl.TILE), (hl.TILE + 1, hl.TILE - 1), (0, hl.TILE + 1), (hl.TILE, 0)):
        M, Ln = (hl.TILE + 20 if Kp else 0), (hl.TILE + 9 if Kl else 0)       # (0, .): a call with M = 0; (., 0): with L = 0
        scene = hl.small_scene(Kp, Kl, M, M + 13 if M else 0, Ln, Ln + 5 if Ln else 0)
        hl_inputs.append((f"small scene K_p={Kp} K_l={Kl} M={M} L={Ln}", [scene], hl.HYPS + 1))
    for label, scenes, T_ in hl_inputs:
        a = stack(scenes, *HL_KEYS)
        for lo in (0, 2):
            out.append((f"gf_hl_ransac {label} lo_iters={lo}", lambda L, a=a, T_=T_, lo=lo: hl_ransac(L, a, T_, lo)))
    return out


def main():
    other, this = load(sys.argv[1]), load(sys.argv[2])
    log = open(sys.argv[3], "w") if len(sys.argv) > 3 else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    say(f"{sys.argv[1]} against {sys.argv[2]} on {torch.cuda.get_device_name(0)}")
    tensors = elements = differ = 0
    for label, run in cases():
        a, b = run(other), run(this)
        bad = []
        for k in a:
            x, y = a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)
            tensors, elements = tensors + 1, elements + a[k].numel()
            if not torch.equal(x, y):
                n = int((a[k] != b[k]).sum())
                fl = a[k].is_floating_point()
                gap = float((a[k].double() - b[k].double()).abs().nan_to_num(float("inf")).max()) if fl else float("nan")
                bad.append(f"{k}: {n} of {a[k].numel()} elements differ, largest difference {gap:.3e}")
        differ += len(bad)
        say(f"  {label}: {len(a)} tensors, " + ("equal" if not bad else "DIFFER: " + "; ".join(bad)))
    sizes = 0
    for B, M, Ln, T in ((1, 1, 0, 1), (1, 0, 1, 1), (2, 40, 7, 10), (3, 257, 257, 257), (32, 2048, 512, 3000)):
        got = [(L.gf_h_ws_bytes(B, M, T), L.gf_e_ws_bytes(B, M, T), L.gf_hl_ws_bytes(B, M, Ln, T)) for L in (other, this)]
        sizes += got[0] != got[1]
        say(f"  workspace bytes at (B, M, L, T) = ({B}, {M}, {Ln}, {T}): h, e, hl = {got[0]} | {got[1]}")
    say(f"total: {tensors} tensors, {elements} elements, {differ} tensors differ; {sizes} workspace shapes differ")
    sys.exit(1 if differ or sizes else 0)


if __name__ == "__main__":
    main()
