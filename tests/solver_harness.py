"""What tests/test_gpu_h_solver.py and tests/test_gpu_e_solver.py share in calling a raw solver entry: guarded buffers and the
"call twice, equal bits, guards intact" wrapper."""
import numpy as np
import torch

G = 64                         # guard elements on either side of every output and of the workspace


def load():
    from glue_factory_amd import lib
    return lib, lib.load()


def guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")
    return buf, buf[G:G + n].view(shape)


def intact(buf, fill, what):
    assert bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all()), f"guard band of {what} overwritten"


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()


def run_once(entry, ws_entry, B, M, T, spec, args):
    """One call of `entry` with a guarded workspace of `ws_entry`(B, M, T) bytes and guarded outputs: spec {name: (shape,
    dtype, fill)} in the order of the entry's output pointers, args(ws pointer, its bytes, output pointers) -> the entry's
    arguments without the stream.  The guards are checked; the outputs come back as clones."""
    lib, L = load()
    nbytes = int(getattr(L, ws_entry)(B, M, T))
    assert nbytes > 0 and nbytes % 16 == 0
    ws_buf, ws = guarded((nbytes,), torch.uint8, 0x5A)
    bufs = {k: guarded(*v) for k, v in spec.items()}
    code = getattr(L, entry)(*args(ws.data_ptr(), nbytes, [view.data_ptr() for _, view in bufs.values()]),
                             torch.cuda.current_stream().cuda_stream)
    lib.check(code, entry)
    torch.cuda.synchronize()
    intact(ws_buf, 0x5A, "workspace")
    for k, (buf, _) in bufs.items():
        intact(buf, spec[k][2], k)
    return {k: v[1].clone() for k, v in bufs.items()}


def run_twice(once):
    """once() twice: equal bits.  numpy outputs, `inliers` and `success` (0 / 1 bytes) as bool."""
    r1, r2 = once(), once()
    for k in r1:
        assert torch.equal(r1[k].view(torch.uint8), r2[k].view(torch.uint8)), f"{k}: two calls differ"
    out = {k: v.cpu().numpy() for k, v in r1.items()}
    assert set(np.unique(out["inliers"])) <= {0, 1} and set(np.unique(out["success"])) <= {0, 1}
    out["inliers"], out["success"] = out["inliers"].astype(bool), out["success"].astype(bool)
    return out
