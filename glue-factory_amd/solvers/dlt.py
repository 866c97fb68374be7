"""Hartley-normalised (weighted) DLT homography on the GPU: gf_h_dlt (csrc/h_solver.hip), the refit stage of the RANSAC solver
on its own.  Gives ``find_homography_dlt(pts0, pts1, scores)`` of gluefactory/eval/utils.py:241-261 its meaning without
kornia: normalise both point sets (centroid, mean distance sqrt 2), build A^T W A, take the eigenvector of the smallest
eigenvalue, de-normalise, scale to H[2][2] == 1.  Batched over pairs with different match counts; no host read."""
import torch

from .. import lib as _lib


def _prep(kpts0, kpts1, matches0):
    if not kpts0.is_cuda:
        raise RuntimeError("homography solver: tensors must be on a HIP device (h_solver.hip has no CPU fallback)")
    b, m = kpts0.shape[:2]
    n = kpts1.shape[1]
    assert kpts0.shape == (b, m, 2) and kpts1.shape == (b, n, 2) and matches0.shape == (b, m)
    return kpts0.float().contiguous(), kpts1.float().contiguous(), matches0.long().contiguous(), b, m, n


def workspace(entry, b, m, t, device):
    """The workspace of a solver call: entry = "gf_h_ws_bytes" or "gf_e_ws_bytes"."""
    nbytes = int(getattr(_lib.load(), entry)(b, m, t))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


@torch.no_grad()
def homography_dlt(kpts0, kpts1, matches0, weights=None):
    """kpts0 [B,M,2], kpts1 [B,N,2], matches0 [B,M] (-1 = no match), weights [B,M] or None -> (H [B,3,3] fp32, success [B]
    bool).  A pair with fewer than 4 matches, or whose solution has h22 ~ 0 or a non-finite entry, gets the identity and
    success False."""
    with torch.autocast(device_type="cuda", enabled=False):
        kp0, kp1, m0, b, m, n = _prep(kpts0, kpts1, matches0)
        dev = kp0.device
        H = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
        success = torch.empty((b,), dtype=torch.bool, device=dev)
        if m == 0 or n == 0:
            H.copy_(torch.eye(3, device=dev))
            return H, success.zero_()
        wt = None
        if weights is not None:
            assert weights.shape == (b, m)
            wt = weights.float().contiguous()
        ws, nbytes = workspace("gf_h_ws_bytes", b, m, 1, dev)
        _lib.check(_lib.load().gf_h_dlt(kp0.data_ptr(), kp1.data_ptr(), m0.data_ptr(), None if wt is None else wt.data_ptr(),
                                        b, m, n, ws.data_ptr(), nbytes, H.data_ptr(), success.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "gf_h_dlt")
    return H, success
