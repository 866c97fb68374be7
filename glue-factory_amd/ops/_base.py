"""Helpers every op family shares: dtype codes, device / stream checks, raw pointers, attention strides."""
import torch

from .. import lib as _lib

F32, BF16 = 0, 1


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise RuntimeError(f"glue_factory_amd kernels take float32 or bfloat16, got {t.dtype}")


def _chk(*ts):
    """Every launcher enqueues on the CURRENT device's current stream with raw pointers: tensors on another
    GPU would be touched from the wrong stream (faults or silent races), so that is an error, not a fallback."""
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("glue_factory_amd ops need tensors on a HIP device (no CPU fallback)")
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise RuntimeError(f"tensor on cuda:{t.device.index} but the current device is cuda:{cur}: call "
                               "torch.cuda.set_device (one process per GPU) before using glue_factory_amd ops")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _s3(t):
    """(batch, token, head) element strides of a [B,N,H,D] view with contiguous D."""
    assert t.dim() == 4 and t.stride(3) == 1, "attention operands must be [B,N,H,D] with contiguous D"
    return _lib.strides(t.stride(0), t.stride(1), t.stride(2))
