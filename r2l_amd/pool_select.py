"""Ranking the hard rays of a step on the device (include/r2l_hip.h r2l_pool_select): the k rows of a batch with the largest
per-ray squared error, picked by a radix select instead of a full sort.

select_spec() restates in numpy what the kernel computes — the per-row error with every operation rounded to fp32, the rank key
and the tie rule; it is the specification the tests hold the kernel to.  select() is the ctypes wrapper HardRayPool's
device_select path goes through.
"""
import numpy as np


def row_errors(rgb, target):
    """e_i = (d0*d0 + d1*d1) + d2*d2 of d = rgb[i] - target[i], each operation rounded to fp32: float32[B]."""
    a, b = np.asarray(rgb, dtype=np.float32), np.asarray(target, dtype=np.float32)
    with np.errstate(all="ignore"):
        d = a - b
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def rank_keys(err):
    """The bit pattern of the (non-negative) error as uint32; any NaN -> 0xFFFFFFFF: uint32[B]."""
    err = np.ascontiguousarray(err, dtype=np.float32)
    keys = err.view(np.uint32).copy()
    keys[np.isnan(err)] = np.uint32(0xFFFFFFFF)
    return keys


def select_spec(rgb, target, k):
    """(hard, err) of r2l_pool_select on the rows of rgb / target ([B, 3] arrays or CPU tensors): the first k rows in the order
    (key descending, index ascending), returned in ascending index order as int64[k], and the errors float32[B]."""
    rgb = rgb.numpy() if hasattr(rgb, "numpy") else rgb
    target = target.numpy() if hasattr(target, "numpy") else target
    err = row_errors(rgb, target)
    B, k = err.shape[0], int(k)
    if not 0 <= k <= B:
        raise ValueError("select_spec: need 0 <= k <= B (got k %d, B %d)" % (k, B))
    order = np.argsort(np.uint32(0xFFFFFFFF) - rank_keys(err), kind="stable")  # stable: a tie goes to the lower index
    return np.sort(order[:k]).astype(np.int64), err


def _rows(x, torch):
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3 or x.stride(1) != 1 or x.stride(0) < 3:
        x = x.float().contiguous()
    return x, x.stride(0)


_work = {}  # device -> scratch of the many-workgroup path, grown on demand; shared by the calls of a device, which the training
#             loop makes on one stream (nothing is kept there between calls)


def select(rgb, target, k):
    """The k hardest of the rows rgb[i], target[i] (CUDA [B, 3] fp32, row strides >= 3 floats): int64[k] on the device, in
    ascending index order.  One r2l_pool_select call on the current stream."""
    import torch
    from . import _lib
    if not (rgb.is_cuda and target.is_cuda):
        raise NotImplementedError("pool_select.select runs on the GPU only (r2l_pool_select of libr2l_hip.so); the inputs are on %s"
                                  % rgb.device)
    lib = _lib.load()
    B, k = int(rgb.shape[0]), int(k)
    if target.shape[0] != B:
        raise ValueError("pool_select.select: rgb has %d rows, target %d" % (B, target.shape[0]))
    (a, sa), (b, sb) = _rows(rgb, torch), _rows(target, torch)
    need = lib.r2l_pool_select_work_bytes(B)
    if need < 0:
        _lib.check(1, "r2l_pool_select_work_bytes")
    work = _work.get(rgb.device)
    if work is None or work.numel() < need:
        work = _work[rgb.device] = torch.empty(need, dtype=torch.uint8, device=rgb.device)
    hard = torch.empty(k, dtype=torch.int64, device=rgb.device)
    p = _lib.ptr
    with torch.cuda.device(rgb.device):
        _lib.check(lib.r2l_pool_select(p(a), p(b), sa, sb, B, k, p(hard), None, p(work), _lib.stream()), "r2l_pool_select")
    return hard
