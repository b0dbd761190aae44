"""TEST INFRASTRUCTURE — tests/clip_u8_ops_emulation.py's CPU stand-ins extended by ops.align_cost and ops.dtw_path, answered by the
restatement of tests/align_reference.py, so that the host logic of storygen_amd.align runs without a GPU.  Never a fallback: the GPU tests
run the real kernels through the same code."""
import contextlib

import numpy as np
import torch

from storygen_amd import ops
from tests import align_reference as A
from tests.clip_u8_ops_emulation import patched_u8_ops

CALLS = []


def align_cost(frame_feats, sent_feats, frame_times, sent_times, out=None):
    assert frame_feats.dtype == sent_feats.dtype == torch.float32 and frame_times.dtype == sent_times.dtype == torch.float64
    assert sent_feats.is_contiguous() and tuple(frame_times.shape) == (frame_feats.shape[0],) and tuple(sent_times.shape) == (sent_feats.shape[0],)
    CALLS.append(("align_cost", tuple(frame_feats.shape), tuple(sent_feats.shape)))
    M = torch.from_numpy(A.cost_matrix(frame_feats.numpy(), sent_feats.numpy(), frame_times.numpy(), sent_times.numpy()))
    return M if out is None else out.copy_(M)


def dtw_path(cost, return_acc=False):
    assert cost.dtype == torch.float64 and cost.dim() == 2
    r, c = cost.shape
    CALLS.append(("dtw_path", (r, c)))
    p, acc, codes = A.dtw(cost.numpy())
    path = torch.full((r + c - 1, 2), -7, dtype=torch.int32)
    path[:len(p)] = torch.tensor(p, dtype=torch.int32)
    out = (path, torch.tensor([len(p)], dtype=torch.int32), torch.from_numpy(codes))
    return out + (torch.from_numpy(np.ascontiguousarray(acc)),) if return_acc else out


@contextlib.contextmanager
def patched_align_ops():
    saved = (ops.align_cost, ops.dtw_path)
    del CALLS[:]
    try:
        with patched_u8_ops():
            ops.align_cost, ops.dtw_path = align_cost, dtw_path
            yield CALLS
    finally:
        ops.align_cost, ops.dtw_path = saved
