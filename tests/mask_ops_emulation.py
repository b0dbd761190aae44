"""TEST INFRASTRUCTURE — CPU stand-ins of ops.det_select / ops.det_nms / ops.box_mask, answered by the restatement of tests/mask_reference.py,
so that the host logic of storygen_amd.mask runs without a GPU.  Never a fallback: the GPU tests run the real kernels through the same
code."""
import contextlib

import numpy as np
import torch

from storygen_amd import ops
from tests import mask_reference as R

CALLS = []
SENTINEL = -12345.0                                               # rows the real kernels leave untouched


def det_select(pred, conf_thres=0.5, classes=(), max_nms=30000, cand=None, ncand=None, workspace=None):
    assert pred.dim() == 3 and pred.dtype in (torch.float16, torch.float32) and cand is None and ncand is None and workspace is None
    B = pred.shape[0]
    CALLS.append(("det_select", tuple(pred.shape), float(conf_thres), tuple(classes), int(max_nms)))
    cand = torch.full((B, max_nms, 6), SENTINEL, dtype=torch.float32)
    ncand = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        c = R.select(pred[b].numpy(), conf_thres, tuple(classes), max_nms)
        cand[b, :len(c)] = torch.from_numpy(c)
        ncand[b] = len(c)
    return cand, ncand


def det_nms(cand, ncand, geom, iou_thres=0.6, agnostic=False, max_det=300, det=None, count=None):
    assert cand.dtype == torch.float32 and ncand.dtype == torch.int32 and geom.dtype == torch.float32 and det is None and count is None
    B = cand.shape[0]
    CALLS.append(("det_nms", tuple(cand.shape), float(iou_thres), bool(agnostic), int(max_det)))
    det = torch.full((B, max_det, 6), SENTINEL, dtype=torch.float32)
    count = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        c = cand[b, :int(ncand[b])].numpy()
        rows = c[R.nms(c, iou_thres, agnostic, max_det)].copy()
        pad_x, pad_y, gain, w0, h0 = (np.float32(v) for v in geom[b].tolist())
        with np.errstate(all="ignore"):
            for k, (pad, hi) in enumerate(((pad_x, w0), (pad_y, h0), (pad_x, w0), (pad_y, h0))):
                v = (rows[:, k] - pad) / gain
                rows[:, k] = np.rint(np.minimum(np.fmax(v, np.float32(0)), hi))
        det[b, :len(rows)] = torch.from_numpy(rows)
        count[b] = len(rows)
    return det, count


def box_mask(h0, w0, det=None, count=None, text=None, out=None, covered=None):
    assert out is None and (det is None) == (count is None)
    CALLS.append(("box_mask", int(h0), int(w0), 0 if text is None else int(text.shape[0])))
    rows = det[:int(count[0])].numpy() if det is not None else None
    mask, n = R.paint(h0, w0, rows, None if text is None else text.numpy())
    if covered is None:
        covered = torch.zeros(1, dtype=torch.int32)
    covered[0] = n
    return torch.from_numpy(mask), covered


@contextlib.contextmanager
def patched_mask_ops():
    """Yields the list of calls."""
    saved = ops.det_select, ops.det_nms, ops.box_mask
    del CALLS[:]
    try:
        ops.det_select, ops.det_nms, ops.box_mask = det_select, det_nms, box_mask
        yield CALLS
    finally:
        ops.det_select, ops.det_nms, ops.box_mask = saved
