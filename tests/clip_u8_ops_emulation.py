"""TEST INFRASTRUCTURE — tests/pick_ops_emulation.py's CPU stand-ins extended by ops.clip_patchify_u8, answered by the restatement of
tests/clip_u8_reference.py, so that the uint8 dispatch of ClipVisionEngine, ClipScorer, PickScorer and StoryGenerator runs without a GPU.
Every call is recorded in U8_CALLS as (input shape, (Hr, Wr, top, left), kpad).  Never a fallback: the GPU tests run the real kernel
through the same code."""
import contextlib

import torch

from storygen_amd import ops
from tests import clip_u8_reference as U
from tests.pick_ops_emulation import patched_pick_ops

U8_CALLS = []
_geometry = ops.clip_u8_geometry


def clip_patchify_u8(x_u8, out, S, ps, mean, std, geometry=None, crop="torchvision", kpad=None, out_u8=None):
    assert x_u8.dtype == torch.uint8 and x_u8.dim() == 4 and x_u8.shape[3] == 3 and out.dtype == torch.float16
    geom = tuple(geometry) if geometry is not None else _geometry(x_u8.shape[1], x_u8.shape[2], S, crop)
    kpad = (3 * ps * ps + 7) & ~7 if kpad is None else kpad
    assert tuple(out.shape[:1]) == (x_u8.shape[0] * (S // ps) ** 2,) and out.shape[1] >= kpad
    U8_CALLS.append((tuple(x_u8.shape), geom, kpad))
    u8, rows = U.reference(x_u8.numpy(), S, ps, geom=geom, kpad=kpad, mean=mean, std=std)
    out[:, :kpad] = torch.from_numpy(rows)
    if out_u8 is not None:
        out_u8.copy_(torch.from_numpy(u8))
    return out


@contextlib.contextmanager
def patched_u8_ops():
    saved = ops.clip_patchify_u8
    del U8_CALLS[:]
    try:
        with patched_pick_ops() as calls:
            ops.clip_patchify_u8 = clip_patchify_u8
            yield U8_CALLS, calls
    finally:
        ops.clip_patchify_u8 = saved
