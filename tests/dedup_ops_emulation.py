"""TEST INFRASTRUCTURE — tests/clip_u8_ops_emulation.py's CPU stand-ins extended by ops.adjacent_cosine, answered by the restatement of
tests/dedup_reference.py, so that the host logic of DinoVitEngine, the drop-in DinoVisionTransformer and storygen_amd.dedup runs without a
GPU.  Never a fallback: the GPU tests run the real kernels through the same code."""
import contextlib

import torch

from storygen_amd import ops
from tests import dedup_reference as D
from tests.clip_u8_ops_emulation import patched_u8_ops

CALLS = []


def adjacent_cosine(feats, threshold=0.75, eps=1e-8, sim=None, drop=None):
    assert feats.dtype == torch.float32 and feats.dim() == 2 and sim is None and drop is None
    CALLS.append(("adjacent_cosine", tuple(feats.shape), float(threshold)))
    s, d = D.adjacent_cosine(feats.numpy(), threshold, eps)
    return torch.from_numpy(s), torch.from_numpy(d.astype("uint8"))


@contextlib.contextmanager
def patched_dedup_ops():
    """Yields (adjacent_cosine calls, clip_patchify_u8 calls, attention / patchify calls)."""
    saved = ops.adjacent_cosine
    del CALLS[:]
    try:
        with patched_u8_ops() as (u8_calls, calls):
            ops.adjacent_cosine = adjacent_cosine
            yield CALLS, u8_calls, calls
    finally:
        ops.adjacent_cosine = saved
