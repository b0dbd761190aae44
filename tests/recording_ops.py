"""TEST INFRASTRUCTURE — a recording stand-in for storygen_amd.ops: every wrapper call becomes one log entry and nothing is computed.
It makes the HOST side of UNetEngine.forward (which launches, in which order, on which views of which buffers, with which scalars) a
fact that can be compared on the CPU (tests/test_engine_launch_trace.py); it says nothing about the kernels.

An entry is {"op": name, "args": [...], "kw": {...}}.  A tensor anywhere inside (also in the tuples of gemm_pair / attention_pair and in
ln= / stats= / split= / short= / pstats=) is written as {"T": [storage ordinal, storage offset, shape, strides, dtype]}; storages are
numbered in order of first appearance since the last reset().  Tuples become lists; anything that is not a number, string, bool or None
is written as its repr.

The host-side queries answer by a fixed rule of the shapes, chosen so that a two-level UNet on a 16x16 latent (256 and 64 tokens)
reaches every branch of the engine:
    groupnorm_uses_pstats    HW >= 256                  (the large level takes producer statistics, the small one does not)
    groupnorm_is_fused       HW <= 64                   (the small level is the one-launch GroupNorm that can reduce split-K slices)
    conv3x3_planned_splits   3 slices from 128 input channels on, else 1
    conv3x3_stats_rows       64, or 0 for an upsampling convolution (a launch that cannot emit statistics)
    gemm_stats_rows          64, or 0 when K > 256 (the merged K = 5C proj_out cannot, the plain one can)
    ff_fused_supported       False;  *_workspace_bytes, attention_f8_bytes, new_workspace: small fixed sizes"""
import contextlib

import torch

from storygen_amd import ops as _real


def _planned_splits(x, w_krsc, out, **kw):
    return 3 if x.shape[3] >= 128 else 1


def _conv_stats_rows(x, w_krsc, out, **kw):
    return 0 if kw.get("upsample2x") else 64


def _gemm_stats_rows(a, w, out, **kw):
    return 64 if a.shape[1] <= 256 else 0


QUERIES = {
    "groupnorm_uses_pstats": lambda HW, Cc, groups: HW >= 256,
    "groupnorm_is_fused": lambda HW, Cc, groups: HW <= 64,
    "conv3x3_planned_splits": _planned_splits,
    "conv3x3_stats_rows": _conv_stats_rows,
    "gemm_stats_rows": _gemm_stats_rows,
    "ff_fused_supported": lambda Cc: False,
    "groupnorm_workspace_bytes": lambda B, groups: 8 * B * groups,
    "gemm_workspace_bytes": lambda M, N, split_k=0: 0,
    "attention_f8_bytes": lambda B, heads, N, transposed: B * heads * N * 40,
    "new_workspace": lambda nbytes, device: torch.empty(256, dtype=torch.uint8, device=device),
}


class RecordingOps:
    """Stands where the engine expects the `ops` module: constants come from the real one, queries from QUERIES, and every other
    attribute is a function that logs its call and returns None."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.log = []
        self._ordinal = {}
        self._alive = []          # keeps every storage seen alive: an address is never handed out twice within one log

    def _enc(self, v):
        if torch.is_tensor(v):
            key = v.untyped_storage().data_ptr()
            if key not in self._ordinal:
                self._ordinal[key] = len(self._ordinal)
                self._alive.append(v)
            return {"T": [self._ordinal[key], v.storage_offset(), list(v.shape), list(v.stride()), str(v.dtype).replace("torch.", "")]}
        if isinstance(v, (tuple, list)):
            return [self._enc(x) for x in v]
        if isinstance(v, dict):
            return {str(k): self._enc(x) for k, x in v.items()}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return repr(v)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name.isupper():
            return getattr(_real, name)
        if not hasattr(_real, name):
            raise AttributeError(f"storygen_amd.ops has no {name}")
        answer = QUERIES.get(name)

        def call(*args, **kw):
            self.log.append({"op": name, "args": self._enc(args), "kw": self._enc(kw)})
            return None if answer is None else answer(*args, **kw)
        return call


@contextlib.contextmanager
def installed(engine_module):
    """Replace `engine_module.ops` by a fresh RecordingOps for the duration of the block (and answer the one stream query forward() makes
    of the device runtime, so that an engine on "cpu" needs none)."""
    rec = RecordingOps()
    saved = engine_module.ops, torch.cuda.is_current_stream_capturing
    engine_module.ops, torch.cuda.is_current_stream_capturing = rec, lambda: False
    try:
        yield rec
    finally:
        engine_module.ops, torch.cuda.is_current_stream_capturing = saved
