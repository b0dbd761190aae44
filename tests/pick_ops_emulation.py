"""TEST INFRASTRUCTURE — tests/clip_ops_emulation.py's torch/CPU stand-ins extended by the two entry points PickScore adds (the encoder attention
and the zero-padded patch rows), so that the host logic of ClipVisionEngine(wide=True), PickScorer and the drop-in CLIPModel runs without a GPU.
Each stand-in records its calls in CALLS (name, T, D) for the dispatch tests.  Never a fallback: the GPU tests run the real kernels through the
same code."""
import contextlib

import torch

from storygen_amd import ops
from tests import clip_ops_emulation as E
from tests import clip_vision_reference as R
from tests.ops_emulation import _store
from tests.ops_emulation import attention_small as _attention_small

CALLS = []


def attention_small(q, k, v, out, heads, scale, causal, key_bias=None):
    CALLS.append(("attention_small", q.shape[1], q.shape[2] // heads))
    return _attention_small(q, k, v, out, heads, scale, causal, key_bias)


def attention_enc(q, k, v, out, heads, scale, causal, key_bias=None):
    B, T, Cq = q.shape
    D = Cq // heads
    assert 1 <= T <= 1024 and D % 8 == 0 and 8 <= D <= 128
    assert all(t.dtype == torch.float16 and t.stride(-1) == 1 and t.stride(1) % 8 == 0 and t.stride(1) >= Cq for t in (q, k, v, out))
    CALLS.append(("attention_enc", T, D))
    qh, kh, vh = (t.float().view(B, T, heads, D).transpose(1, 2) for t in (q, k, v))
    s = (qh * scale) @ kh.transpose(-1, -2)
    if causal:
        s = s + torch.full((T, T), float("-inf")).triu(1)
    if key_bias is not None:
        s = s + key_bias[:, None, None, :]
    return _store(out, (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, T, Cq))


def clip_patchify(x, out, S, ps, mean, std, in_scale=1.0, in_shift=0.0, kpad=None):
    if kpad is None:
        return E.clip_patchify(x, out, S, ps, mean, std, in_scale, in_shift)
    K = 3 * ps * ps
    assert x.dim() == 4 and x.shape[1] == 3 and S % ps == 0 and K % 4 == 0 and kpad % 8 == 0 and K <= kpad <= out.shape[1]
    CALLS.append(("clip_patchify_padk", K, kpad))
    out[:, :K] = R.patch_rows(R.preprocess(x, S, in_scale, in_shift, mean, std), ps).to(out.dtype)
    out[:, K:kpad] = 0
    return out


@contextlib.contextmanager
def patched_pick_ops():
    saved = (ops.clip_patchify, ops.attention_small, ops.attention_enc)
    del CALLS[:]
    try:
        with E.patched_clip_ops():
            ops.clip_patchify, ops.attention_small, ops.attention_enc = clip_patchify, attention_small, attention_enc
            yield CALLS
    finally:
        ops.clip_patchify, ops.attention_small, ops.attention_enc = saved
