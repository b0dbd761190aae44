"""TEST INFRASTRUCTURE — tests/ops_emulation.py's torch/CPU stand-ins extended by the two entry points of the CLIP image tower's front end, so
that the host logic of ClipVisionEngine and ClipScorer (weight layouts, buffer views, the strided class-row LayerNorm, the pairing of
features) runs without a GPU.  Never a fallback: the GPU tests run the real kernels through the same code."""
import contextlib

from storygen_amd import ops
from tests import clip_vision_reference as R
from tests.ops_emulation import _store, patched_ops


def clip_patchify(x, out, S, ps, mean, std, in_scale=1.0, in_shift=0.0):
    assert x.dim() == 4 and x.shape[1] == 3 and S % ps == 0 and (3 * ps * ps) % 8 == 0
    return _store(out, R.patch_rows(R.preprocess(x, S, in_scale, in_shift, mean, std), ps))


def clip_embed_patches(patches, cls, pos, out, T):
    B, Cc = out.shape[0] // T, out.shape[1]
    v = out.view(B, T, Cc)
    v[:, 0] = cls + pos[0]
    v[:, 1:] = patches.view(B, T - 1, Cc) + pos[1:]
    return out


@contextlib.contextmanager
def patched_clip_ops():
    saved = (ops.clip_patchify, ops.clip_embed_patches)
    try:
        with patched_ops():
            ops.clip_patchify, ops.clip_embed_patches = clip_patchify, clip_embed_patches
            yield
    finally:
        ops.clip_patchify, ops.clip_embed_patches = saved
