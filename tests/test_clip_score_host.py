"""Host logic of ClipVisionEngine / ClipScorer on the CPU: the engines run over the torch emulation of the kernels
(tests/clip_ops_emulation.py) and are compared with the restatements of tests/clip_vision_reference.py.  The real kernels run the same
engine code in tests/test_clip_score_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import encoders_oracle as eo
from tests import clip_vision_reference as R
from tests.clip_ops_emulation import patched_clip_ops


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def tiny_states(seed=0, hidden=64, heads=2, image=32, patch=8, proj=32, layers=2):
    """fp16-representable vision + text state dicts with non-trivial LayerNorms (identity norms would hide a swapped weight / bias)."""
    from storygen_amd.encoders import clip_text_param_shapes, clip_vision_param_shapes, init_state
    shapes = clip_vision_param_shapes(hidden, 2 * hidden, layers, image, patch, proj)
    tshapes = clip_text_param_shapes(vocab_size=96, hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=layers)
    tshapes["text_projection.weight"] = (proj, hidden)
    vsd, tsd = init_state(shapes, seed), init_state(tshapes, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    for sd in (vsd, tsd):
        for k in sd:
            if "norm" in k:
                sd[k] = sd[k] + 0.2 * torch.randn(sd[k].shape, generator=g)
            if "patch_embedding" in k or "class_embedding" in k or "position_embedding" in k:
                sd[k] = sd[k] * 10                      # embeddings of the order of a trained model's, not 0.02
            sd[k] = sd[k].half().float()
    return vsd, tsd


@pytest.mark.parametrize("hw", [(32, 32), (81, 48)])
def test_vision_engine_host_logic_matches_restatement(hw):
    from storygen_amd.encoders import ClipVisionEngine
    vsd, _ = tiny_states()
    x = torch.rand(3, 3, *hw, generator=torch.Generator().manual_seed(1))
    want_e, want_h = R.vision_forward(vsd, R.preprocess(x, 32), heads=2)
    with patched_clip_ops():
        eng = ClipVisionEngine(vsd, "cpu", heads=2)
        embeds, hidden = eng(x)
        e2, h2 = eng(x * 2 - 1, in_scale=0.5, in_shift=0.5)
    assert tuple(embeds.shape) == (3, 32) and tuple(hidden.shape) == (3, 17, 64)
    assert rel(hidden, want_h) < 3e-3 and rel(embeds, want_e) < 1e-2
    assert rel(h2, want_h) < 3e-3 and rel(e2, want_e) < 1e-2
    # the emulated engine and the restatement with fp16 rounding points are the same computation
    r_e, r_h = R.vision_forward(vsd, R.preprocess(x, 32), heads=2, round_operands=True)
    assert rel(hidden, r_h) < 2e-4 and rel(embeds, r_e) < 5e-4


def test_encode_pixels_is_the_model_forward():
    from storygen_amd.encoders import ClipVisionEngine
    vsd, _ = tiny_states(seed=3)
    px = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(2))
    want_e, want_h = R.vision_forward(vsd, px, heads=2)
    with patched_clip_ops():
        eng = ClipVisionEngine(vsd, "cpu", heads=2)
        embeds, hidden = eng.encode_pixels(px)
        with pytest.raises(ValueError):
            eng.encode_pixels(torch.zeros(1, 3, 64, 64))
        with pytest.raises(ValueError):
            eng(torch.zeros(3, 32, 32))
    assert rel(hidden, want_h) < 3e-3 and rel(embeds, want_e) < 1e-2


def test_scorer_host_logic():
    from storygen_amd.clip_score import ClipScorer
    vsd, tsd = tiny_states(seed=5)
    vcfg = dict(hidden_size=64, num_attention_heads=2, image_size=32, patch_size=8)
    tcfg = dict(hidden_size=64, num_attention_heads=2)
    g = torch.Generator().manual_seed(9)
    a, b = torch.rand(3, 40, 56, 3, generator=g).numpy(), torch.rand(3, 40, 56, 3, generator=g).numpy()
    ids = torch.randint(0, 95, (3, 77), generator=g)
    ids[:, 20] = 95
    nchw = lambda t: torch.from_numpy(t).permute(0, 3, 1, 2)   # noqa: E731
    fa, fb = (R.vision_forward(vsd, R.preprocess(nchw(t), 32), heads=2)[0] for t in (a, b))
    ft = eo.clip_text_forward(tsd, ids, heads=2)[1] @ tsd["text_projection.weight"].t()
    with patched_clip_ops():
        sc = ClipScorer({**vsd, **tsd}, vcfg, {**vsd, **tsd}, tcfg, device="cpu")       # one CLIPModel-style dict serves both towers
        ci, ct, same = sc.clip_i(a, b), sc.clip_t(a, ids), sc.clip_i(a, a)
        ci_t = sc.clip_i(nchw(a), nchw(b))
        assert rel(sc.text_features(ids), ft) < 1e-2
        with pytest.raises(RuntimeError, match="text tower"):
            ClipScorer(vsd, vcfg, device="cpu").clip_t(a, ids)
        with pytest.raises(ValueError, match="pair up"):
            sc.clip_i(a, b[:2])
    assert ci.dtype == torch.float32 and tuple(ci.shape) == (3,)
    assert torch.equal(ci, ci_t)
    assert float((same - 1).abs().max()) < 1e-6
    assert float((ci - R.cosine(fa, fb)).abs().max()) < 5e-3 and float((ct - R.cosine(fa, ft)).abs().max()) < 5e-3
    assert np.isfinite(float(ci.mean()))
