"""Pins tests/clip_vision_reference.py (the CPU restatements the GPU tests of the CLIP scorer compare against) to independent ground:
the geometry to numbers computed by hand, the resampling to a direct evaluation of the Keys-kernel definition, the tower to
transformers' CLIPVisionModelWithProjection — and the library's own host-side geometry and argument checks to the same numbers.  No GPU."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import clip_vision_reference as R


# 48 x 80: short side 48 -> 32, long side int(32 * 80 / 48) = int(53.33) = 53; crop (53 - 32) / 2 = 10.5 -> 10 (half to even)
# 81 x 48: short side 48 -> 32, long side int(32 * 81 / 48) = 54; crop (54 - 32) / 2 = 11: an odd offset
# 32 x 32: nothing to resize, nothing to crop
HAND = [((48, 80), (32, 53, 0, 10)), ((80, 48), (53, 32, 10, 0)), ((81, 48), (54, 32, 11, 0)), ((48, 81), (32, 54, 0, 11)),
        ((32, 32), (32, 32, 0, 0)), ((512, 512), (32, 32, 0, 0)),
        ((48, 83), (32, 55, 0, 12))]       # int(32 * 83 / 48) = 55; 23 / 2 = 11.5 -> 12 (half to even goes UP here)


@pytest.mark.parametrize("hw,want", HAND)
def test_geometry_matches_hand_computed_sizes(hw, want):
    assert R.resize_geometry(hw[0], hw[1], 32) == want


@pytest.mark.parametrize("hw,want", HAND)
def test_library_geometry_matches_hand_computed_sizes(hw, want):
    """sg_clip_resize_geometry (host code of the library, what the kernel launch uses) against the same numbers."""
    from storygen_amd import ops
    assert ops.clip_resize_geometry(hw[0], hw[1], 32) == want
    assert ops.clip_resize_geometry(300, 517, 224) == R.resize_geometry(300, 517, 224) == (224, 386, 0, 81)


def _keys(x):
    x = x.abs()
    return torch.where(x < 1, (1.5 * x - 2.5) * x * x + 1, torch.where(x < 2, ((x - 5) * x + 8) * x * -0.5 + 2.0, torch.zeros_like(x)))


def _axis_matrix(n_in, n_out):
    """[n_out, n_in] weights of the antialiased bicubic filter, straight from its definition, in float64."""
    scale = n_in / n_out
    support, inv = 2.0 * max(scale, 1.0), 1.0 / max(scale, 1.0)
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n_in)
        w = _keys((torch.arange(lo, hi, dtype=torch.float64) - c + 0.5) * inv)
        m[i, lo:hi] = w / w.sum()
    return m


@pytest.mark.parametrize("hw", [(32, 32), (73, 73), (20, 20), (81, 48), (48, 80)])
def test_preprocess_matches_the_filter_definition(hw):
    """Keys kernel a = -0.5, half-pixel centres, support 2 * max(scale, 1), truncated and renormalised at the edges; then crop, normalise."""
    H, W = hw
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H + W))
    RH, RW, top, left = R.resize_geometry(H, W, 32)
    full = torch.einsum("oh,bchw,pw->bcop", _axis_matrix(H, RH), x.double() * 2 - 1, _axis_matrix(W, RW))
    m, s = torch.tensor(R.CLIP_MEAN, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(R.CLIP_STD, dtype=torch.float64).view(1, 3, 1, 1)
    want = (full[:, :, top:top + 32, left:left + 32] - m) / s
    got = R.preprocess(x, 32, 2.0, -1.0)
    assert tuple(got.shape) == (2, 3, 32, 32) and got.dtype == torch.float32
    assert float((got.double() - want).abs().max()) < 2e-5
    if hw == (32, 32):
        assert torch.equal(got, ((x * 2.0 - 1.0) - m.float()) / s.float())


def test_patch_rows_are_the_convolution_operand():
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(0))
    w = torch.randn(16, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    want = F.conv2d(x, w, stride=8).flatten(2).transpose(1, 2).reshape(-1, 16)
    assert torch.allclose(R.patch_rows(x, 8) @ w.view(16, -1).t(), want, atol=1e-4)


def test_vision_forward_matches_transformers():
    transformers = pytest.importorskip("transformers")
    if not hasattr(transformers, "CLIPVisionModelWithProjection"):
        pytest.skip("this transformers has no CLIPVisionModelWithProjection")
    torch.manual_seed(3)
    cfg = transformers.CLIPVisionConfig(hidden_size=64, intermediate_size=128, projection_dim=48, num_hidden_layers=2, num_attention_heads=2,
                                        image_size=32, patch_size=8, hidden_act="quick_gelu")
    m = transformers.CLIPVisionModelWithProjection(cfg).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    for k in sd:                                   # identity LayerNorms would hide a swapped weight / bias
        if "norm" in k:
            sd[k] = sd[k] + 0.2 * torch.randn(sd[k].shape, generator=g)
    m.load_state_dict(sd)
    px = torch.randn(3, 3, 32, 32, generator=g)
    with torch.no_grad():
        out = m(pixel_values=px)
    embeds, hidden = R.vision_forward(sd, px, heads=2)
    assert tuple(embeds.shape) == (3, 48) and tuple(hidden.shape) == (3, 17, 64)
    assert float((embeds - out.image_embeds).abs().max()) < 1e-4 * float(out.image_embeds.abs().max())
    assert float((hidden - out.last_hidden_state).abs().max()) < 1e-4 * float(out.last_hidden_state.abs().max())
    # the fp16 rounding points move the result a little and only a little
    e16, h16 = R.vision_forward(sd, px, heads=2, round_operands=True)
    d = float((h16 - hidden).norm() / hidden.norm())
    assert 0 < d < 5e-3


# ------------------------------------------------------------------------------------------- host-side argument validation
def test_patchify_entry_point_rejects_before_launch():
    """sg_clip_patchify_f16 validates on the host: these calls return SG_EINVAL without a device (none of the pointers is real)."""
    from storygen_amd import _lib
    lib = _lib.load()
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    z = (C.c_float * 3)(0.5, 0.0, 0.5)
    P = 0x10000
    assert lib.sg_clip_patchify_f16(P, 1, 64, 64, 1.0, 0.0, m, m, 30, 8, P, 192, None) == -1 and b"multiple of the patch size" in lib.sg_last_error()
    assert lib.sg_clip_patchify_f16(P, 1, 64, 64, 1.0, 0.0, m, m, 30, 6, P, 112, None) == -1 and b"multiple of 8" in lib.sg_last_error()
    assert lib.sg_clip_patchify_f16(None, 1, 64, 64, 1.0, 0.0, m, m, 32, 8, P, 192, None) == -1 and b"null" in lib.sg_last_error()
    assert lib.sg_clip_patchify_f16(P, 1, 64, 64, 1.0, 0.0, None, m, 32, 8, P, 192, None) == -1 and b"null" in lib.sg_last_error()
    assert lib.sg_clip_patchify_f16(P, 1, 64, 64, 1.0, 0.0, m, m, 32, 8, None, 192, None) == -1
    for B, H, W, S, ps in [(0, 64, 64, 32, 8), (1, 0, 64, 32, 8), (1, 64, -1, 32, 8), (1, 64, 64, 0, 8), (1, 64, 64, 32, 0)]:
        assert lib.sg_clip_patchify_f16(P, B, H, W, 1.0, 0.0, m, m, S, ps, P, 192, None) == -1, (B, H, W, S, ps)
    assert lib.sg_clip_patchify_f16(P, 1, 64, 64, 1.0, 0.0, m, m, 32, 8, P, 190, None) == -1          # row stride
    assert lib.sg_clip_patchify_f16(P, 1, 64, 64, 1.0, 0.0, m, z, 32, 8, P, 192, None) == -1 and b"std" in lib.sg_last_error()
    assert lib.sg_clip_embed_patches_f32(P, 64, P, P, None, 64, 1, 17, 64, None) == -1
    assert lib.sg_clip_embed_patches_f32(P, 64, P, P, P, 64, 1, 17, 62, None) == -1


def _vision_sd(hidden=64, inter=128, layers=1, image=32, patch=8, proj=32):
    from storygen_amd.encoders import clip_vision_param_shapes, init_state
    return init_state(clip_vision_param_shapes(hidden, inter, layers, image, patch, proj), seed=1)


def test_scorer_and_engine_reject_unsupported_models_on_the_host():
    """More than 128 tokens (ViT-H/14: 257), head dim above 64 (80), a crop that the patches do not tile, a wrong image rank: all refused
    before any tensor reaches the device (there is none on this machine — reaching it would raise something else)."""
    from storygen_amd.clip_score import ClipScorer, as_nchw
    from storygen_amd.encoders import ClipVisionEngine
    from storygen_amd.model import CLIPVisionModelWithProjection
    vit_h = dict(hidden_size=1280, num_attention_heads=16, image_size=224, patch_size=14)
    with pytest.raises(ValueError, match="head dim"):
        ClipScorer({}, vit_h, device="cuda")
    with pytest.raises(ValueError, match="257 tokens"):
        ClipScorer({}, dict(vit_h, hidden_size=1024), device="cuda")                         # D = 64, T = 257
    with pytest.raises(ValueError, match="head dim"):
        ClipScorer({}, dict(hidden_size=160, num_attention_heads=2, image_size=32, patch_size=8), device="cuda")     # D = 80
    with pytest.raises(ValueError, match="not a multiple of patch_size"):
        ClipScorer({}, dict(hidden_size=64, num_attention_heads=2, image_size=30, patch_size=8), device="cuda")
    ok = dict(hidden_size=64, num_attention_heads=2, image_size=32, patch_size=8)
    with pytest.raises(ValueError, match="text_config"):
        ClipScorer({}, ok, text_state_dict={}, device="cuda")
    with pytest.raises(ValueError, match="head dim"):
        ClipScorer({}, ok, text_state_dict={}, text_config=dict(hidden_size=160, num_attention_heads=2), device="cuda")
    with pytest.raises(KeyError, match="text_projection"):
        ClipScorer({}, ok, text_state_dict={}, text_config=dict(hidden_size=64, num_attention_heads=2), device="cuda")
    # the engine reads the geometry off the weights
    with pytest.raises(ValueError, match="tokens"):
        ClipVisionEngine(_vision_sd(image=96, patch=8), "cuda", heads=2)                      # 145 tokens
    with pytest.raises(ValueError, match="head dim"):
        ClipVisionEngine(_vision_sd(hidden=160), "cuda", heads=2)
    with pytest.raises(ValueError, match="image_size"):
        ClipVisionEngine(_vision_sd(), "cuda", heads=2, image_size=64)
    with pytest.raises(ValueError, match="multiple of 8"):
        ClipVisionEngine(_vision_sd(image=30, patch=6), "cuda", heads=2)                      # 3 * 36 = 108
    # the drop-in checks its config
    with pytest.raises(ValueError, match="257 tokens"):
        CLIPVisionModelWithProjection(dict(vit_h, hidden_size=1024, intermediate_size=64, num_hidden_layers=1))
    with pytest.raises(ValueError, match="not a multiple"):
        CLIPVisionModelWithProjection(image_size=30, patch_size=8)
    # image arguments
    for bad in (torch.zeros(3, 32, 32), torch.zeros(1, 4, 32, 32), torch.zeros(1, 3, 32, 32, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\[N,3,H,W\]"):
            as_nchw(bad)
    import numpy as np
    for bad in (np.zeros((32, 32, 3), np.float32), np.zeros((1, 32, 32, 4), np.float32), np.zeros((1, 32, 32, 3), np.uint8)):
        with pytest.raises(ValueError, match=r"\[N,H,W,3\]"):
            as_nchw(bad)
    arr = np.random.default_rng(0).random((2, 5, 7, 3), dtype=np.float32)
    assert torch.equal(as_nchw(arr), torch.from_numpy(arr).permute(0, 3, 1, 2))


def test_dropin_vision_model_adopts_transformers_names(tmp_path):
    from storygen_amd.encoders import clip_vision_param_shapes
    from storygen_amd.model import CLIPVisionModelWithProjection
    cfg = dict(hidden_size=64, intermediate_size=128, projection_dim=48, num_hidden_layers=2, num_attention_heads=2, image_size=32, patch_size=8)
    mine = CLIPVisionModelWithProjection(cfg, seed=2)
    assert mine.config.image_size == 32 and mine.config.projection_dim == 48 and mine.config.model_type == "clip_vision_model"
    assert set(mine.state_dict()) == set(clip_vision_param_shapes(64, 128, 2, 32, 8, 48))
    mine.save_pretrained(str(tmp_path / "v"), safe_serialization=True)
    again = CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), subfolder="v", torch_dtype=torch.float16)
    assert again.dtype == torch.float16 and all(torch.equal(again.state_dict()[k], v.half()) for k, v in mine.state_dict().items())
    with pytest.raises(RuntimeError, match="no CPU path"):
        again(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match="pixel_values"):
        again(torch.zeros(1, 3, 64, 64))
    with pytest.raises(NotImplementedError):
        again.requires_grad_(True)
    with pytest.raises(RuntimeError, match="missing"):
        again.load_state_dict({k: v for k, v in list(mine.state_dict().items())[:-1]})
    transformers = pytest.importorskip("transformers")
    tm = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**cfg)).eval()
    got = CLIPVisionModelWithProjection.from_torch(tm)
    tsd = {k: v for k, v in tm.state_dict().items() if not k.endswith("position_ids")}
    assert set(got.state_dict()) == set(tsd) and all(torch.equal(got.state_dict()[k], v) for k, v in tsd.items())
    full = {"projection_dim": 48, "vision_config": {k: v for k, v in cfg.items() if k != "projection_dim"}, "text_config": {}}
    assert CLIPVisionModelWithProjection(full).config.projection_dim == 48
