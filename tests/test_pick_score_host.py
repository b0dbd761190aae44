"""Host logic of PickScorer, ClipVisionEngine(wide=True) and the drop-in CLIPModel on the CPU, over the torch emulation of the kernels
(tests/pick_ops_emulation.py), against the restatement of tests/pick_score_reference.py; and the host-side refusals of the two new entry points
sg_attn_enc_f16 and sg_clip_patchify_padk_f16 (SG_EINVAL before any launch: none of the pointers is real).  The real kernels run the same host
code in tests/test_pick_score_gpu.py."""
import ctypes as C

import pytest
import torch

from conftest import rel_l2
from tests import pick_score_reference as P
from tests.pick_ops_emulation import patched_pick_ops


@pytest.fixture(scope="module")
def tiny():
    cfg = P.tiny_config()
    sd = P.tiny_state(2, cfg)
    frames, ids = P.tiny_inputs(13)
    px = P.preprocess_frames(frames, cfg["vision_config"]["image_size"])
    return cfg, sd, frames, ids, px


def test_scorer_host_logic(tiny):
    from storygen_amd.pick_score import PickScorer
    cfg, sd, frames, ids, px = tiny
    want_i, want_t, want_s = P.image_features(sd, cfg, px), P.text_features(sd, cfg, ids), P.scores(sd, cfg, ids, px)
    with patched_pick_ops() as calls:
        sc = PickScorer(sd, cfg, device="cpu")
        fi, ft = sc.image_features(frames), sc.text_features(ids)
        # the wide dispatch: the image tower (82 tokens of head dim 80) on the new op with padded patch rows, the text tower (24 x 32) on the old
        assert ("clip_patchify_padk", 588, 592) in calls
        assert {c for c in calls if c[0].startswith("attention")} == {("attention_enc", 82, 80), ("attention_small", 24, 32)}
        s, p = sc.scores(ids, frames), sc.probs(ids, frames)
        idx, pb = sc.best_of(ids, frames)
        nchw = torch.from_numpy(frames).permute(0, 3, 1, 2)
        assert torch.equal(sc.scores(ids, nchw), s)
        two = sc.scores(torch.cat([ids, ids]), frames[:2])
        with pytest.raises(ValueError, match="one prompt"):
            sc.best_of(torch.cat([ids, ids]), frames)
        with pytest.raises(ValueError, match=r"\[N,H,W,3\]"):
            sc.image_features(frames[0])
        signed = PickScorer(sd, cfg, device="cpu", in_scale=0.5, in_shift=0.5).image_features(nchw * 2 - 1)
        assert tuple(sc.vision.wp.shape) == (160, 592) and bool((sc.vision.wp[:, 588:] == 0).all())
    assert fi.dtype == torch.float32 and tuple(fi.shape) == (5, 32) and tuple(ft.shape) == (1, 32) and tuple(s.shape) == (1, 5)
    assert rel_l2(fi, want_i) < 2e-3 and rel_l2(ft, want_t) < 2e-3 and rel_l2(signed, want_i) < 2e-3
    # the emulated engines and the restatement with fp16 rounding points are the same computation
    assert rel_l2(fi, P.image_features(sd, cfg, px, round_operands=True)) < 5e-4
    assert rel_l2(ft, P.text_features(sd, cfg, ids, round_operands=True)) < 5e-4
    assert float((s - want_s).abs().max()) < 100.0 * 5e-4
    assert abs(float(p.sum()) - 1) < 1e-6 and idx == int(want_s[0].argmax()) and torch.equal(pb, p[0])
    assert tuple(two.shape) == (2, 2) and torch.allclose(two[0], two[1], atol=1e-4) and torch.allclose(two[0], s[0, :2], atol=1e-4)    # [P, N]: prompts x images


def test_config_forms_and_state_dict_split(tiny):
    from storygen_amd.pick_score import PickScorer, split_config
    cfg, sd, frames, ids, _ = tiny

    class Conf:                                    # anything with to_dict(): transformers' CLIPConfig
        def __init__(self, d):
            self.d = d

        def to_dict(self):
            return dict(self.d)

    nested = dict(cfg, vision_config=Conf(cfg["vision_config"]), text_config=Conf(cfg["text_config"]))
    for form in (cfg, Conf(cfg), nested):
        vc, tc = split_config(form)
        assert vc["patch_size"] == 14 and tc["hidden_size"] == 64
    with pytest.raises(KeyError, match="vision_config and text_config"):
        split_config(cfg["vision_config"])
    with pytest.raises(KeyError, match="lacks"):
        split_config(dict(cfg, vision_config=dict(hidden_size=160)))
    with patched_pick_ops():
        a = PickScorer(sd, Conf(cfg), device="cpu")
        extra = dict(sd, **{"text_model.embeddings.position_ids": torch.arange(77)[None], "unrelated.weight": torch.zeros(3)})
        b = PickScorer(extra, cfg, device="cpu")
        assert torch.equal(a.scores(ids, frames), b.scores(ids, frames))
        assert float(a.logit_scale.exp()) == pytest.approx(100.0, rel=1e-3)
    # refusals, all before an engine is built
    with pytest.raises(KeyError, match="logit_scale"):
        PickScorer({k: v for k, v in sd.items() if k != "logit_scale"}, cfg, device="cpu")
    with pytest.raises(KeyError, match="text tower"):
        PickScorer({k: v for k, v in sd.items() if not k.startswith("text_")}, cfg, device="cpu")
    with pytest.raises(KeyError, match="image tower"):
        PickScorer({k: v for k, v in sd.items() if not k.startswith("vis")}, cfg, device="cpu")


def _vcfg(**kw):
    return dict(P.tiny_config()["vision_config"], **kw)


def test_limits_of_the_wide_engine():
    from storygen_amd.encoders import ClipVisionEngine, clip_vision_param_shapes, init_state
    from storygen_amd.pick_score import PickScorer
    cfg = P.tiny_config()
    with pytest.raises(ValueError, match="1024"):                      # 33 x 33 + 1 = 1090 tokens
        PickScorer({}, dict(cfg, vision_config=_vcfg(image_size=462)), device="cpu")
    with pytest.raises(ValueError, match="head dim 136"):
        PickScorer({}, dict(cfg, vision_config=_vcfg(hidden_size=272)), device="cpu")
    with pytest.raises(ValueError, match="head dim 84"):
        PickScorer({}, dict(cfg, vision_config=_vcfg(hidden_size=168)), device="cpu")
    with pytest.raises(ValueError, match="head dim"):                  # the text tower stays on sg_attn_small_f16: D <= 64
        PickScorer({}, dict(cfg, text_config=dict(cfg["text_config"], hidden_size=160)), device="cpu")
    with pytest.raises(ValueError, match="not a multiple of patch_size"):
        PickScorer({}, dict(cfg, vision_config=_vcfg(image_size=100)), device="cpu")
    with pytest.raises(ValueError, match="multiple of 4"):             # 3 * 25 = 75
        PickScorer({}, dict(cfg, vision_config=_vcfg(image_size=20, patch_size=5)), device="cpu")
    with pytest.raises(ValueError, match="hidden_act"):
        PickScorer({}, dict(cfg, vision_config=_vcfg(hidden_act="relu")), device="cpu")
    # the engine reads its geometry off the weights; the default engine keeps every refusal
    sd = init_state(clip_vision_param_shapes(160, 320, 1, 126, 14, 32), seed=1)
    with pytest.raises(ValueError, match="head dim"):
        ClipVisionEngine(sd, "cpu", heads=2)
    with pytest.raises(ValueError, match="multiple of 8"):
        ClipVisionEngine(init_state(clip_vision_param_shapes(64, 128, 1, 126, 14, 32), seed=1), "cpu", heads=2)
    with pytest.raises(ValueError, match="1024"):
        ClipVisionEngine(init_state(clip_vision_param_shapes(64, 128, 1, 264, 8, 32), seed=1), "cpu", heads=2, wide=True)
    with pytest.raises(ValueError, match="head dim 136"):
        ClipVisionEngine(init_state(clip_vision_param_shapes(272, 64, 1, 28, 14, 32), seed=1), "cpu", heads=2, wide=True)
    with patched_pick_ops() as calls:
        eng = ClipVisionEngine(sd, "cpu", heads=2, hidden_act="gelu", wide=True)
        with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
            eng(torch.zeros(3, 126, 126))
        # T <= 128 and D <= 64 stay on the old op (and the unpadded patch rows) with wide=True
        small = init_state(clip_vision_param_shapes(64, 128, 1, 32, 8, 32), seed=1)
        del calls[:]
        ClipVisionEngine(small, "cpu", heads=2, wide=True)(torch.rand(1, 3, 40, 40))
        assert calls == [("attention_small", 17, 32)]
        # D <= 64 but more than 128 tokens: the new op
        del calls[:]
        ClipVisionEngine(init_state(clip_vision_param_shapes(64, 128, 1, 96, 8, 32), seed=1), "cpu", heads=2, wide=True)(torch.rand(1, 3, 96, 96))
        assert calls == [("attention_enc", 145, 32)]


def test_dropin_clip_model(tiny, tmp_path):
    from storygen_amd.model import CLIPModel
    cfg, sd, frames, ids, px = tiny
    m = CLIPModel(cfg, seed=3)
    assert set(m.state_dict()) == set(sd) and m.config.projection_dim == 32 and m.config.vision_config["patch_size"] == 14
    assert float(m.logit_scale.exp()) == pytest.approx(100.0, rel=1e-5)
    m.load_state_dict(sd)
    m.save_pretrained(str(tmp_path / "pick"), safe_serialization=True)
    again = CLIPModel.from_pretrained(str(tmp_path), subfolder="pick")
    assert all(torch.equal(again.state_dict()[k], v) for k, v in sd.items())
    assert again.config.text_config["hidden_act"] == "gelu" and again.logit_scale.dim() == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        again.get_image_features(pixel_values=px)
    with pytest.raises(ValueError, match="pixel_values"):
        again.get_image_features(pixel_values=torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="missing"):
        again.load_state_dict({k: v for k, v in sd.items() if k != "logit_scale"})
    with pytest.raises(KeyError, match="vision_config"):
        CLIPModel(cfg["vision_config"])
    # calc_probs of the reference's scripts, on the emulated kernels (the model's device check is what the emulation cannot satisfy)
    from storygen_amd.pick_score import PickScorer
    with patched_pick_ops():
        again._engine = PickScorer(again.state_dict(), again.config, "cpu")
        image_embs = again.get_image_features(pixel_values=px)
        image_embs = image_embs / torch.norm(image_embs, dim=-1, keepdim=True)
        text_embs = again.get_text_features(input_ids=ids, attention_mask=torch.ones_like(ids))
        text_embs = text_embs / torch.norm(text_embs, dim=-1, keepdim=True)
        scores = again.logit_scale.exp() * (text_embs @ image_embs.T)[0]
    assert float((scores - P.scores(sd, cfg, ids, px)[0]).abs().max()) < 100.0 * 5e-4
    transformers = pytest.importorskip("transformers")
    tm = transformers.CLIPModel(transformers.CLIPConfig(text_config=cfg["text_config"], vision_config=cfg["vision_config"],
                                                        projection_dim=32, logit_scale_init_value=cfg["logit_scale_init_value"])).eval()
    got = CLIPModel.from_torch(tm)
    tsd = {k: v for k, v in tm.state_dict().items() if not k.endswith("position_ids")}
    assert set(got.state_dict()) == set(tsd) and all(torch.equal(got.state_dict()[k], v) for k, v in tsd.items())


# --------------------------------------------------------------------------------------------------- host-side argument validation
def _enc(lib, q=0x10000, k=0x20000, v=0x30000, o=0x40000, ld=160, bs=160 * 300, B=1, H=2, T=257, D=80, causal=0, ldo=None, bias=None):
    return lib.sg_attn_enc_f16(q, ld, bs, k, ld, bs, v, ld, bs, o, ld if ldo is None else ldo, bs, bias, B, H, T, D, 0.1, causal, None)


def test_attn_enc_entry_point_rejects_before_launch():
    from storygen_amd import _lib
    lib = _lib.load()
    for name in ("q", "k", "v", "o"):
        assert _enc(lib, **{name: None}) == -1 and b"null" in lib.sg_last_error(), name
    for T in (0, 1025, -3):
        assert _enc(lib, T=T) == -1 and b"1024" in lib.sg_last_error(), T
    for D in (4, 136, 84, 0):
        assert _enc(lib, D=D, ld=1024) == -1 and b"head dim" in lib.sg_last_error(), D
    assert _enc(lib, ld=152) == -1 and b"token stride below" in lib.sg_last_error()
    assert _enc(lib, ldo=152) == -1 and b"token stride below" in lib.sg_last_error()
    assert _enc(lib, ld=164) == -1 and b"multiples of 8" in lib.sg_last_error()
    assert _enc(lib, bs=160 * 300 + 4) == -1 and b"multiples of 8" in lib.sg_last_error()
    for name in ("q", "k", "v", "o"):
        assert _enc(lib, **{name: 0x10008}) == -1 and b"alignment" in lib.sg_last_error(), name
    assert _enc(lib, causal=2) == -1 and b"causal" in lib.sg_last_error()
    assert _enc(lib, B=0) == -1 and _enc(lib, H=0) == -1 and _enc(lib, B=70000) == -1


def test_patchify_padk_entry_point_rejects_before_launch():
    from storygen_amd import _lib
    lib = _lib.load()
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    z = (C.c_float * 3)(0.5, 0.0, 0.5)
    Pn = 0x10000

    def call(x=Pn, mean=m, std=m, out=Pn, B=1, H=64, W=64, S=28, ps=14, Kpad=592, ldo=592):
        return lib.sg_clip_patchify_padk_f16(x, B, H, W, 1.0, 0.0, mean, std, S, ps, Kpad, out, ldo, None)

    for name in ("x", "mean", "std", "out"):
        assert call(**{name: None}) == -1 and b"null" in lib.sg_last_error(), name
    assert call(Kpad=588, ldo=600) == -1 and b"Kpad" in lib.sg_last_error()               # not a multiple of 8
    assert call(Kpad=584, ldo=600) == -1 and b"Kpad" in lib.sg_last_error()               # below 3 * ps * ps
    assert call(Kpad=600, ldo=592) == -1 and b"below Kpad" in lib.sg_last_error()         # above ldo
    assert call(ps=5, S=20, Kpad=80, ldo=80) == -1 and b"multiple of 4" in lib.sg_last_error()      # 75
    assert call(S=30) == -1 and b"multiple of the patch size" in lib.sg_last_error()
    assert call(out=0x10008) == -1 and call(ldo=596) == -1
    assert call(std=z) == -1 and b"std" in lib.sg_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(S=0), dict(ps=0)):
        assert call(**kw) == -1, kw
    # the existing entry point keeps its refusal of patch size 14
    assert lib.sg_clip_patchify_f16(Pn, 1, 64, 64, 1.0, 0.0, m, m, 28, 14, Pn, 592, None) == -1 and b"multiple of 8" in lib.sg_last_error()


def test_ops_wrappers_validate():
    from storygen_amd import ops
    x = torch.zeros(1, 8, 16, dtype=torch.float16)
    with pytest.raises(TypeError):
        ops.attention_enc(x, x, x, x, 2, 1.0, False)                    # CPU tensors are refused
