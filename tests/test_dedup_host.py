"""Near-duplicate keyframe removal, host side: the restatements of tests/dedup_reference.py pinned (the tower to transformers.ViTModel, the
cosine to torch.cosine_similarity, the decisions to the script's loop written literally, the geometry to hand-worked sizes), the C entry
point's and the wrappers' refusals, and the host logic of DinoVitEngine, DinoVisionTransformer and KeyframeDeduper on emulated ops."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from tests import clip_u8_reference as U8
from tests import dedup_reference as D
from tests.dedup_ops_emulation import patched_dedup_ops

U = 2.0 ** -53
HEADS = D.TINY["num_heads"]


# ------------------------------------------------------------------------------------------------------------- the tower, pinned
@pytest.mark.parametrize("over", [dict(), dict(img_size=224, depth=1)], ids=["145_tokens_2_layers", "785_tokens_1_layer"])
def test_tower_restatement_matches_transformers_vit(over):
    """The restated DINO forward against transformers.ViTModel (no pooler, eps 1e-6, erf GELU, the class row of last_hidden_state) through
    the explicit key map of tests/dedup_reference.py.  Both run the same fp32 operations on the same weights; they differ in the order of
    the sums inside the matrix products, the fused attention and LayerNorm, each worth about one unit in the last place (2^-23) of rel-L2
    per operation and not all in one direction over the 8 operations of a layer: 16 x 2^-23 = 1.9e-6 is the bar.  This pins the structure
    (token order, pre-LN blocks, q|k|v row order, scaling, GELU, final norm); DINO's own key names stay restated from upstream."""
    transformers = pytest.importorskip("transformers")
    c = dict(D.TINY, **over)
    sd = D.tiny_state(3, **over)
    conf = transformers.ViTConfig(hidden_size=c["embed_dim"], num_hidden_layers=c["depth"], num_attention_heads=HEADS,
                                  intermediate_size=4 * c["embed_dim"], hidden_act="gelu", layer_norm_eps=1e-6, image_size=c["img_size"],
                                  patch_size=c["patch_size"], num_channels=3, qkv_bias=True, hidden_dropout_prob=0.0,
                                  attention_probs_dropout_prob=0.0)
    model = transformers.ViTModel(conf, add_pooling_layer=False).eval().float()
    mapped = D.to_vit_state(sd)
    own = dict(model.state_dict())
    assert set(own) == set(mapped), sorted(set(own) ^ set(mapped))[:8]
    assert all(tuple(own[k].shape) == tuple(mapped[k].shape) for k in own)
    model.load_state_dict(mapped)
    px = torch.randn(2, 3, c["img_size"], c["img_size"], generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = model(pixel_values=px).last_hidden_state[:, 0]
    got = D.dino_forward(sd, px, HEADS)
    T = (c["img_size"] // c["patch_size"]) ** 2 + 1
    print(f"DINO restatement vs transformers.ViTModel, {T} tokens, {c['depth']} layer(s): rel-L2 {rel_l2(got, want):.2e} (bar {16 * 2.0 ** -23:.2e})")
    assert tuple(got.shape) == (2, c["embed_dim"]) and sd["pos_embed"].shape[1] == T
    assert rel_l2(got, want) < 16 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------- the cosine, pinned
def test_chain_formula_is_torch_cosine_similarity_in_float64():
    """sim[i] against torch.cosine_similarity(f_i, f_{i-1}, dim=1) on float64 CPU tensors (eps 1e-8, the script's call).  torch divides each
    vector by its clamped norm before the dot product; the restatement divides the dot product: the same number up to the sums' order
    ((dim - 1) u each, three sums) and a handful of roundings: the bar is test_dedup_gpu.py's sim_bar."""
    rng = np.random.default_rng(0)
    for N, dim in ((2, 1), (5, 7), (9, 768)):
        f = rng.standard_normal((N, dim)).astype(np.float32)
        sim, _ = D.adjacent_cosine(f)
        t = torch.from_numpy(f).double()
        want = torch.cosine_similarity(t[1:], t[:-1], dim=1).numpy()
        assert sim[0] == 0.0 and np.abs(sim[1:] - want).max() <= 2 * (2 * (dim - 1) + 12 + 1) * U
    # the first frame against the script's zero feature: exactly 0 in torch, which is why sim[0] = 0
    z = torch.cosine_similarity(torch.from_numpy(f[:1]).double(), torch.zeros(1, 768, dtype=torch.float64), dim=1)
    assert float(z) == 0.0 and str(float(z)) == "0.0"
    # a zero row in the chain, two zero rows: exactly 0
    f[3] = 0.0
    f[4] = 0.0
    sim, drop = D.adjacent_cosine(f)
    assert sim[3] == 0.0 and sim[4] == 0.0 and sim[5] == 0.0 and not drop[2:5].any()
    # the exact tie: 3 / (1 * 4) = 0.75 in torch and in the chain, and a tie drops
    tie = np.array([[1, 0, 0, 0, 0], [3, 2, 1, 1, 1]], np.float32)
    assert float(torch.cosine_similarity(torch.from_numpy(tie[1:]).double(), torch.from_numpy(tie[:1]).double(), dim=1)) == 0.75
    sim, drop = D.adjacent_cosine(tie)
    assert sim.tolist() == [0.0, 0.75] and drop.tolist() == [True, False]
    assert D.adjacent_cosine(tie, threshold=np.nextafter(0.75, 1.0))[1].tolist() == [False, False]
    # a NaN row keeps both neighbours' pairs undecided: kept
    bad = np.ones((4, 4), np.float32)                        # identical rows of norm 2: 4 / (2 * 2) = 1 exactly
    bad[2, 1] = np.nan
    sim, drop = D.adjacent_cosine(bad)
    assert sim[1] == 1.0 and np.isnan(sim[2]) and np.isnan(sim[3]) and drop.tolist() == [True, False, False, False]


def test_vectorised_decisions_are_the_scripts_loop():
    rng = np.random.default_rng(1)
    for trial in range(200):
        N = int(rng.integers(1, 40))
        sims = np.round(rng.random(N) * 1.2, 2)              # two decimals: exact ties with the threshold occur
        sims[0] = 0.0
        thr = float(rng.choice([0.75, 0.5, 0.9, 0.0, -1.0]))
        drop = np.zeros(N, bool)
        drop[:-1] = sims[1:] >= thr
        assert set(np.flatnonzero(drop).tolist()) == D.script_loop(sims.tolist(), thr), (trial, thr)
    assert D.script_loop([0.0, 0.8, 0.8, 0.1, 0.75]) == {0, 1, 3}       # a run of similar frames keeps its last; the tie drops


# ------------------------------------------------------------------------------------------------------------------- geometry
def test_geometry_by_hand():
    from storygen_amd import ops
    cases = {
        (720, 1280, 224, 256): (256, 455, 16, 116),          # int(256 * 1280 / 720) = 455; (455 - 224) / 2 = 115.5 -> 116 (odd difference, to even)
        (1280, 720, 224, 256): (455, 256, 116, 16),          # the portrait of it
        (256, 256, 224, 256): (256, 256, 16, 16),            # already at the resize: both passes skipped
        (480, 640, 224, 256): (256, 341, 16, 58),            # 341 - 224 = 117 -> 58.5 -> 58 (to even, down)
        (500, 887, 224, 256): (256, 454, 16, 115),           # int(256 * 887 / 500) = 454; 454 - 224 = 230 = 2 (mod 4) -> 115, no half
        (300, 400, 96, 112): (112, 149, 8, 26),              # 149 - 96 = 53 -> 26.5 -> 26
        (100, 227, 96, 112): (112, 254, 8, 79),              # int(112 * 227 / 100) = 254; 254 - 96 = 158 = 2 (mod 4) -> 79, no half
        (100, 229, 96, 112): (112, 256, 8, 80),              # 256 - 96 = 160 = 0 (mod 4)
        (200, 200, 112, 112): (112, 112, 0, 0),
    }
    for (h, w, S, rz), want in cases.items():
        assert D.geometry(h, w, S, rz) == want, (h, w, S, rz)
        assert ops.dedup_u8_geometry(h, w, S, rz) == want, (h, w, S, rz)
        assert (want[0] - S) >= 0 and (want[1] - S) >= 0
    assert (455 - 224) % 2 == 1 and (454 - 224) % 4 == 2 and (254 - 96) % 4 == 2
    # where this differs from CLIP's rule at the same crop: the resize target is not the crop size
    assert ops.clip_u8_geometry(720, 1280, 224)[:2] == (224, 398)
    for h, w, S, rz in ((100, 100, 224, 200), (50, 500, 96, 95)):
        with pytest.raises(ValueError, match="smaller than"):
            ops.dedup_u8_geometry(h, w, S, rz)
    rng = np.random.default_rng(2)
    for _ in range(300):
        h, w = (int(v) for v in rng.integers(30, 2000, 2))
        assert ops.dedup_u8_geometry(h, w, 224, 256) == D.geometry(h, w, 224, 256), (h, w)


def test_numeric_order_and_extension():
    from storygen_amd.dedup import is_keyframe_file, numeric_key, numeric_order
    names = ["000001_keyframe_0-0-10-0.jpg", "000001_keyframe_0-0-9-500.jpg", "000001_keyframe_0-1-2-40.jpg", "000001_keyframe_0-0-9-60.jpg",
             "10.jpg", "9.jpg", "notes.txt", "000002_keyframe_0-0-1-0.jpg", "frame.jpg"]
    want = sorted(names, key=D.fns)
    assert numeric_order(names) == want
    assert want.index("000001_keyframe_0-0-9-500.jpg") < want.index("000001_keyframe_0-0-10-0.jpg")
    assert sorted(names).index("000001_keyframe_0-0-9-500.jpg") > sorted(names).index("000001_keyframe_0-0-10-0.jpg")      # alphabetic is the other way
    assert want.index("000001_keyframe_0-0-9-60.jpg") < want.index("000001_keyframe_0-0-9-500.jpg") and want.index("9.jpg") < want.index("10.jpg")
    assert numeric_key("7_b12.jpg") == D.fns("7_b12.jpg") == ("a", 7, "_b", 12, ".jpg", 0)
    assert numeric_key("x9") == ("ax", 90)                               # the appended 0 joins a trailing number
    rng = np.random.default_rng(3)
    for _ in range(200):
        s = "".join(rng.choice(list("ab-_.019"), int(rng.integers(0, 12))))
        assert numeric_key(s) == D.fns(s), s
    assert [is_keyframe_file(n) for n in ("a.jpg", "d/e.f/a.jpg", "a.JPG", "a.jpeg", "a.jpg.txt", "jpg", ".jpg")] == [True, True, False, False, False,
                                                                                                                   False, False]


# ----------------------------------------------------------------------------------------------------------------- rejections
@pytest.fixture(scope="module")
def lib():
    from storygen_amd import _lib
    from storygen_amd.build import build
    build(force=False, verbose=False)
    return _lib.load()


def test_entry_point_rejects_before_launch(lib):
    """Fake pointers, no device: every refusal is SG_EINVAL with a message, and nothing is enqueued."""
    P_ = 0x100000

    def call(feats=P_, ldf=768, N=5, dim=768, eps=1e-8, thr=0.75, sim=P_ * 2, drop=P_ * 3):
        return lib.sg_adjacent_cosine_f64(feats, ldf, N, dim, eps, thr, sim, drop, None)

    for kw, msg in ((dict(feats=None), b"null"), (dict(sim=None), b"null"), (dict(drop=None), b"null"), (dict(N=0), b"outside [1, 1048576]"),
                    (dict(N=(1 << 20) + 1), b"outside [1, 1048576]"), (dict(N=-1), b"outside"), (dict(dim=0), b"outside [1, 65536]"),
                    (dict(dim=65537, ldf=65537), b"outside [1, 65536]"), (dict(ldf=767), b"below dim"), (dict(ldf=(1 << 40) + 1), b"2^40"),
                    (dict(eps=-1e-8), b"eps"), (dict(eps=float("nan")), b"eps"),
                    (dict(sim=P_, drop=P_ + 39), b"overlap"), (dict(sim=P_ + 4, drop=P_), b"overlap"), (dict(sim=P_, drop=P_), b"overlap")):
        assert call(**kw) == -1, kw
        assert msg in lib.sg_last_error(), (kw, lib.sg_last_error())
    header = open(__file__.replace("tests/test_dedup_host.py", "include/storygen_hip.h")).read()
    for name, value in (("SG_DEDUP_MAX_FRAMES", 1 << 20), ("SG_DEDUP_MAX_DIM", 65536)):
        assert f"#define {name} {value}\n" in header


def test_ops_wrapper_validates():
    from storygen_amd import ops
    assert (ops.DEDUP_MAX_FRAMES, ops.DEDUP_MAX_DIM) == (1 << 20, 65536)
    assert ops.DEDUP_IMAGE_MEAN == D.MEAN and ops.DEDUP_IMAGE_STD == D.STD
    with pytest.raises(TypeError, match="CUDA/HIP float32"):
        ops.adjacent_cosine(torch.zeros(3, 8))
    with pytest.raises(TypeError, match="CUDA/HIP float32"):
        ops.adjacent_cosine(torch.zeros(3, 8, dtype=torch.float64))
    ops.check_dedup_sides("x", 1, 1)
    ops.check_dedup_sides("x", 1 << 20, 65536)
    for N, dim in ((0, 8), ((1 << 20) + 1, 8), (3, 0), (3, 65537)):
        with pytest.raises(ValueError):
            ops.check_dedup_sides("x", N, dim)


# ------------------------------------------------------------------------------------------------ engine, drop-in, deduper: host logic
def _frames():
    return [U8.content("random", 120, 150, seed=1), U8.content("checker", 200, 130, seed=2), U8.content("random", 112, 112, seed=3),
            U8.content("random", 120, 150, seed=4)]


def test_engine_host_logic_on_emulated_ops():
    from PIL import Image
    from storygen_amd.dino import DinoVitEngine
    sd = D.tiny_state(0)
    frames = _frames()
    with patched_dedup_ops() as (_, u8_calls, calls):
        eng = DinoVitEngine({**sd, "head.weight": torch.zeros(3, 64)}, "cpu", heads=HEADS, resize=112)
        assert (eng.C, eng.ps, eng.T, eng.S, eng.kpad, eng.resize) == (64, 8, 145, 96, 192, 112)
        mixed = [frames[0], Image.fromarray(frames[1]), torch.from_numpy(frames[2]), frames[3]]
        rows = eng.patch_rows_u8(mixed)
        assert np.array_equal(rows.numpy(), D.patch_rows_u8(frames, 96, 8, 112))
        # one launch per size, with the script's geometry, not CLIP's
        assert sorted(u8_calls) == sorted([((2, 120, 150, 3), D.geometry(120, 150, 96, 112), 192), ((1, 200, 130, 3), D.geometry(200, 130, 96, 112), 192),
                                           ((1, 112, 112, 3), (112, 112, 8, 8), 192)])
        got = eng(mixed)
        assert ("attention_enc", 145, 32) in calls and not any(c[0] == "attention_small" for c in calls)
        px = D.pixel_values(frames, 96, 112)
        want, rounded = D.dino_forward(sd, px, HEADS), D.dino_forward(sd, px, HEADS, round_operands=True)
        print(f"engine over emulated ops: {rel_l2(got, want):.2e} from the fp32 restatement (fp16-rounded restatement {rel_l2(rounded, want):.2e}), "
              f"{rel_l2(got, rounded):.2e} from the rounded one")
        assert tuple(got.shape) == (4, 64) and got.dtype == torch.float32 and torch.equal(got, got.half().float())
        assert rel_l2(got, want) < 2e-3 and rel_l2(got, rounded) < 5e-4                  # the bars of tests/test_pick_score_host.py
        assert torch.equal(eng.encode_pixels(px), got)                                   # fp16 patch rows of the same pixels
        assert torch.equal(eng(mixed, batch=3), got) and torch.equal(eng(np.stack([frames[0], frames[3]]), batch=1), got[[0, 3]])
        # refusals
        with pytest.raises(ValueError, match="native token grid"):
            eng.encode_pixels(torch.zeros(1, 3, 104, 104))
        with pytest.raises(ValueError, match="native token grid"):
            eng.encode_pixels(torch.zeros(3, 96, 96))
        with pytest.raises(TypeError, match="8-bit"):
            eng(px)
        with pytest.raises(ValueError, match="RGB"):
            eng([frames[0], frames[0][:, :, 0]])
        with pytest.raises(ValueError, match="convert"):
            eng([Image.fromarray(frames[0]).convert("CMYK")])
        with pytest.raises(ValueError, match="batch"):
            eng(mixed, batch=0)
        with pytest.raises(KeyError, match="unknown \\['blocks.0.ls1.gamma'\\]"):
            DinoVitEngine({**sd, "blocks.0.ls1.gamma": torch.zeros(64)}, "cpu", heads=HEADS)
        with pytest.raises(KeyError, match="missing \\['norm.bias'\\]"):
            DinoVitEngine({k: v for k, v in sd.items() if k != "norm.bias"}, "cpu", heads=HEADS)
        with pytest.raises(ValueError, match="heads"):
            DinoVitEngine(sd, "cpu", heads=3)
        with pytest.raises(ValueError, match="below the crop size"):
            DinoVitEngine(sd, "cpu", heads=HEADS, resize=95)
        with pytest.raises(ValueError, match="square grid"):
            DinoVitEngine({**sd, "pos_embed": sd["pos_embed"][:, :144]}, "cpu", heads=HEADS)
        # dino_vitb8's geometry passes the host checks: 785 tokens, 12 heads of 64, crop 224
        from storygen_amd.dino import dino_param_shapes
        from storygen_amd.encoders import check_clip_dims_wide
        shapes = dino_param_shapes()
        assert shapes["pos_embed"] == (1, 785, 768) and shapes["blocks.11.attn.qkv.weight"] == (2304, 768) and len(shapes) == 4 + 12 * 12 + 2
        check_clip_dims_wide("x", 768, 12, 785)


def test_drop_in_round_trip_and_refusals():
    from storygen_amd.model import DinoVisionTransformer
    cfg = dict(img_size=96, patch_size=8, embed_dim=64, depth=2, num_heads=HEADS)
    sd = D.tiny_state(0)
    m = DinoVisionTransformer(**cfg)
    assert list(m.state_dict()) == list(sd) and all(tuple(m.state_dict()[k].shape) == tuple(sd[k].shape) for k in sd)
    assert m.embed_dim == 64 and float(m.state_dict()["blocks.0.norm1.weight"].min()) == 1.0
    m.load_state_dict({**sd, "head.bias": torch.zeros(5)})
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    m2 = DinoVisionTransformer(**cfg)
    m2.load_state_dict(m.state_dict())
    assert all(torch.equal(m2.state_dict()[k], sd[k]) for k in sd)
    assert m.to(torch.float16).dtype == torch.float16 and m.float().dtype == torch.float32 and m.eval() is m and m.requires_grad_(False) is m
    with pytest.raises(RuntimeError, match="unexpected"):
        m.load_state_dict({**sd, "fc.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="missing"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "cls_token"})
    with pytest.raises(RuntimeError, match="wrong shape"):
        m.load_state_dict({**sd, "pos_embed": torch.zeros(1, 144, 64)})
    with pytest.raises(NotImplementedError):
        m.train()
    with pytest.raises(NotImplementedError):
        m.requires_grad_(True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 3, 96, 96))
    with pytest.raises(ValueError, match="native token grid"):
        m(torch.zeros(1, 3, 104, 104))
    with pytest.raises(TypeError, match="unknown config"):
        DinoVisionTransformer(num_classes=10)
    with pytest.raises(ValueError):
        DinoVisionTransformer(img_size=100, patch_size=8)
    with pytest.raises(ValueError):
        DinoVisionTransformer(embed_dim=768, num_heads=5)
    # a loaded state dict or a move drops the cached engine, as for the other encoder drop-ins
    m._engine = object()
    m.load_state_dict(sd)
    assert m._engine is None


def test_deduper_wiring_on_emulated_ops():
    from storygen_amd.dedup import Dedup, KeyframeDeduper, dedup_features
    sd = D.tiny_state(0)
    frames = _frames()
    frames = [frames[0], frames[0].copy(), frames[1], frames[2], frames[2].copy()]
    with patched_dedup_ops() as (calls, _, _):
        with pytest.raises(ValueError, match="below the crop size"):
            KeyframeDeduper(D.tiny_state(0, patch_size=16, img_size=272), device="cpu", heads=HEADS)       # resize is the script's 256
        dd = KeyframeDeduper(D.tiny_state(0, img_size=96), device="cpu", threshold=0.999999, heads=HEADS)
        assert dd.engine.resize == 256 and dd.engine.S == 96 and dd.threshold == 0.999999
        out = dd.dedup(frames, batch=2)
        assert isinstance(out, Dedup) and calls == [("adjacent_cosine", (5, 64), 0.999999)]
        feats = dd.features(frames)
        sim, drop = D.adjacent_cosine(feats.numpy(), 0.999999)
        assert out.similarity.dtype == np.float64 and out.keep.dtype == out.drop.dtype == np.bool_
        assert np.array_equal(out.similarity, sim) and np.array_equal(out.drop, drop) and np.array_equal(out.keep, ~drop)
        assert out.drop.tolist() == [True, False, False, True, False] and sim[0] == 0.0       # identical frames: the earlier one goes
        again = dedup_features(feats, threshold=0.999999)
        assert np.array_equal(again.drop, out.drop) and np.array_equal(again.similarity, out.similarity)
        with pytest.raises(TypeError, match="8-bit"):
            dd.dedup(torch.rand(2, 3, 96, 96))
        with pytest.raises(ValueError):
            dedup_features(torch.zeros(5))
        with pytest.raises(ValueError):
            dedup_features(torch.zeros(0, 8))
        with pytest.raises(ValueError, match="NaN"):
            KeyframeDeduper(sd, device="cpu", threshold=float("nan"), heads=HEADS)
