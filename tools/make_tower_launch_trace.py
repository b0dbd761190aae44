#!/usr/bin/env python
"""Record, on the CPU, what the ViT / CLIP towers hand to the kernels (tests/recording_ops.py stands in for storygen_amd.ops) for a fixed
set of cases and write tests/golden/tower_launch_trace.json: the launch sequence of every case, and a SHA-256 of every tensor each engine
prepared for the device.  tests/test_tower_launch_trace.py replays the same cases and requires the same file, so the fixture must come
from the code a change starts FROM: run this file in a checkout of the parent commit, never on the changed engines.

    python tools/make_tower_launch_trace.py [out.json]

File format: {"launches": {case: [digest of entry 0, ...]}, "weights": {engine: [[role, shape, dtype, SHA-256 of the bytes], ...]}}.  A
launch digest is the first 10 hex digits of the SHA-256 of the entry's canonical JSON, as in tools/make_engine_launch_trace.py.

One normalisation: the host-only geometry helpers (clip_u8_geometry, dedup_u8_geometry, clip_resize_geometry) answer with the real
functions and are not logged, and a clip_patchify_u8 entry records the resolved (Hr, Wr, top, left) in place of its crop= / geometry=
keywords: a crop name and the tuple it resolves to reach the kernel as the same arguments, so they digest alike."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
GOLDEN = os.path.join(ROOT, "tests", "golden", "tower_launch_trace.json")

import recording_ops  # noqa: E402
from storygen_amd import ops as real_ops  # noqa: E402

GEOMETRY = ("clip_u8_geometry", "dedup_u8_geometry", "clip_resize_geometry")
TRACED = ("encoders", "dino", "clip_score", "pick_score", "align")         # imported first; every storygen_amd module that reads ops is patched
# the smallest towers that reach every branch: 17 tokens of 2 heads of 16 (sg_attn_small_f16's side), 2 layers
NARROW = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, image_size=32, patch_size=8, projection_dim=16)
WIDE14 = dict(hidden_size=160, intermediate_size=64, num_hidden_layers=2, image_size=28, patch_size=14, projection_dim=16)   # K = 588 -> 592, head dim 80
WIDE16 = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, image_size=32, patch_size=16, projection_dim=16)    # K = 768: no padding
TEXT = dict(vocab_size=50, hidden_size=32, intermediate_size=64, num_hidden_layers=2, max_position_embeddings=16)
DINO = dict(embed_dim=64, depth=2, patch_size=8, img_size=96)             # 145 tokens, resize 112: tests/test_dedup_host.py's
HEADS = 2


class TowerRecordingOps(recording_ops.RecordingOps):
    def __getattr__(self, name):
        if name in GEOMETRY:
            return getattr(real_ops, name)
        call = recording_ops.RecordingOps.__getattr__(self, name)
        if name != "clip_patchify_u8":
            return call

        def patchify_u8(x_u8, out, S, ps, mean, std, geometry=None, crop="torchvision", **kw):
            g = real_ops.clip_u8_geometry(x_u8.shape[1], x_u8.shape[2], S, crop) if geometry is None else geometry
            return call(x_u8, out, S, ps, mean, std, geometry=tuple(int(v) for v in g), **kw)
        return patchify_u8


def state(shapes, seed):
    """init_state's weights with every vector (biases, LayerNorm pairs, the class vector) perturbed, so that no two tensors of a tower hold
    the same bytes and a swap shows in the digests."""
    from storygen_amd.encoders import init_state
    g = torch.Generator().manual_seed(1000 + seed)
    tables = {"pos_embed": "pos_embedding", "cls_token": "cls_embedding"}     # DINO's two tables under names init_state's rules know
    sd = init_state({tables.get(k, k): v for k, v in shapes.items()}, seed)
    back = {v: k for k, v in tables.items()}
    return {back.get(k, k): v + 0.1 * torch.randn(v.shape, generator=g) if v.dim() == 1 or k == "cls_embedding" else v for k, v in sd.items()}


def u8(h, w, seed, n=None):
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def prepared(eng) -> list:
    """[role, shape, dtype, SHA-256] of every tensor the engine prepared for the device, in a fixed order.  The tensors are the engine's own
    attributes, or those of the tower object it delegates to."""
    t = getattr(eng, "tower", eng)

    def pick(*names):
        return next((getattr(o, n) for n in names for o in (t, eng) if getattr(o, n, None) is not None), None)

    def pair(role, p):
        return [] if p is None else [(role + ".weight", p[0]), (role + ".bias", p[1])]

    items = [("patch weight", pick("wp")), ("patch bias", pick("bp")), ("token table", pick("tok")), ("class", pick("cls")), ("positions", pick("pos"))]
    items += pair("pre LayerNorm", pick("pre")) + pair("final LayerNorm", pick("post", "norm", "lnf")) + [("projection", pick("proj"))]
    for i, L in enumerate(t.stack.layers):
        for k in ("ln1", "ln2"):
            items += pair(f"layer {i} {k}", L[k])
        items += [(f"layer {i} {k}", L[k]) for k in ("wqkv", "bqkv", "wo", "bo", "w1", "b1", "w2", "b2")]
    out = []
    for role, v in items:
        if v is not None:
            raw = v.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
            out.append([role, list(v.shape), str(v.dtype).replace("torch.", ""), hashlib.sha256(raw).hexdigest()])
    return out


def trace_cases() -> dict:
    """{"launches": case -> entries (tests/recording_ops.py), "weights": engine -> prepared()}, on the engines of the importing tree."""
    import importlib
    mods = {n: importlib.import_module("storygen_amd." + n) for n in TRACED}
    E, D = mods["encoders"], mods["dino"]
    rec = TowerRecordingOps()
    patched = [m for n, m in list(sys.modules.items()) if n.startswith("storygen_amd.") and getattr(m, "ops", None) is real_ops]
    launches, weights = {}, {}

    def done(name):
        launches[name] = rec.log
        rec.reset()

    for m in patched:
        m.ops = rec
    try:
        f32 = lambda *shape: torch.zeros(*shape)   # noqa: E731
        # ---- ClipVisionEngine, narrow
        eng = E.ClipVisionEngine(state(E.clip_vision_param_shapes(**NARROW), 1), "cpu", heads=HEADS, image_size=32)
        weights["vision-narrow"] = prepared(eng)
        rec.reset()
        eng(f32(2, 3, 40, 56), in_scale=0.5, in_shift=0.5)
        done("vision-narrow-float-40x56")
        eng.encode_pixels(f32(3, 3, 32, 32))
        done("vision-narrow-encode-pixels")
        mixed = [u8(40, 50, 1), torch.from_numpy(u8(36, 36, 2)), u8(40, 50, 3)]
        eng(mixed)
        done("vision-narrow-u8-two-sizes")
        for crop in ("torchvision", "floor"):        # 35 - 32 = 3: the two rules differ by one pixel
            eng(u8(32, 35, 4, n=2), crop=crop)
            done(f"vision-narrow-u8-batch-{crop}")
        eng(mixed, crop="floor", mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25))
        done("vision-narrow-u8-two-sizes-floor")
        # ---- ClipVisionEngine(wide=True): padded and unpadded patch rows
        eng = E.ClipVisionEngine(state(E.clip_vision_param_shapes(**WIDE14), 2), "cpu", heads=HEADS, hidden_act="gelu", wide=True)
        weights["vision-wide-14"] = prepared(eng)
        rec.reset()
        eng(f32(2, 3, 30, 44))
        done("vision-wide-14-float-30x44")
        eng([u8(30, 44, 5), u8(28, 28, 6)], crop="floor")
        done("vision-wide-14-u8-two-sizes")
        eng(torch.from_numpy(u8(31, 29, 7, n=3)))
        done("vision-wide-14-u8-batch")
        eng = E.ClipVisionEngine(state(E.clip_vision_param_shapes(**WIDE16), 3), "cpu", heads=HEADS, wide=True)
        weights["vision-wide-16"] = prepared(eng)
        rec.reset()
        eng(f32(1, 3, 48, 33))
        done("vision-wide-16-float-48x33")
        # ---- DinoVitEngine
        eng = D.DinoVitEngine({**state(D.dino_param_shapes(**DINO), 4), "head.weight": torch.zeros(3, 64)}, "cpu", heads=HEADS, resize=112)
        weights["dino"] = prepared(eng)
        rec.reset()
        eng.encode_pixels(f32(2, 3, 96, 96))
        done("dino-encode-pixels")
        frames = [u8(120, 150, 8), u8(200, 130, 9), torch.from_numpy(u8(112, 112, 10)), u8(120, 150, 11)]
        eng.patch_rows_u8(frames)
        done("dino-patch-rows-u8-mixed")
        eng(frames, batch=3)
        done("dino-call-batch-3-of-4")
        eng(u8(120, 150, 12, n=2))
        done("dino-call-whole-batch")
        # ---- ClipTextEngine
        tsd = {**state(E.clip_text_param_shapes(**TEXT), 5), "text_projection.weight": state({"p.weight": (16, 32)}, 6)["p.weight"]}
        eng = E.ClipTextEngine(tsd, "cpu", heads=HEADS)
        weights["text"] = prepared(eng)
        rec.reset()
        ids = torch.tensor([[1, 5, 9, 49, 0, 0], [2, 49, 0, 0, 0, 0]])
        _, pooled = eng(ids)
        done("text-no-mask")
        eng(ids, attention_mask=(ids != 0).long())
        done("text-attention-mask")
        eng.project(pooled)
        done("text-project")
        # ---- the three scorers on one small CLIPModel state dict
        vc = dict(NARROW, num_attention_heads=HEADS, hidden_act="quick_gelu", layer_norm_eps=1e-5)
        tc = dict(TEXT, num_attention_heads=HEADS, hidden_act="gelu", layer_norm_eps=1e-6)
        sd = {**state(E.clip_vision_param_shapes(**NARROW), 7), **tsd, "logit_scale": torch.tensor(4.6052)}
        cfg = dict(vision_config=vc, text_config=tc)
        floats = np.zeros((2, 40, 56, 3), np.float32)
        for name, sc, images in (("pick", mods["pick_score"].PickScorer(sd, cfg, device="cpu"), floats),
                                 ("align", mods["align"].FrameAligner(sd, cfg, device="cpu"), mixed),
                                 ("clip", mods["clip_score"].ClipScorer(sd, vc, sd, tc, device="cpu", crop="floor"), mixed)):
            weights[f"{name}-vision"], weights[f"{name}-text"] = prepared(sc.vision), prepared(sc.text)
            rec.reset()
            sc.image_features(images)
            done(f"{name}-image-features")
            sc.text_features(ids)
            done(f"{name}-text-features")
        sc = mods["clip_score"].ClipScorer(sd, vc, device="cpu")             # no text tower
        weights["clip-image-only-vision"] = prepared(sc.vision)
        rec.reset()
        sc.image_features(floats)
        done("clip-image-only-image-features")
    finally:
        for m in patched:
            m.ops = real_ops
    return {"launches": launches, "weights": weights}


def digest(entry: dict) -> str:
    return hashlib.sha256(json.dumps(entry, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:10]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    got = trace_cases()
    launches = {name: [digest(e) for e in log] for name, log in got["launches"].items()}

    def block(d):
        return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in d.items()) + "\n}"

    with open(path, "w") as f:
        f.write('{"launches": ' + block(launches) + ',\n"weights": ' + block(got["weights"]) + "}\n")
    print(f"{path}: {len(launches)} cases, {sum(map(len, launches.values()))} launches, {sum(map(len, got['weights'].values()))} tensors, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
