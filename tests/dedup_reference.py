"""TEST INFRASTRUCTURE — restatements, on the CPU, of what storygen_amd.dedup computes on the GPU: data_process/dup_remove.py.

  * DINO's VisionTransformer forward (facebookresearch/dino vision_transformer.py, num_classes = 0) on transformed pixels, fp32; with
    `round_operands=True` it rounds to fp16 exactly where DinoVitEngine does (every MFMA operand, the LayerNorm outputs, q|k|v, the
    activation, the final feature): the distance between the two runs is the deviation the number formats alone account for.
    tests/test_dedup_host.py pins the structure to transformers.ViTModel through an explicit key map; DINO's own key names are restated
    from the upstream file, which is not vendored here: unpinned.
  * the script's transform: Resize(256, interpolation=3) + CenterCrop(224) + ToTensor + Normalize — the geometry here, the pixels through
    tests/clip_u8_reference.py's Pillow path with this geometry and the ImageNet constants.
  * the adjacent-cosine chain in float64 NumPy, the script's sequential loop written literally, and its `fns` sort key.

Nothing in the product imports this file."""
import re

import numpy as np
import torch
import torch.nn.functional as F

from tests import clip_u8_reference as U8
from tests.clip_vision_reference import patch_rows

MEAN = (0.485, 0.456, 0.406)                      # dup_remove.py:13
STD = (0.229, 0.224, 0.225)
TINY = dict(embed_dim=64, depth=2, patch_size=8, img_size=96, num_heads=2)      # 145 tokens of 2 heads of 32: the MFMA attention (T > 128)


# ------------------------------------------------------------------------------------------------------------------ the tower
def tiny_state(seed: int = 0, table_scale: float = 10.0, **over) -> dict:
    """fp16-representable DINO state dict for dict(TINY, **over) (without num_heads) with non-trivial LayerNorms; the position table,
    class token and patch projection are scaled by `table_scale` (trunc_normal_(std=.02) tables of a trained model's order at 10)."""
    from storygen_amd.dino import dino_param_shapes
    from storygen_amd.encoders import init_state
    c = dict(TINY, **over)
    shapes = dino_param_shapes(c["embed_dim"], c["depth"], c["patch_size"], c["img_size"], c.get("mlp_ratio", 4.0))
    sd = init_state({k.replace("pos_embed", "pos_embedding").replace("cls_token", "cls_embedding"): v for k, v in shapes.items()}, seed)
    sd = {k.replace("pos_embedding", "pos_embed").replace("cls_embedding", "cls_token"): v for k, v in sd.items()}
    g = torch.Generator().manual_seed(seed + 2)
    for k in sd:
        if "norm" in k:
            sd[k] = sd[k] + 0.2 * torch.randn(sd[k].shape, generator=g)
        if k in ("pos_embed", "cls_token") or k.startswith("patch_embed."):
            sd[k] = sd[k] * table_scale
        sd[k] = sd[k].half().float()
    return sd


def _r(t, on):
    return t.half().float() if on else t


def dino_forward(sd, pixels: torch.Tensor, heads: int, eps: float = 1e-6, round_operands: bool = False) -> torch.Tensor:
    """VisionTransformer.forward(x) on [B,3,S,S] at the native grid (interpolate_pos_encoding is the identity): prepare_tokens =
    cat(cls_token, patch_embed(x)) + pos_embed; blocks x + attn(norm1(x)), x + mlp(norm2(x)) with erf GELU; norm; the class row."""
    g = lambda n: sd[n].float()   # noqa: E731
    r = lambda t: _r(t, round_operands)   # noqa: E731
    wp = g("patch_embed.proj.weight")
    C, ps = wp.shape[0], wp.shape[2]
    B = pixels.shape[0]
    pe = r(patch_rows(pixels.float(), ps)) @ r(wp.reshape(C, -1)).t() + g("patch_embed.proj.bias")      # = conv2d(x, w, b, stride=ps)
    P = pe.shape[0] // B
    x = torch.cat([g("cls_token").expand(B, 1, C), pe.view(B, P, C)], 1) + g("pos_embed")
    T, D = P + 1, C // heads
    i = 0
    while f"blocks.{i}.norm1.weight" in sd:
        p = f"blocks.{i}."
        lin = lambda t, n: r(t) @ r(g(p + n + ".weight")).t() + g(p + n + ".bias")   # noqa: E731
        h = F.layer_norm(x, (C,), g(p + "norm1.weight"), g(p + "norm1.bias"), eps)
        qkv = r(lin(h, "attn.qkv")).view(B, T, 3, heads, D).permute(2, 0, 3, 1, 4)                       # rows in q, k, v order
        a = torch.softmax((qkv[0] * D ** -0.5) @ qkv[1].transpose(-1, -2), -1) @ qkv[2]
        x = x + lin(a.transpose(1, 2).reshape(B, T, C), "attn.proj")
        h = F.layer_norm(x, (C,), g(p + "norm2.weight"), g(p + "norm2.bias"), eps)
        x = x + lin(F.gelu(r(lin(h, "mlp.fc1"))), "mlp.fc2")
        i += 1
    return r(F.layer_norm(x[:, 0], (C,), g("norm.weight"), g("norm.bias"), eps))


def vit_key_map(depth: int) -> dict:
    """DINO name -> transformers.ViTModel name (5.x: layers.{i}.attention.{q,k,v,o}_proj, layernorm_before / after, mlp.fc1 / fc2); the
    fused qkv maps to three names (a tuple)."""
    m = {"cls_token": "embeddings.cls_token", "pos_embed": "embeddings.position_embeddings",
         "patch_embed.proj.weight": "embeddings.patch_embeddings.projection.weight",
         "patch_embed.proj.bias": "embeddings.patch_embeddings.projection.bias", "norm.weight": "layernorm.weight", "norm.bias": "layernorm.bias"}
    for i in range(depth):
        p, q = f"blocks.{i}.", f"layers.{i}."
        for leaf in ("weight", "bias"):
            m[p + "norm1." + leaf] = q + "layernorm_before." + leaf
            m[p + "norm2." + leaf] = q + "layernorm_after." + leaf
            m[p + "attn.proj." + leaf] = q + "attention.o_proj." + leaf
            m[p + "mlp.fc1." + leaf] = q + "mlp.fc1." + leaf
            m[p + "mlp.fc2." + leaf] = q + "mlp.fc2." + leaf
            m[p + "attn.qkv." + leaf] = tuple(q + f"attention.{n}_proj." + leaf for n in "qkv")
    return m


def to_vit_state(sd) -> dict:
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    out = {}
    for k, name in vit_key_map(depth).items():
        if isinstance(name, tuple):
            for part, n in zip(sd[k].chunk(3, 0), name):
                out[n] = part.clone()
        else:
            out[name] = sd[k].clone()
    return out


# -------------------------------------------------------------------------------------------------------------- the transform
def geometry(h: int, w: int, S: int = 224, resize: int = 256):
    """(Hr, Wr, top, left) of Resize(resize) + CenterCrop(S): the shorter side becomes `resize`, the longer int(resize * long / short);
    the crop's offset is int(round((size - S) / 2.0)) — Python's round, halves to even (torchvision's CenterCrop)."""
    short, long_ = (w, h) if w <= h else (h, w)
    new_long = int(resize * long_ / short)
    Hr, Wr = (new_long, resize) if w <= h else (resize, new_long)
    assert min(Hr, Wr) >= S, "the script would pad: out of scope"
    return Hr, Wr, int(round((Hr - S) / 2.0)), int(round((Wr - S) / 2.0))


def pixel_values(frames, S: int = 224, resize: int = 256) -> torch.Tensor:
    """uint8 [h,w,3] frames of any sizes -> what the script's `transform` returns, stacked: fp32 [N,3,S,S]."""
    return torch.from_numpy(np.concatenate([U8.preprocess([a], S, geom=geometry(a.shape[0], a.shape[1], S, resize), mean=MEAN, std=STD)[1]
                                            for a in frames]))


def patch_rows_u8(frames, S: int, ps: int, resize: int, kpad=None) -> np.ndarray:
    """The fp16 patch rows sg_clip_patchify_u8 writes for these frames under the script's transform."""
    return np.concatenate([U8.reference([a], S, ps, geom=geometry(a.shape[0], a.shape[1], S, resize), kpad=kpad, mean=MEAN, std=STD)[1]
                           for a in frames])


def block_image(seed: int, h: int, w: int, cells: int = 6) -> np.ndarray:
    """uint8 [h,w,3]: cells x cells random colour blocks — content a patch embedding tells apart, unlike per-pixel noise."""
    g = np.random.default_rng(seed).integers(0, 256, (cells, cells, 3))
    return g[np.arange(h) * cells // h][:, np.arange(w) * cells // w].astype(np.uint8)


def near_copy(a: np.ndarray, seed: int, amp: int = 3) -> np.ndarray:
    """`a` with every byte moved by at most `amp`: a keyframe of the same shot."""
    d = np.random.default_rng(seed).integers(-amp, amp + 1, a.shape)
    return np.clip(a.astype(np.int16) + d, 0, 255).astype(np.uint8)


def keyframes():
    """Eight frames of mixed sizes in four shots: (0 1 2) (3 4) (5) (6 7).  The script deletes 0, 1, 3 and 6."""
    a, b, c, d = block_image(1, 120, 150), block_image(2, 200, 130), block_image(3, 112, 140), block_image(4, 120, 150)
    return [a, near_copy(a, 10), near_copy(a, 11), b, near_copy(b, 12), c, d, near_copy(d, 13)]


# ------------------------------------------------------------------------------------------------------------ the decisions
def adjacent_cosine(feats: np.ndarray, threshold: float = 0.75, eps: float = 1e-8):
    """(sim float64 [N], drop bool [N]) from fp32 features [N, dim], all in float64: sim[0] = 0 (the zero previous feature),
    sim[i] = f_i . f_{i-1} / (max(|f_i|, eps) max(|f_{i-1}|, eps)); drop[i] = i + 1 < N and sim[i + 1] >= threshold."""
    f = np.asarray(feats)
    assert f.dtype == np.float32 and f.ndim == 2
    f = f.astype(np.float64)
    N = f.shape[0]
    sim = np.zeros(N)
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.maximum(np.sqrt((f * f).sum(1)), eps)
        for i in range(1, N):
            sim[i] = (f[i] * f[i - 1]).sum() / (norm[i] * norm[i - 1])
        drop = np.zeros(N, bool)
        drop[:-1] = sim[1:] >= threshold                     # False for NaN
    return sim, drop


def script_loop(similarities, threshold: float = 0.75):
    """dup_remove.py:23-46 written literally on a sequence of similarities (entry i: frame i against pre_feature): the set of removed
    indices.  `pre_i_path` starts as '' (no file: nothing to remove) and advances on every frame."""
    removed, pre = set(), None
    for i, s in enumerate(similarities):
        if s >= threshold:
            if pre is not None:
                removed.add(pre)
        pre = i
    return removed


def fns(name: str) -> tuple:
    """The sort key of dup_remove.py:27: 'a' + name + '0' read as alternating runs of non-digits and digits — the string starts with a
    non-digit and ends with a digit, so the runs pair up —, flattened to (text, number, text, number, ...)."""
    parts = re.split(r"(\d+)", "a" + name + "0")            # [text, digits, text, digits, ..., ""]
    assert parts[-1] == "" and len(parts) % 2 == 1
    return tuple(int(p) if k % 2 else p for k, p in enumerate(parts[:-1]))
