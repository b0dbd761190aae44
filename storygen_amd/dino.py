"""DINO's ViT (facebookresearch/dino vision_transformer.py: `dino_vitb8` of data_process/dup_remove.py:18) on the HIP kernels: the class
feature after the final LayerNorm, which is what `model(image)` returns there.

The tower is vit.VitTower, the one ClipVisionEngine runs, configured for DINO: erf GELU, LayerNorm eps 1e-6, no pre-LayerNorm (the first
layer reads the fp32 embedding), the patch projection's bias in the patch GEMM's epilogue, no projection head.  8x8 patches of a 224 crop are 785 tokens of 12
heads of 64: sg_attn_enc_f16.  Only the native grid runs: DINO's interpolate_pos_encoding is the identity there, any other input size is
refused.  8-bit frames are preprocessed as the script's transform does it — Pillow's 8-bit bicubic resize (shorter side to 256),
torchvision's CenterCrop(224), ToTensor, Normalize with the ImageNet constants — by sg_clip_patchify_u8 with ops.dedup_u8_geometry, one
launch per frame size.  The final LayerNorm kernel writes fp16, so the returned fp32 feature holds fp16 values.
There is no CPU path: importing this module loads libstorygen_hip.so."""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import ops
from .vit import F32, SD, VitTower, is_uint8_images

_LAYER_NAMES = (("norm1.", "layer_norm1."), ("norm2.", "layer_norm2."), ("attn.proj.", "self_attn.out_proj."), ("mlp.fc1.", "mlp.fc1."),
                ("mlp.fc2.", "mlp.fc2."))


def dino_param_shapes(embed_dim: int = 768, depth: int = 12, patch_size: int = 8, img_size: int = 224, mlp_ratio: float = 4.0
                      ) -> Dict[str, Tuple[int, ...]]:
    """Names and shapes of the state dict of DINO's VisionTransformer (num_classes = 0: its head is an Identity and has no entries)."""
    C, I = embed_dim, int(embed_dim * mlp_ratio)
    out: Dict[str, Tuple[int, ...]] = {"cls_token": (1, 1, C), "pos_embed": (1, (img_size // patch_size) ** 2 + 1, C),
                                       "patch_embed.proj.weight": (C, 3, patch_size, patch_size), "patch_embed.proj.bias": (C,)}
    for i in range(depth):
        p = f"blocks.{i}."
        out[p + "norm1.weight"], out[p + "norm1.bias"] = (C,), (C,)
        out[p + "attn.qkv.weight"], out[p + "attn.qkv.bias"] = (3 * C, C), (3 * C,)
        out[p + "attn.proj.weight"], out[p + "attn.proj.bias"] = (C, C), (C,)
        out[p + "norm2.weight"], out[p + "norm2.bias"] = (C,), (C,)
        out[p + "mlp.fc1.weight"], out[p + "mlp.fc1.bias"] = (I, C), (I,)
        out[p + "mlp.fc2.weight"], out[p + "mlp.fc2.bias"] = (C, I), (C,)
    out["norm.weight"], out["norm.bias"] = (C,), (C,)
    return out


def _depth(sd: SD) -> int:
    return 1 + max((int(k.split(".")[1]) for k in sd if k.startswith("blocks.")), default=-1)


def clip_layer_names(sd: SD, who: str = "DinoVitEngine") -> SD:
    """DINO's `blocks.*` under the names VitTower's layer stack reads (`encoder.layers.*`), the fused qkv rows split into q, k, v in that
    order."""
    out: SD = {}
    for i in range(_depth(sd)):
        p, q = f"blocks.{i}.", f"encoder.layers.{i}."
        for src, dst in _LAYER_NAMES:
            for leaf in ("weight", "bias"):
                out[q + dst + leaf] = sd[p + src + leaf]
        w, b = sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]
        C = w.shape[1]
        if tuple(w.shape) != (3 * C, C) or tuple(b.shape) != (3 * C,):
            raise ValueError(f"{who}: {p}attn.qkv is {tuple(w.shape)} / {tuple(b.shape)}, expected [3C, C] / [3C]")
        for j, n in enumerate(("q_proj.", "k_proj.", "v_proj.")):
            out[q + "self_attn." + n + "weight"], out[q + "self_attn." + n + "bias"] = w[j * C:(j + 1) * C], b[j * C:(j + 1) * C]
    return out


class DinoVitEngine:
    def __init__(self, state_dict: SD, device, heads: int = 12, eps: float = 1e-6, resize: int = 256):
        """state_dict: DINO's VisionTransformer.state_dict() (cls_token, pos_embed, patch_embed.proj.*, blocks.{i}.{norm1, attn.qkv,
        attn.proj, norm2, mlp.fc1, mlp.fc2}.*, norm.*; head.* ignored, anything else refused).  Patch size, token grid and crop size come
        from the weights; the limits are check_clip_dims_wide's."""
        who = "DinoVitEngine"
        sd = {k: v for k, v in state_dict.items() if not k.startswith("head.")}
        depth = _depth(sd)
        known = set(dino_param_shapes(8, depth, 1, 1))          # (the names do not depend on the geometry)
        unknown = sorted(k for k in sd if k not in known)
        missing = sorted(k for k in known if k not in sd)
        if unknown or missing or depth == 0:
            raise KeyError(f"{who}: not a DINO VisionTransformer state dict: unknown {unknown[:4]}, missing {missing[:4]}")
        wp, pos, cls = sd["patch_embed.proj.weight"], sd["pos_embed"], sd["cls_token"]
        if wp.dim() != 4 or pos.dim() != 3 or pos.shape[0] != 1 or cls.dim() != 3:
            raise ValueError(f"{who}: patch weight {tuple(wp.shape)} / pos_embed {tuple(pos.shape)} are not [C,3,ps,ps] / [1,T,C]")
        # erf GELU, no pre-LayerNorm, the patch projection's bias in the patch GEMM's epilogue, `norm` on the class rows
        t = self.tower = VitTower(who, device, wp, pos[0], cls[0, 0], clip_layer_names(sd, who), (sd["norm.weight"], sd["norm.bias"]), heads, eps,
                                  "gelu", True, patch_bias=sd["patch_embed.proj.bias"])
        self.C, self.ps, self.T, self.S, self.kpad, self.heads, self.eps, self.wp, self.ws, self.dev = \
            t.C, t.ps, t.T, t.S, t.kpad, t.heads, t.eps, t.wp, t.ws, t.dev
        self.resize = int(resize)
        if self.resize < self.S:
            raise ValueError(f"{who}: resize {resize} is below the crop size {self.S} (the script would pad; out of scope)")

    def patch_rows_u8(self, frames) -> torch.Tensor:
        """8-bit frames -> the patch GEMM's fp16 operand [B * (T - 1), kpad] under the script's transform; frames of one size share a launch."""
        return self.tower.patch_rows_u8(frames, ops.DEDUP_IMAGE_MEAN, ops.DEDUP_IMAGE_STD,
                                        lambda h, w: ops.dedup_u8_geometry(h, w, self.S, self.resize))

    def _features(self, a16: torch.Tensor) -> torch.Tensor:
        """The tower on patch rows -> the class feature, fp32 [B, C] holding fp16 values."""
        return self.tower.encode(a16, a16.shape[0] // (self.T - 1))[1].float()

    def encode_pixels(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """Already transformed [B,3,S,S] float input (what the script's `transform` returns) -> fp32 [B, C]; cut into patches as it is."""
        if not isinstance(pixel_values, torch.Tensor) or pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, self.S, self.S) or \
                not pixel_values.is_floating_point() or pixel_values.shape[0] == 0:
            got = tuple(pixel_values.shape) if isinstance(pixel_values, torch.Tensor) else type(pixel_values).__name__
            raise ValueError(f"DinoVitEngine: pixel_values must be float [B,3,{self.S},{self.S}] (only the native token grid runs), got {got}")
        return self._features(self.tower.patch_rows(pixel_values, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))

    def __call__(self, frames, batch: int = 16) -> torch.Tensor:
        """8-bit frames (a uint8 [N,h,w,3] array or tensor, a list of PIL RGB images or uint8 [h,w,3] arrays / tensors, sizes may differ)
        -> class features fp32 [N, C] on the device, at most `batch` frames per pass of the tower."""
        if not is_uint8_images(frames):
            raise TypeError("DinoVitEngine: frames are 8-bit (PIL RGB images or uint8 arrays), as the script reads them from disk; "
                            "transformed float input goes to encode_pixels")
        batch = int(batch)
        if batch < 1:
            raise ValueError(f"DinoVitEngine: batch must be at least 1, got {batch}")
        n = len(frames)
        if n == 0:
            raise ValueError("DinoVitEngine: no frames")
        out = torch.empty(n, self.C, dtype=F32, device=self.dev)
        for lo in range(0, n, batch):
            part = frames[lo:lo + batch]
            out[lo:lo + len(part)] = self._features(self.patch_rows_u8(part))
        return out
