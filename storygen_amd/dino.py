"""DINO's ViT (facebookresearch/dino vision_transformer.py: `dino_vitb8` of data_process/dup_remove.py:18) on the HIP kernels: the class
feature after the final LayerNorm, which is what `model(image)` returns there.

The tower is the pre-LN stack the CLIP towers run (_ClipLayers, unchanged): erf GELU, LayerNorm eps 1e-6, no pre-LayerNorm (the first
layer reads the fp32 embedding), the patch projection's bias in the patch GEMM's epilogue.  8x8 patches of a 224 crop are 785 tokens of 12
heads of 64: sg_attn_enc_f16.  Only the native grid runs: DINO's interpolate_pos_encoding is the identity there, any other input size is
refused.  8-bit frames are preprocessed as the script's transform does it — Pillow's 8-bit bicubic resize (shorter side to 256),
torchvision's CenterCrop(224), ToTensor, Normalize with the ImageNet constants — by sg_clip_patchify_u8 with ops.dedup_u8_geometry, one
launch per frame size.  The final LayerNorm kernel writes fp16, so the returned fp32 feature holds fp16 values.
There is no CPU path: importing this module loads libstorygen_hip.so."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch

from . import ops
from .encoders import F16, F32, SD, _ClipLayers, _count, check_clip_dims_wide, is_uint8_images

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


def clip_layer_names(sd: SD, who: str = "DinoVitEngine") -> SD:
    """DINO's `blocks.*` under the names _ClipLayers reads (`encoder.layers.*`), the fused qkv rows split into q, k, v in that order."""
    depth = _count(sd, "blocks.")
    out: SD = {}
    for i in range(depth):
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


def _frame_groups(frames, who: str):
    """8-bit frames (is_uint8_images) -> (count, {(h, w, 3): a uint8 [B,h,w,3] tensor or [(index, uint8 [h,w,3])]}), RGB only."""
    from .image import _as_u8
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 4 or frames.shape[3] != 3 or 0 in frames.shape:
            raise ValueError(f"{who}: uint8 frames must be [B,h,w,3], got {tuple(frames.shape)}")
        return frames.shape[0], {tuple(frames.shape[1:]): frames}
    groups = {}
    for i, im in enumerate(frames):
        t = _as_u8(im, 3, who)
        if t.shape[2] != 3:
            raise ValueError(f"{who}: frames are RGB [h,w,3], got {tuple(t.shape)} (.convert('RGB') stays with the caller)")
        groups.setdefault(tuple(t.shape), []).append((i, t))
    return len(frames), groups


class DinoVitEngine:
    def __init__(self, state_dict: SD, device, heads: int = 12, eps: float = 1e-6, resize: int = 256):
        """state_dict: DINO's VisionTransformer.state_dict() (cls_token, pos_embed, patch_embed.proj.*, blocks.{i}.{norm1, attn.qkv,
        attn.proj, norm2, mlp.fc1, mlp.fc2}.*, norm.*; head.* ignored, anything else refused).  Patch size, token grid and crop size come
        from the weights; the limits are check_clip_dims_wide's."""
        who = "DinoVitEngine"
        sd = {k: v for k, v in state_dict.items() if not k.startswith("head.")}
        depth = _count(sd, "blocks.")
        known = set(dino_param_shapes(8, depth, 1, 1))          # (the names do not depend on the geometry)
        unknown = sorted(k for k in sd if k not in known)
        missing = sorted(k for k in known if k not in sd)
        if unknown or missing or depth == 0:
            raise KeyError(f"{who}: not a DINO VisionTransformer state dict: unknown {unknown[:4]}, missing {missing[:4]}")
        wp, pos = sd["patch_embed.proj.weight"], sd["pos_embed"]
        if wp.dim() != 4 or pos.dim() != 3 or pos.shape[0] != 1:
            raise ValueError(f"{who}: patch weight {tuple(wp.shape)} / pos_embed {tuple(pos.shape)} are not [C,3,ps,ps] / [1,T,C]")
        self.C, self.ps, self.T = wp.shape[0], wp.shape[2], pos.shape[1]
        grid = math.isqrt(max(self.T - 1, 0))
        if wp.shape[1] != 3 or wp.shape[3] != self.ps or grid * grid != self.T - 1 or grid == 0 or pos.shape[2] != self.C or \
                tuple(sd["cls_token"].shape) != (1, 1, self.C):
            raise ValueError(f"{who}: patch weight {tuple(wp.shape)} / pos_embed {tuple(pos.shape)} are not a square grid of RGB patches")
        self.S = grid * self.ps
        check_clip_dims_wide(who, self.C, heads, self.T)
        K = 3 * self.ps * self.ps
        if K % 4:
            raise ValueError(f"{who}: 3 * patch_size^2 = {K} must be a multiple of 4")
        self.kpad = (K + 7) & ~7
        self.resize = int(resize)
        if self.resize < self.S:
            raise ValueError(f"{who}: resize {resize} is below the crop size {self.S} (the script would pad; out of scope)")
        self.dev = torch.device(device)
        self.heads, self.eps = heads, eps

        def d16(t):
            return t.detach().to(self.dev, F32).to(F16).contiguous()

        self.wp = d16(wp.reshape(self.C, K))                               # (c, dy, dx) columns: the patchify kernel's order
        if self.kpad != K:
            self.wp = torch.nn.functional.pad(self.wp, (0, self.kpad - K)).contiguous()
        self.bp = d16(sd["patch_embed.proj.bias"])
        self.cls = sd["cls_token"].detach().to(self.dev, F32).reshape(self.C).contiguous()
        self.pos = pos.detach().to(self.dev, F32).reshape(self.T, self.C).contiguous()
        self.norm = (d16(sd["norm.weight"]), d16(sd["norm.bias"]))
        self.stack = _ClipLayers(clip_layer_names(sd, who), self.dev, heads, eps, "gelu", who)
        self.ws = self.stack.ws

    # ------------------------------------------------------------------------------------------------------------ front ends
    def patch_rows_u8(self, frames) -> torch.Tensor:
        """8-bit frames -> the patch GEMM's fp16 operand [B * (T - 1), kpad] under the script's transform; frames of one size share a launch."""
        who = "DinoVitEngine"
        B, groups = _frame_groups(frames, who)
        if B == 0:
            raise ValueError(f"{who}: no frames")
        P = self.T - 1
        a16 = torch.empty(B * P, self.kpad, dtype=F16, device=self.dev)
        for (h, w, _), members in groups.items():
            geometry = ops.dedup_u8_geometry(h, w, self.S, self.resize)
            whole = isinstance(members, torch.Tensor) or len(members) == B
            batch = members.to(self.dev) if isinstance(members, torch.Tensor) else torch.stack([t.to(self.dev) for _, t in members])
            if batch.stride(3) != 1 or batch.stride(2) != 3:
                batch = batch.contiguous()
            rows = a16 if whole else torch.empty(len(members) * P, self.kpad, dtype=F16, device=self.dev)
            ops.clip_patchify_u8(batch, rows, self.S, self.ps, ops.DEDUP_IMAGE_MEAN, ops.DEDUP_IMAGE_STD, geometry=geometry, kpad=self.kpad)
            if not whole:
                a16.view(B, P, self.kpad)[torch.tensor([i for i, _ in members], device=self.dev)] = rows.view(len(members), P, self.kpad)
        return a16

    def _encode(self, a16: torch.Tensor, B: int) -> torch.Tensor:
        """The tower on the patch rows a16 [B * (T - 1), kpad] -> the class feature, fp32 [B, C] holding fp16 values."""
        dev, C, T = self.dev, self.C, self.T
        pe = torch.empty(B * (T - 1), C, dtype=F32, device=dev)
        ops.gemm(a16, self.wp, pe, bias=self.bp, workspace=self.ws)
        e = torch.empty(B * T, C, dtype=F32, device=dev)
        ops.clip_embed_patches(pe, self.cls, self.pos, e, T)               # cat(cls_token, patches) + pos_embed
        self.stack.run(e, e, B, T, False)                                  # no pre-LayerNorm: the first layer reads the fp32 stream
        f16 = torch.empty(B, C, dtype=F16, device=dev)
        ops.layernorm(e.view(B, T * C)[:, :C], self.norm[0], self.norm[1], f16, self.eps)      # `norm` on the class rows
        return f16.float()

    def encode_pixels(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """Already transformed [B,3,S,S] float input (what the script's `transform` returns) -> fp32 [B, C]; cut into patches as it is."""
        if not isinstance(pixel_values, torch.Tensor) or pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, self.S, self.S) or \
                not pixel_values.is_floating_point() or pixel_values.shape[0] == 0:
            got = tuple(pixel_values.shape) if isinstance(pixel_values, torch.Tensor) else type(pixel_values).__name__
            raise ValueError(f"DinoVitEngine: pixel_values must be float [B,3,{self.S},{self.S}] (only the native token grid runs), got {got}")
        B, K = pixel_values.shape[0], 3 * self.ps * self.ps
        img = pixel_values.detach().to(self.dev, F32).contiguous()
        a16 = torch.empty(B * (self.T - 1), self.kpad, dtype=F16, device=self.dev)
        ident = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        if self.kpad == K:
            ops.clip_patchify(img, a16, self.S, self.ps, *ident)
        else:
            ops.clip_patchify(img, a16, self.S, self.ps, *ident, kpad=self.kpad)
        return self._encode(a16, B)

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
            out[lo:lo + len(part)] = self._encode(self.patch_rows_u8(part), len(part))
        return out
