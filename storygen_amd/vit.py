"""The ViT pieces that are not CLIP's alone: the pre-LN layer stack every tower runs (_ClipLayers), the host-side limits of its attention
kernels, the grouping of 8-bit frames by size, and VitTower — patch rows -> patch GEMM -> sg_clip_embed_patches -> layer stack ->
LayerNorm on the class rows — which ClipVisionEngine (encoders.py) and DinoVitEngine (dino.py) configure and nothing else repeats.
Launch sequences over the kernels of ops.py; the residual stream is fp32, every MFMA operand fp16.  There is no CPU path."""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from . import ops

F16, F32 = torch.float16, torch.float32
SD = Dict[str, torch.Tensor]
Pair = Tuple[torch.Tensor, torch.Tensor]


def _count(sd: SD, prefix: str) -> int:
    idx = {int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix)}
    return 1 + max(idx) if idx else 0


def check_clip_dims(who: str, hidden: int, heads: int, tokens: int) -> None:
    """The limits of sg_attn_small_f16 / sg_gemm_f16 for a CLIP tower: raises ValueError before anything touches the device."""
    if heads <= 0 or hidden % heads or hidden // heads > 64 or hidden % 8:
        raise ValueError(f"{who}: hidden size {hidden} / {heads} heads is outside sg_attn_small_f16 (head dim <= 64)")
    if tokens > 128:
        raise ValueError(f"{who}: {tokens} tokens exceed sg_attn_small_f16's 128 (ViT-H/14, 257 tokens of head dim 80, is out of scope)")


def check_clip_dims_wide(who: str, hidden: int, heads: int, tokens: int) -> None:
    """The limits of sg_attn_enc_f16 / sg_gemm_f16 for a ViT tower (VitTower(wide=True): ViT-H/14, PickScore; DINO)."""
    if heads <= 0 or hidden % heads or hidden % 8:
        raise ValueError(f"{who}: hidden size {hidden} does not split into {heads} heads of whole 8-channel groups")
    d = hidden // heads
    if d % 8 or d < 8 or d > 128:
        raise ValueError(f"{who}: head dim {d} is outside sg_attn_enc_f16 (a multiple of 8 in [8, 128])")
    if tokens < 1 or tokens > 1024:
        raise ValueError(f"{who}: {tokens} tokens exceed sg_attn_enc_f16's 1024")


class _ClipLayers:
    """The pre-LN transformer layers the towers share (transformers CLIPEncoder): weights of `encoder.layers.*` and the launch
    sequence of one pass over them.  The residual stream is fp32, every MFMA operand fp16."""

    def __init__(self, sd: SD, dev: torch.device, heads: int, eps: float, hidden_act: str, who: str):
        if hidden_act not in ("quick_gelu", "gelu"):
            raise ValueError(f"{who}: unsupported hidden_act {hidden_act!r}")
        self.dev, self.heads, self.eps = dev, heads, eps
        self.act = ops.ACT_QUICK_GELU if hidden_act == "quick_gelu" else ops.ACT_GELU

        def d16(t):
            return t.detach().to(dev, F32).to(F16).contiguous()

        self.layers = []
        for i in range(_count(sd, "encoder.layers.")):
            p = f"encoder.layers.{i}."
            a = p + "self_attn."
            self.layers.append(dict(
                ln1=(d16(sd[p + "layer_norm1.weight"]), d16(sd[p + "layer_norm1.bias"])),
                ln2=(d16(sd[p + "layer_norm2.weight"]), d16(sd[p + "layer_norm2.bias"])),
                wqkv=d16(torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]], 0)),
                bqkv=d16(torch.cat([sd[a + "q_proj.bias"], sd[a + "k_proj.bias"], sd[a + "v_proj.bias"]], 0)),
                wo=d16(sd[a + "out_proj.weight"]), bo=d16(sd[a + "out_proj.bias"]),
                w1=d16(sd[p + "mlp.fc1.weight"]), b1=d16(sd[p + "mlp.fc1.bias"]),
                w2=d16(sd[p + "mlp.fc2.weight"]), b2=d16(sd[p + "mlp.fc2.bias"])))
        self.inner = self.layers[0]["w1"].shape[0]
        self.ws = ops.new_workspace(64 << 20, dev)

    def run(self, x: torch.Tensor, xo: torch.Tensor, B: int, T: int, causal: bool, key_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The first layer reads the stream x [B*T, C] (fp32, or the fp16 output of a LayerNorm), every layer leaves its result in the fp32
        stream xo (which may be x itself).  Returns an fp16 [B*T, C] scratch buffer for the caller's final LayerNorm."""
        M, C = xo.shape
        H, dev = self.heads, self.dev
        x2 = torch.empty_like(xo)
        h16 = torch.empty(M, C, dtype=F16, device=dev)
        qkv = torch.empty(M, 3 * C, dtype=F16, device=dev)
        a16 = torch.empty(M, C, dtype=F16, device=dev)
        u16 = torch.empty(M, self.inner, dtype=F16, device=dev)
        q3 = qkv.view(B, T, 3 * C)
        scale = (C // H) ** -0.5
        # per tower: the scalar LDS-resident kernel where it fits (CLIP text, ViT-B/32), the MFMA encoder kernel beyond it (ViT-H/14)
        attn = ops.attention_small if T <= 128 and C // H <= 64 else ops.attention_enc
        for L in self.layers:
            ops.layernorm(x, L["ln1"][0], L["ln1"][1], h16, self.eps)
            ops.gemm(h16, L["wqkv"], qkv, bias=L["bqkv"], workspace=self.ws)
            attn(q3[:, :, :C], q3[:, :, C:2 * C], q3[:, :, 2 * C:], a16.view(B, T, C), H, scale, causal, key_bias)
            ops.gemm(a16, L["wo"], x2, bias=L["bo"], res1=x, workspace=self.ws)
            ops.layernorm(x2, L["ln2"][0], L["ln2"][1], h16, self.eps)
            ops.gemm(h16, L["w1"], u16, bias=L["b1"], workspace=self.ws)
            ops.act_rows(u16, self.act)
            ops.gemm(u16, L["w2"], xo, bias=L["b2"], res1=x2, workspace=self.ws)
            x = xo
        return h16


def is_uint8_images(images) -> bool:
    """True for what the scorers and the image towers treat as 8-bit frames: a uint8 array or tensor, or a list / tuple whose first entry is
    a PIL image or a uint8 array / tensor.  Anything else (float tensors and arrays) takes the float path."""
    if isinstance(images, (list, tuple)):
        if len(images) == 0:
            return False
        first = images[0]
        if hasattr(first, "mode") and hasattr(first, "size") and not isinstance(first, (np.ndarray, torch.Tensor)):      # a PIL image
            return True
        images = first
    if isinstance(images, np.ndarray):
        return images.dtype == np.uint8
    return isinstance(images, torch.Tensor) and images.dtype == torch.uint8


def u8_frame_groups(frames, who: str):
    """8-bit frames (is_uint8_images) -> (count, {(h, w, 3): a uint8 [B,h,w,3] tensor or [(index, uint8 [h,w,3])]}), RGB only."""
    from .image import _as_u8
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 4 or frames.shape[3] != 3 or 0 in frames.shape:
            raise ValueError(f"{who}: uint8 frames must be [B,h,w,3], got {tuple(frames.shape)}")
        return frames.shape[0], {tuple(frames.shape[1:]): frames}
    if len(frames) == 0:
        raise ValueError(f"{who}: no frames")
    groups = {}
    for i, im in enumerate(frames):
        t = _as_u8(im, 3, who)
        if t.shape[2] != 3:
            raise ValueError(f"{who}: frames are RGB [h,w,3], got {tuple(t.shape)} (.convert('RGB') stays with the caller)")
        groups.setdefault(tuple(t.shape), []).append((i, t))
    return len(frames), groups


class VitTower:
    """A ViT image tower on the HIP kernels: geometry from the weights (C, ps, T, S = grid * ps, the patch row 3 * ps^2 padded to kpad),
    the fp16 patch weight wp [C, kpad], the two front ends that cut images into patch rows, and the tower itself.  The narrow tower
    (sg_attn_small_f16: at most 128 tokens, head dim <= 64) needs 3 * ps^2 to be a multiple of 8; wide=True lifts the limits to
    sg_attn_enc_f16's (up to 1024 tokens, head dim a multiple of 8 up to 128) and rounds a patch row that is a multiple of 4 up to 8
    (patch size 14: 588 -> 592, zero columns appended once to wp).  Refusals are raised under the caller's name `who`."""

    def __init__(self, who: str, device, patch_weight: torch.Tensor, positions: torch.Tensor, cls: torch.Tensor, layers: SD, final_ln: Pair,
                 heads: int, eps: float, hidden_act: str, wide: bool, patch_bias: Optional[torch.Tensor] = None, pre_ln: Optional[Pair] = None,
                 image_size: Optional[int] = None):
        """patch_weight [C,3,ps,ps], positions [T,C], cls [C], layers: the `encoder.layers.*` entries _ClipLayers reads; image_size: what
        the caller's config says S is, refused if the weights say otherwise."""
        wp, pos = patch_weight, positions
        shapes = f"{who}: patch weight {tuple(wp.shape)} / positions {tuple(pos.shape)} are not a square grid of RGB patches"
        if wp.dim() != 4 or pos.dim() != 2:
            raise ValueError(shapes)
        self.who, self.C, self.ps, self.T = who, wp.shape[0], wp.shape[2], pos.shape[0]
        grid = math.isqrt(max(self.T - 1, 0))
        if wp.shape[1] != 3 or wp.shape[3] != self.ps or grid * grid != self.T - 1 or grid == 0 or pos.shape[1] != self.C or \
                tuple(cls.shape) != (self.C,):
            raise ValueError(shapes)
        self.S = grid * self.ps
        if image_size is not None and image_size != self.S:
            raise ValueError(f"{who}: image_size {image_size} does not match {grid} x {grid} patches of {self.ps}")
        K = 3 * self.ps * self.ps
        self.wide, self.kpad = bool(wide), K
        if wide:
            check_clip_dims_wide(who, self.C, heads, self.T)
            if K % 4:
                raise ValueError(f"{who}: 3 * patch_size^2 = {K} must be a multiple of 4")
            self.kpad = (K + 7) & ~7
        else:
            check_clip_dims(who, self.C, heads, self.T)
            if K % 8:
                raise ValueError(f"{who}: 3 * patch_size^2 = {K} must be a multiple of 8")
        self.dev = torch.device(device)
        self.heads, self.eps = heads, eps

        def d16(t):
            return t.detach().to(self.dev, F32).to(F16).contiguous()

        self.wp = d16(wp.reshape(self.C, K))                               # (c, dy, dx) columns: the patchify kernels' order
        if self.kpad != K:                                                 # zero columns against the zero columns of the padded patch rows
            self.wp = torch.nn.functional.pad(self.wp, (0, self.kpad - K)).contiguous()
        self.bp = None if patch_bias is None else d16(patch_bias)
        self.cls = cls.detach().to(self.dev, F32).contiguous()
        self.pos = pos.detach().to(self.dev, F32).contiguous()
        self.pre = None if pre_ln is None else (d16(pre_ln[0]), d16(pre_ln[1]))
        self.post = (d16(final_ln[0]), d16(final_ln[1]))
        self.stack = _ClipLayers(layers, self.dev, heads, eps, hidden_act, who)
        self.ws = self.stack.ws

    # ------------------------------------------------------------------------------------------------------------ front ends
    def _rows(self, B: int) -> torch.Tensor:
        return torch.empty(B * (self.T - 1), self.kpad, dtype=F16, device=self.dev)

    def patch_rows(self, img: torch.Tensor, mean, std, *affine) -> torch.Tensor:
        """Float NCHW [B,3,H,W] -> the patch GEMM's fp16 operand [B * (T - 1), kpad] (ops.clip_patchify: resize, centre crop, Normalize(mean,
        std)); affine: optionally (in_scale, in_shift), applied to the pixel values first."""
        a16 = self._rows(img.shape[0])
        img = img.detach().to(self.dev, F32).contiguous()
        if self.kpad == 3 * self.ps * self.ps:
            ops.clip_patchify(img, a16, self.S, self.ps, mean, std, *affine)
        else:
            ops.clip_patchify(img, a16, self.S, self.ps, mean, std, *affine, kpad=self.kpad)
        return a16

    def patch_rows_u8(self, frames, mean, std, geometry: Callable[[int, int], tuple]) -> torch.Tensor:
        """8-bit frames -> the same operand through sg_clip_patchify_u8 (Pillow's 8-bit bicubic resize bit for bit, crop, ToTensor,
        Normalize(mean, std)); geometry(h, w) -> (Hr, Wr, top, left).  Frames of one size share a launch, as image.py groups them."""
        B, groups = u8_frame_groups(frames, self.who)
        P = self.T - 1
        a16 = self._rows(B)
        for (h, w, _), members in groups.items():
            whole = isinstance(members, torch.Tensor) or len(members) == B
            batch = members.to(self.dev) if isinstance(members, torch.Tensor) else torch.stack([t.to(self.dev) for _, t in members])
            if batch.stride(3) != 1 or batch.stride(2) != 3:
                batch = batch.contiguous()
            rows = a16 if whole else self._rows(len(members))
            ops.clip_patchify_u8(batch, rows, self.S, self.ps, mean, std, geometry=geometry(h, w), kpad=self.kpad)
            if not whole:
                a16.view(B, P, self.kpad)[torch.tensor([i for i, _ in members], device=self.dev)] = rows.view(len(members), P, self.kpad)
        return a16

    # ----------------------------------------------------------------------------------------------------------------- tower
    def encode(self, a16: torch.Tensor, B: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The tower on the patch rows a16 [B * (T - 1), kpad] -> (the fp32 stream after the last layer [B * T, C], the final LayerNorm of
        its class rows fp16 [B, C])."""
        dev, C, T = self.dev, self.C, self.T
        pe = torch.empty(B * (T - 1), C, dtype=F32, device=dev)
        if self.bp is None:
            ops.gemm(a16, self.wp, pe, workspace=self.ws)
        else:
            ops.gemm(a16, self.wp, pe, bias=self.bp, workspace=self.ws)
        x = torch.empty(B * T, C, dtype=F32, device=dev)
        ops.clip_embed_patches(pe, self.cls, self.pos, x, T)               # cat(class, patches) + positions
        if self.pre is None:
            self.stack.run(x, x, B, T, False)                              # the first layer reads the fp32 stream
        else:
            h0 = torch.empty(B * T, C, dtype=F16, device=dev)
            ops.layernorm(x, self.pre[0], self.pre[1], h0, self.eps)       # CLIP's pre_layrnorm: the stream the first layer reads and adds to
            x = torch.empty(B * T, C, dtype=F32, device=dev)
            self.stack.run(h0, x, B, T, False)
        c16 = torch.empty(B, C, dtype=F16, device=dev)
        ops.layernorm(x.view(B, T * C)[:, :C], self.post[0], self.post[1], c16, self.eps)
        return x, c16
