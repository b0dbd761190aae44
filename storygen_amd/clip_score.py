"""CLIP-I / CLIP-T scoring of generated frames on the HIP kernels: what the reference's evaluation/calc_CLIP_image.py and
evaluation/calc_CLIP_text.py compute with the `clip` package's ViT-B/32 (image-to-image and image-to-text cosine similarity of the
projected, L2-normalised features; the scripts print the mean over pairs).

    scorer = ClipScorer(vision_sd, vision_cfg, text_sd, text_cfg, device="cuda")
    frames = pipe(..., output_type="np").images                       # [N, H, W, 3] in [0, 1]
    scorer.clip_i(frames, gt_frames).mean(), scorer.clip_t(frames, tokenizer(prompts, ...).input_ids).mean()

Weights are state dicts in transformers naming (CLIPVisionModelWithProjection / CLIPTextModelWithProjection, or one CLIPModel state
dict passed for both); the tokenizer is the caller's.  The scripts score saved 8-bit images, and so does this when it is given 8-bit
frames (a uint8 [N,h,w,3] array or tensor, a list of PIL RGB images or uint8 arrays, sizes may differ): sg_clip_patchify_u8 runs Pillow's
8-bit bicubic resize bit for bit, the centre crop (`crop`, default "torchvision": CenterCrop of the `clip` package), ToTensor and Normalize —
the scripts' preprocessing exactly.  Float frames are not quantised on the way: they go through sg_clip_patchify_f16, an antialiased float
bicubic with the same geometry, which differs from the scripts' by up to about one 8-bit level per pixel.  Then ClipVisionEngine; texts
through ClipTextEngine and its projection.
Models outside sg_attn_small_f16 (more than 128 tokens, head dim above 64: ViT-H/14) are refused on the host; PickScore's ViT-H/14 runs in
storygen_amd/pick_score.py.  There is no CPU path."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import ops
from .encoders import ClipTextEngine, ClipVisionEngine, check_clip_dims, is_uint8_images

SD = Dict[str, torch.Tensor]
VISION_KEYS = ("hidden_size", "num_attention_heads", "image_size", "patch_size")
TEXT_KEYS = ("hidden_size", "num_attention_heads")
VISION_PREFIXES, TEXT_PREFIXES = ("vision_model.", "visual_projection."), ("text_model.", "text_projection.")


def _cfg(config, keys, who: str) -> dict:
    cfg = config.to_dict() if hasattr(config, "to_dict") else dict(config)
    missing = [k for k in keys if k not in cfg]
    if missing:
        raise KeyError(f"{who}: config lacks {missing}")
    return cfg


def _sub(sd: SD, prefixes) -> SD:
    return {k: v for k, v in sd.items() if k.startswith(prefixes)}


def clip_grid_tokens(cfg, who: str, size_key: str = "image_size", patch_key: str = "patch_size") -> Tuple[int, int, int]:
    """(image size S, patch size ps, tokens of the S / ps grid plus the class token) of a vision config; refuses a grid that does not tile."""
    S, ps = int(cfg[size_key]), int(cfg[patch_key])
    if S <= 0 or ps <= 0 or S % ps:
        raise ValueError(f"{who}: {size_key} {S} is not a multiple of {patch_key} {ps}")
    return S, ps, (S // ps) ** 2 + 1


def build_clip_towers(sd: SD, vc: dict, tc: Optional[dict], dev, wide: bool, who: str):
    """One state dict in CLIPModel naming and the towers' config dicts -> (ClipVisionEngine, ClipTextEngine); tc None: no text tower."""
    for c, prefixes, name in ((tc, TEXT_PREFIXES, "text"), (vc, VISION_PREFIXES, "image")):            # both refusals before either engine is built
        if c is not None and (not any(k.startswith(prefixes[0]) for k in sd) or prefixes[1] + "weight" not in sd):
            raise KeyError(f"{who}: the state dict has no {name} tower ({prefixes[0]}* and {prefixes[1]}weight, CLIPModel naming)")

    def engine(cls, c, prefixes, **kw):
        return cls(_sub(sd, prefixes), dev, heads=int(c["num_attention_heads"]), eps=float(c.get("layer_norm_eps", 1e-5)),
                   hidden_act=c.get("hidden_act", "quick_gelu"), **kw)

    vision = engine(ClipVisionEngine, vc, VISION_PREFIXES, image_size=int(vc["image_size"]), wide=wide)
    text = None if tc is None else engine(ClipTextEngine, tc, TEXT_PREFIXES)
    if text is not None and text.proj.shape[0] != vision.pdim:
        raise ValueError(f"{who}: text projection {text.proj.shape[0]} and image projection {vision.pdim} differ")
    return vision, text


def as_nchw(images) -> torch.Tensor:
    """The pipeline's output_type="np" array [N, H, W, 3] (values in [0, 1]) or a float NCHW tensor [N, 3, H, W] -> float32 NCHW tensor."""
    if isinstance(images, torch.Tensor):
        if images.dim() != 4 or images.shape[1] != 3 or not images.is_floating_point():
            raise ValueError(f"ClipScorer: an image tensor must be float [N,3,H,W], got {images.dtype} {tuple(images.shape)}")
        return images.detach().float()
    arr = torch.as_tensor(images)
    if arr.dim() != 4 or arr.shape[3] != 3 or not arr.is_floating_point():
        raise ValueError(f"ClipScorer: an image array must be float [N,H,W,3], got {arr.dtype} {tuple(arr.shape)}")
    return arr.float().permute(0, 3, 1, 2).contiguous()


class ClipScorer:
    def __init__(self, vision_state_dict: SD, vision_config, text_state_dict: Optional[SD] = None, text_config=None, device="cuda",
                 in_scale: float = 1.0, in_shift: float = 0.0, crop: str = "torchvision"):
        """in_scale / in_shift map the caller's float pixel values onto [0, 1] (defaults: they already are; (0.5, 0.5) for [-1, 1] tensors);
        crop is the centre-crop rule for 8-bit frames (ops.clip_u8_geometry; calc_CLIP_*.py use the `clip` package: "torchvision")."""
        if crop not in ops.CLIP_CROPS:
            raise ValueError(f"ClipScorer: crop must be one of {ops.CLIP_CROPS}, got {crop!r}")
        self.crop = crop
        vc = _cfg(vision_config, VISION_KEYS, "ClipScorer(vision_config)")
        check_clip_dims("ClipScorer (image tower)", int(vc["hidden_size"]), int(vc["num_attention_heads"]), clip_grid_tokens(vc, "ClipScorer")[2])
        tc, sd = None, _sub(vision_state_dict, VISION_PREFIXES)
        if text_state_dict is not None:
            if text_config is None:
                raise ValueError("ClipScorer: text_state_dict needs text_config")
            tc = _cfg(text_config, TEXT_KEYS, "ClipScorer(text_config)")
            check_clip_dims("ClipScorer (text tower)", int(tc["hidden_size"]), int(tc["num_attention_heads"]),
                            int(tc.get("max_position_embeddings", 77)))
            sd.update(_sub(text_state_dict, TEXT_PREFIXES))
        self.dev = torch.device(device)
        self.in_scale, self.in_shift = float(in_scale), float(in_shift)
        self.vision, self.text = build_clip_towers(sd, vc, tc, self.dev, False, "ClipScorer")

    def image_features(self, images) -> torch.Tensor:
        """Projected image embeddings, fp32 [N, projection_dim] on the device (not normalised).  images: float frames ([N,H,W,3] array in
        [0, 1] or NCHW tensor), or 8-bit frames (module docstring)."""
        if is_uint8_images(images):
            return self.vision(images, crop=self.crop)[0]
        return self.vision(as_nchw(images), self.in_scale, self.in_shift)[0]

    def text_features(self, input_ids: torch.Tensor) -> torch.Tensor:
        """Projected text embeddings of tokenised prompts [N, T], fp32 [N, projection_dim] on the device (not normalised)."""
        if self.text is None:
            raise RuntimeError("ClipScorer: built without a text tower (pass text_state_dict and text_config)")
        return self.text.project(self.text(input_ids)[1])

    @staticmethod
    def cosine(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        if a.shape != b.shape:
            raise ValueError(f"ClipScorer: {tuple(a.shape)} and {tuple(b.shape)} do not pair up")
        return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))

    def clip_i(self, images, gt_images) -> torch.Tensor:
        """Cosine similarity of each image with its ground-truth image, fp32 [N]."""
        return self.cosine(self.image_features(images), self.image_features(gt_images))

    def clip_t(self, images, input_ids: torch.Tensor) -> torch.Tensor:
        """Cosine similarity of each image with its tokenised prompt, fp32 [N]."""
        return self.cosine(self.image_features(images), self.text_features(input_ids))
