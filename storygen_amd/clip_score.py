"""CLIP-I / CLIP-T scoring of generated frames on the HIP kernels: what the reference's evaluation/calc_CLIP_image.py and
evaluation/calc_CLIP_text.py compute with the `clip` package's ViT-B/32 (image-to-image and image-to-text cosine similarity of the
projected, L2-normalised features; the scripts print the mean over pairs).

    scorer = ClipScorer(vision_sd, vision_cfg, text_sd, text_cfg, device="cuda")
    frames = pipe(..., output_type="np").images                       # [N, H, W, 3] in [0, 1]
    scorer.clip_i(frames, gt_frames).mean(), scorer.clip_t(frames, tokenizer(prompts, ...).input_ids).mean()

Weights are state dicts in transformers naming (CLIPVisionModelWithProjection / CLIPTextModelWithProjection, or one CLIPModel state
dict passed for both); the tokenizer is the caller's.  Images go through sg_clip_patchify_f16 — the `clip` package's resize (antialiased
bicubic on the float image), centre crop and normalisation — and ClipVisionEngine; texts through ClipTextEngine and its projection.
Models outside sg_attn_small_f16 (more than 128 tokens, head dim above 64: ViT-H/14) are refused on the host; PickScore's ViT-H/14 runs in
storygen_amd/pick_score.py.  There is no CPU path."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .encoders import ClipTextEngine, ClipVisionEngine, check_clip_dims

SD = Dict[str, torch.Tensor]
VISION_KEYS = ("hidden_size", "num_attention_heads", "image_size", "patch_size")
TEXT_KEYS = ("hidden_size", "num_attention_heads")


def _cfg(config, keys, who: str) -> dict:
    cfg = config.to_dict() if hasattr(config, "to_dict") else dict(config)
    missing = [k for k in keys if k not in cfg]
    if missing:
        raise KeyError(f"{who}: config lacks {missing}")
    return cfg


def _sub(sd: SD, prefixes) -> SD:
    return {k: v for k, v in sd.items() if k.startswith(prefixes)}


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
                 in_scale: float = 1.0, in_shift: float = 0.0):
        """in_scale / in_shift map the caller's pixel values onto [0, 1] (defaults: they already are; (0.5, 0.5) for [-1, 1] tensors)."""
        vc = _cfg(vision_config, VISION_KEYS, "ClipScorer(vision_config)")
        S, ps = int(vc["image_size"]), int(vc["patch_size"])
        if S <= 0 or ps <= 0 or S % ps:
            raise ValueError(f"ClipScorer: image_size {S} is not a multiple of patch_size {ps}")
        check_clip_dims("ClipScorer (image tower)", int(vc["hidden_size"]), int(vc["num_attention_heads"]), (S // ps) ** 2 + 1)
        tc = None
        if text_state_dict is not None:
            if text_config is None:
                raise ValueError("ClipScorer: text_state_dict needs text_config")
            tc = _cfg(text_config, TEXT_KEYS, "ClipScorer(text_config)")
            check_clip_dims("ClipScorer (text tower)", int(tc["hidden_size"]), int(tc["num_attention_heads"]),
                            int(tc.get("max_position_embeddings", 77)))
            if "text_projection.weight" not in text_state_dict:
                raise KeyError("ClipScorer: text_state_dict has no text_projection.weight (CLIPTextModelWithProjection / CLIPModel naming)")
        self.dev = torch.device(device)
        self.in_scale, self.in_shift = float(in_scale), float(in_shift)
        self.vision = ClipVisionEngine(_sub(vision_state_dict, ("vision_model.", "visual_projection.")), self.dev,
                                       heads=int(vc["num_attention_heads"]), eps=float(vc.get("layer_norm_eps", 1e-5)),
                                       hidden_act=vc.get("hidden_act", "quick_gelu"), image_size=S)
        self.text = None
        if tc is not None:
            self.text = ClipTextEngine(_sub(text_state_dict, ("text_model.", "text_projection.")), self.dev, heads=int(tc["num_attention_heads"]),
                                       eps=float(tc.get("layer_norm_eps", 1e-5)), hidden_act=tc.get("hidden_act", "quick_gelu"))

    def image_features(self, images) -> torch.Tensor:
        """Projected image embeddings, fp32 [N, projection_dim] on the device (not normalised)."""
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
