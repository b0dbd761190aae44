"""PickScore of generated frames on the HIP kernels: what the reference's evaluation/calc_Pickscore.py computes with transformers'
CLIPModel (yuvalkirstain/PickScore_v1, a fine-tuned CLIP ViT-H/14), and what inference_COCO_val.py:23-40,143-148 uses inside the
generation loop to keep the best of ten samples per prompt.

    scorer = PickScorer(model.state_dict(), model.config, device="cuda")
    frames = pipe(..., output_type="np").images                       # [N, H, W, 3] in [0, 1]
    ids = tokenizer(prompt, padding=True, truncation=True, max_length=77, return_tensors="pt").input_ids
    scorer.scores(ids, frames)[0]                                     # calc_Pickscore.py:21
    index, probs = scorer.best_of(ids, frames)                        # inference_COCO_val.py:146-147

Weights are ONE state dict in transformers CLIPModel naming (vision_model.*, visual_projection.weight, text_model.*,
text_projection.weight, logit_scale); the tokenizer is the caller's.  The image tower is ClipVisionEngine(wide=True): sg_attn_enc_f16
(257 tokens, 16 heads of 80) and the zero-padded patch rows of sg_clip_patchify_padk_f16 (patch size 14: 588 -> 592 columns).  The text
tower (77 tokens, 16 heads of 64, gelu) is the unchanged ClipTextEngine.

Preprocessing.  The reference's scripts score decoded JPEG / PIL images through transformers' CLIPImageProcessor for this checkpoint
(laion/CLIP-ViT-H-14-laion2B-s32B-b79K): Pillow's 8-bit bicubic shortest-edge resize, a 224 x 224 centre crop at (size - 224) // 2, rescale,
mean and std of the `clip` package.  8-bit frames (a uint8 [N,h,w,3] array or tensor, a list of PIL RGB images or uint8 arrays, sizes may
differ) get exactly that in one kernel (sg_clip_patchify_u8, `crop` = "floor"): the pixel_values are the processor's, bit for bit.  Float
frames are not quantised on the way; they keep the path of clip_score.py (antialiased float bicubic, torchvision's crop offset), which
differs from the processor's by up to about one 8-bit level per pixel.  There is no CPU path."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import ops
from .clip_score import TEXT_KEYS, VISION_KEYS, _cfg, as_nchw, build_clip_towers, clip_grid_tokens
from .encoders import check_clip_dims, check_clip_dims_wide, is_uint8_images

SD = Dict[str, torch.Tensor]


def split_config(config, who: str = "PickScorer") -> Tuple[dict, dict]:
    """A transformers CLIPConfig, or a dict with `vision_config` and `text_config` (dicts or config objects) -> (vision dict, text dict)."""
    cfg = config.to_dict() if hasattr(config, "to_dict") else dict(config)
    if "vision_config" not in cfg or "text_config" not in cfg:
        raise KeyError(f"{who}: config needs vision_config and text_config")
    vc = _cfg(cfg["vision_config"], VISION_KEYS, f"{who}(vision_config)")
    tc = _cfg(cfg["text_config"], TEXT_KEYS, f"{who}(text_config)")
    return vc, tc


def check_pick_config(vc: dict, tc: dict, who: str = "PickScorer") -> None:
    """Refuses on the host what the kernels cannot run (sg_attn_enc_f16 for the image tower, sg_attn_small_f16 for the text tower)."""
    _, ps, tokens = clip_grid_tokens(vc, who)
    check_clip_dims_wide(f"{who} (image tower)", int(vc["hidden_size"]), int(vc["num_attention_heads"]), tokens)
    if (3 * ps * ps) % 4:
        raise ValueError(f"{who}: 3 * patch_size^2 = {3 * ps * ps} must be a multiple of 4")
    check_clip_dims(f"{who} (text tower)", int(tc["hidden_size"]), int(tc["num_attention_heads"]), int(tc.get("max_position_embeddings", 77)))
    for c, n in ((vc, "vision"), (tc, "text")):
        if c.get("hidden_act", "quick_gelu") not in ("quick_gelu", "gelu"):
            raise ValueError(f"{who}: unsupported {n} hidden_act {c.get('hidden_act')!r}")


class PickScorer:
    def __init__(self, state_dict: SD, config, device="cuda", in_scale: float = 1.0, in_shift: float = 0.0, crop: str = "floor"):
        """in_scale / in_shift map the caller's float pixel values onto [0, 1] (defaults: they already are; (0.5, 0.5) for [-1, 1] tensors);
        crop is the centre-crop rule for 8-bit frames (ops.clip_u8_geometry; transformers' processor, which the scripts use: "floor")."""
        if crop not in ops.CLIP_CROPS:
            raise ValueError(f"PickScorer: crop must be one of {ops.CLIP_CROPS}, got {crop!r}")
        self.crop = crop
        vc, tc = split_config(config)
        check_pick_config(vc, tc)
        if "logit_scale" not in state_dict:
            raise KeyError("PickScorer: the state dict has no logit_scale (CLIPModel naming)")
        self.dev = torch.device(device)
        self.in_scale, self.in_shift = float(in_scale), float(in_shift)
        self.logit_scale = state_dict["logit_scale"].detach().to(self.dev, torch.float32).reshape(())
        self.vision, self.text = build_clip_towers(state_dict, vc, tc, self.dev, True, "PickScorer")

    def image_features(self, images) -> torch.Tensor:
        """Projected image embeddings, fp32 [N, projection_dim] on the device (not normalised).  images: the pipeline's output_type="np" frames
        [N, H, W, 3] or a float NCHW tensor, or 8-bit frames (module docstring)."""
        if is_uint8_images(images):
            return self.vision(images, crop=self.crop)[0]
        return self.vision(as_nchw(images), self.in_scale, self.in_shift)[0]

    def pixel_features(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """The same for already preprocessed pixel_values [N, 3, S, S] (what a CLIPImageProcessor returns)."""
        return self.vision.encode_pixels(pixel_values)[0]

    def text_features(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Projected text embeddings of tokenised prompts [P, T], fp32 [P, projection_dim] on the device (not normalised)."""
        return self.text.project(self.text(input_ids, attention_mask)[1])

    def _scores(self, t: torch.Tensor, i: torch.Tensor) -> torch.Tensor:
        t = t / t.norm(dim=-1, keepdim=True)
        i = i / i.norm(dim=-1, keepdim=True)
        return self.logit_scale.exp() * (t @ i.t())

    def scores(self, input_ids: torch.Tensor, images, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """exp(logit_scale) * cosine of every prompt with every image, fp32 [P, N] (calc_Pickscore.py:21 is row 0 with one image)."""
        return self._scores(self.text_features(input_ids, attention_mask), self.image_features(images))

    def probs(self, input_ids: torch.Tensor, images, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """softmax of the scores over the images, per prompt, fp32 [P, N] (inference_COCO_val.py:38)."""
        return torch.softmax(self.scores(input_ids, images, attention_mask), dim=-1)

    def best_of(self, input_ids: torch.Tensor, images, attention_mask: Optional[torch.Tensor] = None) -> Tuple[int, torch.Tensor]:
        """One prompt, N candidate images -> (index of the most probable image, probs fp32 [N]) (inference_COCO_val.py:146-147)."""
        if input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError(f"PickScorer.best_of: one prompt [1, T] at a time, got {tuple(input_ids.shape)}")
        p = self.probs(input_ids, images, attention_mask)[0]
        return int(p.argmax()), p
