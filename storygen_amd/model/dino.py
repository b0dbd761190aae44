"""Drop-in for the model data_process/dup_remove.py loads — `torch.hub.load('facebookresearch/dino:main', 'dino_vitb8')`, DINO's
VisionTransformer — as far as the script uses it:

  model.cuda()                      dup_remove.py:19
  model(image) -> [1, embed_dim]    dup_remove.py:37, on `transform(Image.open(p)).unsqueeze(0)`: [B, 3, 224, 224], already normalised

Weights keep DINO's names and shapes, so `load_state_dict(hub_model.state_dict())` adopts the checkpoint.  Inference only, like the other
encoder drop-ins (model/encoders.py); the forward is DinoVitEngine.encode_pixels and there is no CPU path.  Only the native token grid
runs (224 x 224 for dino_vitb8)."""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import torch

from ..clip_score import clip_grid_tokens
from ..dino import DinoVitEngine, dino_param_shapes
from ..encoders import check_clip_dims_wide, init_state
from .encoders import SD, _HipModule
from .unet_2d_condition import FrozenConfig

DINO_DEFAULTS = OrderedDict(img_size=224, patch_size=8, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, layer_norm_eps=1e-6)


class DinoVisionTransformer(_HipModule):
    def __init__(self, seed: int = 0, **config):
        unknown = [k for k in config if k not in DINO_DEFAULTS]
        if unknown:
            raise TypeError(f"DinoVisionTransformer: unknown config keys {unknown}")
        cfg = OrderedDict(DINO_DEFAULTS)
        cfg.update(config)
        S, ps, tokens = clip_grid_tokens(cfg, "DinoVisionTransformer", "img_size")
        if (3 * ps * ps) % 4:
            raise ValueError(f"DinoVisionTransformer: 3 * patch_size^2 = {3 * ps * ps} must be a multiple of 4")
        check_clip_dims_wide("DinoVisionTransformer", int(cfg["embed_dim"]), int(cfg["num_heads"]), tokens)
        self._config = FrozenConfig(cfg).freeze()
        self._shapes = dino_param_shapes(cfg["embed_dim"], cfg["depth"], ps, S, cfg["mlp_ratio"])
        # init_state's rules by name: `pos_embed` / `cls_token` are tables like DINO's trunc_normal_(std=.02) ones
        sd = init_state({k.replace("pos_embed", "pos_embedding").replace("cls_token", "cls_embedding"): v for k, v in self._shapes.items()}, seed)
        self._sd: SD = {k.replace("pos_embedding", "pos_embed").replace("cls_embedding", "cls_token"): v for k, v in sd.items()}

    @property
    def embed_dim(self) -> int:
        return self._config["embed_dim"]

    def load_state_dict(self, state_dict: SD, strict: bool = True):
        """DINO's VisionTransformer names; `head.*` entries (an Identity has none, a fine-tuned head may) are ignored."""
        self._adopt({k: v for k, v in state_dict.items() if not k.startswith("head.")}, self._shapes, strict)

    @classmethod
    def from_torch(cls, module, num_heads: Optional[int] = None) -> "DinoVisionTransformer":
        """Adopt a constructed DINO VisionTransformer (its `.state_dict()`; geometry from the weights, heads from the module or given)."""
        sd = {k: v for k, v in module.state_dict().items() if not k.startswith("head.")}
        wp, pos = sd["patch_embed.proj.weight"], sd["pos_embed"]
        depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        heads = num_heads if num_heads is not None else module.blocks[0].attn.num_heads
        grid = round((pos.shape[1] - 1) ** 0.5)
        model = cls(img_size=grid * wp.shape[2], patch_size=wp.shape[2], embed_dim=wp.shape[0], depth=depth, num_heads=heads,
                    mlp_ratio=sd["blocks.0.mlp.fc1.weight"].shape[0] / wp.shape[0])
        model.load_state_dict(sd)
        return model.to(wp.device, wp.dtype)

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device) if not isinstance(device, torch.device)
                       else device)

    def cpu(self):
        return self.to("cpu")

    def _eng(self) -> DinoVitEngine:
        if self._engine is None:
            if self.device.type != "cuda":
                raise RuntimeError("DinoVisionTransformer: move the model to the HIP device first (.cuda()); there is no CPU path")
            c = self._config
            self._engine = DinoVitEngine(self._sd, self.device, heads=c["num_heads"], eps=c["layer_norm_eps"], resize=c["img_size"])
        return self._engine

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, 3, img_size, img_size], already resized, cropped and normalised -> the class feature [B, embed_dim]."""
        S = self._config["img_size"]
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (3, S, S):
            got = tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__
            raise ValueError(f"DinoVisionTransformer: input must be [B,3,{S},{S}] (only the native token grid runs), got {got}")
        return self._eng().encode_pixels(x).to(self.dtype)

    __call__ = forward
