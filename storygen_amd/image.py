"""Reference images and masks from raw 8-bit images of any size, on the device: what the reference builds on the host for every frame
it conditions on (inference.py:84-89: `ToTensor(Image.open(p).convert('RGB').resize((512, 512)))`) and for every training image, mask
and reference frame (dataset.py:37-43: `.resize((512, 512))`, `ToTensor`, `RandomHorizontalFlip`).

    frames = load_reference_images([Image.open(p).convert("RGB") for p in paths], size=(512, 512), device="cuda")     # fp16 [K,3,512,512]
    pipeline(..., image_prompt=frames[None], ...)

Pillow's resize on 8-bit images is a two-pass fixed-point bicubic that rounds to uint8 between the passes; ops.image_resize
(sg_image_resize_u8) restates it bit for bit and applies ToTensor and the pipeline's cast to fp16 in the same launch, so the tensor is the
one the host chain gives, whatever the size of the source.  Resampling any other way (F.interpolate, torchvision on tensors) gives
different context frames than the reference's script.

Stays with the caller: reading the files and `.convert(...)`."""
from __future__ import annotations

from typing import Sequence, Union

import numpy as np
import torch

from . import ops


def _as_u8(image, channels: int, what: str) -> torch.Tensor:
    """One image -> uint8 [h,w,C] tensor (C = 1 or `channels`), wherever it lives."""
    if hasattr(image, "mode") and hasattr(image, "size") and not isinstance(image, (np.ndarray, torch.Tensor)):       # a PIL image
        if image.mode not in ("RGB", "L") or (channels == 1 and image.mode != "L"):
            want = "RGB" if channels == 3 else "L"
            raise ValueError(f"{what}: PIL image in mode {image.mode!r}; pass image.convert({want!r}) (conversion stays with the caller)")
        image = np.array(image)
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise ValueError(f"{what}: arrays must be uint8, got {image.dtype}")
        image = torch.from_numpy(np.ascontiguousarray(image))
    if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8:
        raise ValueError(f"{what}: expected a PIL image, a uint8 array or a uint8 tensor, got {type(image).__name__}"
                         + (f" of {image.dtype}" if isinstance(image, torch.Tensor) else ""))
    if image.dim() == 2:
        image = image[..., None]
    if image.dim() != 3 or image.shape[2] not in (1, channels) or image.shape[0] == 0 or image.shape[1] == 0:
        raise ValueError(f"{what}: images are [h,w,{channels}]" + (" or [h,w]" if channels == 1 else " (or [h,w] / [h,w,1] grey)")
                         + f", got {tuple(image.shape)}")
    return image


def _load(images, size, device, channels: int, flip, what: str) -> torch.Tensor:
    if isinstance(images, torch.Tensor) and images.dim() == 4:
        images = list(images)
    if not isinstance(images, (list, tuple)) or len(images) == 0:
        raise ValueError(f"{what}: expected a non-empty list of images or a uint8 [K,h,w,{channels}] tensor")
    W, H = (int(s) for s in size)
    flips = [bool(f) for f in flip] if isinstance(flip, (list, tuple)) else [bool(flip)] * len(images)
    if len(flips) != len(images):
        raise ValueError(f"{what}: {len(flips)} flip flags for {len(images)} images")
    device = torch.device("cuda" if device is None else device)
    groups = {}                                          # images of one size, channel count and flip share a launch
    for i, im in enumerate(images):
        t = _as_u8(im, channels, what)
        groups.setdefault((tuple(t.shape), flips[i]), []).append((i, t))
    out = None
    for (_, flipped), members in groups.items():
        batch = torch.stack([t for _, t in members]).to(device)
        _, f16 = ops.image_resize(batch, (W, H), flip=flipped, out_u8=False)
        if f16.shape[1] != channels:                     # grey -> RGB replicates the channel (Pillow's convert('RGB') of an L image);
            f16 = f16.expand(-1, channels, -1, -1)       # channels are resampled independently, so before or after the resize is the same
        if len(members) == len(images):
            return f16.contiguous()
        if out is None:
            out = torch.empty(len(images), channels, H, W, dtype=torch.float16, device=device)
        out[torch.tensor([i for i, _ in members], device=device)] = f16
    return out


Images = Union[Sequence, torch.Tensor]


def load_reference_images(images: Images, size=(512, 512), device=None, flip=False) -> torch.Tensor:
    """images: a list of PIL images in mode RGB (or L: replicated to three channels, as convert('RGB') does), uint8 arrays or tensors
    [h,w,3], or one uint8 [K,h,w,3] tensor; their sizes may differ.  -> fp16 [K,3,H,W] in [0, 1] on `device`, size = (W, H) as Pillow's:
    exactly ToTensor(image.resize(size)) cast to fp16 — `[None]` of it is the pipeline's `image_prompt`.  flip (one flag, or one per
    image) mirrors the columns after the resize.  Any other PIL mode raises ValueError."""
    return _load(images, size, device, 3, flip, "load_reference_images")


def load_masks(images: Images, size=(512, 512), device=None, flip=False) -> torch.Tensor:
    """The same for one-channel images (PIL mode L, uint8 [h,w] or [h,w,1]): fp16 [K,1,H,W] in [0, 1], ToTensor(mask.resize(size)) of
    dataset.py:39,42."""
    return _load(images, size, device, 1, flip, "load_masks")
