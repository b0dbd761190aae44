"""Removing near-duplicate keyframes on the HIP kernels: what the reference's data_process/dup_remove.py computes with DINO ViT-B/8 on
torch — the step between extract.py and align.py (storygen_amd.align) in its data pipeline.

    names = [n for n in numeric_order(os.listdir(folder)) if is_keyframe_file(n)]
    frames = [Image.open(os.path.join(folder, n)).convert("RGB") for n in names]
    d = KeyframeDeduper(dino.state_dict(), device="cuda").dedup(frames)
    for n, gone in zip(names, d.drop):
        if gone: os.remove(os.path.join(folder, n))

The script walks a folder in numerical order and deletes the PREVIOUS keyframe whenever the current one's class feature has cosine
similarity >= 0.75 with it; the feature it compares with advances whether or not that file was deleted, so every pair is decided on its
own and the last frame always stays.  Here the features are DinoVitEngine's (8-bit frames preprocessed as the script's transform does
it), and similarity and decision are one launch (ops.adjacent_cosine = sg_adjacent_cosine_f64); only `sim` and `drop` reach the host.

The script compares a float32 cosine's `.item()`; here the cosine and the comparison are float64 on the fp32 features.
Listing, opening, decoding, converting (`.convert('RGB')`) and deleting files stay with the caller; a non-RGB frame is refused where
the script fails the whole video.  There is no CPU path."""
from __future__ import annotations

import itertools
import os
from typing import Dict, List, NamedTuple, Sequence

import numpy as np
import torch

from . import ops
from .dino import DinoVitEngine
from .encoders import is_uint8_images

SD = Dict[str, torch.Tensor]


def numeric_key(name: str) -> tuple:
    """dup_remove.py:27's `fns`: the name cut into (non-digits, number) pairs after an 'a' is put in front and a '0' behind, so that digit
    runs compare as numbers (`..._0-0-9-500.jpg` before `..._0-0-10-0.jpg`; the appended 0 multiplies a trailing number by ten)."""
    runs = ("".join(g) for _, g in itertools.groupby("a" + name + "0", key=str.isdecimal))      # text, digits, text, digits, ...
    return tuple(int(r) if k % 2 else r for k, r in enumerate(runs))


def numeric_order(names: Sequence[str]) -> List[str]:
    """The names in the order the script visits them: sorted by numeric_key, numerical rather than alphabetic."""
    return sorted(names, key=numeric_key)


def is_keyframe_file(name: str) -> bool:
    """dup_remove.py:34: only files whose extension is exactly `.jpg` are keyframes; everything else in the folder is passed over."""
    return os.path.splitext(os.path.basename(name))[1] == ".jpg"


class Dedup(NamedTuple):
    keep: np.ndarray                               # bool [N]: ~drop
    drop: np.ndarray                               # bool [N]: the files the script deletes
    similarity: np.ndarray                         # float64 [N]: frame i against frame i - 1; [0] = 0


def _decide(feats: torch.Tensor, threshold: float) -> Dedup:
    sim, drop = ops.adjacent_cosine(feats, threshold=threshold)
    drop_h = drop.cpu().numpy().astype(bool)       # (synchronises; sim follows as one more small copy)
    return Dedup(~drop_h, drop_h, sim.cpu().numpy())


def dedup_features(feats: torch.Tensor, threshold: float = 0.75) -> Dedup:
    """The script's decisions on features in hand: fp32 [N, dim] on the device, frames in the script's order."""
    if not isinstance(feats, torch.Tensor) or feats.dim() != 2:
        raise ValueError(f"dedup_features: features must be a [N, dim] tensor, got {tuple(feats.shape) if isinstance(feats, torch.Tensor) else type(feats).__name__}")
    ops.check_dedup_sides("dedup_features", feats.shape[0], feats.shape[1])
    return _decide(feats, threshold)


class KeyframeDeduper:
    def __init__(self, dino_state_dict: SD, device="cuda", threshold: float = 0.75, heads: int = 12):
        """dino_state_dict: DINO's VisionTransformer.state_dict() (dino_vitb8: 785 tokens, 12 heads of 64), or anything else within
        DinoVitEngine's limits.  threshold: the script's 0.75."""
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("KeyframeDeduper: threshold is NaN")
        self.dev = torch.device(device)
        self.threshold = threshold
        self.engine = DinoVitEngine(dino_state_dict, self.dev, heads=heads)

    def features(self, frames, batch: int = 16) -> torch.Tensor:
        """8-bit frames (a uint8 [N,h,w,3] array or tensor, a list of PIL RGB images or uint8 arrays, sizes may differ) -> fp32 [N, dim]."""
        if not is_uint8_images(frames):
            raise TypeError("KeyframeDeduper: frames are 8-bit (PIL RGB images or uint8 arrays), as the script reads them from disk")
        return self.engine(frames, batch=batch)

    def dedup(self, frames, batch: int = 16) -> Dedup:
        """frames in the script's order (numeric_order of the folder's .jpg files) -> which of them it deletes."""
        if not is_uint8_images(frames):
            raise TypeError("KeyframeDeduper: frames are 8-bit (PIL RGB images or uint8 arrays), as the script reads them from disk")
        ops.check_dedup_sides("KeyframeDeduper", len(frames), self.engine.C)       # refused before the tower runs
        return _decide(self.features(frames, batch), self.threshold)
