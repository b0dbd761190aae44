"""Aligning a story's frames with its narration on the HIP kernels: what the reference's data_process/align.py computes with the `clip`
package's ViT-B/16, NumPy and a Python double loop — the (frame, sentences) pairs StorySalonDataset trains on.

    aligner = FrameAligner(model.state_dict(), model.config, device="cuda")        # one CLIPModel, transformers naming
    ids = tokenizer(sentences, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    a = aligner.align(frames, ["0-0-12-480", ...], ids, ["0-0-10-0", ...], ocr_ids=[None, ocr_token_ids, ...])
    for frame, sentence_indices in a.groups: ...

Features (align.py:89-117): every sentence is its CLIP text feature; a frame on which OCR found text is the text feature of that text,
any other frame its CLIP image feature; all projected, none normalised.  The image tower is ClipVisionEngine(wide=True) (ViT-B/16: 197
tokens, 12 heads of 64, sg_attn_enc_f16) on 8-bit frames preprocessed as the `clip` package preprocesses them (sg_clip_patchify_u8,
crop "torchvision"); the text tower is ClipTextEngine and its projection.  Cost (ops.align_cost), recurrence and backtrace (ops.dtw_path)
run on the device; only the path and its length come back.

The script's model is fp16 and its cosine runs in fp16 NumPy; that arithmetic is not reproduced.  Here the features are the engines' fp32
outputs and cost and recurrence are float64.  The tokenizer, the 77-character cut of align.py:91-92,108-109, OCR and
punctuation restoration stay with the caller.  There is no CPU path."""
from __future__ import annotations

import re
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import ops
from .clip_score import build_clip_towers
from .encoders import is_uint8_images
from .pick_score import check_pick_config, split_config

SD = Dict[str, torch.Tensor]
_STAMP = re.compile(r"\d+-\d+-\d+-\d+")


def timestamp_seconds(stamp: str) -> float:
    """Seconds of an `H-M-S-ms` stamp as align.py's time_dist reads it (align.py:20,27-30): the script appends a "0" before parsing, so
    the last field counts tenths of a millisecond: h * 3600 + m * 60 + s are added as integers, then (10 * ms) * 0.0001 in float64."""
    if not isinstance(stamp, str) or not _STAMP.fullmatch(stamp):
        raise ValueError(f"timestamp_seconds: expected 'H-M-S-ms' with decimal fields, got {stamp!r}")
    h, m, s, ms = (int(v) for v in stamp.split("-"))
    return h * 3600 + m * 60 + s + (10 * ms) * 0.0001


def as_seconds(times, n: int, who: str) -> torch.Tensor:
    """n times, each float seconds or an `H-M-S-ms` string (or a float64 tensor / array of seconds) -> float64 [n] on the host."""
    if isinstance(times, torch.Tensor):
        t = times.detach().to("cpu", torch.float64).reshape(-1)
    elif hasattr(times, "dtype") and hasattr(times, "shape"):
        t = torch.as_tensor(times).to(torch.float64).reshape(-1)
    else:
        t = torch.tensor([timestamp_seconds(v) if isinstance(v, str) else float(v) for v in times], dtype=torch.float64)
    if t.numel() != n:
        raise ValueError(f"{who}: {t.numel()} times for {n} entries")
    return t


def group_path(path: Sequence[Tuple[int, int]]) -> List[Tuple[int, List[int]]]:
    """Consecutive path entries with one frame index -> (frame, its sentences in order): the lines align.py:166-176 writes."""
    groups: List[Tuple[int, List[int]]] = []
    for i, j in path:
        if not groups or groups[-1][0] != i:
            groups.append((int(i), []))
        groups[-1][1].append(int(j))
    return groups


class Alignment(NamedTuple):
    path: List[Tuple[int, int]]                    # (frame, sentence) from (0, 0) to (r - 1, c - 1)
    groups: List[Tuple[int, List[int]]]            # (frame, [sentences])
    cost: torch.Tensor                             # float64 [r, c], on the device


def _align(frame_feats: torch.Tensor, sent_feats: torch.Tensor, ft: torch.Tensor, st: torch.Tensor) -> Alignment:
    """Both launches on features and float64 host times that the caller has checked; the path and its length are all that comes back."""
    dev = frame_feats.device
    cost = ops.align_cost(frame_feats, sent_feats.contiguous(), ft.to(dev), st.to(dev))
    path, path_len, _ = ops.dtw_path(cost)
    host = path.cpu()                              # (synchronises; path_len follows as one more small copy)
    n = int(path_len.cpu())
    pairs = [(int(i), int(j)) for i, j in host[:n].tolist()]
    return Alignment(pairs, group_path(pairs), cost)


def align_features(frame_feats: torch.Tensor, sent_feats: torch.Tensor, frame_times, sent_times) -> Alignment:
    """The alignment of r frame features fp32 [r, dim] with c sentence features fp32 [c, dim] on the device; times as in as_seconds."""
    if frame_feats.dim() != 2 or sent_feats.dim() != 2:
        raise ValueError(f"align_features: features must be [r, dim] and [c, dim], got {tuple(frame_feats.shape)} and {tuple(sent_feats.shape)}")
    r, c = frame_feats.shape[0], sent_feats.shape[0]
    ft, st = as_seconds(frame_times, r, "align_features (frames)"), as_seconds(sent_times, c, "align_features (sentences)")
    ops.check_align_sides("align_features", r, c, dtw=True)
    return _align(frame_feats, sent_feats, ft, st)


class FrameAligner:
    def __init__(self, clip_model_state_dict: SD, clip_config, device="cuda"):
        """One CLIPModel state dict in transformers naming (vision_model.*, visual_projection.weight, text_model.*, text_projection.weight)
        and its CLIPConfig (or a dict with vision_config and text_config): ViT-B/16, or anything else within check_clip_dims_wide for the
        image tower and sg_attn_small_f16 for the text tower; quick_gelu or gelu per tower from the config."""
        vc, tc = split_config(clip_config, "FrameAligner")
        check_pick_config(vc, tc, "FrameAligner")
        self.dev = torch.device(device)
        self.crop = "torchvision"                  # the `clip` package's CenterCrop, as align.py:114 preprocesses
        self.vision, self.text = build_clip_towers(clip_model_state_dict, vc, tc, self.dev, True, "FrameAligner")

    def image_features(self, frames) -> torch.Tensor:
        """8-bit frames (a uint8 [N,h,w,3] array or tensor, a list of PIL RGB images or uint8 arrays, sizes may differ) -> fp32 [N, dim]."""
        if not is_uint8_images(frames):
            raise TypeError("FrameAligner: frames are 8-bit (PIL RGB images or uint8 arrays), as the script reads them from disk")
        return self.vision(frames, crop=self.crop)[0]

    def text_features(self, input_ids: torch.Tensor) -> torch.Tensor:
        """Token ids [P, T] -> fp32 [P, dim]: encode_text of the `clip` package (causal mask only, pooled at the largest id)."""
        return self.text.project(self.text(input_ids)[1])

    def frame_features(self, frames, ocr_ids: Optional[Sequence] = None) -> torch.Tensor:
        """The script's per-frame feature (align.py:101-117): the text feature of ocr_ids[i] where it is not None, else the image feature."""
        n = len(frames)
        ocr = [None] * n if ocr_ids is None else list(ocr_ids)
        if len(ocr) != n:
            raise ValueError(f"FrameAligner: {len(ocr)} ocr_ids entries for {n} frames")
        text_at = [i for i, o in enumerate(ocr) if o is not None]
        image_at = [i for i, o in enumerate(ocr) if o is None]
        rows = [torch.as_tensor(ocr[i]).reshape(-1) for i in text_at]
        if any(t.numel() != rows[0].numel() for t in rows):
            raise ValueError("FrameAligner: ocr_ids entries must be padded to one length")
        feats = torch.empty(n, self.vision.pdim, dtype=torch.float32, device=self.dev)
        if image_at:
            feats[torch.tensor(image_at, device=self.dev)] = self.image_features(frames if not text_at else [frames[i] for i in image_at])
        if text_at:
            feats[torch.tensor(text_at, device=self.dev)] = self.text_features(torch.stack(rows))
        return feats

    def align(self, frames, frame_times, sentence_ids: torch.Tensor, sentence_times, ocr_ids: Optional[Sequence] = None) -> Alignment:
        """frames: r 8-bit frames; sentence_ids: [c, T] token ids; times: float64 seconds or `H-M-S-ms` strings, one per frame / sentence."""
        sentence_ids = torch.as_tensor(sentence_ids)
        if sentence_ids.dim() != 2:
            raise ValueError(f"FrameAligner: sentence_ids must be [c, T], got {tuple(sentence_ids.shape)}")
        r, c = len(frames), sentence_ids.shape[0]
        ft, st = as_seconds(frame_times, r, "FrameAligner (frames)"), as_seconds(sentence_times, c, "FrameAligner (sentences)")
        ops.check_align_sides("FrameAligner", r, c, dtw=True)          # times and sizes are refused before the towers run
        return _align(self.frame_features(frames, ocr_ids), self.text_features(sentence_ids), ft, st)
