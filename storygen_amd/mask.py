"""Human and text masks on the HIP kernels: what the reference's data_process/yolov7/human_ocr_mask.py computes between the detector's
output and the mask file — the step whose files training reads back through load_masks.

    imgsz = check_img_size(640, s=stride)
    h1, w1 = letterbox_shape(h0, w0, imgsz, stride)               # what LoadImages hands the detector for an h0 x w0 frame
    pred = model(img)[0]                                           # the caller's detector, [B, A, 5 + nc] on the device
    m = HumanTextMasker().mask(pred, (h1, w1), [(h0, w0)], [reader.readtext(path)])[0]
    if m.removed: os.remove(path)
    else: cv2.imwrite(mask_path, m.mask.cpu().numpy())

The script runs non_max_suppression (confidence filter, best class, class filter, torchvision's greedy NMS on class-offset boxes, the
first 300), takes the boxes to the frame with scale_coords and .round(), paints them into a mask, deletes the frame when the person
boxes cover more than a fifth of it, and otherwise adds EasyOCR's text boxes and writes mask * 255.  Here that is ops.det_select,
ops.det_nms and one ops.box_mask per frame, all on the device, and one readback of the counts at the end.  The arithmetic is fp32, the
script's CPU path; its CUDA path runs the same steps in fp16 and is not reproduced.  Equal scores keep anchor order.

Listing files, LoadImages, the detector, EasyOCR, JPEG encoding and deleting stay with the caller.  There is no CPU path."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import ops

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def check_img_size(img_size: int, s: int = 32) -> int:
    """utils/general.py:check_img_size: img_size rounded up to a multiple of the stride."""
    return math.ceil(img_size / int(s)) * int(s)


def letterbox_shape(h0: int, w0: int, img_size: int = 640, stride: int = 32) -> tuple:
    """(h1, w1) of utils/datasets.py:letterbox(auto=True) on an h0 x w0 frame: the frame scaled by r = min(img_size / h0, img_size / w0)
    and rounded, plus the padding np.mod(img_size - side, stride) split into int(round(d / 2 - 0.1)) and int(round(d / 2 + 0.1))."""
    if h0 < 1 or w0 < 1 or img_size < 1 or stride < 1:
        raise ValueError(f"letterbox_shape: sizes must be positive, got {(h0, w0, img_size, stride)}")
    r = min(img_size / h0, img_size / w0)
    uw, uh = int(round(w0 * r)), int(round(h0 * r))
    dw, dh = np.mod(img_size - uw, stride) / 2, np.mod(img_size - uh, stride) / 2
    return (uh + int(round(dh - 0.1)) + int(round(dh + 0.1)), uw + int(round(dw - 0.1)) + int(round(dw + 0.1)))


def scale_geometry(input_shape: Sequence[int], frame_shape: Sequence[int]) -> tuple:
    """(pad_x, pad_y, gain) of utils/general.py:scale_coords in Python doubles, as the script computes them."""
    (h1, w1), (h0, w0) = input_shape, frame_shape
    gain = min(h1 / h0, w1 / w0)
    return (w1 - w0 * gain) / 2, (h1 - h0 * gain) / 2, gain


def text_rectangles(entries) -> np.ndarray:
    """int32 [T, 4] (x1, y1, x2, y2) of one frame's text boxes: an EasyOCR result (entry[0] = four points) gives int() of points 0 and 2,
    as human_ocr_mask.py:64-65 reads it; a plain (x1, y1, x2, y2) is taken as it is.  Values beyond int32 are clamped to it, which no
    slice of a frame tells apart."""
    rows = []
    for e in entries:
        first = e[0]
        if isinstance(first, (list, tuple, np.ndarray)):
            c = first
            r = (int(c[0][0]), int(c[0][1]), int(c[2][0]), int(c[2][1]))
        elif len(e) == 4:
            r = tuple(int(v) for v in e)
        else:
            raise ValueError(f"text_rectangles: an entry is an EasyOCR result or (x1, y1, x2, y2), got {e!r}")
        rows.append([min(max(v, I32_MIN), I32_MAX) for v in r])
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


class HumanTextMask(NamedTuple):
    mask: Optional[torch.Tensor]                   # uint8 [h0, w0, 3] of 0 / 255 on the device; None for a removed frame
    detections: torch.Tensor                       # fp32 [n, 6] on the device: rounded x1 y1 x2 y2 in the frame, conf, cls
    human_ratio: float                             # the script's np.sum(mask) / mask.size before the text boxes
    removed: bool                                  # human_ratio > mask_ratio_thres: the script deletes the frame and writes no mask


class HumanTextMasker:
    def __init__(self, conf_thres: float = 0.5, iou_thres: float = 0.6, mask_ratio_thres: float = 0.2, classes=(0,), agnostic: bool = False,
                 max_det: int = 300, max_nms: int = 30000):
        """The defaults are the script's argparse defaults and non_max_suppression's constants; classes=(0,) is its `--classes 0`, person
        only; classes=None or () keeps every class."""
        self.conf_thres, self.iou_thres, self.mask_ratio_thres = float(conf_thres), float(iou_thres), float(mask_ratio_thres)
        if any(v != v for v in (self.conf_thres, self.iou_thres, self.mask_ratio_thres)):
            raise ValueError("HumanTextMasker: a threshold is NaN")
        self.classes = () if classes is None else tuple(int(c) for c in ((classes,) if isinstance(classes, int) else classes))
        if any(c < 0 for c in self.classes):
            raise ValueError(f"HumanTextMasker: classes {self.classes} hold a negative id")
        self.agnostic, self.max_det, self.max_nms = bool(agnostic), int(max_det), int(max_nms)
        ops.check_det_sides("HumanTextMasker", 1, 1, 1, self.max_nms, self.max_det)

    def mask(self, pred: torch.Tensor, input_shape: Sequence[int], frame_shapes: Sequence[Sequence[int]], text_boxes=None) -> List[HumanTextMask]:
        """pred: what `model(img)[0]` returns, fp32 or fp16 [B, A, 5 + nc] on the device; input_shape: (h1, w1) of the detector's input;
        frame_shapes: (h0, w0) per image; text_boxes: per image a list of EasyOCR results or (x1, y1, x2, y2) rectangles (None: no text)."""
        if not isinstance(pred, torch.Tensor) or pred.dim() != 3:
            raise ValueError(f"HumanTextMasker: pred must be a [B, A, 5 + nc] tensor, got {tuple(pred.shape) if isinstance(pred, torch.Tensor) else type(pred).__name__}")
        B = pred.shape[0]
        h1, w1 = (int(v) for v in input_shape)
        frames = [(int(h), int(w)) for h, w in frame_shapes]
        if len(frames) != B or h1 < 1 or w1 < 1:
            raise ValueError(f"HumanTextMasker: {B} images, {len(frames)} frame shapes, input shape {(h1, w1)}")
        for h0, w0 in frames:
            ops.check_mask_frame("HumanTextMasker", h0, w0)
        texts = [np.zeros((0, 4), np.int32)] * B if text_boxes is None else [text_rectangles(t or ()) for t in text_boxes]
        if len(texts) != B or any(len(t) > ops.MASK_MAX_TEXT for t in texts):
            raise ValueError(f"HumanTextMasker: {len(texts)} text lists for {B} images, or one beyond {ops.MASK_MAX_TEXT} rectangles")
        ops.check_det_sides("HumanTextMasker", B, pred.shape[1], pred.shape[2] - 5, self.max_nms, self.max_det)
        dev = pred.device
        # both uploads before the first launch; gain and pad rounded to fp32 are what torch's in-place ops with a Python scalar use
        geom = torch.tensor([[*scale_geometry((h1, w1), f)[:2], scale_geometry((h1, w1), f)[2], f[1], f[0]] for f in frames],
                            dtype=torch.float64).to(torch.float32).to(dev)
        starts = np.cumsum([0] + [len(t) for t in texts])
        text_dev = torch.from_numpy(np.concatenate(texts, 0)).to(dev) if starts[-1] else None
        cand, ncand = ops.det_select(pred, self.conf_thres, self.classes, self.max_nms)
        det, count = ops.det_nms(cand, ncand, geom, self.iou_thres, self.agnostic, self.max_det)
        covered = torch.empty(B, dtype=torch.int32, device=dev)
        masks = []
        for b, (h0, w0) in enumerate(frames):
            t = text_dev[starts[b]:starts[b + 1]] if starts[b + 1] > starts[b] else None
            masks.append(ops.box_mask(h0, w0, det[b], count[b:b + 1], t, covered=covered[b:b + 1])[0])
        host = torch.stack((count, covered)).cpu().tolist()            # the call's one synchronisation
        out = []
        for b, (h0, w0) in enumerate(frames):
            ratio = 3 * host[1][b] / (3 * h0 * w0)
            removed = ratio > self.mask_ratio_thres
            out.append(HumanTextMask(None if removed else masks[b], det[b, :host[0][b]], ratio, removed))
        return out
