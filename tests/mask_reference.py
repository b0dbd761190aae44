"""TEST INFRASTRUCTURE — the chain of data_process/yolov7/human_ocr_mask.py from the detector's output to the mask bytes, restated in fp32 on
the CPU with NumPy scalars and torch-CPU in-place ops: the filter and best-class pick of non_max_suppression, torchvision's greedy NMS as
the literal double loop, scale_coords + round through torch's own `-=`, `/=`, `clamp_`, `round`, and the painter as literal NumPy slicing.
torchvision and cv2 are not installed where the tests run: the NMS loop and the `mask * 255` cast are restated, not pinned; the rescale IS
torch's arithmetic.  Defined here where the script leaves it open: equal scores keep anchor order (a stable sort), a NaN coordinate
becomes 0 after the clamp."""
import numpy as np
import torch

F = np.float32
MAX_WH = F(4096.0)


def select(pred, conf_thres=0.5, classes=(), max_nms=30000):
    """pred [A, 5 + nc] of one image (any float dtype; converted to fp32 first) -> fp32 [n, 6] x1 y1 x2 y2 conf cls, n <= max_nms."""
    x = np.asarray(pred).astype(F)
    nc = x.shape[1] - 5
    thr = F(conf_thres)
    rows = []
    with np.errstate(all="ignore"):
        for a in range(x.shape[0]):
            obj = x[a, 4]
            if not obj > thr:
                continue
            if nc == 1:
                conf, cls = obj, 0
            else:
                confs = x[a, 5:] * obj                            # fp32 products, one rounding each
                if np.isnan(confs).any():
                    continue                                      # torch.max returns the NaN, which fails `> conf_thres`
                cls = int(np.argmax(confs))                       # the first maximum
                conf = confs[cls]
            if not conf > thr:
                continue
            if len(classes) and cls not in classes:
                continue
            hw, hh = x[a, 2] / F(2), x[a, 3] / F(2)
            rows.append([x[a, 0] - hw, x[a, 1] - hh, x[a, 0] + hw, x[a, 1] + hh, conf, F(cls)])
    out = np.asarray(rows, dtype=F).reshape(-1, 6)
    order = np.argsort(-out[:, 4], kind="stable")                 # score descending, equal scores in anchor order
    return out[order[:max_nms]]


def _max(a, b):                                                    # std::max / std::min as torchvision's CPU kernel calls them
    return b if a < b else a


def _min(a, b):
    return b if b < a else a


def nms(cand, iou_thres=0.6, agnostic=False, max_det=300):
    """cand fp32 [n, 6] in score order -> indices of the kept rows, at most max_det (torchvision.ops.nms's greedy loop on box + cls * 4096)."""
    n = cand.shape[0]
    thr = F(iou_thres)
    with np.errstate(all="ignore"):
        off = np.zeros(n, F) if agnostic else cand[:, 5] * MAX_WH
        x1, y1, x2, y2 = (cand[:, k] + off if not agnostic else cand[:, k] for k in range(4))
        areas = (x2 - x1) * (y2 - y1)
        removed = np.zeros(n, bool)
        keep = []
        for i in range(n):
            if removed[i]:
                continue
            keep.append(i)
            if len(keep) == max_det:
                break
            for j in range(i + 1, n):
                if removed[j]:
                    continue
                xx1, yy1 = _max(x1[i], x1[j]), _max(y1[i], y1[j])
                xx2, yy2 = _min(x2[i], x2[j]), _min(y2[i], y2[j])
                w, h = _max(F(0), xx2 - xx1), _max(F(0), yy2 - yy1)
                inter = w * h
                if inter / ((areas[i] + areas[j]) - inter) > thr:
                    removed[j] = True
    return np.asarray(keep, dtype=np.int64)


def scale_geometry(input_shape, frame_shape):
    """scale_coords' gain and pad, Python doubles."""
    (h1, w1), (h0, w0) = input_shape, frame_shape
    gain = min(h1 / h0, w1 / w0)
    return (w1 - w0 * gain) / 2, (h1 - h0 * gain) / 2, gain


def rescale(boxes, input_shape, frame_shape):
    """scale_coords(...).round() on fp32 [n, 4] with torch's own in-place ops on the CPU; a NaN becomes 0."""
    pad_x, pad_y, gain = scale_geometry(input_shape, frame_shape)
    c = torch.from_numpy(np.array(boxes, dtype=F).reshape(-1, 4)).clone()
    c[:, [0, 2]] -= pad_x
    c[:, [1, 3]] -= pad_y
    c[:, :4] /= gain
    c = torch.nan_to_num(c, nan=0.0, posinf=float("inf"), neginf=float("-inf"))
    c[:, 0].clamp_(0, frame_shape[1])
    c[:, 1].clamp_(0, frame_shape[0])
    c[:, 2].clamp_(0, frame_shape[1])
    c[:, 3].clamp_(0, frame_shape[0])
    return c.round().numpy()


def detect(pred, input_shape, frame_shape, conf_thres=0.5, iou_thres=0.6, classes=(), agnostic=False, max_det=300, max_nms=30000):
    """One image: pred [A, 5 + nc] -> (candidates fp32 [n, 6], det fp32 [k, 6] with the boxes in the frame)."""
    cand = select(pred, conf_thres, classes, max_nms)
    keep = nms(cand, iou_thres, agnostic, max_det)
    det = cand[keep].copy()
    if len(det):
        det[:, :4] = rescale(det[:, :4], input_shape, frame_shape)
    return cand, det


def paint(h0, w0, det=None, text=None):
    """-> (uint8 [h0, w0, 3] of 0 / 255, number of pixels under the det rectangles): human_ocr_mask.py:41-70 with NumPy's own slicing."""
    mask = np.zeros((h0, w0, 3))
    for row in (det if det is not None else ()):
        c1, c2 = (int(row[0]), int(row[1])), (int(row[2]), int(row[3]))
        mask[c1[1]:c2[1], c1[0]:c2[0]] = 1
    covered = int(np.sum(mask)) // 3
    for x1, y1, x2, y2 in (text if text is not None else ()):
        mask[int(y1):int(y2), int(x1):int(x2), :] = 1
    return np.clip(np.rint(mask * 255), 0, 255).astype(np.uint8), covered


def human_text_mask(pred, input_shape, frame_shape, text=None, conf_thres=0.5, iou_thres=0.6, mask_ratio_thres=0.2, classes=(0,),
                    agnostic=False, max_det=300, max_nms=30000):
    """One image as the script treats it -> (mask or None, det, ratio, removed)."""
    _, det = detect(pred, input_shape, frame_shape, conf_thres, iou_thres, classes, agnostic, max_det, max_nms)
    h0, w0 = frame_shape
    person = np.zeros((h0, w0, 3))
    for row in det:
        person[int(row[1]):int(row[3]), int(row[0]):int(row[2])] = 1
    ratio = np.sum(person) / (person.shape[0] * person.shape[1] * person.shape[2])
    removed = bool(ratio > mask_ratio_thres)
    mask, _ = paint(h0, w0, det, text)
    return (None if removed else mask), det, float(ratio), removed
