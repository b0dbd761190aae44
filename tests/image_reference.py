"""TEST INFRASTRUCTURE: Pillow's `Image.resize(size)` (its default bicubic filter on 8-bit images: Resample.c, two passes in fixed point
with a rounding to uint8 in between) followed by ToTensor and the pipeline's cast to fp16, restated in NumPy one rounding per line, and
the host chain it restates.  tests/test_image_host.py pins the restatement to Pillow byte for byte; the GPU tests compare
sg_image_resize_u8 with the restatement, so the GPU box needs no Pillow."""
import numpy as np
import torch

PRECISION_BITS = 22          # 32 - 8 - 2: coefficients are fixed point with 22 fractional bits
A = -0.5                     # the bicubic's free parameter

# W x H -> w x h: upscale, downscale, mixed, one axis or both untouched, 1 x 1 sources, the largest admitted ratio (32) on either axis
GEOMETRIES = [((7, 5), (16, 16)), ((5, 7), (16, 16)), ((33, 17), (16, 24)), ((16, 16), (16, 16)), ((16, 40), (16, 16)), ((40, 16), (16, 16)),
              ((100, 75), (16, 16)), ((1, 1), (8, 8)), ((2, 3), (9, 4)), ((129, 67), (16, 8)), ((500, 375), (64, 64)), ((17, 16), (16, 16)),
              ((15, 16), (16, 16)), ((256, 3), (8, 8)), ((3, 256), (8, 8))]
CONTENTS = ("random", "extremes")


def geometry_id(g):
    return "%dx%d-%dx%d" % (g[0] + g[1])


def content(kind: str, h: int, w: int, c: int, seed: int = 0, n: int = None) -> np.ndarray:
    """uint8 [h,w,c] ([n,h,w,c] with n): "random" bytes, or "extremes", 0 and 255 only — the filter's negative lobes then overshoot on both
    sides, so accumulators go below 0 (arithmetic shift of a negative value) and above 255 << 22, in both passes."""
    rng = np.random.default_rng(1000003 * seed + 7919 * h + 31 * w + c)
    shape = (h, w, c) if n is None else (n, h, w, c)
    if kind == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (rng.integers(0, 2, shape, dtype=np.uint8) * 255).astype(np.uint8)


def bicubic(x: float) -> float:
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * A
    return 0.0


def ksize(n_in: int, n_out: int) -> int:
    scale = n_in / n_out
    support = 2.0 * max(scale, 1.0)
    return 2 * int(np.ceil(support)) + 1


def table(n_in: int, n_out: int):
    """(coefficients int32 [n_out, ksize], bounds int32 [n_out, 2] = (first input sample, number of taps)) of one axis; Python floats are
    C doubles and every operation below is one C operation of precompute_coeffs / normalize_coeffs_8bpc."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ks = ksize(n_in, n_out)
    coef, bounds = np.zeros((n_out, ks), np.int32), np.zeros((n_out, 2), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [bicubic((x + xmin - center + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            coef[xx, x] = int(v * (1 << PRECISION_BITS) + (-0.5 if v < 0 else 0.5))          # int(): C truncation
        bounds[xx] = (xmin, n)
    return coef, bounds


def _pass_last_axis(a: np.ndarray, n_out: int) -> np.ndarray:
    """One pass along the last axis of a uint8 array: int32 accumulation from 2^21, arithmetic shift, clip, uint8."""
    coef, bounds = table(a.shape[-1], n_out)
    out = np.empty(a.shape[:-1] + (n_out,), np.uint8)
    wide = a.astype(np.int64)
    for xx in range(n_out):
        xmin, n = bounds[xx]
        ss = (1 << (PRECISION_BITS - 1)) + (wide[..., xmin:xmin + n] * coef[xx, :n].astype(np.int64)).sum(-1)
        assert np.abs(ss).max() < 2 ** 31                                                    # the int32 of the C code never wraps
        out[..., xx] = np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize_reference(a: np.ndarray, size) -> np.ndarray:
    """a uint8 [..., h, w, c] -> uint8 [..., size[1], size[0], c] (size = (width, height) as Pillow's): horizontal pass into uint8, then
    the vertical pass on that; a pass that would not change its axis is skipped; channels are independent."""
    assert a.dtype == np.uint8 and a.ndim >= 3
    w_out, h_out = size
    if a.shape[-2] != w_out:
        a = np.moveaxis(_pass_last_axis(np.moveaxis(a, -2, -1), w_out), -1, -2)
    if a.shape[-3] != h_out:
        a = np.moveaxis(_pass_last_axis(np.moveaxis(a, -3, -1), h_out), -1, -3)
    return np.ascontiguousarray(a)


def to_tensor_f16(u8: np.ndarray) -> np.ndarray:
    """uint8 [..., h, w, c] -> fp16 [..., c, h, w]: ToTensor's fp32 u8 / 255, then the pipeline's cast to fp16."""
    f = (u8.astype(np.float32) / np.float32(255)).astype(np.float16)
    return np.ascontiguousarray(np.moveaxis(f, -1, -3))


def ingest_reference(a: np.ndarray, size, flip: bool = False):
    """(uint8 [..., H, W, c], fp16 [..., c, H, W]) as sg_image_resize_u8 documents them; flip mirrors the columns after the resize."""
    u8 = resize_reference(a, size)
    if flip:
        u8 = np.ascontiguousarray(u8[..., ::-1, :])
    return u8, to_tensor_f16(u8)


def host_chain(a: np.ndarray, size) -> torch.Tensor:
    """The chain the kernel replaces (inference.py:84-89, dataset.py:37-43), on one uint8 [h,w,3] or [h,w] / [h,w,1] array:
    ToTensor(Image.fromarray(a).resize(size)) — fp32 [c,H,W] in [0, 1] — cast to fp16 as the pipeline does."""
    from PIL import Image
    im = Image.fromarray(a[..., 0] if a.ndim == 3 and a.shape[-1] == 1 else a)
    r = np.asarray(im.resize(tuple(size)))
    r = r[..., None] if r.ndim == 2 else r
    return (torch.from_numpy(r.copy()).permute(2, 0, 1).float() / 255).half()


def pillow_resize(a: np.ndarray, size) -> np.ndarray:
    """Pillow itself on one uint8 [h,w,c] array (c = 1: mode L) -> uint8 [H,W,c]."""
    from PIL import Image
    im = Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a)
    r = np.asarray(im.resize(tuple(size)))
    return r[..., None] if r.ndim == 2 else r
