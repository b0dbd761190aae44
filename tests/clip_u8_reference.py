"""TEST INFRASTRUCTURE — what the reference's evaluation scripts feed their CLIP towers, restated on the CPU: PIL's
`Image.resize((Wr, Hr), Image.BICUBIC)` of an 8-bit RGB frame, the centre crop, ToTensor + Normalize in fp32 NumPy (one rounding per
operation), and the patch rows of the patch GEMM.  tests/test_clip_u8_host.py pins it to transformers' PIL image processor (crop "floor");
the GPU tests compare sg_clip_patchify_u8 and everything above it with it bit for bit.  Nothing in the product imports this file."""
import numpy as np
import torch

from tests.clip_vision_reference import CLIP_MEAN, CLIP_STD

CROPS = ("torchvision", "floor")


def geometry(h: int, w: int, S: int, crop: str):
    """(Hr, Wr, top, left): the shorter side becomes S, the longer int(S * long / short) (torchvision's Resize(S) and transformers'
    shortest_edge alike); the offset is int(round((size - S) / 2.0)) — Python's round, halves to even — for torchvision's CenterCrop and
    (size - S) // 2 for transformers' center_crop."""
    assert crop in CROPS
    short, long_ = (w, h) if w <= h else (h, w)
    new_long = int(S * long_ / short)
    Hr, Wr = (new_long, S) if w <= h else (S, new_long)
    if crop == "torchvision":
        return Hr, Wr, int(round((Hr - S) / 2.0)), int(round((Wr - S) / 2.0))
    return Hr, Wr, (Hr - S) // 2, (Wr - S) // 2


def content(kind: str, h: int, w: int, seed: int = 0, n: int = None) -> np.ndarray:
    """uint8 [h,w,3] ([n,h,w,3] with n): "random" bytes; "checker", 0 / 255 cells of 3 x 3 pixels (phase per channel and image), under which
    Pillow's clip acts at both ends in both passes; "white", constant 255; "ramp", every byte value in every channel (needs h * w >= 256)."""
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    if kind == "random":
        return np.random.default_rng(7919 * seed + 31 * h + w).integers(0, 256, shape, dtype=np.uint8)
    if kind == "white":
        return np.full(shape, 255, np.uint8)
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    if kind == "checker":
        one = lambda s: ((((y + s + c) // 3 + (x + 2 * c) // 3) % 2) * 255).astype(np.uint8)      # noqa: E731
    else:
        assert kind == "ramp" and h * w >= 256
        one = lambda s: ((y * w + x + 85 * c + 7 * s) % 256).astype(np.uint8)                     # noqa: E731
    return one(seed) if n is None else np.stack([one(seed + i) for i in range(n)])


def resize_crop(a: np.ndarray, geom, S: int) -> np.ndarray:
    """One uint8 [h,w,3] frame -> uint8 [S,S,3]: Pillow's resize to Wr x Hr, then the window at (top, left)."""
    from PIL import Image
    Hr, Wr, top, left = geom
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and 0 <= top <= Hr - S and 0 <= left <= Wr - S
    r = np.asarray(Image.fromarray(a).resize((Wr, Hr), Image.BICUBIC))
    return np.ascontiguousarray(r[top:top + S, left:left + S])


def normalise(u8: np.ndarray, mean=CLIP_MEAN, std=CLIP_STD) -> np.ndarray:
    """uint8 [..., S, S, 3] -> fp32 [..., 3, S, S]: ToTensor's u8 / 255, then (v - mean) / std, each rounded to fp32 on its own."""
    v = u8.astype(np.float32) / np.float32(255)
    v = (v - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    assert v.dtype == np.float32
    return np.ascontiguousarray(np.moveaxis(v, -1, -3))


def patch_rows(pixels: np.ndarray, ps: int, kpad: int = None) -> np.ndarray:
    """fp32 [N,3,S,S] -> fp16 [N * (S/ps)^2, kpad]: row-major patches, columns (c, dy, dx), zeros in [3 ps^2, kpad)."""
    N, C, S, _ = pixels.shape
    G, K = S // ps, 3 * ps * ps
    kpad = (K + 7) & ~7 if kpad is None else kpad
    rows = np.zeros((N * G * G, kpad), np.float16)
    rows[:, :K] = pixels.reshape(N, C, G, ps, G, ps).transpose(0, 2, 4, 1, 3, 5).reshape(N * G * G, K).astype(np.float16)
    return rows


def preprocess(frames, S: int, crop: str = "torchvision", geom=None, mean=CLIP_MEAN, std=CLIP_STD):
    """frames: uint8 [N,h,w,3] or a list of uint8 [h,w,3] arrays of any sizes -> (uint8 [N,S,S,3], pixel_values fp32 [N,3,S,S])."""
    u8 = np.stack([resize_crop(a, geom or geometry(a.shape[0], a.shape[1], S, crop), S) for a in frames])
    return u8, normalise(u8, mean, std)


def reference(frames, S: int, ps: int, crop: str = "torchvision", geom=None, kpad: int = None, mean=CLIP_MEAN, std=CLIP_STD):
    """(uint8 [N,S,S,3], fp16 [N * P, kpad]): both outputs of sg_clip_patchify_u8."""
    u8, px = preprocess(frames, S, crop, geom, mean, std)
    return u8, patch_rows(px, ps, kpad)


def pixel_values(frames, S: int, crop: str) -> torch.Tensor:
    """The reference scripts' pixel_values as a tensor, fp32 [N,3,S,S] (what engine.encode_pixels takes)."""
    return torch.from_numpy(preprocess(frames, S, crop)[1])
