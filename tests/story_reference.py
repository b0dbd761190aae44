"""TEST INFRASTRUCTURE: the frame hand-off of story generation (sg_frame_handoff_f16) restated in NumPy, one rounding per line, and the
host round trip it replaces.  tests/test_story_host.py pins the restatement to the pipeline's own decode_latents / numpy_to_pil followed
by the reload of the saved image (inference.py:86-92) on every fp16 bit pattern."""
import numpy as np
import torch

NAN_PATTERNS = 2046          # fp16 bit patterns that are NaN: exponent 31 and a non-zero mantissa, either sign (2 * 1023)


def all_fp16_patterns() -> torch.Tensor:
    """Every fp16 bit pattern once, in bit order: fp16 [65536]."""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.float16).copy())


def as_image(values: torch.Tensor):
    """A flat fp16 vector zero-padded to the smallest square [1,3,S,S] image that holds it -> (image, number of values)."""
    n = values.numel()
    S = int(np.ceil(np.sqrt(n / 3.0)))
    flat = torch.zeros(3 * S * S, dtype=torch.float16)
    flat[:n] = values
    return flat.view(1, 3, S, S), n


def handoff_reference(x: torch.Tensor):
    """x fp16 [N,3,H,W] (the decoder's output) -> (uint8 [N,H,W,3], fp16 [N,3,H,W]) as the kernel documents them; NaN -> 0 in both."""
    assert x.dtype == torch.float16 and x.dim() == 4 and x.shape[1] == 3
    h = x.detach().cpu().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        t = (h.astype(np.float32) * np.float32(0.5)).astype(np.float16)              # image / 2      in fp16
        s = (t.astype(np.float32) + np.float32(0.5)).astype(np.float16)              # + 0.5          in fp16
        c = np.where(np.isnan(s), np.float16(0), np.clip(s, np.float16(0), np.float16(1)))   # .clamp(0, 1); NaN -> 0 (documented)
        f = c.astype(np.float32) * np.float32(255)                                   # .float() ... * 255 in fp32
        u8 = np.rint(f).astype(np.uint8)                                             # .round() half to even, .astype("uint8")
        y = (u8.astype(np.float32) / np.float32(255)).astype(np.float16)             # ToTensor: fp32 / 255; the pipeline's cast to fp16
    return torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))), torch.from_numpy(y)


def host_round_trip(pil_images) -> torch.Tensor:
    """What inference.py:86-92 makes of saved images (no resize: they have the size already): float32 [K,3,H,W] in [0, 1] — the `* 2 - 1`
    of :90-91 is not applied (it rebinds the loop variable)."""
    return torch.stack([(torch.from_numpy(np.asarray(im.convert("RGB")).copy()) / 255).permute(2, 0, 1) for im in pil_images]).float()
