"""Image ingest on the GPU: sg_image_resize_u8 (ops.image_resize) against the NumPy restatement of Pillow's resize + ToTensor that
tests/test_image_host.py pins to Pillow byte for byte — every comparison is exact, on the uint8 bytes and on the fp16 bit patterns — at
its geometry, tile, stride, window and alignment edges, and end to end: a story started from raw images of two sizes and a pipeline call
on load_reference_images' tensor give what the host chain's tensor gives, bit for bit (the tiny pipeline of tests/test_story_gpu.py)."""
import numpy as np
import pytest
import torch

from test_story_gpu import PROMPTS, SIZE, _pipeline, rig  # noqa: F401  (rig: that module's fixture, built once for this one too)
from tests import image_reference as IR

pytestmark = pytest.mark.gpu
F16, I16 = torch.float16, torch.int16


def _check(gpu, a, size, flip=False, what=""):
    """a uint8 [N,h,w,C] on the host -> both outputs of one launch equal the restatement."""
    from storygen_amd import ops
    u8, y = ops.image_resize(torch.from_numpy(a).to(gpu), size, flip=flip)
    want_u8, want_y = IR.ingest_reference(a, size, flip)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == want_u8.shape and y.dtype == F16 and tuple(y.shape) == want_y.shape
    bad = int((u8.cpu().numpy() != want_u8).sum()), int((y.cpu().view(I16).numpy() != want_y.view(np.int16)).sum())
    assert bad == (0, 0), f"{what} {a.shape} -> {size}: {bad[0]} uint8 and {bad[1]} fp16 mismatches of {want_u8.size}"
    return want_u8


@pytest.mark.parametrize("geometry", IR.GEOMETRIES, ids=IR.geometry_id)
def test_every_geometry_channel_count_and_content(gpu, geometry):
    """Upscale, downscale, mixed, one pass or both skipped (16x16 -> 16x16 is a copy), 1x1 sources (every tap clipped on both sides) and
    the largest admitted ratio on either axis (256x3, 3x256 -> 8x8); C = 3 and C = 1; random bytes and 0 / 255 only (overshoot on both
    sides: negative accumulators under the arithmetic shift, clip at 255)."""
    (W, H), size = geometry
    for c in (3, 1):
        for kind in IR.CONTENTS:
            out = _check(gpu, IR.content(kind, H, W, c)[None], size, what=f"C{c} {kind}")
            if (W, H) == tuple(size):
                assert np.array_equal(out[0], IR.content(kind, H, W, c))


def test_tile_edges_in_width(gpu):
    """Output widths at SG_IMAGE_TILE_W - 1, exactly, + 1 (and the same around two tiles), upscaled and downscaled, both channel counts."""
    from storygen_amd import ops
    T = ops.IMAGE_TILE_W
    for w_in in (50, 3 * T + 7):
        for w_out in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
            for c in (3, 1):
                _check(gpu, IR.content("random", 9, w_in, c, seed=w_out)[None], (w_out, 5), what="width")
                _check(gpu, IR.content("extremes", 5, w_in, c, seed=w_out)[None], (w_out, 5), what="width, rows untouched")


# (Hin / Hout ratio, C) -> rows per tile: the LDS image of a tile is (rows its taps read) x 64 x C bytes <= 64 KiB, i.e. 341 rows at C = 3
# and 1024 at C = 1; 16 output rows read at most 19 ratio + 2 input rows, so C = 3 leaves 16 rows per tile at ratio 17 and not at 18.
TILE_ROWS = [(0.5, 3, 16), (1, 3, 16), (5, 3, 16), (17, 3, 16), (18, 3, 15), (24, 3, 11), (32, 3, 7), (32, 1, 16)]


@pytest.mark.parametrize("ratio,c,rows", TILE_ROWS, ids=lambda v: str(v))
def test_tile_edges_in_height(gpu, ratio, c, rows):
    """Output heights at the rows per tile - 1, exactly, + 1 and the same around two tiles (and one past three), for every rows-per-tile
    value on either side of the ratio at which the host changes it.  A source short enough to fit the LDS budget whole keeps 16 rows per
    tile whatever the ratio (the small heights at the large ratios); from two tiles on the sources here are taller than that."""
    from storygen_amd import ops
    for h_out in sorted({max(rows - 1, 1), rows, rows + 1, 2 * rows - 1, 2 * rows, 2 * rows + 1, 3 * rows + 1}):
        h_in = max(1, int(h_out * ratio))
        th = ops.image_resize_tile_rows(h_in, h_out, c)
        assert th == rows or (th == ops.IMAGE_TILE_H and h_out < 2 * rows - 1 and h_in * ops.IMAGE_TILE_W * c <= ops.IMAGE_LDS_BYTES), (h_in, h_out, th)
        for w_in in (20, 11):                                   # both passes (staged through LDS) | vertical pass alone (from global memory)
            _check(gpu, IR.content("random" if w_in == 20 else "extremes", h_in, w_in, c, seed=h_out)[None], (11, h_out), what="height")


@pytest.mark.parametrize("offset", [0, 1, 3], ids=lambda o: f"byte{o}")
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("geometry", [((7, 5), (16, 16)), ((100, 75), (16, 16)), ((16, 40), (16, 16)), ((40, 16), (16, 16)), ((16, 16), (16, 16)),
                                      ((70, 9), (67, 19))], ids=IR.geometry_id)
def test_windows_batches_flip_and_unaligned_bases(gpu, geometry, flip, offset):
    """N = 3.  Input = a window (batch and row stride) of a larger buffer; both outputs = windows of buffers pre-filled with a bit pattern,
    whose other elements must stay as they were; all three buffers start `offset` bytes (fp16: elements) past an aligned address.  Then
    each output alone, into fresh windows."""
    from storygen_amd import ops
    (W, H), (w, h) = geometry
    N, c = 3, 3 if offset != 1 else 1
    a = IR.content("random", H, W, c, seed=offset, n=N)
    want_u8, want_y = IR.ingest_reference(a, (w, h), flip)
    Wb, wb = W + 5, w + 4

    def buffers():
        xflat = torch.full((offset + N * (H + 2) * Wb * c,), 0xA5, dtype=torch.uint8, device=gpu)
        xbuf = xflat[offset:].view(N, H + 2, Wb, c)
        xbuf[:, 1:1 + H, 2:2 + W] = torch.from_numpy(a).to(gpu)
        uflat = (torch.arange(offset + N * (h + 2) * wb * c, device=gpu) * 7 % 251).to(torch.uint8)
        yflat = (torch.arange(offset + N * c * (h + 2) * wb, device=gpu) % 2039 - 1000).to(I16).view(F16)
        return xbuf[:, 1:1 + H, 2:2 + W], uflat, yflat, uflat[offset:].view(N, h + 2, wb, c), yflat[offset:].view(N, c, h + 2, wb)
    for outputs in ("both", "u8", "f16"):
        xin, uflat, yflat, ubuf, ybuf = buffers()
        u0, y0 = uflat.clone(), yflat.clone()
        uout, yout = ubuf[:, 1:1 + h, 3:3 + w], ybuf[:, :, 1:1 + h, 3:3 + w]
        assert not xin.is_contiguous()
        got = ops.image_resize(xin, (w, h), flip=flip, out_u8=uout if outputs != "f16" else False, out_f16=yout if outputs != "u8" else False)
        assert (got[0] is uout) if outputs != "f16" else got[0] is None
        assert (got[1] is yout) if outputs != "u8" else got[1] is None
        if outputs != "f16":
            u0[offset:].view(N, h + 2, wb, c)[:, 1:1 + h, 3:3 + w] = torch.from_numpy(want_u8).to(gpu)
        if outputs != "u8":
            y0[offset:].view(N, c, h + 2, wb)[:, :, 1:1 + h, 3:3 + w] = torch.from_numpy(want_y).to(gpu)
        assert torch.equal(uflat, u0), f"{outputs}: uint8 window or its guard elements"
        assert torch.equal(yflat.view(I16), y0.view(I16)), f"{outputs}: fp16 window or its guard elements"


@pytest.mark.parametrize("geometry", [((500, 375), (512, 512)), ((2048, 1536), (512, 512))], ids=IR.geometry_id)
def test_real_geometries(gpu, geometry):
    (W, H), size = geometry
    _check(gpu, IR.content("random", H, W, 3)[None], size, what="real")


def test_ops_rejections(gpu):
    from storygen_amd import ops
    x = torch.zeros(1, 6, 10, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(TypeError):
        ops.image_resize(x.cpu(), (8, 4))
    with pytest.raises(TypeError):
        ops.image_resize(x.float(), (8, 4))
    with pytest.raises(TypeError):
        ops.image_resize(x, (8, 4), out_f16=torch.zeros(1, 3, 4, 8, device=gpu))
    with pytest.raises(ValueError, match=r"\[N,h,w,1\] or \[N,h,w,3\]"):
        ops.image_resize(x[..., :2], (8, 4))
    with pytest.raises(ValueError, match="out_u8 must be"):
        ops.image_resize(x, (8, 4), out_u8=torch.zeros(1, 8, 4, 3, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError, match="contiguous pixels"):
        ops.image_resize(x.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), (8, 4))
    with pytest.raises(ValueError, match="no output"):
        ops.image_resize(x, (8, 4), out_u8=False, out_f16=False)
    with pytest.raises(ValueError, match="positive"):
        ops.image_resize(x, (8, 0))
    with pytest.raises(RuntimeError, match="in / out <= 32"):
        ops.image_resize(torch.zeros(1, 6, 257, 3, dtype=torch.uint8, device=gpu), (8, 4))
    with pytest.raises(RuntimeError, match="overlaps the input"):
        ops.image_resize(x, (10, 6), out_u8=x, out_f16=False)


# ------------------------------------------------------------------------------------------------------ end to end
def _raw_frames():
    return [IR.content("random", 50, 70, 3, seed=5), IR.content("extremes", 90, 33, 3, seed=6)]        # 70 x 50 and 33 x 90


def _host_chain_tensor(arrays):
    """ToTensor(Image.fromarray(a).resize((SIZE, SIZE))) stacked: float32 [K,3,SIZE,SIZE] — through the restatement, which the CPU suite
    pins to Pillow, so that this box needs none."""
    return torch.stack([torch.from_numpy(IR.resize_reference(a, (SIZE, SIZE))).permute(2, 0, 1).float() / 255 for a in arrays])


def test_story_from_raw_first_frames_equals_the_host_chain(gpu, rig):  # noqa: F811
    from storygen_amd.story import StoryGenerator
    pipe = _pipeline(rig)
    raw, runs = _raw_frames(), []
    for first in (raw, _host_chain_tensor(raw)):
        torch.manual_seed(21)
        runs.append(StoryGenerator(pipe).generate(PROMPTS[3:5], context_frames=2, first_frames=first, first_prompts=PROMPTS[1:3],
                                                  num_inference_steps=3, height=SIZE, width=SIZE,
                                                  generator=torch.Generator(device=gpu).manual_seed(4), output_type="uint8").frames)
    diff = int((runs[0] != runs[1]).sum())
    print(f"story from raw first frames vs the host chain's tensor: {diff} of {runs[0].size} bytes differ; distinct byte values per frame "
          f"{[len(np.unique(f)) for f in runs[0]]}")
    assert runs[0].shape == (2, SIZE, SIZE, 3) and all(len(np.unique(f)) > 16 for f in runs[0]) and (runs[0][0] != runs[0][1]).any()
    assert diff == 0


def test_loader_output_as_image_prompt_gives_the_same_latents(gpu, rig):  # noqa: F811
    from storygen_amd.image import load_masks, load_reference_images
    pipe = _pipeline(rig)
    raw = _raw_frames()
    loaded, chain = load_reference_images(raw, size=(SIZE, SIZE), device=gpu), _host_chain_tensor(raw)
    assert loaded.dtype == F16 and loaded.device.type == "cuda" and tuple(loaded.shape) == (2, 3, SIZE, SIZE)
    assert torch.equal(loaded.cpu().view(I16), chain.half().view(I16))
    lat = []
    for frames in (loaded[None], chain[None]):
        torch.manual_seed(8)
        lat.append(pipe(stage="auto-regressive", prompt=PROMPTS[3], image_prompt=frames, prev_prompt=PROMPTS[1:3], height=SIZE, width=SIZE,
                        num_inference_steps=3, guidance_scale=7.0, image_guidance_scale=3.5,
                        generator=torch.Generator(device=gpu).manual_seed(2), output_type="latent").images)
    assert lat[0].float().abs().max() > 0 and torch.isfinite(lat[0].float()).all()
    assert torch.equal(lat[0], lat[1])
    # masks: one channel, mixed sizes, one flipped
    masks = [IR.content("extremes", 40, 24, 1, seed=1), IR.content("random", 24, 40, 1, seed=2)[..., 0]]
    got = load_masks(masks, size=(SIZE, SIZE), device=gpu, flip=[False, True])
    want = [IR.ingest_reference(masks[0], (SIZE, SIZE))[1], IR.ingest_reference(masks[1][..., None], (SIZE, SIZE), flip=True)[1]]
    assert tuple(got.shape) == (2, 1, SIZE, SIZE) and np.array_equal(got.cpu().view(I16).numpy(), np.stack(want).view(np.int16))
