"""Image ingest on the host (no GPU): the NumPy restatement of Pillow's 8-bit bicubic resize pinned to Pillow byte for byte, the
library's host table builder against the restatement's tables, the host-side rejections of sg_image_resize_u8, and the argument
handling of load_reference_images / load_masks / StoryGenerator.generate(first_frames=<raw images>) on a recording stand-in of ops."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import image_reference as IR

PAIRS = sorted({(g[0][i], g[1][i]) for g in IR.GEOMETRIES for i in (0, 1)} | {(500, 512), (375, 512), (4000, 512), (16384, 512), (1, 512)})


# ------------------------------------------------------------------------------------------------- the restatement is Pillow
@pytest.mark.parametrize("kind", IR.CONTENTS)
@pytest.mark.parametrize("geometry", IR.GEOMETRIES, ids=IR.geometry_id)
def test_restatement_equals_pillow_bit_for_bit(geometry, kind):
    (W, H), size = geometry
    for c in (3, 1):                                                     # mode RGB and mode L
        a = IR.content(kind, H, W, c)
        got, want = IR.resize_reference(a, size), IR.pillow_resize(a, size)
        assert got.shape == want.shape == (size[1], size[0], c)
        assert int((got != want).sum()) == 0, (geometry, kind, c)
        u8, f16 = IR.ingest_reference(a, size)
        assert np.array_equal(u8, want) and torch.equal(torch.from_numpy(f16).view(torch.int16), IR.host_chain(a, size).view(torch.int16))


def test_extremes_overshoot_on_both_sides():
    """0 / 255 contents under an upscale: the filter's negative lobes push accumulators below 0 (where `>>` must be the arithmetic shift)
    and above 255 << 22, so both clips are exercised by the cases that use this content."""
    a = IR.content("extremes", 5, 7, 3).astype(np.int64)
    coef, bounds = IR.table(7, 16)
    ss = np.array([(1 << 21) + (a[:, b[0]:b[0] + b[1]] * k[:b[1], None]).sum(1) for k, b in zip(coef.astype(np.int64), bounds)])
    assert ss.min() < 0 and (ss.max() >> 22) > 255
    assert (ss.min() >> 22) < 0 and -((-ss.min()) >> 22) != (ss.min() >> 22)               # floor, not truncation


def test_flip_and_batch_of_the_restatement():
    a = IR.content("random", 9, 7, 3, n=2)
    u8, f16 = IR.ingest_reference(a, (5, 6), flip=True)
    for i in range(2):
        one = IR.pillow_resize(a[i], (5, 6))[:, ::-1]                    # RandomHorizontalFlip after the resize (dataset.py:37-43)
        assert np.array_equal(u8[i], one) and np.array_equal(f16[i], IR.to_tensor_f16(np.ascontiguousarray(one)))


# ------------------------------------------------------------------------------------------------- the library's host table builder
@pytest.fixture(scope="module")
def lib():
    from storygen_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_table_builder_equals_the_restatement(lib, pair):
    from storygen_amd import ops
    n_in, n_out = pair
    assert lib.sg_image_resample_ksize(n_in, n_out) == IR.ksize(n_in, n_out) <= ops.IMAGE_MAX_KSIZE
    coef, bounds = ops.image_resample_table(n_in, n_out)
    want_coef, want_bounds = IR.table(n_in, n_out)
    assert coef.dtype == torch.int32 and tuple(coef.shape) == want_coef.shape and tuple(bounds.shape) == (n_out, 2)
    assert np.array_equal(bounds.numpy(), want_bounds) and np.array_equal(coef.numpy(), want_coef)
    # what the kernel relies on: taps inside the input and the table row; int32 cannot wrap
    assert (want_bounds[:, 0] >= 0).all() and (want_bounds[:, 1] >= 1).all() and (want_bounds.sum(1) <= n_in).all()
    assert (want_bounds[:, 1] <= coef.shape[1]).all()
    assert int(np.abs(want_coef.astype(np.int64)).sum(1).max()) * 255 + 2 ** 21 < 2 ** 31


def test_limits_of_the_table_calls(lib):
    from storygen_amd import ops
    assert (ops.IMAGE_MAX_SIDE, ops.IMAGE_MAX_RATIO, ops.IMAGE_MAX_KSIZE) == (16384, 32, 129)
    assert lib.sg_image_resample_ksize(256, 8) == 129 == IR.ksize(256, 8)                  # ratio 32: the largest kernel
    assert lib.sg_image_resample_ksize(16384, 512) == 129
    assert lib.sg_image_resample_ksize(8, 8) == 5 and lib.sg_image_resample_ksize(1, 16384) == 5
    buf = (C.c_int32 * (8 * 131))()
    for n_in, n_out in ((257, 8), (33, 1), (16385, 16385), (8, 16385), (0, 8), (8, 0), (-1, 8)):
        assert lib.sg_image_resample_ksize(n_in, n_out) == -1 and b"in / out <= 32" in lib.sg_last_error(), (n_in, n_out)
        assert lib.sg_image_resample_table(n_in, n_out, buf, buf) == -1, (n_in, n_out)
    assert lib.sg_image_resample_table(8, 8, None, buf) == -1 and b"null" in lib.sg_last_error()
    with pytest.raises(RuntimeError, match="in / out <= 32"):
        ops.image_resample_table(257, 8)


def test_rows_per_tile_keep_the_staged_image_inside_the_lds_budget(lib):
    """The host picks the output rows per tile so that the horizontal pass's uint8 rows a tile needs fit SG_IMAGE_LDS_BYTES: checked with
    the real spans of the restatement's bounds for every tile, at ratios on both sides of the points where the row count changes."""
    from storygen_amd import ops
    seen = set()
    for n_out in (8, 19, 64):
        for ratio in (0.1, 1.0, 4.0, 7.3, 13.0, 14.0, 20.0, 21.3, 30.0, 32.0):
            n_in = max(1, int(n_out * ratio))
            _, bounds = IR.table(n_in, n_out)
            for c in (1, 3):
                th = ops.image_resize_tile_rows(n_in, n_out, c)
                seen.add(th)
                assert 1 <= th <= ops.IMAGE_TILE_H
                if n_in == n_out:
                    assert th == ops.IMAGE_TILE_H
                    continue
                for y0 in range(0, n_out, th):
                    b = bounds[y0:y0 + th]
                    rows = int((b[:, 0] + b[:, 1]).max() - b[:, 0].min())
                    assert rows * ops.IMAGE_TILE_W * c <= ops.IMAGE_LDS_BYTES, (n_in, n_out, c, th, rows)
    assert len(seen) > 3 and ops.IMAGE_TILE_H in seen
    assert lib.sg_image_resize_tile_rows(8, 8, 2) == -1 and lib.sg_image_resize_tile_rows(257, 8, 3) == -1


# ------------------------------------------------------------------------------------------------- the entry point's host checks
def test_image_resize_rejects_on_the_host(lib):
    """sg_image_resize_u8 validates before it launches: these return SG_EINVAL without a device (fake pointers)."""
    X, U, Y, T = 0x100000, 0x200000, 0x300000, 0x400000

    def call(x=X, u=U, y=Y, N=1, Hin=6, Win=10, Cc=3, H=4, W=8, sx=None, su=None, sy=None, h=(T, T + 0x1000), v=(T + 0x2000, T + 0x3000), flip=0):
        sx = sx or (Hin * Win * Cc, Win * Cc)
        su = su or (H * W * Cc, W * Cc)
        sy = sy or (Cc * H * W, H * W, W)
        return lib.sg_image_resize_u8(x, *sx, N, Hin, Win, Cc, u, *su, y, *sy, H, W, *h, *v, flip, None)
    none = (None, None)
    for kw, msg in ((dict(x=None), b"null input"), (dict(u=None, y=None), b"both outputs are null"), (dict(N=0), b"N = 0"), (dict(N=-1), b"N = -1"),
                    (dict(N=65536), b"N = 65536"), (dict(Hin=0), b"sizes must be positive"), (dict(Win=-3), b"sizes must be positive"),
                    (dict(H=0), b"sizes must be positive"), (dict(W=0), b"sizes must be positive"), (dict(Cc=2), b"C = 2"), (dict(Cc=4), b"C = 4"),
                    (dict(Cc=0), b"C = 0"), (dict(flip=2), b"flip = 2"),
                    (dict(Win=16385), b"above 16384"), (dict(H=16385), b"above 16384"),
                    (dict(Win=257), b"more than 32"), (dict(Hin=129), b"more than 32"),
                    (dict(sx=(180, 29)), b"input strides"), (dict(N=2, sx=(179, 30)), b"input strides"),
                    (dict(su=(96, 23)), b"uint8 output strides"), (dict(N=2, su=(95, 24)), b"uint8 output strides"),
                    (dict(sy=(96, 32, 7)), b"fp16 output strides"), (dict(sy=(96, 31, 8)), b"fp16 output strides"),
                    (dict(N=2, sy=(95, 32, 8)), b"fp16 output strides"),
                    (dict(u=Y + 10), b"outputs overlap"), (dict(y=U + 8), b"outputs overlap"), (dict(y=X), b"overlaps the input"),
                    (dict(u=X + 2), b"overlaps the input"), (dict(u=None, y=X + 100), b"overlaps the input"),
                    (dict(h=none), b"horizontal tables are missing"), (dict(h=(T, None)), b"horizontal tables are missing"),
                    (dict(v=none), b"vertical tables are missing"), (dict(v=(None, T)), b"vertical tables are missing"),
                    (dict(Win=8), b"horizontal tables are given"), (dict(Hin=4), b"vertical tables are given"),
                    (dict(Win=8, h=(None, T)), b"horizontal tables are given"), (dict(Hin=4, Win=8, h=none), b"vertical tables are given")):
        assert call(**kw) == -1, kw
        assert msg in lib.sg_last_error(), (kw, lib.sg_last_error())
    assert C.sizeof(C.c_void_p) == 8
    # ops refuses tensors that are not on the device, like every other op
    from storygen_amd import ops
    with pytest.raises(TypeError, match="CUDA/HIP uint8"):
        ops.image_resize(torch.zeros(1, 6, 10, 3, dtype=torch.uint8), (8, 4))


# ------------------------------------------------------------------------------------------------- loaders and StoryGenerator
class RecordingOps:
    """Stands in for storygen_amd.ops inside storygen_amd.image: records every launch and answers with the restatement."""

    def __init__(self):
        self.calls = []

    def image_resize(self, x_u8, size, flip=False, out_u8=None, out_f16=None):
        assert x_u8.dtype == torch.uint8 and x_u8.dim() == 4 and out_u8 is False and out_f16 is None
        self.calls.append((tuple(x_u8.shape), tuple(size), bool(flip)))
        _, f16 = IR.ingest_reference(x_u8.numpy(), size, flip)
        return None, torch.from_numpy(f16)


@pytest.fixture
def rec(monkeypatch):
    import storygen_amd.image as IM
    r = RecordingOps()
    monkeypatch.setattr(IM, "ops", r)
    return r


def _chain(arrays, size):
    return torch.stack([IR.host_chain(np.repeat(a, 3, -1) if a.shape[-1] == 1 else a, size) for a in arrays])


def test_loader_groups_equal_sizes_per_launch_and_keeps_the_order(rec):
    from PIL import Image
    from storygen_amd.image import load_masks, load_reference_images
    a = [IR.content("random", h, w, 3, seed=i) for i, (h, w) in enumerate([(9, 7), (5, 12), (9, 7), (5, 12), (9, 7), (8, 8)])]
    images = [a[0], Image.fromarray(a[1]), torch.from_numpy(a[2]), a[3], Image.fromarray(a[4]), a[5]]
    out = load_reference_images(images, size=(8, 6), device="cpu")
    assert rec.calls == [((3, 9, 7, 3), (8, 6), False), ((2, 5, 12, 3), (8, 6), False), ((1, 8, 8, 3), (8, 6), False)]
    assert out.dtype == torch.float16 and tuple(out.shape) == (6, 3, 6, 8)
    assert torch.equal(out.view(torch.int16), _chain(a, (8, 6)).view(torch.int16))          # Image.fromarray(a).resize((8, 6)) + ToTensor
    # one size: one launch, a [K,h,w,3] tensor is the same as the list of its images; flags per image split the launch
    rec.calls.clear()
    same = np.stack([a[0], a[2], a[4]])
    out = load_reference_images(torch.from_numpy(same), size=(4, 5), device="cpu")
    assert rec.calls == [((3, 9, 7, 3), (4, 5), False)] and torch.equal(out, _chain(list(same), (4, 5)))
    rec.calls.clear()
    out = load_reference_images(list(same), size=(4, 5), device="cpu", flip=[False, True, False])
    assert rec.calls == [((2, 9, 7, 3), (4, 5), False), ((1, 9, 7, 3), (4, 5), True)]
    want = _chain(list(same), (4, 5))
    want[1] = want[1].flip(-1)
    assert torch.equal(out, want)
    # mode L among RGB images: one channel resized, then replicated — what .convert('RGB').resize(.) gives
    rec.calls.clear()
    grey = IR.content("random", 9, 7, 1, seed=9)
    out = load_reference_images([a[0], Image.fromarray(grey[..., 0])], size=(4, 5), device="cpu")
    assert rec.calls == [((1, 9, 7, 3), (4, 5), False), ((1, 9, 7, 1), (4, 5), False)]
    via_convert = IR.host_chain(np.asarray(Image.fromarray(grey[..., 0]).convert("RGB")), (4, 5))
    assert torch.equal(out[1], via_convert) and torch.equal(out[0], IR.host_chain(a[0], (4, 5)))
    # masks: C = 1, [K,1,H,W]
    rec.calls.clear()
    out = load_masks([Image.fromarray(grey[..., 0]), grey[..., 0], grey], size=(4, 5), device="cpu")
    assert rec.calls == [((3, 9, 7, 1), (4, 5), False)] and tuple(out.shape) == (3, 1, 5, 4)
    assert all(torch.equal(o, IR.host_chain(grey, (4, 5))) for o in out)


def test_loader_rejections(rec):
    from PIL import Image
    from storygen_amd.image import load_masks, load_reference_images
    rgb = IR.content("random", 4, 4, 3)
    for mode in ("RGBA", "P", "1", "CMYK", "I;16", "F"):
        im = Image.new(mode, (4, 4))
        with pytest.raises(ValueError, match=r"convert\('RGB'\)"):
            load_reference_images([im], device="cpu")
        with pytest.raises(ValueError, match=r"convert\('L'\)"):
            load_masks([im], device="cpu")
    with pytest.raises(ValueError, match=r"convert\('L'\)"):
        load_masks([Image.fromarray(rgb)], device="cpu")
    for bad in ([], None, "path.png", rgb.astype(np.float32)[None], [rgb.astype(np.float32)], [torch.zeros(4, 4, 3)], [rgb[..., :2]],
                [np.zeros((0, 4, 3), np.uint8)], [rgb[None]], ["path.png"]):
        with pytest.raises(ValueError):
            load_reference_images(bad, device="cpu")
    with pytest.raises(ValueError, match="flip flags"):
        load_reference_images([rgb, rgb], device="cpu", flip=[True])
    with pytest.raises(ValueError):
        load_masks([rgb], device="cpu")
    assert rec.calls == []


def test_story_generator_ingests_raw_first_frames_and_leaves_float_tensors_alone(rec):
    from test_story_host import FakePipeline, H, W
    from storygen_amd.story import StoryGenerator
    a = [IR.content("random", 50, 70, 3, seed=1), IR.content("random", 90, 33, 3, seed=2)]
    want = _chain(a, (W, H))
    runs = {}
    for name, first in (("list", a), ("tuple", tuple(a)), ("float", want.float())):
        pipe = FakePipeline()
        StoryGenerator(pipe).generate(["g0", "g1"], context_frames=2, first_frames=first, first_prompts=["f0", "f1"], height=H, width=W,
                                      num_inference_steps=3, output_type="uint8")
        runs[name] = pipe.calls
        assert pipe.calls[0]["stage"] == "auto-regressive" and pipe.calls[0]["prev_prompt"] == ["f0", "f1"]
        assert torch.equal(pipe.calls[0]["image_prompt"].view(torch.int16), want[None].view(torch.int16)), name
        assert torch.equal(pipe.calls[1]["image_prompt"][0, 0], want[1])
    assert rec.calls == [((1, 50, 70, 3), (W, H), False), ((1, 90, 33, 3), (W, H), False)] * 2        # the float tensor launched nothing
    # a uint8 [K,h,w,3] tensor of any size: one launch
    rec.calls.clear()
    pipe = FakePipeline()
    both = torch.from_numpy(np.stack([a[0], a[0][::-1].copy()]))
    StoryGenerator(pipe).generate(["g0"], first_frames=both, first_prompts=["f0", "f1"], height=H, width=W, num_inference_steps=3)
    assert rec.calls == [((2, 50, 70, 3), (W, H), False)]
    assert torch.equal(pipe.calls[0]["image_prompt"][0], _chain(list(both.numpy()), (W, H)))
    # the rules of first_frames hold for raw images too, and the float path keeps its message
    gen = StoryGenerator(FakePipeline())
    with pytest.raises(ValueError, match="first prompts"):
        gen.generate(["g"], first_frames=a, first_prompts=["f0"], height=H, width=W)
    with pytest.raises(ValueError, match="go together"):
        gen.generate(["g"], first_frames=a, height=H, width=W)
    with pytest.raises(ValueError, match="first_frames must be"):
        gen.generate(["g"], first_frames=torch.rand(1, 3, H, W + 1), first_prompts=["f"], height=H, width=W)
    with pytest.raises(ValueError, match=r"convert\('RGB'\)"):
        from PIL import Image
        gen.generate(["g"], first_frames=[Image.new("RGBA", (4, 4))], first_prompts=["f"], height=H, width=W)
    assert gen.pipeline.calls == []
