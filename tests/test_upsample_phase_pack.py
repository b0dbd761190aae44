"""The weight pack of the phase form of the upsampling convolution (repack.upsample_phase_sums / upsample_phase_pack,
sg_conv3x3_desc.upsample2x = 2), on the CPU: nearest-2x upsampling followed by the 3x3 convolution equals, for every output parity (a, b),
the 2x2 convolution of the input-resolution image with the packed tap sums, scattered to pixels (2i + a, 2j + b).  In float64 the two
differ by round-off only (the sums associate differently); EngineWeights builds the pack and rebuilds it in place on reload_()."""
import pytest
import torch
import torch.nn.functional as F

from storygen_amd import repack

# float64: a 3x3xCin contraction of O(1) terms re-associated — a few hundred ulps of 2.2e-16 at most
TOL = 1e-12
# two levels, one Upsample2D (the description tools/make_engine_launch_trace.py records the engine on)
SMALL = dict(block_out_channels=(64, 128), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), layers_per_block=1,
             up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), cross_attention_dim=64, attention_head_dim=2)


def phase_conv(x: torch.Tensor, wp: torch.Tensor) -> torch.Tensor:
    """x [B, Cin, H, W], wp [4, Cout, 2, 2, Cin] -> [B, Cout, 2H, 2W]: the four 2x2 convolutions as the kernel evaluates them — tap (ty, tx)
    of phase (a, b) at output (i, j) reads pixel (i + a + ty, j + b + tx) of the image with a one-pixel zero border."""
    B, _, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros(B, wp.shape[1], 2 * H, 2 * W)
    for a in range(2):
        for b in range(2):
            w = wp[2 * a + b].permute(0, 3, 1, 2)                      # [Cout, Cin, 2, 2]
            out[:, :, a::2, b::2] = F.conv2d(xp[:, :, a: a + H + 1, b: b + W + 1], w)
    return out


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 5, 5, 64, 24), (1, 4, 7, 128, 16), (1, 1, 3, 64, 8)])
def test_phase_sums_are_the_upsampled_convolution(B, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(Cin + H)
    x = torch.randn(B, Cin, H, W, dtype=torch.float64, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, dtype=torch.float64, generator=g) / (9 * Cin) ** 0.5
    wp = repack.upsample_phase_sums(w)
    assert tuple(wp.shape) == (4, Cout, 2, 2, Cin) and wp.dtype == torch.float64
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    got = phase_conv(x, wp)
    err = float((got - want).abs().max())
    print(f"B{B} {H}x{W} {Cin}->{Cout}: max |phase - upsampled 3x3| = {err:.3e}")
    assert err <= TOL * max(1.0, float(want.abs().max()))
    # every tap is used exactly once per phase: the four taps of a phase add up to the nine of the kernel
    assert torch.allclose(wp.sum(dim=(2, 3)), w.sum(dim=(2, 3)).permute(0, 1)[None].expand(4, -1, -1), atol=1e-12)


def test_pack_sums_in_fp32_and_rounds_once():
    g = torch.Generator().manual_seed(3)
    w16 = (torch.randn(16, 64, 3, 3, generator=g) / 24).to(torch.float16)
    wp = repack.upsample_phase_pack(w16)
    assert wp.dtype == torch.float16 and wp.is_contiguous() and tuple(wp.shape) == (4, 16, 2, 2, 64)
    exact = repack.upsample_phase_sums(w16.double())                   # sums of at most four fp16 values are exact in fp32
    assert torch.equal(wp, exact.to(torch.float16))


def test_engine_weights_rebuild_the_pack_on_reload():
    from storygen_amd.arch import build_arch
    from storygen_amd.engine import EngineWeights
    from storygen_amd.synth import synthetic_state_dict

    arch = build_arch(SMALL)
    sd = synthetic_state_dict(arch, seed=0)
    wts = EngineWeights(arch, sd, "cpu")
    ups = [b.sampler_prefix for b in arch.up if b.sampler_prefix]
    assert ups and sorted(wts.sampler_phases) == sorted(ups)
    held = {p: wts.sampler_phases[p] for p in ups}
    for p in ups:
        assert torch.equal(held[p], repack.upsample_phase_pack(sd[f"{p}.weight"].to(torch.float16)))
    sd2 = {k: v.clone() for k, v in sd.items()}
    for p in ups:
        sd2[f"{p}.weight"] = sd2[f"{p}.weight"] * 0.5 + 0.01
    wts.reload_(sd2)
    for p in ups:
        assert wts.sampler_phases[p] is held[p], "refreshed in place: captured graphs hold the address"
        assert torch.equal(held[p], repack.upsample_phase_pack(sd2[f"{p}.weight"].to(torch.float16)))
        assert not torch.equal(held[p], repack.upsample_phase_pack(sd[f"{p}.weight"].to(torch.float16)))
