"""UNetArch.schedule (the flat layer walk the engine and the trainer follow) against facts obtained without it: the key order and the
shapes of param_shapes(), which keeps its own block-by-block walk, the samplers counted along the way, feature_level, and the
per-block skip_channels.  Configs: SD-1.5, the tiny two-level one of the CPU tests, and a lopsided one with attention only at the
deepest level and none at level 0."""
import re

import pytest

from storygen_amd.arch import SD15_CONFIG, build_arch, param_shapes

TINY = dict(block_out_channels=(32, 64), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
            up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), cross_attention_dim=48, attention_head_dim=2, norm_num_groups=8, sample_size=64)
LOPSIDED = dict(block_out_channels=(32, 64), layers_per_block=1, down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"),
                up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"), norm_num_groups=8, attention_head_dim=4)


@pytest.fixture(scope="module", params=[SD15_CONFIG, TINY, LOPSIDED], ids=["sd15", "tiny", "lopsided"])
def case(request):
    arch = build_arch(request.param)
    return arch, param_shapes(arch)


def _prefixes(shapes, pattern):
    return [m.group(1) for m in (re.match(pattern, k) for k in shapes) if m]


def _levels(schedule):
    """Level of every step's input and output, counted from the samplers alone."""
    lvl, out = 0, []
    for s in schedule:
        after = lvl + (0 if s.sampler is None else 1 if "downsamplers" in s.sampler else -1)
        out.append((lvl, after))
        lvl = after
    assert lvl == 0
    return out


def test_blocks_is_down_mid_up(case):
    arch, _ = case
    assert arch.blocks == arch.down + [arch.mid] + arch.up


def test_resnets_follow_the_state_dict_order_with_its_widths(case):
    arch, shapes = case
    layers = [s for s in arch.schedule if s.resnet is not None]
    assert [s.resnet.prefix for s in layers] == _prefixes(shapes, r"(.*\.resnets\.\d+)\.norm1\.weight$")
    for s in layers:
        p = s.resnet.prefix
        assert (s.resnet.cin,) == shapes[f"{p}.norm1.weight"] and (s.resnet.cout,) == shapes[f"{p}.norm2.weight"]
        assert s.cout == s.resnet.cout and s.sampler is None


def test_transformers_and_samplers_follow_the_state_dict_order(case):
    arch, shapes = case
    xfs = [s for s in arch.schedule if s.xf is not None]
    assert [s.xf.prefix for s in xfs] == _prefixes(shapes, r"(.*\.attentions\.\d+)\.norm\.weight$")
    for s in xfs:       # a transformer follows the resnet of the same block and index, at that resnet's width
        assert s.xf.prefix.replace("attentions", "resnets") == s.resnet.prefix
        assert (s.cout,) == shapes[f"{s.xf.prefix}.norm.weight"]
    samplers = [s for s in arch.schedule if s.sampler is not None]
    assert [s.sampler for s in samplers] == _prefixes(shapes, r"(.*samplers\.0\.conv)\.weight$")
    for s in samplers:
        assert s.resnet is None and s.xf is None and shapes[f"{s.sampler}.weight"][:2] == (s.cout, s.cout)


def test_levels_count_the_samplers(case):
    arch, _ = case
    deepest = len(arch.config["block_out_channels"]) - 1
    for s, (lvl, after) in zip(arch.schedule, _levels(arch.schedule)):
        assert (s.level, s.out_level) == (lvl, after)
        if s.xf is not None:
            assert s.level == arch.feature_level[s.xf.feature_key]
    mid = [s for s in arch.schedule if s.resnet is not None and s.resnet.prefix.startswith("mid_block")]
    assert [(s.level, s.xf is not None, s.push, s.pop) for s in mid] == [(deepest, True, None, None), (deepest, False, None, None)]


def test_skips_are_pushed_and_popped_last_in_first_out(case):
    arch, shapes = case
    assert arch.skips[0] == (0, shapes["conv_in.weight"][0])
    stack, widths = [0], [c for blk in arch.up for c in blk.skip_channels]
    for s, (lvl, after) in zip(arch.schedule, _levels(arch.schedule)):
        if s.push is not None:      # what the producing layer outputs: its level, and its output channels as the checkpoint has them
            assert s.pop is None
            key = f"{s.sampler}.weight" if s.sampler else f"{s.resnet.prefix}.norm2.weight"
            assert arch.skips[s.push] == (after, shapes[key][0])
            stack.append(s.push)
        if s.pop is not None:
            assert s.pop == stack.pop()
            assert s.skip == arch.skips[s.pop][1] == widths.pop(0) and arch.skips[s.pop][0] == lvl
        else:
            assert s.skip == 0
    assert not stack and not widths
    down = [s for s in arch.schedule if (s.resnet.prefix if s.sampler is None else s.sampler).startswith("down_blocks")]
    assert [s.push for s in down] == list(range(1, len(arch.skips)))      # every down-path output, and nothing else, is a skip


def test_up_layers_concatenate_the_previous_output_and_their_skip(case):
    arch, shapes = case
    for prev, s in zip(arch.schedule, arch.schedule[1:]):
        if s.pop is not None:
            key = f"{prev.sampler}.weight" if prev.sampler else f"{prev.resnet.prefix}.norm2.weight"
            assert s.resnet.cin - s.skip == prev.cout == shapes[key][0]
    ups = [s for s in arch.schedule if s.resnet is not None and s.resnet.prefix.startswith("up_blocks")]
    assert all(s.pop is not None for s in ups) and arch.schedule[0].pop is None
