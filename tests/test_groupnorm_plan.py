"""ops.groupnorm_plan (sg_groupnorm_plan) on the host: nothing is launched.  The variant against what the two queries it replaced
answered on the parent library (tests/golden/groupnorm_variants.json, tools/make_groupnorm_variants.py), the geometry against values
worked out by hand from the parent's formulas."""
import contextlib
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "groupnorm_variants.json")
DEFAULTS = dict(gn_no_fused=0, gn_wide=1, gn_fused_max=-1, gn_fused_nt=1024, gn_chunks=0)
LETTER = {"one_launch": "f", "wide": "p", "narrow": "n"}       # is_fused / uses_pstats / neither


@contextlib.contextmanager
def _options(**kw):
    from storygen_amd import ops
    try:
        for name, value in kw.items():
            ops.debug_set_option(name, value)
        yield
    finally:
        for name in kw:
            ops.debug_set_option(name, DEFAULTS[name])


def _answers(g) -> str:
    from storygen_amd import ops
    out = []
    for hw in g["HW"]:
        for c in g["C"]:
            for groups in g["groups"]:
                variant = ops.groupnorm_plan(hw, c, groups)[0]
                assert ops.groupnorm_is_fused(hw, c, groups) == (variant == "one_launch")
                assert ops.groupnorm_uses_pstats(hw, c, groups) == (variant == "wide")
                out.append(LETTER[variant])
    return "".join(out)


def test_plan_variant_answers_what_the_two_queries_answered():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert set(g["answers"]) == {"default", "gn_no_fused=1", "gn_wide=0", "gn_fused_max=0", "gn_fused_max=4096"}
    for setting, want in g["answers"].items():
        assert len(want) == len(g["HW"]) * len(g["C"]) * len(g["groups"])
        opts = {} if setting == "default" else {setting.split("=")[0]: int(setting.split("=")[1])}
        with _options(**opts):
            got = _answers(g)
        assert got == want, setting
    assert _answers(g) == g["answers"]["default"], "options not restored"


# (variant, threads, launches, chunks, rows per chunk, apply blocks, apply rows); rpp = thread rows per pass, cdiv rounds up
def test_wide_pair_geometry():
    from storygen_amd.ops import groupnorm_plan as plan
    # C = 320: 40 vectors per row, rpp = 1024 / 40 = 25.  B = 3: 256 / 3 = 85 chunks wanted, cdiv(4096, 85) = 49 rows, cdiv(4096, 49) = 84
    assert plan(4096, 320, 32, B=3) == ("wide", 1024, 2, 84, 49, 0, 0)
    assert plan(4096, 320, 32, B=3, pstats=True) == ("wide", 1024, 1, 84, 49, 0, 0)
    assert plan(4096, 320, 32, B=3, x_f32=True) == ("wide", 1024, 2, 84, 49, 0, 0)
    # B = 1: 256 chunks wanted, cdiv(4096, 256) = 16 rows < rpp -> 25 rows, cdiv(4096, 25) = 164
    assert plan(4096, 320, 32, B=1) == ("wide", 1024, 2, 164, 25, 0, 0)
    # B = 300: 256 / 300 = 0 -> 1 chunk wanted: all 4096 rows
    assert plan(4096, 320, 32, B=300) == ("wide", 1024, 2, 1, 4096, 0, 0)
    with _options(gn_chunks=64):
        assert plan(4096, 320, 32, B=3) == ("wide", 1024, 2, 64, 64, 0, 0)     # min(85, 64) chunks wanted: 64 rows each
        assert plan(4096, 320, 32, B=8) == ("wide", 1024, 2, 32, 128, 0, 0)    # 256 / 8 = 32 < 64: the cap does not bind
    assert plan(4096, 320, 32, B=3)[3:5] == (84, 49)


def test_narrow_pair_geometry():
    from storygen_amd.ops import groupnorm_plan as plan
    # C = 192 (cpg 6), HW = 2100, fp16: 24 threads per row, rpp = 256 / 24 = 10.  Statistics: cdiv(2100, 80) = 27 chunks wanted (< 512 / B,
    # < 64), cdiv(2100, 27) = 78 rows, cdiv(2100, 78) = 27.  Apply: 384-byte rows, cdiv(32768, 384) = 86 rows at least (> 2 rpp),
    # cdiv(2100, 86) = 25 blocks wanted (< 1024 / B), cdiv(2100, 25) = 84 rows, cdiv(2100, 84) = 25
    assert plan(2100, 192, 32, B=1) == ("narrow", 256, 2, 27, 78, 25, 84)
    assert plan(2100, 192, 32, B=1, pstats=True) == ("narrow", 256, 2, 27, 78, 25, 84)       # keeps its own statistics pass
    # C = 64 (cpg 2), HW = 1001, B = 3: 8 threads per row, rpp = 32.  Statistics: cdiv(1001, 256) = 4 chunks, cdiv(1001, 4) = 251 rows.
    # Apply, fp32: 256-byte rows, 128 rows at least, cdiv(1001, 128) = 8 blocks, cdiv(1001, 8) = 126 rows, cdiv(1001, 126) = 8;
    # fp16: 128-byte rows, 256 rows at least, 4 blocks of 251 rows
    assert plan(1001, 64, 32, B=3, x_f32=True) == ("narrow", 256, 2, 4, 251, 8, 126)
    assert plan(1001, 64, 32, B=3) == ("narrow", 256, 2, 4, 251, 4, 251)
    # C = 128, HW = 9216: rpp = 16, cdiv(9216, 128) = 72 chunks wanted -> the cap of 64: 144 rows; B = 16, HW = 4608: 36 wanted -> 512 / 16 = 32
    assert plan(9216, 128, 32, B=1)[3:5] == (64, 144)
    assert plan(4608, 128, 32, B=16)[3:5] == (32, 144)


def test_one_launch_threads_and_split_refusals():
    from storygen_amd.ops import groupnorm_plan as plan
    one = lambda nt: ("one_launch", nt, 1, 0, 0, 0, 0)
    assert plan(256, 1280, 32, B=4) == one(1024)                 # slab 256 x 40 = 10240: the default threshold
    assert plan(257, 1280, 32, B=4)[0] == "wide"
    with _options(gn_fused_nt=256):
        assert plan(256, 1280, 32, B=4) == one(256)
        assert plan(256, 1280, 32, B=4, splits=4) == one(1024)   # a split-K input has the 1024-thread form only
    assert plan(256, 1280, 32, B=4, splits=4) == one(1024)
    # C = 2048: 64 channels per group; 256 pixels = 16384 values, the most the 1024-thread form holds (4 items of 4 values per thread)
    with _options(gn_fused_max=24576):
        assert plan(256, 2048, 32) == one(1024)
        assert plan(257, 2048, 32) == one(256)
        assert plan(384, 2048, 32) == one(256)                   # 24576 = 256 threads x 24 items x 4 values: the last slab it holds
        assert plan(385, 2048, 32)[0] == "wide"
        assert plan(256, 2048, 32, splits=2) == one(1024)
        with pytest.raises(RuntimeError, match="16384 values"):
            plan(257, 2048, 32, splits=2)
        with _options(gn_fused_nt=256):
            assert plan(256, 2048, 32) == one(256)
    with pytest.raises(RuntimeError, match="needs the one-launch variant"):
        plan(4096, 320, 32, B=3, splits=2)                       # the wide pair
    with pytest.raises(RuntimeError, match="needs the one-launch variant"):
        plan(2100, 192, 32, splits=2)                            # the narrow pair
    with pytest.raises(RuntimeError, match="multiple of 8 and of groups"):
        plan(64, 320, 3)
