"""What UNetEngine._alloc allocates, as a CPU-checkable fact beside the launch trace: the trace (tests/test_engine_launch_trace.py) sees
the views a launch gets, not the size of the allocation behind them (x16 is a flat M * Cw buffer).  tests/golden/engine_buffers.json
was recorded by tools/make_engine_buffers.py on the engine as it was BEFORE _alloc read UNetArch.schedule, for every engine the trace
cases build: every per-level, conv-input, concat and context buffer as name -> (shape, dtype, numel), and for every skip tensor the
concat buffer it views, its column offset, its shape and its (level, channels)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_engine_buffers as tool  # noqa: E402


def test_every_engine_allocates_the_recorded_buffers():
    with open(tool.GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(tool.buffer_records()))
    assert list(got) == list(want)
    for name in want:
        rec, now = want[name], got[name]
        if isinstance(rec, str):                 # an engine whose record equals an earlier one's holds that one's key
            assert now == rec, name
            continue
        assert list(now) == list(rec), f"{name}: buffer names or their order differ"
        assert {k: v for k, v in now.items() if v != rec[k]} == {}, name
    assert any("x16" in k for k in want[next(iter(want))])
