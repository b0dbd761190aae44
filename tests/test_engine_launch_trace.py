"""The launch sequence of UNetEngine.forward as a CPU-checkable fact: tests/recording_ops.py stands in for storygen_amd.ops and logs
every wrapper call (op, every tensor argument as storage ordinal / offset / shape / strides / dtype, every scalar and keyword), and the
log of each case of tools/make_engine_launch_trace.py must equal the recorded one entry by entry.  tests/golden/engine_launch_trace.json
holds a digest per entry; it was recorded by that tool on the engine as it was BEFORE UNetEngine._transformer was split into stages, so
equality says that the split changed no launch, operand, order or buffer.  Cases: the CFG main pass (batch 3, two prior frames) with
and without cfg_shared_head and the text cache, each module switch flipped alone (LN_FOLD also under the shared head), short context
rows, per-group image attention, fp8 attention at head dim 40, externally projected K / V^T; reference passes with harvest_slot, a
strided-copy plan, a direct plan with K / V^T projections and harvest_only, and a list of two plans with a source offset.

Limit: EngineWeights packs the fused feed-forward weights only on a GPU, so the fused feed-forward branches (FF_FUSED, the hidden
split) are not in the trace; the parity tests of tests/test_unet_gpu.py cover them on hardware."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_engine_launch_trace as tool  # noqa: E402

with open(tool.GOLDEN) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def traces():
    return tool.trace_cases()


def test_the_cases_reach_the_branches_they_are_meant_to_pin_down(traces):
    assert list(traces) == list(GOLDEN)
    entries = [e for log in traces.values() for e in log]
    assert {"gemm_pair", "attention_pair", "attention_f8", "layernorm", "copy_rows", "gemm_stats_rows",
            "conv3x3_planned_splits"} <= {e["op"] for e in entries}
    assert any(e["kw"].get("defer_reduce") for e in entries)
    assert any(e["op"] == "groupnorm" and e["kw"].get("pstats") for e in entries)
    assert any(e["op"] == "gemm" and e["kw"].get("stats") for e in entries)


@pytest.mark.parametrize("case", list(GOLDEN))
def test_launch_sequence_equals_the_recorded_one(traces, case):
    want, got = GOLDEN[case], traces[case]
    for i, (w, e) in enumerate(zip(want, got)):
        if w != tool.digest(e):
            before = json.dumps(got[i - 1], sort_keys=True) if i else "(first entry)"
            pytest.fail(f"{case}: entry {i} of {len(want)} is not the recorded one ({w})\n  now:        {json.dumps(e, sort_keys=True)}\n  the one before (equal): {before}")
    assert len(got) == len(want), f"{case}: {len(got)} launches, recorded {len(want)}" \
        + (f"; first extra entry: {json.dumps(got[len(want)], sort_keys=True)}" if len(got) > len(want) else "")
