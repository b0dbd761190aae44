"""What the ViT / CLIP towers hand to the kernels as a CPU-checkable fact: tests/recording_ops.py stands in for storygen_amd.ops and logs
every wrapper call, and the log of each case of tools/make_tower_launch_trace.py must equal the recorded one entry by entry; every tensor
an engine prepared for the device (padded patch weight, patch bias, class vector and tables, LayerNorm pairs, projection, every tensor of
every layer) must have the recorded shape, dtype and SHA-256.  tests/golden/tower_launch_trace.json was recorded by that tool on
ClipVisionEngine, DinoVitEngine and ClipTextEngine as they were BEFORE the shared ViT tower was factored out of the first two, so equality
says that the refactor changed no launch, operand, order, buffer or weight bit (the split of DINO's fused qkv, the column padding and
the fp32 -> fp16 rounding included).  Cases: the narrow image tower on float input of a foreign size, on preprocessed pixels, on 8-bit
frames of two sizes in one list (the scatter branch) and as one [B,h,w,3] batch under both crop rules; the wide tower with padded
(patch 14) and unpadded (patch 16) patch rows; DINO's tower on pixels, on mixed 8-bit frames and in passes smaller than the frame count;
the text tower with and without an attention mask and its projection; PickScorer, FrameAligner and ClipScorer built from one CLIPModel
state dict.

The one normalisation: a clip_patchify_u8 entry holds the resolved (Hr, Wr, top, left), whether the caller passed crop= or geometry=
(module docstring of the tool).  Limit: the index scatter of a partial group is a torch operation, not a launch; tests/test_clip_u8_host.py
and tests/test_dedup_host.py check its result on emulated ops."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_tower_launch_trace as tool  # noqa: E402

with open(tool.GOLDEN) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def traces():
    return tool.trace_cases()


def test_the_cases_reach_the_branches_they_are_meant_to_pin_down(traces):
    logs = traces["launches"]
    assert list(logs) == list(GOLDEN["launches"]) and list(traces["weights"]) == list(GOLDEN["weights"])
    entries = [e for log in logs.values() for e in log]
    assert {"clip_patchify", "clip_patchify_u8", "clip_embed_patches", "embed_tokens", "attention_small", "attention_enc", "gemm", "layernorm",
            "act_rows"} <= {e["op"] for e in entries}
    patchify = [e for e in entries if e["op"] == "clip_patchify"]
    assert any("kpad" in e["kw"] for e in patchify) and any("kpad" not in e["kw"] for e in patchify)
    # the narrow tower takes the plain kernel, and so does the wide one whose patch row needs no padding
    assert all("kpad" not in e["kw"] for n in logs if n.startswith(("vision-narrow", "vision-wide-16")) for e in logs[n] if e["op"] == "clip_patchify")
    u8 = {n: [e for e in log if e["op"] == "clip_patchify_u8"] for n, log in logs.items()}
    assert len(u8["vision-narrow-u8-two-sizes"]) == 2 and len(u8["vision-narrow-u8-batch-floor"]) == 1 and len(u8["dino-call-batch-3-of-4"]) == 4
    assert all(set(e["kw"]) == {"geometry", "kpad"} for log in u8.values() for e in log)
    assert u8["vision-narrow-u8-batch-torchvision"][0]["kw"]["geometry"] == [32, 35, 0, 2]
    assert u8["vision-narrow-u8-batch-floor"][0]["kw"]["geometry"] == [32, 35, 0, 1]
    assert u8["dino-call-whole-batch"][0]["kw"]["geometry"] == [112, 140, 8, 22]
    assert any(e["op"] == "attention_small" and e["args"][7] is not None for e in logs["text-attention-mask"])
    # the patch GEMM is the launch after the patchify: DINO's carries a bias, CLIP's none
    assert logs["dino-encode-pixels"][1]["op"] == "gemm" and "bias" in logs["dino-encode-pixels"][1]["kw"]
    assert logs["vision-narrow-encode-pixels"][1]["op"] == "gemm" and "bias" not in logs["vision-narrow-encode-pixels"][1]["kw"]


@pytest.mark.parametrize("case", list(GOLDEN["launches"]))
def test_launch_sequence_equals_the_recorded_one(traces, case):
    want, got = GOLDEN["launches"][case], traces["launches"][case]
    for i, (w, e) in enumerate(zip(want, got)):
        if w != tool.digest(e):
            before = json.dumps(got[i - 1], sort_keys=True) if i else "(first entry)"
            pytest.fail(f"{case}: entry {i} of {len(want)} is not the recorded one ({w})\n  now:        {json.dumps(e, sort_keys=True)}\n  the one before (equal): {before}")
    assert len(got) == len(want), f"{case}: {len(got)} launches, recorded {len(want)}" \
        + (f"; first extra entry: {json.dumps(got[len(want)], sort_keys=True)}" if len(got) > len(want) else "")


@pytest.mark.parametrize("engine", list(GOLDEN["weights"]))
def test_prepared_tensors_equal_the_recorded_ones(traces, engine):
    want, got = GOLDEN["weights"][engine], traces["weights"][engine]
    assert [t[:3] for t in got] == [t[:3] for t in want]
    assert [t[0] for t, w in zip(got, want) if t[3] != w[3]] == []
