#!/usr/bin/env python
"""Record the launch sequence of UNetEngine.forward on the CPU (tests/recording_ops.py stands in for storygen_amd.ops) for a fixed set
of cases and write tests/golden/engine_launch_trace.json.  tests/test_engine_launch_trace.py replays the same cases and requires the
same entries in the same order, so the fixture must come from the code a change starts FROM: run this file in a checkout of the parent
commit (with this file and tests/recording_ops.py copied in), never on the changed engine.

    python tools/make_engine_launch_trace.py [out.json]

File format: {case name: [digest of entry 0, digest of entry 1, ...]} — the first 10 hex digits of the SHA-256 of each entry's canonical
JSON (a whole entry is ~150 bytes and a case has ~140 of them: the entries themselves would be a fixture nobody reads).  To see the
recorded side of a difference, run trace_cases() in a checkout of the recording commit."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_launch_trace.json")

# two levels of one layer each, transformers at the first and in the middle: 256 and 64 tokens on a 16x16 latent
SMALL = dict(block_out_channels=(64, 128), down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), layers_per_block=1,
             up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), cross_attention_dim=64, attention_head_dim=2)
D40 = dict(SMALL, block_out_channels=(320, 64), attention_head_dim=8)        # head dim 40 at the first level (the fp8 attention path)
HW, S, R = 16, 5, 2
CFG3 = dict(ctx_rows=2, attn3_groups=[(0, 2, 0), (2, 1, 1)])                 # batch 3 = (zero-image, frames, frames) on two context rows
SWITCHES = (("LN_FOLD", False), ("PAIR_GEMMS", False), ("FF_PROJ_MERGE", False), ("SPLITK_IN_GN", False), ("GN_EPILOGUE_STATS", False),
            ("ATTN_PAIR", True), ("FP16_BLOCK_STREAM", True))


def trace_cases() -> dict:
    """case name -> list of entries (tests/recording_ops.py), recorded on the engine of the importing tree."""
    import recording_ops
    from storygen_amd import engine as E
    from storygen_amd.arch import build_arch, feature_shapes
    from storygen_amd.synth import synthetic_state_dict
    out = {}
    with recording_ops.installed(E) as rec:
        wts = {}

        def engine(batch, n_ref, cfg=SMALL, **kw):
            key = json.dumps(cfg, sort_keys=True)
            if key not in wts:
                arch = build_arch(cfg)
                wts[key] = (arch, E.EngineWeights(arch, synthetic_state_dict(arch, 3), "cpu"))
            arch, w = wts[key]
            eng = E.UNetEngine(arch, None, "cpu", batch, HW, HW, n_ref=n_ref, seq_len=S, splitk_workspace_mb=1, weights=w, **kw)
            for t in (eng.x_in, eng.t_in, eng.text_in):          # cfg_shared_head compares its inputs on the first pass
                t.zero_()
            rec.reset()
            return eng

        def done(name):
            out[name] = rec.log
            rec.reset()

        def kv_buffers(eng, slots):
            return {k: (torch.empty(slots * n, c, dtype=E.F16), torch.empty(c, slots * n, dtype=E.F16))
                    for k, (n, c) in feature_shapes(eng.arch, HW, HW).items()}

        def main_pass(name, text_cache=False, cfg=SMALL, **kw):
            eng = engine(3, R, cfg, **{**CFG3, **kw})
            if text_cache:
                eng.cache_text_kv()
            eng.forward(consume=True, text_cache=text_cache)
            done(name)

        for head in (False, True):
            for cache in (False, True):
                main_pass(f"main{'-shared-head' if head else ''}{'-text-cache' if cache else ''}", cache, cfg_shared_head=head)
        for sw, val in SWITCHES:
            old = getattr(E, sw)
            setattr(E, sw, val)
            try:
                main_pass(f"main-{sw}={val}")
                if sw == "LN_FOLD":          # the shared head's two halves on the unfolded LayerNorm form
                    main_pass(f"main-shared-head-{sw}={val}", cfg_shared_head=True)
            finally:
                setattr(E, sw, old)
        main_pass("main-ctx-short", ctx_short=1)
        main_pass("main-attn3-groups", attn3_groups=[(0, 1, 0), (1, 1, 1), (2, 1, 0)])
        main_pass("main-fp8-d40", cfg=D40, fp8_attention=True)
        eng = engine(3, R, **CFG3)
        eng.kv_ext = kv_buffers(eng, eng.ctx_slots)              # attn3 K / V^T that a reference pass left (the sampler's schedule)
        eng.forward(consume=True)
        done("main-kv-ext")

        engine(3, R).forward(harvest_slot=1)
        done("ref-harvest-slot")
        main = engine(3, R, **CFG3)
        ref = engine(3, 0)
        # strided copies: the zero-image sample broadcast into both slots of row 0, two frames into row 1
        ref.forward(harvest=E.HarvestPlan(main.ctx, [(0, 0, 0, 0, 2), (1, 1, 1, 0, 2)]))
        done("ref-plan-copies")
        ref = engine(4, 0)
        plan = E.HarvestPlan(main.ctx, [(0, 1, 0, 0, 2), (2, 1, 1, 0, 2)], kv=kv_buffers(main, main.ctx_slots), direct=True)
        assert plan.is_direct(4, R)
        assert ref.forward(harvest=plan, harvest_only=True) is None
        done("ref-direct-kv-harvest-only")
        other = engine(3, R, **CFG3)
        ref = engine(8, 0)
        ops_ = [(0, 1, 0, 0, 2), (2, 1, 1, 0, 2)]
        ref.forward(harvest=[E.HarvestPlan(main.ctx, ops_, kv=kv_buffers(main, main.ctx_slots)),
                             E.HarvestPlan(other.ctx, ops_, src_offset=4)], text_cache=False)
        done("ref-two-plans-src-offset")
    return out


def digest(entry: dict) -> str:
    return hashlib.sha256(json.dumps(entry, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:10]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    cases = {name: [digest(e) for e in log] for name, log in trace_cases().items()}
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in cases.items()) + "\n}\n")
    print(f"{path}: {len(cases)} cases, {sum(map(len, cases.values()))} launches, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
