#!/usr/bin/env python
"""Record what UNetEngine._alloc allocates for every engine the cases of tools/make_engine_launch_trace.py build, and write
tests/golden/engine_buffers.json.  The launch trace sees views, not allocation sizes (x16 is a flat M * Cw buffer of which a launch
sees [M, cin]); this record closes that gap.  Like the trace, the fixture must come from the code a change starts FROM: run this file
in a checkout of the parent commit, never on the changed engine.

    python tools/make_engine_buffers.py [out.json]

File format: {"<ordinal> <constructor arguments>": {buffer name: [shape, dtype, numel], "skips[i]": [up_cats index, column offset,
shape, (level, channels)]}}, in allocation order; an engine whose record equals an earlier one's holds that one's key instead."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_engine_launch_trace as trace  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_buffers.json")


def inventory(eng) -> dict:
    rec = {}
    named = [(f"lv[{l}].{n}", t) for l, d in enumerate(eng.lv) for n, t in d.items() if t is not None]
    named += [(f"padded[{l},{c}]", t) for (l, c), t in eng.padded.items()]
    named += [(f"up_cats[{i}]", t) for i, t in enumerate(eng.up_cats)]
    named += [(f"ctx[{k}]", t) for k, t in eng.ctx.items()]
    for name, t in named:
        rec[name] = [list(t.shape), str(t.dtype), t.numel()]
    bases = [t.untyped_storage().data_ptr() for t in eng.up_cats]
    for i, (sk, meta) in enumerate(zip(eng.skips, eng.skip_meta)):
        rec[f"skips[{i}]"] = [bases.index(sk.untyped_storage().data_ptr()), sk.storage_offset(), list(sk.shape), list(meta)]
    return rec


def buffer_records() -> dict:
    from storygen_amd import engine as E
    out, alloc = {}, E.UNetEngine._alloc

    def recording_alloc(eng, splitk_mb):
        alloc(eng, splitk_mb)
        rec = inventory(eng)
        same = next((k for k, v in out.items() if v == rec), None)
        boc = "x".join(map(str, eng.cfg["block_out_channels"]))
        switches = "".join(f" {sw}" for sw, val in trace.SWITCHES if getattr(E, sw) == val)
        out[f"{len(out):02d} B={eng.B} R={eng.R} boc={boc} ctx_rows={eng.ctx_rows} ctx_short={eng.ctx_short} fp8={eng.fp8_attention}{switches}"] = same or rec

    E.UNetEngine._alloc = recording_alloc
    try:
        trace.trace_cases()
    finally:
        E.UNetEngine._alloc = alloc
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    recs = buffer_records()
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in recs.items()) + "\n}\n")
    print(f"{path}: {len(recs)} engines, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
