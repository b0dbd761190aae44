#!/usr/bin/env python
"""Record which forward GroupNorm variant the library picks over a sweep of shapes and development options, as the answers of
ops.groupnorm_uses_pstats and ops.groupnorm_is_fused, and write tests/golden/groupnorm_variants.json.  tests/test_groupnorm_plan.py
requires the same answers from the plan of the changed library, so the fixture must come from the code a change starts FROM: run this
file in a checkout of the parent commit (with this file copied in), never on the changed library.  Host only: nothing is launched.

    python tools/make_groupnorm_variants.py [out.json]

File format: {"HW": [...], "C": [...], "groups": [...], "answers": {option setting: string}} — one character per (HW, C, groups) in
that nesting order (groups fastest): "f" = is_fused, "p" = uses_pstats, "n" = neither (the narrow pair)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "groupnorm_variants.json")

HWS = (16, 64, 256, 1024, 4096, 9216)
# every GroupNorm width of the UNet (320 .. 1280 and the concats 960, 1920, 2560), the VAE (128, 256, 512) and tests/ (32, 64, 192, 2048)
CS = (32, 64, 128, 192, 256, 320, 512, 640, 960, 1280, 1920, 2048, 2560)
GROUPS = (1, 8, 32)
# (option, value in the sweep, the library's default)
SETTINGS = ((None, 0, 0), ("gn_no_fused", 1, 0), ("gn_wide", 0, 1), ("gn_fused_max", 0, -1), ("gn_fused_max", 4096, -1))


def setting_name(opt, val) -> str:
    return "default" if opt is None else f"{opt}={val}"


def sweep(answer) -> dict:
    """answer(HW, C, groups) -> "f" / "p" / "n", asked over the whole sweep under every setting (each option restored afterwards)."""
    from storygen_amd import ops
    out = {}
    for opt, val, default in SETTINGS:
        if opt is not None:
            ops.debug_set_option(opt, val)
        try:
            out[setting_name(opt, val)] = "".join(answer(hw, c, g) for hw in HWS for c in CS for g in GROUPS)
        finally:
            if opt is not None:
                ops.debug_set_option(opt, default)
    return out


def two_queries(hw, c, g) -> str:
    from storygen_amd import ops
    fused, pstats = bool(ops.groupnorm_is_fused(hw, c, g)), bool(ops.groupnorm_uses_pstats(hw, c, g))
    assert not (fused and pstats)
    return "f" if fused else "p" if pstats else "n"


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    answers = sweep(two_queries)
    with open(path, "w") as f:
        f.write('{"HW": %s, "C": %s, "groups": %s, "answers": {\n' % (json.dumps(list(HWS)), json.dumps(list(CS)), json.dumps(list(GROUPS))))
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in answers.items()) + "\n}}\n")
    print(f"{path}: {len(answers)} settings x {len(HWS) * len(CS) * len(GROUPS)} shapes")


if __name__ == "__main__":
    main()
