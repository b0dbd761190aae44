"""ORACLE tooling — tests/golden/step_tables.json: what the sampler's host side gives for every update rule, on file.

What it pins (tests/test_update_rules.py, CPU, `==` on Python floats — the same host arithmetic, so no tolerance): the rows of
`storygen_amd.sampler.step_table` for DDIM, DDIM with clip_sample / eta, PNDM/PLMS and DPM-Solver(++) over G, overlap and stage
(tests/update_rule_helpers.py::TABLES), and, for a 10-evaluation loop of each rule at G = 1 and G = 5 on the stand-in engine, which
`ops` entry point every step calls with which state buffer, plus the latents the loop ends with (::LOOPS).  The committed file was
recorded from the commit before the schedules handed out UpdateRule objects; regenerate it only when a table is MEANT to change.

torch's vectorised fp32 CPU kernels round the schedules' tables 1 ulp differently on CPUs with other vector units, so the file holds
one recording per host arithmetic (update_rule_helpers.host_arithmetic_fingerprint): a run adds or replaces this host's and keeps
the others.  Every committed recording was made by that one commit.

Usage:  python oracle/make_golden_step_tables.py        (no GPU; updates tests/golden/step_tables.json)
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import update_rule_helpers as H  # noqa: E402


def main():
    path = os.path.join(ROOT, "tests", "golden", "step_tables.json")
    out = {"made_by": "oracle/make_golden_step_tables.py", "recordings": {}}
    if os.path.exists(path):                   # recordings made on hosts with other fp32 arithmetic stay
        with open(path) as f:
            out["recordings"] = json.load(f)["recordings"]
    out["recordings"][H.host_arithmetic_fingerprint()] = {
        "tables": {name: H.table_of(case) for name, case in H.TABLES.items()},
        "loops": {f"{name}_g{G}": H.record_calls(case, G) for name, case in H.LOOPS.items() for G in (1, 5)}}
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(out["recordings"]), "recording(s)")


if __name__ == "__main__":
    main()
