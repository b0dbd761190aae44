"""Times a 300-frame x 500-sentence alignment with the features in hand, on the GPU: sg_align_cost_f64 + sg_dtw_path_f64 (two launches and
the copy of the path to the host) beside the NumPy restatement of tests/align_reference.py on the same box — its cell-by-cell cost loop,
as data_process/align.py runs it, and its recurrence (one anti-diagonal at a time, and the script's plain double loop) — alternating in
one process.  Checks on the way that both give the same path.

    python tools/bench_align.py [--out FILE] [--rounds N]

An untimed pass first; device figures are medians over rounds of device-event time, host figures medians of perf_counter."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align: needs the GPU (no CPU path)")
    from storygen_amd import ops
    from storygen_amd.align import align_features
    from tests import align_reference as A
    dev = torch.device("cuda:0")
    r, c, dim = 300, 500, 512
    rng = np.random.default_rng(0)
    f, s = rng.standard_normal((r, dim)).astype(np.float32), rng.standard_normal((c, dim)).astype(np.float32)
    tf, ts = np.sort(rng.random(r)) * 1500.0, np.sort(rng.random(c)) * 1500.0          # a 25-minute video
    df, ds, dtf, dts = (torch.from_numpy(x).to(dev) for x in (f, s, tf, ts))
    cost = ops.align_cost(df, ds, dtf, dts)
    got = align_features(df, ds, dtf, dts)
    torch.cuda.synchronize()
    reps = 20
    t = {"cost": [], "dtw": [], "whole": [], "np_cost": [], "np_dtw": [], "np_loops": []}
    for n in range(args.rounds):
        t["cost"].append(timed(lambda: ops.align_cost(df, ds, dtf, dts, out=cost), reps))
        t["dtw"].append(timed(lambda: ops.dtw_path(cost), reps))
        t0 = time.perf_counter()
        align_features(df, ds, dtf, dts)
        t["whole"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        M = A.cost_matrix(f, s, tf, ts)
        t1 = time.perf_counter()
        want = A.dtw(M)[0]
        t2 = time.perf_counter()
        t["np_cost"].append((t1 - t0) * 1e3)
        t["np_dtw"].append((t2 - t1) * 1e3)
        if n == 0:
            t0 = time.perf_counter()
            acc, codes = A.accumulate_loops(M)
            A.backtrace_values(acc)
            t["np_loops"].append((time.perf_counter() - t0) * 1e3)
    same = got.path == want
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"{r} frames x {c} sentences, dim {dim}, features in hand; {args.rounds} alternating rounds",
             f"  sg_align_cost_f64 (one launch)                               median {med['cost'] * 1e3:9.1f} us (min {min(t['cost']) * 1e3:.1f}, max {max(t['cost']) * 1e3:.1f})",
             f"  sg_dtw_path_f64 (one launch, one workgroup)                  median {med['dtw'] * 1e3:9.1f} us (min {min(t['dtw']) * 1e3:.1f}, max {max(t['dtw']) * 1e3:.1f})",
             f"  align_features: both launches + path to the host + grouping  median {med['whole']:9.3f} ms wall",
             f"  NumPy restatement, cost matrix cell by cell                  median {med['np_cost']:9.1f} ms",
             f"  NumPy restatement, recurrence by anti-diagonals + backtrace  median {med['np_dtw']:9.1f} ms",
             f"  NumPy restatement, recurrence and backtrace as double loops  {med['np_loops']:9.1f} ms (once)",
             f"  path of the kernels on the kernel's cost == path of the restatement on its own cost: {same} ({len(want)} entries)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if not same:
        raise SystemExit("bench_align: paths differ")


if __name__ == "__main__":
    main()
