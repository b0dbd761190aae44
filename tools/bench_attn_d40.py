#!/usr/bin/env python
"""In-graph cost of the D = 40 attention launches of the contract step (development tool; conventions of tools/bench_chain.py: a captured
linear chain of identical launches on one stream, replayed, µs per node), the tile loop of attn_d40_body (default) against the shared
loop of attn_fwd_body (option attn_d40_loop = 1) in ONE process, alternating:

    python tools/bench_attn_d40.py [alternations=6] [nodes=20] [replays=20]

Shapes: the main pass's image attention (B3 H8 Nq4096, K/V rows of 4 096 | 12 288 | 12 288 keys: one short row) and the batched reference
pass's self-attention (B20 H8 Nq4096 Nk4096).  Gate of the round-7 issue: new faster than old by more than 3x the spread of old's repeats."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from storygen_amd import ops  # noqa: E402
from bench_chain import chain_us  # noqa: E402

dev = torch.device("cuda:0")
H, D = 8, 40
C = H * D


def rnd(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 1.5).half().to(dev)


def main():
    nums = [int(a) for a in sys.argv[1:]]
    alts, nodes, reps = (nums + [6, 20, 20][len(nums):])[:3]     # one figure = reps replays of the chain (>= 0.1 s of kernel time)
    scale = D ** -0.5
    hw, R = 4096, 3
    q = rnd(3, hw, C, seed=1)
    kflat, vflat = rnd(hw + R * hw, C, seed=2), rnd(hw + R * hw, C, seed=3)
    vt = vflat.t().contiguous()
    k_s, k_l = kflat[:hw].view(1, hw, C), kflat[hw:].view(1, R * hw, C)
    vt_s = vt[:, :hw].unflatten(1, (1, hw)).permute(1, 0, 2)
    vt_l = vt[:, hw:].unflatten(1, (1, R * hw)).permute(1, 0, 2)
    out3 = torch.empty(3, hw, C, dtype=torch.float16, device=dev)
    q20, k20 = rnd(20, hw, C, seed=4), rnd(20, hw, C, seed=5)
    vt20 = rnd(20, hw, C, seed=6).transpose(1, 2).contiguous()
    out20 = torch.empty(20, hw, C, dtype=torch.float16, device=dev)
    shapes = [("B3 H8 Nq4096 Nk12288 (1x Nk4096)", lambda: ops.attention(q, k_l, vt_l, out3, H, scale, short=(k_s, vt_s)), out3),
              ("B20 H8 Nq4096 Nk4096", lambda: ops.attention(q20, k20, vt20, out20, H, scale), out20)]
    print(f"{nodes} dependent launches per captured chain x {reps} replays per figure, {alts} alternations old / new; us per launch")
    ok = True
    for name, fn, out in shapes:
        res, outs = {0: [], 1: []}, {}
        for old in (1, 0):                  # both code objects loaded, clocks settled: not timed
            ops.debug_set_option("attn_d40_loop", old)
            chain_us(fn, nodes=nodes, reps=reps)
        for _ in range(alts):
            for old in (1, 0):
                ops.debug_set_option("attn_d40_loop", old)
                res[old].append(chain_us(fn, nodes=nodes, reps=reps))
                outs[old] = out.clone()
        ops.debug_set_option("attn_d40_loop", 0)
        same = torch.equal(outs[0], outs[1])
        o, n = res[1], res[0]
        spread = max(o) - min(o)
        gain = sum(o) / len(o) - sum(n) / len(n)
        passed = max(n) < min(o) and gain > 3 * spread
        ok = ok and passed and same
        print(f"{name}\n  old " + " ".join(f"{x:7.1f}" for x in o) + f"   mean {sum(o) / len(o):7.1f}  spread {spread:5.1f}")
        print("  new " + " ".join(f"{x:7.1f}" for x in n) + f"   mean {sum(n) / len(n):7.1f}  spread {max(n) - min(n):5.1f}")
        print(f"  gain {gain:6.1f} us = {100 * gain / (sum(o) / len(o)):4.1f} %   3 x spread(old) = {3 * spread:5.1f}   gate {'PASS' if passed else 'FAIL'}"
              f"   outputs bit-identical: {same}", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
