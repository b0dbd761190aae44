"""Records what the host-side planner of gemm_conv.hip decides for a fixed sweep of descriptors and development options:

    python tools/dump_launch_plans.py > tests/golden/launch_plans.json

Host-only (made-up pointers, nothing is launched; runs without a GPU).  tests/test_abi.py re-runs sweep() and compares row by row
with the committed recording, which was made with the library of the commit BEFORE the planner was restructured.

Rows (one dict each; "id" names the inputs):
  GEMM          plan   the six integers of sg_gemm_launch_plan, or [error code, first 40 bytes of sg_last_error()]
                qplan  the same for q = the descriptor with a stats buffer (a launch that cannot deliver statistics fails); omitted
                       where it equals plan
                stats  sg_gemm_stats_tile_rows(q) (0: the launch cannot deliver them), or the error pair
  convolution   plan / qplan / stats likewise, splits = sg_conv3x3_planned_splits asked without and with defer_reduce
  pair          pair   [one launch?, six integers of problem 0, six of problem 1 as launched, paired grid or 0], or the error code

A library that exports sg_gemm_pair_launch_plan answers the pair rows itself.  One that does not (the recording's) has its pair rule
restated here on single-problem queries: sg_gemm_pair_f16 plans both problems as "part of a pair" — development option lat_mask, bit 1 —
which a single-problem query cannot say, so the option is mapped for the duration of the query (_as_in_pair)."""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from storygen_amd import _lib                                         # noqa: E402
from storygen_amd._lib import ConvDesc, GemmDesc                      # noqa: E402

EPI_LINEAR, EPI_GEGLU = 0, 1
BIG_WS = 64 << 20
LAT_MASK_DEFAULT = 62                                                 # storygen_amd/csrc/common.h SgOptions::lat_mask
PIPE_TILES = ((256, 128), (128, 128), (256, 64), (128, 64), (64, 128), (64, 64))
HINTS = ([(0, 0, 0), (0, 0, -1)] + [(bm, bn, w) for bm, bn in PIPE_TILES for w in (0, (bm // 64) * (bn // 64))] +
         [(64, 64, 4), (64, 128, 8), (512, 128, 8), (256, 256, 8), (96, 64, 0), (128, 128, 3)])
OPTION_SETS = ({"no_pipe": 1}, {"no_split": 1}, {"no_nmajor": 1}, {"tile_m": 128, "tile_n": 64}, {"tile_m": 256, "tile_n": 128},
               {"lat_tiles": 0}, {"lat_mask": 63}, {"lat_mask": 0}, {"lat_stages": 8}, {"lat_wide": 1}, {"fat_m": 4096},
               {"big_m": 4096, "big_bm": 128, "big_bn": 64})


def _err(lib, rc):
    return [rc, lib.sg_last_error()[:40].decode(errors="replace")]


def _ws(d, M, N, ws, split, base=0x1000000):
    if ws != "none":
        d.workspace = base
        d.workspace_bytes = BIG_WS if ws == "big" else M * N * 4 * max(split - 1, 0)     # "short": one slice less than the forced split


def gemm_desc(M, N, K, epi=EPI_LINEAR, split=0, ws="big", tile=(0, 0, 0), ln_mode=0, ln_out=False, base=0):
    d = GemmDesc()
    d.A, d.W, d.C = 0x10000 + base, 0x20000 + base, 0x30000 + base
    d.M, d.N, d.K, d.lda, d.ldw, d.ldc, d.epilogue, d.split_k = M, N, K, K, K, N, epi, split
    d.tile_m, d.tile_n, d.tile_waves = tile
    _ws(d, M, N, ws, split, 0x1000000 + base * 0x1000)
    if ln_mode:
        d.ln_mode, d.ln_parts, d.ln_eps = ln_mode, K // 64, 1e-5
        d.ln_stats, d.ln_c, d.ln_d = 0x40000, 0x50000, 0x60000
    if ln_out:
        d.ln_stats_out = 0x70000
    return d


def conv_desc(B, H, W, Cin, Cout, stride=1, ups=0, padded=1, split=0, ws="big", tile=(0, 0, 0), stats=False, defer=0):
    d = ConvDesc()
    d.x, d.w, d.y = 0x10000, 0x20000, 0x30000
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldx, d.ldy = B, H, W, Cin, Cout, Cin, Cout
    d.stride, d.upsample2x, d.x_padded, d.split_k, d.defer_reduce = stride, ups, padded, split, defer
    d.tile_m, d.tile_n, d.tile_waves = tile
    hin, win = H << ups, W << ups
    _ws(d, B * ((hin - 1) // stride + 1) * ((win - 1) // stride + 1), Cout, ws, split)
    if stats:
        d.stats = 0x80000
    return d


def _copy(d):
    return type(d).from_buffer_copy(d)


def _plan(lib, fn, d):
    out = (C.c_int32 * 6)()
    rc = fn(C.byref(d), out)
    return _err(lib, rc) if rc else list(out)


def _rows_or_err(lib, rc):
    return rc if rc >= 0 else _err(lib, rc)


def _row(rid, plan, qplan, stats):
    row = {"id": rid, "plan": plan, "stats": stats}
    if qplan != plan:                       # (written only where the stats buffer changes the answer)
        row["qplan"] = qplan
    return row


def gemm_row(lib, rid, d):
    q = _copy(d)
    q.stats = 0x80000
    q.stats_batch_rows = 256 if d.M % 256 == 0 else 64 if d.M % 64 == 0 else d.M
    return _row(rid, _plan(lib, lib.sg_gemm_launch_plan, d), _plan(lib, lib.sg_gemm_launch_plan, q),
                _rows_or_err(lib, lib.sg_gemm_stats_tile_rows(C.byref(q))))


def conv_row(lib, rid, d):
    q, n, f = _copy(d), _copy(d), _copy(d)
    q.stats = 0x80000
    n.defer_reduce, f.defer_reduce = 0, 1
    row = _row(rid, _plan(lib, lib.sg_conv3x3_launch_plan, d), _plan(lib, lib.sg_conv3x3_launch_plan, q),
               _rows_or_err(lib, lib.sg_conv3x3_stats_tile_rows(C.byref(q))))
    row["splits"] = [_rows_or_err(lib, lib.sg_conv3x3_planned_splits(C.byref(n))), _rows_or_err(lib, lib.sg_conv3x3_planned_splits(C.byref(f)))]
    return row


class _as_in_pair:
    """A single-problem query that plans as sg_gemm_pair_f16 does: there every launch kind is "paired" (lat_mask bit 1; bit 8, K
    slices, is independent of the kind)."""

    def __init__(self, lib, options):
        self.lib, self.mask = lib, options.get("lat_mask", LAT_MASK_DEFAULT)

    def __enter__(self):
        self.lib.sg_debug_set_option(b"lat_mask", (55 if self.mask & 1 else 0) | (self.mask & 8))

    def __exit__(self, *exc):
        self.lib.sg_debug_set_option(b"lat_mask", self.mask)


def _pair_restated(lib, d0, d1, options):
    """sg_gemm_pair_f16's decision, from single-problem plan queries (for a library without sg_gemm_pair_launch_plan)."""
    out = (C.c_int32 * 6)()
    w0, w1 = d0.workspace or 0, d1.workspace or 0
    if w0 and w1 and not (w0 + d0.workspace_bytes <= w1 or w1 + d1.workspace_bytes <= w0):
        return -1                       # the two problems run concurrently and need disjoint workspaces
    with _as_in_pair(lib, options):
        rc = lib.sg_gemm_launch_plan(C.byref(d0), out)
        if rc:
            return rc
        p0 = list(out)
        bm, bn, fam = p0[0], p0[1], p0[5]
        p1 = None
        if fam != 2:                    # (a 128x64-per-wave tile is no hint the second problem can take: two launches)
            q = _copy(d1)
            q.tile_m, q.tile_n, q.tile_waves = bm, bn, ((8 if bn == 128 else 4) if fam >= 16 else 0)
            rc = lib.sg_gemm_launch_plan(C.byref(q), out)
            if rc:
                return rc
            p1 = list(out)
        if p1 and fam and p1[5] and p1[:2] == [bm, bn] and (fam >= 16) == (p1[5] >= 16) and not (fam >= 16 and bn == 128):
            return [1] + p0 + p1 + [((max(p0[3], p1[3]) + 7) & ~7) * 2]
        rc = lib.sg_gemm_launch_plan(C.byref(d1), out)
        if rc:
            return rc
        return [0] + p0 + list(out) + [0]


def pair_row(lib, rid, d0, d1, options):
    if not hasattr(lib, "sg_gemm_pair_launch_plan"):
        return {"id": rid, "pair": _pair_restated(lib, d0, d1, options)}
    out = (C.c_int32 * 14)()
    rc = lib.sg_gemm_pair_launch_plan(C.byref(d0), C.byref(d1), out)
    return {"id": rid, "pair": rc if rc else list(out)}


def _gid(M, N, K, **kw):
    return f"g M{M} N{N} K{K}" + "".join(f" {k}={v}" for k, v in kw.items())


def _gemm_cases():
    """(id, descriptor) of the GEMM sweep."""
    NK = ((72, 72), (320, 136), (320, 320), (640, 320), (1280, 640), (1280, 1280), (2560, 640), (10240, 1280), (640, 2560), (1280, 5120))
    for M in (64, 100, 192, 256, 768, 1000, 4096, 12288, 20480):
        for N, K in NK:
            yield _gid(M, N, K), gemm_desc(M, N, K)
            if N % 64 == 0 and M in (256, 4096):
                yield _gid(M, N, K, epi=1), gemm_desc(M, N, K, epi=EPI_GEGLU)
    for M in (256, 1000, 4096):
        for N, K in ((320, 320), (1280, 640), (2560, 1280)):
            yield _gid(M, N, K, ln=1), gemm_desc(M, N, K, ln_mode=1, split=1)
            yield _gid(M, N, K, ln=1, epi=1), gemm_desc(M, N, K, ln_mode=1, epi=EPI_GEGLU)
            yield _gid(M, N, K, ln=2), gemm_desc(M, N, K, ln_mode=2)
            yield _gid(M, N, K, lnout=1), gemm_desc(M, N, K, ln_out=True)
    for M, N, K in ((256, 1280, 1280), (100, 72, 136), (4096, 320, 320), (64, 640, 5120), (768, 1280, 2560)):
        for split in (0, 1, 3, 7, 64):
            for ws in ("none", "big", "short"):
                yield _gid(M, N, K, split=split, ws=ws), gemm_desc(M, N, K, split=split, ws=ws)
    for M, N, K in ((256, 1280, 1280), (4096, 640, 640), (1000, 320, 136), (12288, 320, 320)):
        for tile in HINTS:
            yield _gid(M, N, K, tile=tile), gemm_desc(M, N, K, tile=tile)
    for tile in HINTS:
        yield _gid(768, 1280, 1280, tile=tile, split=3), gemm_desc(768, 1280, 1280, tile=tile, split=3)
        yield _gid(4096, 1280, 320, tile=tile, epi=1), gemm_desc(4096, 1280, 320, tile=tile, epi=EPI_GEGLU)
    # rejected descriptors
    d = gemm_desc(64, 64, 60); yield "g K%8", d
    d = gemm_desc(64, 64, 64); d.A = 0x10004; yield "g A misaligned", d
    yield "g split 65", gemm_desc(64, 64, 64, split=65)
    yield "g ln split 3", gemm_desc(256, 320, 320, ln_mode=1, split=3)
    yield "g geglu N%64", gemm_desc(256, 72, 320, epi=EPI_GEGLU)
    yield "g ln parts", gemm_desc(256, 320, 2560, ln_mode=1)
    yield "g lnout N%64", gemm_desc(256, 72, 320, ln_out=True)
    d = gemm_desc(64, 64, 64); d.flags = 0x100; yield "g flags", d
    d = gemm_desc(64, 64, 64); d.workspace = 0x1000004; yield "g ws misaligned", d


def _cid(*shape, **kw):
    return "c " + ":".join(str(s) for s in shape) + "".join(f" {k}={v}" for k, v in kw.items())


TUNED_CONVS = ((3, 16, 16, 1280, 1280, 1, 1), (3, 32, 32, 320, 640, 1, 0), (3, 64, 64, 320, 320, 2, 0), (3, 64, 64, 960, 320, 1, 0),
               (4, 64, 64, 960, 320, 1, 0))                              # storygen_amd/tuning/mi355x_tiles.json
SMALL_CONVS = ((3, 8, 8, 1280, 1280, 1, 0), (3, 16, 16, 1280, 1280, 1, 0))


def _conv_cases():
    for s in TUNED_CONVS + SMALL_CONVS + ((3, 16, 16, 1280, 1280, 2, 0), (1, 32, 32, 640, 640, 1, 1), (1, 12, 2, 64, 64, 1, 0), (2, 24, 24, 320, 72, 1, 0)):
        B, H, W, Cin, Cout, stride, ups = s
        for padded in (1, 0):
            for stats in (False, True):
                yield _cid(*s, padded=padded, stats=int(stats)), conv_desc(B, H, W, Cin, Cout, stride, ups, padded, stats=stats)
    for s in SMALL_CONVS:
        B, H, W, Cin, Cout, stride, ups = s
        for split in (0, 1, 3, 7, 64):
            for ws in ("none", "big", "short"):
                for stats in (False, True):
                    yield (_cid(*s, split=split, ws=ws, stats=int(stats)),
                           conv_desc(B, H, W, Cin, Cout, stride, ups, 1, split=split, ws=ws, stats=stats))
    for s in (SMALL_CONVS[1], TUNED_CONVS[3]):
        B, H, W, Cin, Cout, stride, ups = s
        for tile in HINTS:
            yield _cid(*s, tile=tile), conv_desc(B, H, W, Cin, Cout, stride, ups, 1, tile=tile)
            yield _cid(*s, tile=tile, stats=1), conv_desc(B, H, W, Cin, Cout, stride, ups, 1, tile=tile, stats=True)
    yield "c Cin%64", conv_desc(1, 8, 8, 60, 64)
    yield "c stride 3", conv_desc(1, 8, 8, 64, 64, stride=3)
    yield "c ups stride 2", conv_desc(1, 8, 8, 64, 64, stride=2, ups=1)
    yield "c defer stats", conv_desc(1, 8, 8, 64, 64, stats=True, defer=1)
    yield "c padded 2", conv_desc(1, 8, 8, 64, 64, padded=2)
    d = conv_desc(1, 8, 8, 64, 64); d.flags = 0x100; yield "c flags", d
    d = conv_desc(1, 8, 8, 64, 64); d.ldx = 60; yield "c ldx", d


def _pair_cases():
    """(id, d0, d1): the engine's pairs (q|k with V^T, two projections of one operand, a LayerNorm-folded first problem with a
    columns-are-tokens second one) and the ways a pair falls apart (K % 64, a forced split, hints)."""
    shapes = (((4096, 640, 320), (320, 4096, 320)), ((1024, 1280, 640), (640, 1024, 640)), ((256, 2560, 1280), (1280, 256, 1280)),
              ((1024, 640, 640), (1024, 640, 640)), ((232, 640, 768), (640, 232, 768)), ((256, 1280, 2560), (256, 1280, 2560)),
              ((100, 72, 72), (100, 72, 72)), ((1024, 640, 640), (1024, 640, 72)), ((64, 64, 64), (20480, 2560, 640)))
    for (M0, N0, K0), (M1, N1, K1) in shapes:
        rid = f"p {M0}x{N0}x{K0} + {M1}x{N1}x{K1}"
        yield rid, gemm_desc(M0, N0, K0), gemm_desc(M1, N1, K1, base=0x100000)
        if K0 <= 1280 and K0 % 64 == 0 and K0 == K1:
            yield rid + " ln", gemm_desc(M0, N0, K0, ln_mode=1), gemm_desc(M1, N1, K1, ln_mode=2, base=0x100000)
        yield rid + " split 3", gemm_desc(M0, N0, K0, split=3), gemm_desc(M1, N1, K1, split=3, base=0x100000)
        yield rid + " split 0/7 short", gemm_desc(M0, N0, K0), gemm_desc(M1, N1, K1, split=7, ws="short", base=0x100000)
    for tile in HINTS:
        yield f"p tile0={tile}", gemm_desc(1024, 1280, 640, tile=tile), gemm_desc(640, 1024, 640, base=0x100000)
    for tile in ((64, 64, 4), (64, 128, 8), (256, 128, 0), (512, 128, 8)):
        yield f"p tile1={tile}", gemm_desc(1024, 640, 640), gemm_desc(1024, 640, 72, tile=tile, base=0x100000)
    yield "p same workspace", gemm_desc(256, 1280, 1280), gemm_desc(256, 1280, 1280)


def _subsweep(cases, step):
    return [c for i, c in enumerate(cases) if i % step == 0]


def sweep(lib):
    """All rows, in a fixed order: {"options": {...}, "rows": [...]} per option setting (the defaults first, on the whole sweep; each
    development option on every few cases of it)."""
    out = []
    try:
        for options in ({},) + OPTION_SETS:
            for name, value in options.items():
                assert lib.sg_debug_set_option(name.encode(), value) == 0, name
            every = 1 if not options else 11
            rows = [gemm_row(lib, rid, d) for rid, d in _subsweep(list(_gemm_cases()), every)]
            rows += [conv_row(lib, rid, d) for rid, d in _subsweep(list(_conv_cases()), every)]
            rows += [pair_row(lib, rid, d0, d1, options) for rid, d0, d1 in _subsweep(list(_pair_cases()), 1 if not options else 3)]
            out.append({"options": options, "rows": rows})
            assert lib.sg_debug_set_option(b"reset", 0) == 0
        out.append({"options": {"after": "reset"}, "rows": [gemm_row(lib, rid, d) for rid, d in _subsweep(list(_gemm_cases()), 29)]})
    finally:
        lib.sg_debug_set_option(b"reset", 0)
    return out


def main():
    rec = sweep(_lib.load())
    print(f"{sum(len(s['rows']) for s in rec)} rows", file=sys.stderr)
    print("[")
    for i, s in enumerate(rec):
        print(' {"options": ' + json.dumps(s["options"]) + ', "rows": [')
        print(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in s["rows"]))
        print(" ]}" + ("," if i + 1 < len(rec) else ""))
    print("]")


if __name__ == "__main__":
    main()
