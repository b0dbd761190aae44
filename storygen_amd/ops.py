"""Tensor-level wrappers over the C ABI (include/storygen_hip.h).

Each wrapper borrows `data_ptr()`s of caller-owned torch tensors for the duration of the enqueue and launches on
torch's *current* HIP stream, so PyTorch's caching allocator keeps stream ordering and `torch.cuda.graph` capture
just works.  Nothing here computes: no op has a torch fallback, and importing this module without the built
library raises (storygen_amd/_lib.py).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import AttnDesc, AttnPairPlan, AttnPlan, ConvDesc, FfDesc, GemmDesc, GnPlan, GroupNormDesc, check

lib = _lib.load()

EPI_LINEAR = 0
EPI_GEGLU = 1
F_OUT_F32, F_RES1_F32, F_RES2_F32 = 1, 2, 4
EUNSUP = -2           # SG_EUNSUP: a valid request the library has no launch for

# Per-shape tile / split-K choices measured on an MI355X by tools/tune_tiles.py (storygen_amd/tuning/mi355x_tiles.json);
# anything not listed uses the library's cost model.  TUNE_SINK: when set, every gemm/conv3x3 call appends its
# signature and a recipe to rebuild it (the tuning tool's shape census).
TILE_TABLE = {}
TUNE_SINK = None


def _apply_tile(d, tile, split_k, sig, mn):
    """tile = (bm, bn) or (bm, bn, waves) from the caller, else the tuned table entry (bm, bn, split[, waves]).  mn = M * N of the launch:
    a tuned split-K count is taken only when the CALLER's workspace holds its split * M * N fp32 partials — the table is keyed by shape,
    and a caller of the same shape without split-K scratch (the training blocks) keeps the library's own choice for its workspace."""
    if tile is not None:
        d.tile_m, d.tile_n = tile[0], tile[1]
        if len(tile) > 2:
            d.tile_waves = tile[2]
    elif split_k == 0 and sig in TILE_TABLE:
        e = TILE_TABLE[sig]
        d.tile_m, d.tile_n = e[0], e[1]
        d.split_k = e[2] if e[2] <= 1 or d.workspace_bytes >= e[2] * mn * 4 else 0
        if len(e) > 3:
            d.tile_waves = e[3]


def load_tile_table(path: Optional[str] = None) -> int:
    """Loads the per-shape tile table (default: tuning/mi355x_tiles.json); path="none" empties it (heuristic tiles only)."""
    import json
    import os
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning", "mi355x_tiles.json")
    TILE_TABLE.clear()
    if os.path.exists(path) and path != "none":
        with open(path) as f:
            TILE_TABLE.update({k: tuple(v) for k, v in json.load(f)["tiles"].items()})
    return len(TILE_TABLE)


# Optional in-situ kernel timer (bench.py): when set, every MFMA-class launch is bracketed by HIP events recorded
# on the launch stream and reported as (family, algorithmic_flops, start_event, end_event).
PROFILE_SINK = None
LN_GUARD_RANGE, LN_GUARD_OFFSET, LN_GUARD_RATIO = 1, 2, 16.0      # include/storygen_hip.h SG_LN_GUARD_*
# Measurement tooling (bench.py --dump-algorithmic): when a list, every GEMM / convolution launch reports the profiler class it
# will fall into and its ALGORITHMIC bytes: (kernel instantiation as rocprofv3 prints it, grid size in threads, bytes, family, shape)
PLAN_SINK = None
# Same for the bandwidth-bound kernels (tools/profile_step.py): (family, algorithmic_bytes, start, end, shape).
AUX_SINK = None


class _timed:
    __slots__ = ("family", "flops", "start", "shape", "aux")

    def __init__(self, family: str, flops: float, shape: str = "", aux: bool = False):
        self.family, self.flops, self.shape, self.aux = family, flops, shape, aux

    def __enter__(self):
        if (AUX_SINK if self.aux else PROFILE_SINK) is not None:
            self.start = torch.cuda.Event(enable_timing=True)
            self.start.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        sink = AUX_SINK if self.aux else PROFILE_SINK
        if sink is not None and exc[0] is None:
            end = torch.cuda.Event(enable_timing=True)
            end.record(torch.cuda.current_stream())
            sink.append((self.family, self.flops, self.start, end, self.shape))
        return False


load_tile_table()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _f16(t: torch.Tensor, name: str):
    if t.dtype != torch.float16 or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA/HIP float16 tensor, got {t.dtype} on {t.device}")


def _act(t: torch.Tensor, name: str) -> bool:
    """Activation tensors may be fp16 (MFMA operands) or fp32 (residual stream); returns True for fp32."""
    if t.dtype not in (torch.float16, torch.float32) or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA/HIP float16/float32 tensor, got {t.dtype} on {t.device}")
    return t.dtype == torch.float32


def _f32(t: torch.Tensor, name: str):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA/HIP float32 tensor, got {t.dtype} on {t.device}")


def _row_stride(t: torch.Tensor, name: str) -> int:
    """t is [..., rows, cols] with unit column stride; returns the row stride in elements."""
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost dimension must be contiguous")
    return t.stride(-2)


def _view3(t: torch.Tensor) -> tuple:
    """(pointer, token stride, batch stride) of a 3-D view, in the order the C ABI takes them."""
    return t.data_ptr(), t.stride(1), t.stride(0)


def device_arch() -> int:
    return lib.sg_device_arch()


def gemm_workspace_bytes(M: int, N: int, split_k: int = 0) -> int:
    return lib.sg_gemm_workspace_bytes(M, N, split_k)


# Development: when set to an int64 CUDA tensor, gemm() / conv3x3() launch the instrumented mainloop (sg_debug_*_anatomy) and
# the tensor receives 10 cycle counters per wave (tools/anatomy.py).
ANATOMY: Optional[torch.Tensor] = None


def new_workspace(nbytes: int, device) -> torch.Tensor:
    """A split-K workspace for gemm / conv3x3 (fp32 partial tiles; no initialisation needed)."""
    return torch.empty((int(nbytes) + 15) & ~15, dtype=torch.uint8, device=device)


# Split-K scratch of the gemm / conv3x3 calls that do not pass `workspace=` themselves (round 6).  The library splits K only when the caller
# owns scratch for the partial tiles; the training classes (train.py, train_blocks.py: ~50 call sites, ONE stream) had none, so their
# small-M / long-K launches — weight gradients (M = N = 320, K = 12 288 tokens), the 8x8 and 16x16 convolutions at batch 4 — ran 25 - 80
# workgroups down 180-slab chains (110 us where the sampler's batch-3 twin takes 21).  `with ops.default_workspace(ws):` lends them one
# buffer for the duration of a step; only for callers whose launches are ordered on one stream.
DEFAULT_WORKSPACE: Optional[torch.Tensor] = None


class default_workspace:
    def __init__(self, ws: Optional[torch.Tensor]):
        self.ws, self.prev = ws, None

    def __enter__(self):
        global DEFAULT_WORKSPACE
        self.prev, DEFAULT_WORKSPACE = DEFAULT_WORKSPACE, self.ws
        return self.ws

    def __exit__(self, *exc):
        global DEFAULT_WORKSPACE
        DEFAULT_WORKSPACE = self.prev
        return False


def _ws(workspace: Optional[torch.Tensor], d):
    if workspace is None:
        workspace = DEFAULT_WORKSPACE
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()


def _gemm_desc(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, bias: Optional[torch.Tensor] = None,
               rowbias: Optional[torch.Tensor] = None, rows_per_batch: int = 1, res1: Optional[torch.Tensor] = None,
               res2: Optional[torch.Tensor] = None, epilogue: int = EPI_LINEAR, split_k: int = 0,
               workspace: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None,
               tile: Optional[tuple] = None, use_table: bool = True, stats: Optional[tuple] = None,
               ln: Optional[tuple] = None, ln_out: Optional[torch.Tensor] = None, guard: Optional[torch.Tensor] = None):
    """Builds the sg_gemm_desc of one problem; returns (desc, flops, shape string).  stats = (fp32 buffer, rows per image): the
    epilogue also writes the GroupNorm partial statistics of the output (sg_gemm_desc.stats).
    ln = (mode, stats [tokens, K/64 rounded up to even, 2] fp32, c fp32, d fp32, eps): LayerNorm folded into this GEMM (sg_gemm_desc.ln_*: mode 1 =
    the rows of `a` are the normalised tokens, 2 = the rows of `w` are); ln_out = fp32 [M, N/64 rounded up to even, 2]: also write the LayerNorm
    partials of THIS output (sg_gemm_desc.ln_stats_out); guard = int32 [1] CUDA tensor receiving the sticky SG_LN_GUARD_* flags of
    a launch with ln / ln_out (LN_GUARD_RANGE: the raw fp16 copy saturated; LN_GUARD_OFFSET: a token with |mean| / sigma > 16)."""
    _f16(a, "a"), _f16(w, "w")
    flags = F_OUT_F32 if _act(out, "out") else 0
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"gemm: a is [{M},{K}] but w is {tuple(w.shape)}")
    n_out = N // 2 if epilogue == EPI_GEGLU else N
    if tuple(out.shape) != (M, n_out):
        raise ValueError(f"gemm: out must be [{M},{n_out}], got {tuple(out.shape)}")
    d = GemmDesc()
    d.A, d.lda = a.data_ptr(), _row_stride(a, "a")
    d.W, d.ldw = w.data_ptr(), _row_stride(w, "w")
    d.C, d.ldc = out.data_ptr(), _row_stride(out, "out")
    d.M, d.N, d.K = M, N, K
    d.epilogue = epilogue
    d.bias = _p(bias)
    if bias is not None:
        _f16(bias, "bias")
    if rowbias is not None:
        _f32(rowbias, "rowbias")
        d.rowbias, d.rowbias_ld = rowbias.data_ptr(), _row_stride(rowbias, "rowbias")
    d.rows_per_batch = rows_per_batch
    d.split_k = split_k
    if res1 is not None:
        flags |= F_RES1_F32 if _act(res1, "res1") else 0
        d.res1, d.ldr1 = res1.data_ptr(), _row_stride(res1, "res1")
    if res2 is not None:
        flags |= F_RES2_F32 if _act(res2, "res2") else 0
        d.res2, d.ldr2 = res2.data_ptr(), _row_stride(res2, "res2")
    if out2 is not None:
        _f16(out2, "out2")
        d.C2, d.ldc2 = out2.data_ptr(), _row_stride(out2, "out2")
    d.flags = flags
    _ws(workspace, d)
    if stats is not None:
        _f32(stats[0], "stats")
        d.stats, d.stats_batch_rows = stats[0].data_ptr(), int(stats[1])
    if ln is not None:
        mode, lst, lc, ld_, eps = ln
        _f32(lst, "ln stats"), _f32(lc, "ln c"), _f32(ld_, "ln d")
        tokens = M if mode == 1 else N
        if tuple(lst.shape) != (tokens, (K // 64 + 1) & ~1, 2) or not lst.is_contiguous() or lc.numel() != (N if mode == 1 else M) or ld_.numel() != lc.numel():
            raise ValueError(f"gemm: ln operands do not match mode {mode}, {tokens} tokens, K = {K}")
        d.ln_mode, d.ln_parts, d.ln_eps = int(mode), K // 64, float(eps)
        d.ln_stats, d.ln_c, d.ln_d = lst.data_ptr(), lc.data_ptr(), ld_.data_ptr()
    if ln_out is not None:
        _f32(ln_out, "ln_out")
        if ln_out.numel() != M * ((N // 64 + 1) & ~1) * 2 or not ln_out.is_contiguous():
            raise ValueError(f"gemm: ln_out must hold [{M}, {(N // 64 + 1) & ~1}, 2] floats (N / 64 blocks rounded up to even)")
        d.ln_stats_out = ln_out.data_ptr()
    if guard is not None:
        if guard.dtype != torch.int32 or not guard.is_cuda or guard.numel() < 1:
            raise TypeError("gemm: guard must be a CUDA int32 tensor")
        d.ln_guard = guard.data_ptr()
    sig = f"g:{M}:{N}:{K}:{epilogue}:{flags}:{int(bias is not None)}{int(rowbias is not None)}{int(res1 is not None)}{int(res2 is not None)}{int(out2 is not None)}"
    if ln is not None:
        sig += f":ln{ln[0]}"
    if ln_out is not None:
        sig += ":lo"
    if use_table or tile is not None:
        _apply_tile(d, tile, split_k, sig, M * N)
    if TUNE_SINK is not None and use_table:
        TUNE_SINK.append((sig, dict(kind="gemm", M=M, N=N, K=K, epilogue=epilogue, out_f32=bool(flags & F_OUT_F32), bias=bias is not None,
                                    rowbias=rowbias is not None, rows_per_batch=rows_per_batch, out2=out2 is not None,
                                    res1=None if res1 is None else str(res1.dtype), res2=None if res2 is None else str(res2.dtype),
                                    ln=0 if ln is None else int(ln[0]), ln_out=ln_out is not None)))
    return d, 2.0 * M * N * K, f"M{M} N{N} K{K}{' geglu' if epilogue else ''}"


def _gemm_bytes(d) -> float:
    """Algorithmic bytes of one GEMM problem: each operand once (A, W fp16; C fp32 / fp16; residuals; the second fp16 output)."""
    n_out = d.N // 2 if d.epilogue == EPI_GEGLU else d.N
    osz = 4 if d.flags & F_OUT_F32 else 2
    b = 2.0 * d.M * d.K + 2.0 * d.N * d.K + osz * d.M * n_out
    if d.res1:
        b += (4 if d.flags & F_RES1_F32 else 2) * d.M * n_out
    if d.res2:
        b += (4 if d.flags & F_RES2_F32 else 2) * d.M * n_out
    if d.C2:
        b += 2.0 * d.M * n_out
    return b


def _plan_of(fn, d):
    out = (C.c_int32 * 6)()
    check(fn(C.byref(d), out), "launch plan")
    return list(out)


def _kernel_name(bm: int, bn: int, pipe: int, conv: bool) -> str:
    """The instantiation a plan launches, as rocprofv3 prints it (pipe: 0 = register-staged, 1 = LDS-DMA ring of 64x64-per-wave tiles,
    16 + S = the 32x32-per-wave kernel on an S-stage ring)."""
    c = "true" if conv else "false"
    if pipe == 2:
        return f"mma_fat_kernel<{bm // 128}, {bn // 64}, {c}>"
    if pipe >= 16:
        return f"mma_lat_kernel<{bm // 32}, {bn // 32}, {c}, {pipe - 16}>"
    return f"mma_pipe_kernel<{bm // 64}, {bn // 64}, {c}, 3>" if pipe else f"mma_kernel<{bm}, {bn}, {c}>"


def _report_plan(kind: str, d, nbytes: float, family: str, shape: str, second=None):
    """PLAN_SINK record of one launch (see PLAN_SINK).  second = (desc, bytes) of the other problem of a paired launch
    (sg_gemm_pair_launch_plan says whether the two share a launch).  The queries launch nothing and leave the descriptors as they are:
    the instrumented step launches exactly what the uninstrumented one does."""
    if second is not None:
        d1, b1 = second
        out = (C.c_int32 * 14)()
        check(lib.sg_gemm_pair_launch_plan(C.byref(d), C.byref(d1), out), "launch plan")
        (bm, bn, _, wgs, threads, pipe), (bm1, bn1, _, wgs1, threads1, pipe1) = out[1:7], out[7:13]
        if out[0]:
            name = f"mma_lat_pair_kernel<{pipe - 16}>" if pipe >= 16 else f"mma_pipe_pair_kernel<{bm // 64}, {bn // 64}>"
            PLAN_SINK.append((name, out[13] * threads, nbytes + b1, family, shape))
            return
        # not pairable: two plain launches, each on its own plan
        PLAN_SINK.append((_kernel_name(bm1, bn1, pipe1, False), wgs1 * threads1, b1, family, shape + " [2nd]"))
    else:
        bm, bn, _, wgs, threads, pipe = _plan_of(lib.sg_conv3x3_launch_plan if kind == "conv" else lib.sg_gemm_launch_plan, d)
        if kind == "conv" and d.upsample2x == 2:
            PLAN_SINK.append((f"mma_phase_kernel<{bm // 64}, {bn // 64}>", wgs * threads, nbytes, family, shape))
            return
    PLAN_SINK.append((_kernel_name(bm, bn, pipe, kind == "conv"), wgs * threads, nbytes, family, shape))


def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, **kw) -> torch.Tensor:
    """out[M, N'] = epi(a[M,K] @ w[N,K]^T); a/out/res* may be row-strided 2-D views; out/res* fp16 or fp32;
    out2 = optional extra fp16 copy of the result.  Keywords: bias, rowbias, rows_per_batch, res1, res2, epilogue, split_k,
    workspace, out2, tile."""
    d, flops, shape = _gemm_desc(a, w, out, **kw)
    if PLAN_SINK is not None:
        _report_plan("gemm", d, _gemm_bytes(d), "gemm", shape)
    with _timed("gemm", flops, shape):
        if ANATOMY is not None:
            check(lib.sg_debug_gemm_anatomy(C.byref(d), ANATOMY.data_ptr(), ANATOMY.numel() * ANATOMY.element_size(), _stream()),
                  "sg_debug_gemm_anatomy")
        else:
            check(lib.sg_gemm_f16(C.byref(d), _stream()), "sg_gemm_f16")
    return out


def ff_fused_supported(Cc: int) -> bool:
    """Is there a fused GEGLU feed-forward kernel for this width (sg_ff_fused_pack_bytes != 0)?"""
    return lib.sg_ff_fused_pack_bytes(int(Cc)) != 0


def ff_fused(x: torch.Tensor, wpack: torch.Tensor, b2: torch.Tensor, out: torch.Tensor, eps: float = 1e-5, split: bool = False) -> torch.Tensor:
    """out[M, C] (fp16) = Linear2(a * gelu(g)) + b2 + x with [a | g] = Linear1(LayerNorm(x)) + b1 in ONE launch (sg_ff_geglu_fused_f16):
    x fp32 [M, C] (row-strided view allowed), wpack = repack.ff_fused_pack(...) (uint8), b2 fp16 [C].
    split=True (sg_ff_desc.hidden_split): out is [M, 2C] — two workgroups per 128 tokens, each over half of the hidden units; columns
    [0, C) + columns [C, 2C) = the result (the consumer contracts [y_a | y_b] with [W | W]).
    Range: the kernel holds the hidden activation as fp16(a * 2 gelu(g)) (W2 is packed halved) — finite up to |a gelu(g)| = 32752, inf
    from 32760 on, half the range of the two-launch path (gemm with EPI_GEGLU, then gemm); beyond it that token's output row is
    inf / NaN."""
    _f32(x, "x"), _f16(b2, "b2"), _f16(out, "out")
    M, Cc = x.shape
    if tuple(out.shape) != (M, 2 * Cc if split else Cc) or b2.numel() != Cc or wpack.dtype != torch.uint8 or not wpack.is_cuda or not wpack.is_contiguous():
        raise ValueError("ff_fused: out must be [M, C] fp16 ([M, 2C] with split), b2 [C], wpack a contiguous CUDA uint8 tensor")
    d = FfDesc()
    d.x, d.ldx = x.data_ptr(), _row_stride(x, "x")
    d.wpack, d.wpack_bytes = wpack.data_ptr(), wpack.numel()
    d.b2 = b2.data_ptr()
    d.y, d.ldy = out.data_ptr(), _row_stride(out, "out")
    d.M, d.C, d.eps = M, Cc, float(eps)
    d.hidden_split = 2 if split else 0
    with _timed("ff_fused", 24.0 * M * Cc * Cc, f"M{M} C{Cc}" + (" split" if split else "")):
        if ANATOMY is not None:
            check(lib.sg_debug_ff_anatomy(C.byref(d), ANATOMY.data_ptr(), ANATOMY.numel() * ANATOMY.element_size(), _stream()), "sg_debug_ff_anatomy")
        else:
            check(lib.sg_ff_geglu_fused_f16(C.byref(d), _stream()), "sg_ff_geglu_fused_f16")
    return out


def gemm_stats_rows(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, **kw) -> int:
    """Rows per partial (= the tile height) a gemm() call with these arguments (incl. stats=...) will write statistics for, or 0
    when that launch cannot emit them (sg_gemm_stats_tile_rows; no launch happens)."""
    d, _, _ = _gemm_desc(a, w, out, **kw)
    rc = lib.sg_gemm_stats_tile_rows(C.byref(d))
    if rc < 0:
        check(rc, "sg_gemm_stats_tile_rows")
    return rc


def gemm_launch_plan(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, **kw) -> tuple:
    """The decomposition a gemm() call with these arguments will use (sg_gemm_launch_plan; no launch): (tile rows, tile columns, K slices,
    workgroups, threads per workgroup, kernel family: 0 register-staged, 1 LDS-DMA pipeline, 2 fat waves, 16 + ring depth latency kernel)."""
    d, _, _ = _gemm_desc(a, w, out, **kw)
    return tuple(_plan_of(lib.sg_gemm_launch_plan, d))


def gemm_pair(first: tuple, second: tuple) -> None:
    """Two independent GEMMs in one launch (sg_gemm_pair_f16).  Each argument is ((a, w, out), {keywords of gemm()}); the
    outputs must not overlap and the two workspaces, if given, must be different buffers."""
    (a0, kw0), (a1, kw1) = first, second
    d0, f0, s0 = _gemm_desc(*a0, use_table=False, **kw0)
    d1, f1, s1 = _gemm_desc(*a1, use_table=False, **kw1)
    if PLAN_SINK is not None:
        _report_plan("gemm", d0, _gemm_bytes(d0), "gemm", f"{s0} + {s1}", second=(d1, _gemm_bytes(d1)))
    with _timed("gemm", f0 + f1, f"{s0} + {s1}"):
        check(lib.sg_gemm_pair_f16(C.byref(d0), C.byref(d1), _stream()), "sg_gemm_pair_f16")


def gemm_pair_launch_plan(first: tuple, second: tuple) -> tuple:
    """What a gemm_pair() call with these arguments will launch (sg_gemm_pair_launch_plan; no launch): (1 if one launch serves both problems,
    the six integers of gemm_launch_plan for problem 0, for problem 1, workgroups of the shared launch or 0)."""
    (a0, kw0), (a1, kw1) = first, second
    d0, _, _ = _gemm_desc(*a0, use_table=False, **kw0)
    d1, _, _ = _gemm_desc(*a1, use_table=False, **kw1)
    out = (C.c_int32 * 14)()
    check(lib.sg_gemm_pair_launch_plan(C.byref(d0), C.byref(d1), out), "sg_gemm_pair_launch_plan")
    return tuple(out)


def _conv_desc(x: torch.Tensor, w_krsc: torch.Tensor, out: torch.Tensor, *, stride: int = 1, upsample2x: bool = False,
               bias: Optional[torch.Tensor] = None, rowbias: Optional[torch.Tensor] = None,
               res1: Optional[torch.Tensor] = None, split_k: int = 0, workspace: Optional[torch.Tensor] = None,
               x_padded: bool = False, tile: Optional[tuple] = None, stats: Optional[torch.Tensor] = None,
               defer_reduce: bool = False):
    """Builds the sg_conv3x3_desc; returns (desc, flops, shape string)."""
    _f16(x, "x"), _f16(w_krsc, "w")
    flags = F_OUT_F32 if _act(out, "out") else 0
    B, H, W, Cin = x.shape
    if x_padded:
        H, W = H - 2, W - 2
    phases = upsample2x is not True and int(upsample2x) == 2       # the phase form: w is repack.upsample_phase_pack's [4,Cout,2,2,Cin]
    Cout = w_krsc.shape[1 if phases else 0]
    if tuple(w_krsc.shape) != ((4, Cout, 2, 2, Cin) if phases else (Cout, 3, 3, Cin)) or not w_krsc.is_contiguous():
        raise ValueError(f"conv3x3: w must be contiguous {'[4,Cout,2,2,' if phases else '[Cout,3,3,'}{Cin}], got {tuple(w_krsc.shape)}")
    hin, win = (H * 2, W * 2) if upsample2x else (H, W)
    Ho, Wo = (hin - 1) // stride + 1, (win - 1) // stride + 1
    if tuple(out.shape) != (B, Ho, Wo, Cout):
        raise ValueError(f"conv3x3: out must be {(B, Ho, Wo, Cout)}, got {tuple(out.shape)}")

    def pix_stride(t, name):
        if t.stride(-1) != 1 or t.stride(1) != t.shape[2] * t.stride(2) or t.stride(0) != t.shape[1] * t.stride(1):
            raise ValueError(f"{name}: must be [B,H,W,C] with a single pixel stride")
        return t.stride(2)

    d = ConvDesc()
    d.x, d.ldx = x.data_ptr(), pix_stride(x, "x")
    d.w = w_krsc.data_ptr()
    d.y, d.ldy = out.data_ptr(), pix_stride(out, "out")
    d.B, d.H, d.W, d.Cin, d.Cout = B, H, W, Cin, Cout
    d.stride, d.upsample2x, d.x_padded = stride, int(upsample2x), int(x_padded)
    if bias is not None:
        _f16(bias, "bias")
        d.bias = bias.data_ptr()
    if rowbias is not None:
        _f32(rowbias, "rowbias")
        d.rowbias, d.rowbias_ld = rowbias.data_ptr(), _row_stride(rowbias, "rowbias")
    if res1 is not None:
        flags |= F_RES1_F32 if _act(res1, "res1") else 0
        d.res1, d.ldr1 = res1.data_ptr(), pix_stride(res1, "res1")
    d.flags = flags
    d.split_k = split_k
    _ws(workspace, d)
    if stats is not None:
        _f32(stats, "stats")
        d.stats = stats.data_ptr()
    d.defer_reduce = int(bool(defer_reduce))
    sig = f"c:{B}:{H}:{W}:{Cin}:{Cout}:{stride}:{int(upsample2x)}:{int(x_padded)}:{flags}:{int(bias is not None)}{int(rowbias is not None)}{int(res1 is not None)}"
    _apply_tile(d, tile, split_k, sig, B * Ho * Wo * Cout)
    if TUNE_SINK is not None:
        TUNE_SINK.append((sig, dict(kind="conv", B=B, H=H, W=W, Cin=Cin, Cout=Cout, stride=stride, ups=bool(upsample2x), padded=bool(x_padded),
                                    out_f32=bool(flags & F_OUT_F32), bias=bias is not None, rowbias=rowbias is not None,
                                    res1=None if res1 is None else str(res1.dtype))))
    # (the phase form executes 4 of the 9 taps: its FLOPs are reported as executed)
    return d, 2.0 * B * Ho * Wo * Cout * (4 if phases else 9) * Cin, f"B{B} {Ho}x{Wo} {Cin}->{Cout} s{stride}{(' up4' if phases else ' up') if upsample2x else ''}"


def conv3x3(x: torch.Tensor, w_krsc: torch.Tensor, out: torch.Tensor, **kw) -> torch.Tensor:
    """x [B,H,W,Cin] (channels-last, pixel-strided view allowed; or the zero-bordered [B,H+2,W+2,Cin] with
    x_padded=True) -> out [B,Ho,Wo,Cout] (fp16 or fp32); w_krsc [Cout,3,3,Cin]; res1 fp16 or fp32.  Keywords: stride, upsample2x
    (True: nearest 2x folded into the gather; 2: the same result as four 2x2 phase convolutions, w_krsc = repack.upsample_phase_pack's
    [4,Cout,2,2,Cin], x_padded and bias only — sg_conv3x3_desc.upsample2x; conv3x3_upsample picks between the two),
    bias, rowbias, res1, split_k, workspace, x_padded, tile, stats (fp32 buffer: GroupNorm partial statistics of the output),
    defer_reduce (a split-K launch leaves its partial tiles in the workspace for groupnorm(split=...): sg_conv3x3_desc.defer_reduce)."""
    d, flops, shape = _conv_desc(x, w_krsc, out, **kw)
    if PLAN_SINK is not None:
        Ho, Wo = out.shape[1], out.shape[2]
        nb = 2.0 * d.B * d.H * d.W * d.Cin + 2.0 * d.Cout * (16 if d.upsample2x == 2 else 9) * d.Cin + (4 if d.flags & F_OUT_F32 else 2) * d.B * Ho * Wo * d.Cout
        if d.res1:
            nb += (4 if d.flags & F_RES1_F32 else 2) * d.B * Ho * Wo * d.Cout
        _report_plan("conv", d, nb, "conv3x3", shape)
    with _timed("conv3x3", flops, shape):
        if ANATOMY is not None:
            check(lib.sg_debug_conv_anatomy(C.byref(d), ANATOMY.data_ptr(), ANATOMY.numel() * ANATOMY.element_size(), _stream()),
                  "sg_debug_conv_anatomy")
        else:
            check(lib.sg_conv3x3_nhwc_f16(C.byref(d), _stream()), "sg_conv3x3_nhwc_f16")
    return out


def conv3x3_phases_fit(x: torch.Tensor, w_phases: torch.Tensor, out: torch.Tensor, **kw) -> bool:
    """Does the phase form (upsample2x=2) have a launch for these arguments?  (sg_conv3x3_launch_plan; no launch.)  False when no row tile
    of the LDS-DMA kernels divides the H W pixels of the input (SG_EUNSUP); an invalid descriptor raises as conv3x3 would."""
    d, _, _ = _conv_desc(x, w_phases, out, **{**kw, "upsample2x": 2})
    rc = lib.sg_conv3x3_launch_plan(C.byref(d), (C.c_int32 * 6)())
    if rc == EUNSUP:
        return False
    check(rc, "sg_conv3x3_launch_plan")
    return True


def conv3x3_upsample(x: torch.Tensor, w_krsc: torch.Tensor, w_phases: torch.Tensor, out: torch.Tensor, **kw) -> torch.Tensor:
    """Nearest-2x upsampling + 3x3 convolution of the zero-bordered x: the phase form on w_phases (repack.upsample_phase_pack) where it has a
    launch, else conv3x3(..., upsample2x=True) on w_krsc.  Keywords as conv3x3 (no stride / upsample2x)."""
    if conv3x3_phases_fit(x, w_phases, out, **kw):
        return conv3x3(x, w_phases, out, upsample2x=2, **kw)
    return conv3x3(x, w_krsc, out, upsample2x=True, **kw)


def conv3x3_planned_splits(x: torch.Tensor, w_krsc: torch.Tensor, out: torch.Tensor, **kw) -> int:
    """Number of K slices a conv3x3() call with these arguments will use (sg_conv3x3_planned_splits; no launch).  > 1: the call may
    pass defer_reduce=True and hand its workspace to groupnorm(split=...)."""
    d, _, _ = _conv_desc(x, w_krsc, out, **kw)
    rc = lib.sg_conv3x3_planned_splits(C.byref(d))
    if rc < 0:
        check(rc, "sg_conv3x3_planned_splits")
    return rc


def conv3x3_launch_plan(x: torch.Tensor, w_krsc: torch.Tensor, out: torch.Tensor, **kw) -> tuple:
    """The decomposition a conv3x3() call with these arguments will use (sg_conv3x3_launch_plan; no launch): as gemm_launch_plan."""
    d, _, _ = _conv_desc(x, w_krsc, out, **kw)
    return tuple(_plan_of(lib.sg_conv3x3_launch_plan, d))


def conv3x3_stats_rows(x: torch.Tensor, w_krsc: torch.Tensor, out: torch.Tensor, **kw) -> int:
    """Rows per partial a conv3x3() call with these arguments (incl. stats=...) will write statistics for, or 0 (no launch)."""
    d, _, _ = _conv_desc(x, w_krsc, out, **kw)
    rc = lib.sg_conv3x3_stats_tile_rows(C.byref(d))
    if rc < 0:
        check(rc, "sg_conv3x3_stats_tile_rows")
    return rc


def conv_in(x_nchw: torch.Tensor, w_kn: torch.Tensor, bias: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    _f32(x_nchw, "x"), _f16(w_kn, "w"), _f16(bias, "bias")
    y_f32 = _act(out, "out")
    B, Cin, H, W = x_nchw.shape
    Cout = w_kn.shape[1]
    if not x_nchw.is_contiguous() or tuple(w_kn.shape) != (9 * Cin, Cout) or tuple(out.shape) != (B, H, W, Cout):
        raise ValueError("conv_in: bad shapes")
    check(lib.sg_conv_in_f16(x_nchw.data_ptr(), w_kn.data_ptr(), bias.data_ptr(), out.data_ptr(), out.stride(2), int(y_f32),
                             B, H, W, Cin, Cout, _stream()), "sg_conv_in_f16")
    return out


def conv_out(x: torch.Tensor, w_krsc: torch.Tensor, bias: torch.Tensor, out_nchw: torch.Tensor) -> torch.Tensor:
    _f16(x, "x"), _f16(w_krsc, "w"), _f16(bias, "bias"), _f32(out_nchw, "out")
    B, H, W, Cin = x.shape
    Cout = w_krsc.shape[0]
    if tuple(out_nchw.shape) != (B, Cout, H, W) or not out_nchw.is_contiguous() or not w_krsc.is_contiguous():
        raise ValueError("conv_out: bad shapes")
    check(lib.sg_conv_out_f16(x.data_ptr(), x.stride(2), w_krsc.data_ptr(), bias.data_ptr(), out_nchw.data_ptr(), B, H, W,
                              Cin, Cout, _stream()), "sg_conv_out_f16")
    return out_nchw


def _attn_fwd_desc(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, heads: int, scale: float, nk: Optional[int],
                   short: Optional[tuple] = None):
    for n, t in (("q", q), ("k", k), ("vt", vt), ("out", out)):
        _f16(t, n)
        if t.dim() != 3 or t.stride(-1) != 1:
            raise ValueError(f"attention: {n} must be 3-D with a contiguous last dimension")
    B, Nq, Cq = q.shape
    Bk = k.shape[0]
    Nk = k.shape[1] if nk is None else nk
    D = Cq // heads
    if vt.shape[0] != Bk or vt.shape[1] != Cq or k.shape[2] != Cq or Nk > k.shape[1] or vt.shape[2] < ((Nk + 7) & ~7):
        raise ValueError(f"attention: k {tuple(k.shape)} / vt {tuple(vt.shape)} do not match q {tuple(q.shape)}, nk={Nk}")
    d = AttnDesc()
    d.q, d.ldq, d.bsq = q.data_ptr(), q.stride(1), q.stride(0)
    d.k, d.ldk, d.bsk = k.data_ptr(), k.stride(1), k.stride(0)
    d.vt, d.ldvt, d.bsvt = vt.data_ptr(), vt.stride(1), vt.stride(0)
    d.o, d.ldo, d.bso = out.data_ptr(), out.stride(1), out.stride(0)
    d.B, d.H, d.Nq, d.Nk, d.D = B, heads, Nq, Nk, D
    d.kv_batches = Bk
    d.scale = scale
    keys = [Nk] * B
    if short is not None:          # leading K/V rows with their own key count (sg_attn_desc.k2 ...)
        k2, vt2 = short
        _f16(k2, "k2"), _f16(vt2, "vt2")
        n2, Nk2 = k2.shape[0], k2.shape[1]
        if (k2.dim() != 3 or vt2.dim() != 3 or k2.shape[2] != Cq or tuple(vt2.shape[:2]) != (n2, Cq) or vt2.shape[2] < ((Nk2 + 7) & ~7)
                or k2.stride(-1) != 1 or vt2.stride(-1) != 1 or k2.stride(1) != k.stride(1) or vt2.stride(1) != vt.stride(1)):
            raise ValueError("attention: short rows must be [n, Nk2, H*D] / [n, H*D, Nk2] views with the token / row strides of k / vt")
        d.k2, d.bsk2, d.vt2, d.bsvt2 = k2.data_ptr(), k2.stride(0), vt2.data_ptr(), vt2.stride(0)
        d.Nk2, d.kv2_batches = Nk2, n2
        d.kv_batches = Bk = Bk + n2
        keys = [Nk2 if (b if b < Bk else b - (B - Bk)) < n2 else Nk for b in range(B)]
    if d.kv_batches > B:
        raise ValueError(f"attention: {d.kv_batches} K/V rows for {B} query batches")
    shape = f"B{B} H{heads} Nq{Nq} Nk{Nk}" + (f" ({d.kv2_batches}x Nk{d.Nk2})" if short is not None else "")
    return d, 4.0 * heads * Nq * D * float(sum(keys)), shape


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, heads: int, scale: float,
              nk: Optional[int] = None, short: Optional[tuple] = None) -> torch.Tensor:
    """q [B,Nq,H*D], k [Bk,Nk',H*D] (token- and batch-strided views allowed), vt [Bk,H*D,Nk''] = V transposed (keys
    contiguous; rows finite up to nk rounded up to 8), out [B,Nq,H*D].  nk = number of valid keys (default k.shape[1]).
    Bk < B: query batch b uses K/V batch (b if b < Bk else b - (B - Bk)).
    short = (k2 [n, Nk2, H*D], vt2 [n, H*D, Nk2]): n more K/V rows IN FRONT of k's, with Nk2 keys each (all of them valid)."""
    d, flops, shape = _attn_fwd_desc(q, k, vt, out, heads, scale, nk, short)
    with _timed(f"attention_d{d.D}", flops, shape):
        check(lib.sg_attn_fwd_f16(C.byref(d), _stream()), "sg_attn_fwd_f16")
    return out


def attention_pair(a: tuple, b: tuple, heads: int, scale: float) -> None:
    """Two attentions of the same query geometry in one launch (sg_attn_fwd_pair_f16): a, b = (q, k, vt, out, nk[, short]) as in
    attention() — the text and the image cross-attention of one transformer block (attention.py:271-276,285-290)."""
    da, fa, sa = _attn_fwd_desc(*a[:4], heads, scale, *a[4:])
    db, fb, sb = _attn_fwd_desc(*b[:4], heads, scale, *b[4:])
    with _timed(f"attention_d{da.D}", fa + fb, f"{sa} + {sb}"):
        check(lib.sg_attn_fwd_pair_f16(C.byref(da), C.byref(db), _stream()), "sg_attn_fwd_pair_f16")


# kernel families of a forward-attention plan (SG_ATTN_* of include/storygen_hip.h, in that order)
ATTN_FAMILIES = ("d40_loop", "shared_body", "general", "lean", "ksplit", "lse", "f8")


def _attn_plan_tuple(pl) -> tuple:
    return (ATTN_FAMILIES[pl.family], pl.waves, pl.stages, pl.workgroups)


def attention_plan(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, heads: int, scale: float,
                   nk: Optional[int] = None, short: Optional[tuple] = None, lse: bool = False) -> tuple:
    """The launch an attention() call (lse=True: attention_lse()) with these arguments gets (sg_attn_fwd_plan; no launch):
    (family, waves per workgroup, ring stages, workgroups), family one of ATTN_FAMILIES."""
    d, _, _ = _attn_fwd_desc(q, k, vt, out, heads, scale, nk, short)
    pl = AttnPlan()
    check(lib.sg_attn_fwd_plan(C.byref(d), int(lse), C.byref(pl)), "sg_attn_fwd_plan")
    return _attn_plan_tuple(pl)


def attention_pair_plan(a: tuple, b: tuple, heads: int, scale: float) -> tuple:
    """The launch(es) an attention_pair() call with these arguments gets (sg_attn_fwd_pair_plan; no launch): (one grid serves both,
    index of the problem numbered first in it, plan of a, plan of b, workgroups of the shared grid or 0)."""
    da, _, _ = _attn_fwd_desc(*a[:4], heads, scale, *a[4:])
    db, _, _ = _attn_fwd_desc(*b[:4], heads, scale, *b[4:])
    pr = AttnPairPlan()
    check(lib.sg_attn_fwd_pair_plan(C.byref(da), C.byref(db), C.byref(pr)), "sg_attn_fwd_pair_plan")
    return (bool(pr.shared), pr.first, _attn_plan_tuple(pr.p0), _attn_plan_tuple(pr.p1), pr.workgroups)


def attention_f8_plan(B: int, heads: int, Nq: int) -> tuple:
    """The launch shape attention_f8() uses for these queries (sg_attn_fwd_f8_plan; no launch): as attention_plan."""
    pl = AttnPlan()
    check(lib.sg_attn_fwd_f8_plan(B, heads, Nq, C.byref(pl)), "sg_attn_fwd_f8_plan")
    return _attn_plan_tuple(pl)


def attention_f8_bytes(B: int, heads: int, N: int, transposed: bool) -> int:
    return lib.sg_attn_f8_bytes(B, heads, N, int(transposed))


def attention_f8(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, heads: int, scale: float,
                 scratch: torch.Tensor, nk: Optional[int] = None) -> torch.Tensor:
    """`attention` for head dim 40 on the fp8 (e4m3) MFMA path: packs q / k / vt (same operands and layouts as attention()) into
    e4m3 images inside `scratch` (uint8, >= the three attention_f8_bytes) and runs sg_attn_fwd_f8_d40."""
    for n, t in (("q", q), ("k", k), ("vt", vt), ("out", out)):
        _f16(t, n)
        if t.dim() != 3 or t.stride(-1) != 1:
            raise ValueError(f"attention_f8: {n} must be 3-D with a contiguous last dimension")
    B, Nq, Cq = q.shape
    Bk = k.shape[0]
    Nk = k.shape[1] if nk is None else nk
    if Cq != heads * 40:
        raise ValueError("attention_f8: head dim must be 40")
    if vt.shape[0] != Bk or vt.shape[1] != Cq or k.shape[2] != Cq or Nk > k.shape[1] or vt.shape[2] < ((Nk + 7) & ~7):
        raise ValueError(f"attention_f8: k {tuple(k.shape)} / vt {tuple(vt.shape)} do not match q {tuple(q.shape)}, nk={Nk}")
    nq8, nk8, nv8 = attention_f8_bytes(B, heads, Nq, False), attention_f8_bytes(Bk, heads, Nk, False), attention_f8_bytes(Bk, heads, Nk, True)
    if scratch.dtype != torch.uint8 or not scratch.is_cuda or scratch.numel() < nq8 + nk8 + nv8 + 512:
        raise ValueError(f"attention_f8: scratch must be a CUDA uint8 tensor of at least {nq8 + nk8 + nv8 + 512} bytes")
    base = (scratch.data_ptr() + 255) & ~255
    q8, k8, v8 = base, base + ((nq8 + 255) & ~255), base + ((nq8 + 255) & ~255) + ((nk8 + 255) & ~255)
    if v8 + nv8 > scratch.data_ptr() + scratch.numel():
        raise ValueError("attention_f8: scratch too small after alignment")
    st = _stream()
    check(lib.sg_attn_f8_pack(*_view3(q), q8, B, heads, Nq, 0, st), "sg_attn_f8_pack(q)")
    check(lib.sg_attn_f8_pack(*_view3(k), k8, Bk, heads, Nk, 0, st), "sg_attn_f8_pack(k)")
    check(lib.sg_attn_f8_pack(*_view3(vt), v8, Bk, heads, Nk, 1, st), "sg_attn_f8_pack(vt)")
    with _timed("attention_f8_d40", 4.0 * B * heads * Nq * Nk * 40, f"B{B} H{heads} Nq{Nq} Nk{Nk}"):
        check(lib.sg_attn_fwd_f8_d40(q8, k8, v8, *_view3(out), B, heads, Nq, Nk, Bk, scale, st), "sg_attn_fwd_f8_d40")
    return out


def softmax_rows(scores: torch.Tensor, probs: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """probs[m, :N] = softmax(scale * scores[m, :N]) (fp32 -> fp16); probs has N rounded up to 8 columns, the extra ones zeroed."""
    _f32(scores, "scores"), _f16(probs, "probs")
    M, N = scores.shape
    if probs.shape[0] != M or probs.shape[1] != ((N + 7) & ~7):
        raise ValueError(f"softmax_rows: probs must be [{M},{(N + 7) & ~7}], got {tuple(probs.shape)}")
    with _timed("softmax", M * N * 6.0, f"M{M} N{N}", aux=True):
        check(lib.sg_softmax_rows_f16(scores.data_ptr(), _row_stride(scores, "scores"), probs.data_ptr(), _row_stride(probs, "probs"), M, N,
                                      float(scale), _stream()), "sg_softmax_rows_f16")
    return probs


def _attention_qkv(fn, who: str, q, k, v, out, heads, scale, causal, key_bias):
    """The body of attention_small / attention_enc: `fn` is the library's entry point, `who` the wrapper's name."""
    for n, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        _f16(t, n)
        if t.dim() != 3 or t.stride(-1) != 1 or t.shape != q.shape:
            raise ValueError(f"{who}: {n} must be [B,T,H*D] with a contiguous last dimension")
    B, T, Cq = q.shape
    if heads <= 0 or Cq % heads:
        raise ValueError(f"{who}: {Cq} channels do not split into {heads} heads")
    if key_bias is not None:
        _f32(key_bias, "key_bias")
        if tuple(key_bias.shape) != (B, T) or not key_bias.is_contiguous():
            raise ValueError(f"{who}: key_bias must be a contiguous [B,T] tensor")
    check(fn(*_view3(q), *_view3(k), *_view3(v), *_view3(out), _p(key_bias), B, heads, T, Cq // heads, float(scale), int(causal), _stream()),
          fn.__name__)
    return out


def attention_small(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int, scale: float, causal: bool,
                    key_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Short-sequence attention (T <= 128, head dim <= 64), q/k/v/out [B,T,H*D] token-/batch-strided fp16 views, V not transposed;
    key_bias = optional fp32 [B,T] additive term (padding mask)."""
    return _attention_qkv(lib.sg_attn_small_f16, "attention_small", q, k, v, out, heads, scale, causal, key_bias)


def attention_enc(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, heads: int, scale: float, causal: bool,
                  key_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Encoder-class attention on the matrix cores (1 <= T <= 1024, head dim a multiple of 8 up to 128: CLIP ViT-H/14), the contract of
    attention_small: q/k/v/out [B,T,H*D] token-/batch-strided fp16 views, V not transposed; key_bias = optional fp32 [B,T] additive term."""
    return _attention_qkv(lib.sg_attn_enc_f16, "attention_enc", q, k, v, out, heads, scale, causal, key_bias)


ACT_QUICK_GELU, ACT_GELU = 0, 1


def act_rows(x: torch.Tensor, act: int) -> torch.Tensor:
    """In-place quick_gelu / gelu over a row-strided fp16 [M,N] view."""
    _f16(x, "x")
    check(lib.sg_act_rows_f16(x.data_ptr(), _row_stride(x, "x"), x.shape[0], x.shape[1], act, _stream()), "sg_act_rows_f16")
    return x


def embed_tokens(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, out: torch.Tensor, T: int) -> torch.Tensor:
    """out[r] = tok[ids[r]] + pos[r % T]; ids int64 [rows] (already validated against the vocabulary), fp32 tables / output."""
    _f32(tok, "tok"), _f32(pos, "pos"), _f32(out, "out")
    if ids.dtype != torch.int64 or not ids.is_cuda or not ids.is_contiguous() or ids.numel() != out.shape[0]:
        raise ValueError("embed_tokens: ids must be a contiguous CUDA int64 tensor with one id per output row")
    if not tok.is_contiguous() or not pos.is_contiguous() or tok.shape[1] != out.shape[1] or pos.shape[1] != out.shape[1] or pos.shape[0] < T:
        raise ValueError("embed_tokens: table shapes do not match the output")
    check(lib.sg_embed_tokens_f32(ids.data_ptr(), tok.data_ptr(), pos.data_ptr(), out.data_ptr(), _row_stride(out, "out"), out.shape[0], T,
                                  out.shape[1], _stream()), "sg_embed_tokens_f32")
    return out


def gaussian_sample(mean: torch.Tensor, logvar: Optional[torch.Tensor], noise: Optional[torch.Tensor], out: torch.Tensor,
                    scale: float = 1.0) -> torch.Tensor:
    """out = (mean + exp(0.5 clamp(logvar, -30, 20)) * noise) * scale; noise None -> mean * scale.  Contiguous fp32 tensors."""
    for n, t in (("mean", mean), ("logvar", logvar), ("noise", noise), ("out", out)):
        if t is not None:
            _f32(t, n)
            if not t.is_contiguous() or t.numel() != mean.numel():
                raise ValueError(f"gaussian_sample: {n} must be contiguous with {mean.numel()} elements")
    check(lib.sg_gaussian_sample_f32(mean.data_ptr(), _p(logvar), _p(noise), out.data_ptr(), float(scale), mean.numel(), _stream()),
          "sg_gaussian_sample_f32")
    return out


def clip_resize_geometry(H: int, W: int, S: int) -> tuple:
    """(resized H, resized W, top, left) of torchvision's Resize(S) + CenterCrop(S) on an H x W image (sg_clip_resize_geometry; host only)."""
    g = (C.c_int32 * 4)()
    check(lib.sg_clip_resize_geometry(int(H), int(W), int(S), g), "sg_clip_resize_geometry")
    return tuple(g)


def clip_patchify(x: torch.Tensor, out: torch.Tensor, S: int, ps: int, mean, std, in_scale: float = 1.0, in_shift: float = 0.0,
                  kpad: Optional[int] = None) -> torch.Tensor:
    """x fp32 NCHW [B,3,H,W] -> out fp16 [B * (S/ps)^2, 3*ps*ps]: (in_scale * x + in_shift) resized (antialiased bicubic) so that the shorter
    side is S, centre-cropped to S x S, normalised with the per-channel mean / std (3 floats each) and cut into patches, columns (c, dy, dx).
    kpad (a multiple of 8, >= 3*ps*ps): out is [rows, >= kpad] and columns [3*ps*ps, kpad) are written as zeros (sg_clip_patchify_padk_f16:
    patch size 14); columns beyond kpad are left alone."""
    _f32(x, "x"), _f16(out, "out")
    if x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
        raise ValueError(f"clip_patchify: x must be a contiguous [B,3,H,W] tensor, got {tuple(x.shape)}")
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("clip_patchify: mean and std hold one value per channel")
    B, _, H, W = x.shape
    if S <= 0 or ps <= 0 or S % ps:
        raise ValueError(f"clip_patchify: crop size {S} is not a multiple of patch size {ps}")
    m, s = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    if kpad is not None:
        if out.dim() != 2 or out.shape[0] != B * (S // ps) ** 2 or out.shape[1] < kpad:
            raise ValueError(f"clip_patchify: out must be [{B * (S // ps) ** 2}, >= {kpad}], got {tuple(out.shape)}")
        check(lib.sg_clip_patchify_padk_f16(x.data_ptr(), B, H, W, float(in_scale), float(in_shift), m, s, int(S), int(ps), int(kpad),
                                            out.data_ptr(), _row_stride(out, "out"), _stream()), "sg_clip_patchify_padk_f16")
        return out
    if out.dim() != 2 or tuple(out.shape) != (B * (S // ps) ** 2, 3 * ps * ps):
        raise ValueError(f"clip_patchify: out must be [{B * (S // ps) ** 2},{3 * ps * ps}], got {tuple(out.shape)}")
    check(lib.sg_clip_patchify_f16(x.data_ptr(), B, H, W, float(in_scale), float(in_shift), m, s, int(S), int(ps), out.data_ptr(),
                                   _row_stride(out, "out"), _stream()), "sg_clip_patchify_f16")
    return out


def clip_embed_patches(patches: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, out: torch.Tensor, T: int) -> torch.Tensor:
    """out[b*T] = cls + pos[0]; out[b*T + t] = patches[b*(T-1) + t-1] + pos[t] (fp32): CLIPVisionEmbeddings on the residual stream."""
    _f32(patches, "patches"), _f32(cls, "cls"), _f32(pos, "pos"), _f32(out, "out")
    Cc = out.shape[1]
    if out.shape[0] % T or patches.shape[0] != out.shape[0] // T * (T - 1) or patches.shape[1] != Cc:
        raise ValueError("clip_embed_patches: patches must hold T - 1 rows for every T rows of out")
    if not cls.is_contiguous() or not pos.is_contiguous() or cls.numel() != Cc or tuple(pos.shape) != (T, Cc):
        raise ValueError("clip_embed_patches: cls must be [C] and pos [T,C]")
    check(lib.sg_clip_embed_patches_f32(patches.data_ptr(), _row_stride(patches, "patches"), cls.data_ptr(), pos.data_ptr(), out.data_ptr(),
                                        _row_stride(out, "out"), out.shape[0] // T, T, Cc, _stream()), "sg_clip_embed_patches_f32")
    return out


def groupnorm_workspace_bytes(B: int, groups: int) -> int:
    return lib.sg_groupnorm_workspace_bytes(B, groups)


# forward GroupNorm variants of a plan (SG_GN_* of include/storygen_hip.h, in that order)
GN_VARIANTS = ("narrow", "wide", "one_launch")


def groupnorm_plan(HW: int, Cc: int, groups: int, B: int = 1, x_f32: bool = False, pstats: bool = False, splits: int = 0) -> tuple:
    """The launch a groupnorm() call of this shape gets (sg_groupnorm_plan; no launch): (variant, threads per workgroup, launches, chunks
    and rows per chunk of the statistics pass, workgroups and rows per workgroup of the narrow apply pass), variant one of GN_VARIANTS.
    pstats: producer statistics are supplied; splits: K slices of a split=... input (refused unless the variant is "one_launch")."""
    pl = GnPlan()       # passed as it is (ctypes takes its address): cheaper than C.byref, and the engine asks on every forward
    check(lib.sg_groupnorm_plan(B, HW, Cc, groups, x_f32, pstats, splits, pl), "sg_groupnorm_plan")
    return (GN_VARIANTS[pl.variant], pl.threads, pl.launches, pl.chunks, pl.rows_per_chunk, pl.apply_blocks, pl.apply_rows)


def groupnorm_uses_pstats(HW: int, Cc: int, groups: int) -> bool:
    """True when a GroupNorm of this shape consumes producer statistics (the two-launch wide variant)."""
    return groupnorm_plan(HW, Cc, groups)[0] == "wide"


def groupnorm_is_fused(HW: int, Cc: int, groups: int) -> bool:
    """True when a GroupNorm of this shape runs as the one-launch kernel (the only variant that takes split=...)."""
    return groupnorm_plan(HW, Cc, groups)[0] == "one_launch"


def groupnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: torch.Tensor, groups: int, eps: float,
              silu: bool, workspace: torch.Tensor, xcopy: Optional[torch.Tensor] = None, pstats: Optional[list] = None,
              split: Optional[dict] = None) -> torch.Tensor:
    """x [B, HW, C] channels-last fp16/fp32 (row-strided views allowed).  out is either [B, HW, C] fp16 or the
    zero-bordered image [B, H+2, W+2, C] (then only the interior is written); xcopy = optional fp16 [B, HW, C] raw copy.
    pstats = [(buffer, rows per partial, channels), ...] (one or two sources, in channel order): statistics written by the
    producers' epilogues (gemm / conv3x3 stats=...) — the wide variant then skips its own statistics pass.
    split = dict(ws=workspace of a conv3x3(defer_reduce=True) launch, splits=its K slices, bias=, rowbias= [B, >= C] fp32, res1= [B, HW, C]
    fp16 / fp32, store=bool): x is that launch's UNREDUCED output — the kernel sums the slices and applies bias / rowbias / res1 while it
    loads (sg_groupnorm_desc.split_*); `x` itself is then only the destination of the reduced tensor, written when store=True (its dtype
    also says whether the normalisation sees fp16-rounded values)."""
    x_f32 = _act(x, "x")
    _f16(gamma, "gamma"), _f16(beta, "beta"), _f16(out, "out")
    B, HW, Cc = x.shape
    if x.stride(0) != HW * x.stride(1):
        raise ValueError("groupnorm: batch stride of x must equal HW * row stride")
    d = GroupNormDesc()
    d.x, d.ldx, d.x_f32 = x.data_ptr(), x.stride(1), int(x_f32)
    if out.dim() == 4:
        Hp, Wp = out.shape[1], out.shape[2]
        if (Hp - 2) * (Wp - 2) != HW or out.stride(1) != Wp * out.stride(2) or out.stride(0) != Hp * out.stride(1):
            raise ValueError("groupnorm: padded output must be a dense [B, H+2, W+2, C] image")
        d.y, d.ldy, d.y_pad_w = out.data_ptr(), out.stride(2), Wp - 2
    else:
        if out.stride(0) != HW * out.stride(1):
            raise ValueError("groupnorm: batch stride of out must equal HW * row stride")
        d.y, d.ldy, d.y_pad_w = out.data_ptr(), out.stride(1), 0
    if xcopy is not None:
        _f16(xcopy, "xcopy")
        if xcopy.stride(0) != HW * xcopy.stride(1):
            raise ValueError("groupnorm: batch stride of xcopy must equal HW * row stride")
        d.xcopy, d.ldxc = xcopy.data_ptr(), xcopy.stride(1)
    d.gamma, d.beta = gamma.data_ptr(), beta.data_ptr()
    d.B, d.HW, d.C, d.groups, d.eps, d.silu = B, HW, Cc, groups, eps, int(silu)
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if pstats:
        c0 = 0
        for i, (buf, rows, nc) in enumerate(pstats):
            _f32(buf, "pstats")
            d.pstats[i], d.pstats_rows[i], d.pstats_c0[i], d.pstats_nc[i] = buf.data_ptr(), int(rows), c0, int(nc)
            c0 += int(nc)
    nbytes = B * HW * Cc * ((4 if x_f32 else 2) + 2 + (2 if xcopy is not None else 0))
    shape = f"B{B} HW{HW} C{Cc}"
    if split is not None:
        ws, ns = split["ws"], int(split["splits"])
        if ws.numel() * ws.element_size() < ns * B * HW * Cc * 4:
            raise ValueError("groupnorm: split workspace smaller than splits * B * HW * C floats")
        d.split_ws, d.split_count = ws.data_ptr(), ns
        if split.get("bias") is not None:
            _f16(split["bias"], "split bias")
            d.split_bias = split["bias"].data_ptr()
        if split.get("rowbias") is not None:
            _f32(split["rowbias"], "split rowbias")
            d.split_rowbias, d.split_rowbias_ld = split["rowbias"].data_ptr(), _row_stride(split["rowbias"], "split rowbias")
        r = split.get("res1")
        if r is not None:
            if tuple(r.shape) != (B, HW, Cc) or r.stride(0) != HW * r.stride(1) or r.stride(2) != 1:
                raise ValueError("groupnorm: split res1 must be a [B, HW, C] view with one row stride")
            d.split_res, d.split_ldr, d.split_res_f32 = r.data_ptr(), r.stride(1), int(_act(r, "split res1"))
        if split.get("store"):
            d.split_out, d.split_ldo, d.split_out_f32 = x.data_ptr(), x.stride(1), int(x_f32)
        d.split_round_f16 = int(not x_f32)
        nbytes = B * HW * Cc * (4 * ns + 2 + (4 if r is not None and r.dtype == torch.float32 else 0) + ((4 if x_f32 else 2) if split.get("store") else 0))
        shape += f" split{ns}"
    with _timed("groupnorm", nbytes, shape, aux=True):
        check(lib.sg_groupnorm_nhwc_f16(C.byref(d), _stream()), "sg_groupnorm_nhwc_f16")
    return out


def layernorm(x: torch.Tensor, g1: torch.Tensor, b1: torch.Tensor, y1: torch.Tensor, eps: float = 1e-5,
              g2: Optional[torch.Tensor] = None, b2: Optional[torch.Tensor] = None,
              y2: Optional[torch.Tensor] = None) -> None:
    x_f32 = _act(x, "x")
    _f16(y1, "y1")
    M, Cc = x.shape
    with _timed("layernorm", M * Cc * ((4 if x_f32 else 2) + (2 if y2 is None else 4)), f"M{M} C{Cc}{' x2' if y2 is not None else ''}", aux=True):
        check(lib.sg_layernorm_f16(x.data_ptr(), _row_stride(x, "x"), int(x_f32), M, Cc, eps, g1.data_ptr(), b1.data_ptr(), y1.data_ptr(),
                                   _row_stride(y1, "y1"), _p(g2), _p(b2), _p(y2),
                                   0 if y2 is None else _row_stride(y2, "y2"), _stream()), "sg_layernorm_f16")


def timestep_embed(t: torch.Tensor, freqs: torch.Tensor, out: torch.Tensor, flip_sin_to_cos: bool) -> torch.Tensor:
    _f32(t, "t"), _f32(freqs, "freqs"), _f32(out, "out")
    B, dim = out.shape
    check(lib.sg_timestep_embed_f32(t.data_ptr(), freqs.data_ptr(), out.data_ptr(), B, dim, int(flip_sin_to_cos),
                                    _stream()), "sg_timestep_embed_f32")
    return out


def lookup_rows(keys: torch.Tensor, table_keys: torch.Tensor, table: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[b] = table[j] for table_keys[j] == keys[b] (fp32, exact match; NaN rows otherwise) — sg_lookup_rows_f32."""
    _f32(keys, "keys"), _f32(table_keys, "table_keys"), _f32(table, "table"), _f32(out, "out")
    B, N = out.shape
    if keys.numel() != B or table.shape[0] != table_keys.numel() or table.shape[1] != N:
        raise ValueError("lookup_rows: keys [B], table_keys [T], table [T, N], out [B, N]")
    check(lib.sg_lookup_rows_f32(keys.data_ptr(), B, table_keys.data_ptr(), table_keys.numel(), table.data_ptr(), _row_stride(table, "table"),
                                 out.data_ptr(), _row_stride(out, "out"), N, _stream()), "sg_lookup_rows_f32")
    return out


def linear_rows(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, act_in: bool = False,
                act_out: bool = False) -> torch.Tensor:
    _f32(x, "x"), _f16(w, "w"), _f32(out, "out")
    B, K = x.shape
    N = w.shape[0]
    check(lib.sg_linear_rows_f32(x.data_ptr(), _row_stride(x, "x"), w.data_ptr(), _row_stride(w, "w"), _p(bias),
                                 out.data_ptr(), _row_stride(out, "out"), B, N, K, int(act_in), int(act_out), _stream()),
          "sg_linear_rows_f32")
    return out


def add_noise(src: torch.Tensor, noise: torch.Tensor, coef: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[u] = coef[u,0]*src[u] + coef[u,1]*noise[u % N]; src/out [U,...], noise [N,...], coef [U,2] (device)."""
    for n, t in (("src", src), ("noise", noise), ("coef", coef), ("out", out)):
        _f32(t, n)
        if not t.is_contiguous():
            raise ValueError(f"add_noise: {n} must be contiguous")
    U, N = src.shape[0], noise.shape[0]
    if out.shape != src.shape or src.shape[1:] != noise.shape[1:] or coef.numel() != 2 * U:
        raise ValueError("add_noise: shape mismatch")
    check(lib.sg_add_noise_f32(src.data_ptr(), noise.data_ptr(), coef.data_ptr(), out.data_ptr(), U, N, src[0].numel(),
                               _stream()), "sg_add_noise_f32")
    return out


def _cfg_step(fn_name: str, eps3: torch.Tensor, latents: torch.Tensor, latents3: Optional[torch.Tensor], coef: torch.Tensor,
              n_coef: int, *extra: Optional[torch.Tensor]) -> torch.Tensor:
    """The checks and the call every update rule shares: sg_<fn_name>_f32(eps3, latents, latents3, *extra, coef, N, n, stream) with
    eps3 = 3 latents, latents3 = None or 3 latents, coef = the 2 guidance scales + the rule's row (n_coef floats), all fp32."""
    for n, t in (("eps3", eps3), ("latents", latents), ("coef", coef)):
        _f32(t, n)
    if eps3.numel() != 3 * latents.numel() or coef.numel() != n_coef:
        raise ValueError(f"{fn_name}: eps3 must hold 3 latents, coef {n_coef} floats")
    if latents3 is not None and (latents3.dtype != torch.float32 or latents3.numel() != 3 * latents.numel()):
        raise ValueError(f"{fn_name}: latents3 must be fp32 and hold 3 latents")
    name = f"sg_{fn_name}_f32"
    check(getattr(lib, name)(eps3.data_ptr(), latents.data_ptr(), _p(latents3), *map(_p, extra), coef.data_ptr(), latents.shape[0],
                             latents[0].numel(), _stream()), name)
    return latents


def cfg_ddim_step(eps3: torch.Tensor, latents: torch.Tensor, latents3: Optional[torch.Tensor], coef: torch.Tensor
                  ) -> torch.Tensor:
    """Guidance combine + DDIM update, eta = 0 (sg_cfg_ddim_step_f32); coef = the 2 guidance scales + DDIMSchedule.step_coef."""
    return _cfg_step("cfg_ddim_step", eps3, latents, latents3, coef, 6)


def cfg_ddim_var_step(eps3: torch.Tensor, latents: torch.Tensor, latents3: Optional[torch.Tensor], noise: Optional[torch.Tensor],
                      coef: torch.Tensor) -> torch.Tensor:
    """Guidance combine + DDIM update with eta > 0 and / or clip_sample (sg_cfg_ddim_var_step_f32); noise fp32 like latents (None
    only when std = coef[6] is 0: the library then reads it back to check), coef = the 2 guidance scales +
    (*DDIMSchedule.var_step_coef, clip) (8 floats)."""
    if noise is not None and (noise.dtype != torch.float32 or noise.numel() != latents.numel() or not noise.is_contiguous()):
        raise ValueError("cfg_ddim_var_step: noise must be contiguous fp32 of the latents' size")
    return _cfg_step("cfg_ddim_var_step", eps3, latents, latents3, coef, 8, noise)


def cfg_plms_step(eps3: torch.Tensor, latents: torch.Tensor, latents3: Optional[torch.Tensor], history: torch.Tensor,
                  kept: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """Guidance combine + PNDM/PLMS update (sg_cfg_plms_step_f32); history fp32 [4, *latents.shape], kept like latents, coef = the 2
    guidance scales + PNDMSchedule.step_row (15 floats)."""
    _f32(history, "history"), _f32(kept, "kept")
    if history.numel() != 4 * latents.numel() or kept.numel() != latents.numel():
        raise ValueError("cfg_plms_step: history must hold 4 latents, kept 1")
    return _cfg_step("cfg_plms_step", eps3, latents, latents3, coef, 15, history, kept)


def cfg_dpm_step(eps3: torch.Tensor, latents: torch.Tensor, latents3: Optional[torch.Tensor], history: torch.Tensor,
                 coef: torch.Tensor) -> torch.Tensor:
    """Guidance combine + DPM-Solver multistep update (sg_cfg_dpm_step_f32); history fp32 [3, *latents.shape] (converted model
    outputs), coef = the 2 guidance scales + DPMSolverMultistepSchedule.step_row (12 floats)."""
    _f32(history, "history")
    if history.numel() != 3 * latents.numel():
        raise ValueError("cfg_dpm_step: history must hold 3 latents")
    return _cfg_step("cfg_dpm_step", eps3, latents, latents3, coef, 12, history)


def copy_rows(dst: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """dst[b, r, :cols] = src[b, r, :cols] for 3-D views with unit channel stride; fp16->fp16, fp32->fp32 or
    fp32->fp16 (cast)."""
    s32, d32 = _act(src, "src"), _act(dst, "dst")
    if d32 and not s32:
        raise TypeError("copy_rows: fp16 -> fp32 is not supported")
    mode = 0 if not s32 else (1 if d32 else 2)
    Bn, rows, cols = src.shape
    if tuple(dst.shape) != (Bn, rows, cols) or dst.stride(-1) != 1 or src.stride(-1) != 1:
        raise ValueError("copy_rows: shape/stride mismatch")
    with _timed("copy_rows", Bn * rows * cols * ((4 if s32 else 2) + (4 if d32 else 2)), f"B{Bn} R{rows} C{cols}", aux=True):
        check(lib.sg_copy_rows(dst.data_ptr(), dst.stride(1), dst.stride(0), src.data_ptr(), src.stride(1), src.stride(0),
                               Bn, rows, cols, mode, _stream()), "sg_copy_rows")
    return dst


def pad_cast(x: torch.Tensor, out_padded: torch.Tensor) -> torch.Tensor:
    """x [B,H,W,C] fp16/fp32 (single pixel stride) -> interior of the zero-bordered fp16 [B,H+2,W+2,C]."""
    x_f32 = _act(x, "x")
    _f16(out_padded, "out")
    B, H, W, Cc = x.shape
    if tuple(out_padded.shape) != (B, H + 2, W + 2, Cc) or not out_padded.is_contiguous():
        raise ValueError("pad_cast: out must be a contiguous [B,H+2,W+2,C]")
    if x.stride(-1) != 1 or x.stride(1) != W * x.stride(2) or x.stride(0) != H * x.stride(1):
        raise ValueError("pad_cast: x must be [B,H,W,C] with a single pixel stride")
    check(lib.sg_pad_cast_f16(x.data_ptr(), x.stride(2), int(x_f32), out_padded.data_ptr(), Cc, B, H, W, Cc, _stream()),
          "sg_pad_cast_f16")
    return out_padded


FRAME_HANDOFF_MAX_BLOCKS = 1024          # SG_FRAME_HANDOFF_MAX_BLOCKS: the grid-stride loop wraps above this many workgroups of 256


def frame_handoff(x: torch.Tensor, out_u8: Optional[torch.Tensor] = None, out_f16: Optional[torch.Tensor] = None):
    """The VAE decoder's output x, fp16 [N,3,H,W] roughly in [-1,1] (any batch / channel / row stride, unit pixel stride) ->
    (the frames as saved, uint8 [N,H,W,3]; the same frames as the next call's `image_prompt` entries, fp16 [N,3,H,W] in [0,1]),
    sg_frame_handoff_f16.  The uint8 frame equals numpy_to_pil(decode_latents(.)) of model/pipeline.py bit for bit; the fp16 frame is
    fp16(fp32(uint8) / 255), what the reference's inference.py:86-92 feeds back from the saved image — in [0, 1]: the `* 2 - 1` of
    inference.py:90-91 rebinds its loop variable and is never applied to the tensor, and that convention is kept.  NaN -> 0 in both.
    Outputs are allocated when not given; given ones may be windows of larger buffers ([N,H,W,3] with pixel stride 3, [N,3,H,W] with
    unit pixel stride)."""
    _f16(x, "x")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"frame_handoff: x must be [N,3,H,W], got {tuple(x.shape)}")
    N, _, H, W = x.shape
    if out_u8 is None:
        out_u8 = torch.empty(N, H, W, 3, dtype=torch.uint8, device=x.device)
    if out_f16 is None:
        out_f16 = torch.empty(N, 3, H, W, dtype=torch.float16, device=x.device)
    _f16(out_f16, "out_f16")
    if out_u8.dtype != torch.uint8 or not out_u8.is_cuda:
        raise TypeError(f"out_u8: expected a CUDA/HIP uint8 tensor, got {out_u8.dtype} on {out_u8.device}")
    if tuple(out_u8.shape) != (N, H, W, 3) or tuple(out_f16.shape) != (N, 3, H, W):
        raise ValueError(f"frame_handoff: outputs must be [N,H,W,3] and [N,3,H,W] for x {tuple(x.shape)}")
    if N * H * W:      # (strides of an empty tensor say nothing; the library refuses the empty shape itself)
        if x.stride(3) != 1 or out_f16.stride(3) != 1 or out_u8.stride(3) != 1 or out_u8.stride(2) != 3:
            raise ValueError("frame_handoff: unit pixel stride on x and out_f16, [.., W, 3] contiguous pixels on out_u8")
    check(lib.sg_frame_handoff_f16(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), out_u8.data_ptr(), out_u8.stride(0), out_u8.stride(1),
                                   out_f16.data_ptr(), out_f16.stride(0), out_f16.stride(1), out_f16.stride(2), N, H, W, _stream()),
          "sg_frame_handoff_f16")
    return out_u8, out_f16


# SG_IMAGE_*: limits and tile of sg_image_resize_u8 (include/storygen_hip.h)
IMAGE_MAX_SIDE, IMAGE_MAX_RATIO, IMAGE_MAX_KSIZE, IMAGE_TILE_W, IMAGE_TILE_H, IMAGE_LDS_BYTES = 16384, 32, 129, 64, 16, 65536
_image_tables = {}       # (in, out, device) -> (coef int32 [out, ksize], bounds int32 [out, 2]) on that device


def image_resample_table(n_in: int, n_out: int):
    """Pillow's fixed-point bicubic coefficients of one axis from the library's host builder (sg_image_resample_table), as CPU tensors:
    (coef int32 [n_out, ksize], bounds int32 [n_out, 2] = (first input sample, taps))."""
    ks = lib.sg_image_resample_ksize(n_in, n_out)
    check(min(ks, 0), "sg_image_resample_ksize")
    coef, bounds = torch.empty(n_out, ks, dtype=torch.int32), torch.empty(n_out, 2, dtype=torch.int32)
    check(lib.sg_image_resample_table(n_in, n_out, coef.data_ptr(), bounds.data_ptr()), "sg_image_resample_table")
    return coef, bounds


def image_resize_tile_rows(h_in: int, h_out: int, channels: int) -> int:
    """Output rows per workgroup tile that image_resize uses for this geometry (sg_image_resize_tile_rows)."""
    th = lib.sg_image_resize_tile_rows(h_in, h_out, channels)
    check(min(th, 0), "sg_image_resize_tile_rows")
    return th


def _image_table(n_in: int, n_out: int, device):
    if n_in == n_out:
        return None, None
    key = (n_in, n_out, str(device))
    if key not in _image_tables:
        _image_tables[key] = tuple(t.to(device) for t in image_resample_table(n_in, n_out))
    return _image_tables[key]


def image_resize(x_u8: torch.Tensor, size, flip: bool = False, out_u8=None, out_f16=None):
    """x_u8 uint8 [N,h,w,C], C = 1 or 3 (any batch / row stride, contiguous pixels) -> (uint8 [N,H,W,C]: Image.resize(size) of Pillow on
    every image, bit for bit — its bicubic default, two 8-bit fixed-point passes; fp16 [N,C,H,W]: ToTensor of that, cast to fp16), in one
    launch of sg_image_resize_u8.  size = (W, H), as Pillow's.  flip mirrors the columns after the resize.  Outputs are allocated when
    None and may be windows of larger buffers; pass False for one that is not wanted (None comes back in its place).  The coefficient
    tables come from the library's host builder and are kept on the device per (in, out) pair."""
    if x_u8.dtype != torch.uint8 or not x_u8.is_cuda:
        raise TypeError(f"x_u8: expected a CUDA/HIP uint8 tensor, got {x_u8.dtype} on {x_u8.device}")
    if x_u8.dim() != 4 or x_u8.shape[3] not in (1, 3):
        raise ValueError(f"image_resize: x_u8 must be [N,h,w,1] or [N,h,w,3], got {tuple(x_u8.shape)}")
    N, h, w, Cc = x_u8.shape
    W, H = (int(s) for s in size)
    if out_u8 is False and out_f16 is False:
        raise ValueError("image_resize: no output is wanted")
    if H <= 0 or W <= 0:
        raise ValueError(f"image_resize: size must be positive, got {(W, H)}")
    if out_u8 is None:
        out_u8 = torch.empty(N, H, W, Cc, dtype=torch.uint8, device=x_u8.device)
    if out_f16 is None:
        out_f16 = torch.empty(N, Cc, H, W, dtype=torch.float16, device=x_u8.device)
    out_u8, out_f16 = (None if o is False else o for o in (out_u8, out_f16))
    if out_u8 is not None:
        if out_u8.dtype != torch.uint8 or not out_u8.is_cuda:
            raise TypeError(f"out_u8: expected a CUDA/HIP uint8 tensor, got {out_u8.dtype} on {out_u8.device}")
        if tuple(out_u8.shape) != (N, H, W, Cc):
            raise ValueError(f"image_resize: out_u8 must be {(N, H, W, Cc)}, got {tuple(out_u8.shape)}")
    if out_f16 is not None:
        _f16(out_f16, "out_f16")
        if tuple(out_f16.shape) != (N, Cc, H, W):
            raise ValueError(f"image_resize: out_f16 must be {(N, Cc, H, W)}, got {tuple(out_f16.shape)}")
    if any(t is not None and (t.stride(3) != 1 or t.stride(2) != Cc) for t in (x_u8, out_u8)) or (out_f16 is not None and out_f16.stride(3) != 1):
        raise ValueError("image_resize: [.., w, C] contiguous pixels on x_u8 and out_u8, unit pixel stride on out_f16")
    (hc, hb), (vc, vb) = _image_table(w, W, x_u8.device), _image_table(h, H, x_u8.device)      # (refuses sizes beyond the limits)
    su = (out_u8.stride(0), out_u8.stride(1)) if out_u8 is not None else (0, 0)
    sy = (out_f16.stride(0), out_f16.stride(1), out_f16.stride(2)) if out_f16 is not None else (0, 0, 0)
    check(lib.sg_image_resize_u8(x_u8.data_ptr(), x_u8.stride(0), x_u8.stride(1), N, h, w, Cc, _p(out_u8), *su, _p(out_f16), *sy, H, W,
                                 _p(hc), _p(hb), _p(vc), _p(vb), int(bool(flip)), _stream()), "sg_image_resize_u8")
    return out_u8, out_f16


CLIP_CROPS = ("torchvision", "floor")


def clip_u8_geometry(h: int, w: int, S: int, crop: str = "torchvision") -> tuple:
    """(resized H, resized W, top, left) of the CLIP preprocessing of an h x w image (host only).  Both rules resize alike: the shorter side
    becomes S, the longer int(S * long / short).  The centre crop's offset per axis is int(round((size - S) / 2.0)), halves to the even
    integer, under crop="torchvision" (CenterCrop of the `clip` package: sg_clip_resize_geometry) and (size - S) // 2 under crop="floor"
    (transformers' CLIPImageProcessor); they differ by one pixel where size - S = 3 (mod 4)."""
    if crop not in CLIP_CROPS:
        raise ValueError(f"clip_u8_geometry: crop must be one of {CLIP_CROPS}, got {crop!r}")
    Hr, Wr, top, left = clip_resize_geometry(h, w, S)
    return (Hr, Wr, top, left) if crop == "torchvision" else (Hr, Wr, (Hr - S) // 2, (Wr - S) // 2)


def clip_patchify_u8(x_u8: torch.Tensor, out: torch.Tensor, S: int, ps: int, mean, std, geometry=None, crop: str = "torchvision",
                     kpad: Optional[int] = None, out_u8: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x_u8 uint8 [N,h,w,3] (any batch / row stride, contiguous pixels) -> out fp16 [N * (S/ps)^2, >= kpad] (kpad defaults to 3*ps*ps rounded
    up to 8): every frame resized by Pillow's 8-bit bicubic Image.resize, bit for bit, to geometry[:2] = (Hr, Wr), cropped to the S x S
    window at geometry[2:] = (top, left), normalised as ToTensor + Normalize(mean, std) and cut into patch rows, columns (c, dy, dx), zero
    in [3*ps*ps, kpad); columns beyond kpad are left alone (sg_clip_patchify_u8, one launch).  geometry None: clip_u8_geometry(h, w, S,
    crop).  out_u8: optional uint8 [N,S,S,3] receiving the cropped image.  The coefficient tables are image_resize's, kept per (in, out)."""
    if x_u8.dtype != torch.uint8 or not x_u8.is_cuda:
        raise TypeError(f"x_u8: expected a CUDA/HIP uint8 tensor, got {x_u8.dtype} on {x_u8.device}")
    _f16(out, "out")
    if x_u8.dim() != 4 or x_u8.shape[3] != 3:
        raise ValueError(f"clip_patchify_u8: x_u8 must be [N,h,w,3], got {tuple(x_u8.shape)}")
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("clip_patchify_u8: mean and std hold one value per channel")
    N, h, w, _ = x_u8.shape
    S, ps = int(S), int(ps)
    if S <= 0 or ps <= 0 or S % ps:
        raise ValueError(f"clip_patchify_u8: crop size {S} is not a multiple of patch size {ps}")
    kpad = (3 * ps * ps + 7) & ~7 if kpad is None else int(kpad)
    rows = N * (S // ps) ** 2
    if out.dim() != 2 or out.shape[0] != rows or out.shape[1] < kpad:
        raise ValueError(f"clip_patchify_u8: out must be [{rows}, >= {kpad}], got {tuple(out.shape)}")
    if out_u8 is not None:
        if out_u8.dtype != torch.uint8 or not out_u8.is_cuda:
            raise TypeError(f"out_u8: expected a CUDA/HIP uint8 tensor, got {out_u8.dtype} on {out_u8.device}")
        if tuple(out_u8.shape) != (N, S, S, 3):
            raise ValueError(f"clip_patchify_u8: out_u8 must be {(N, S, S, 3)}, got {tuple(out_u8.shape)}")
    if any(t is not None and (t.stride(3) != 1 or t.stride(2) != 3) for t in (x_u8, out_u8)):
        raise ValueError("clip_patchify_u8: [.., w, 3] contiguous pixels on x_u8 and out_u8")
    Hr, Wr, top, left = (int(v) for v in (clip_u8_geometry(h, w, S, crop) if geometry is None else geometry))
    if Hr <= 0 or Wr <= 0:
        raise ValueError(f"clip_patchify_u8: the resized size must be positive, got {(Wr, Hr)}")
    (hc, hb), (vc, vb) = _image_table(w, Wr, x_u8.device), _image_table(h, Hr, x_u8.device)      # (refuses sizes beyond the limits)
    m, s = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    su = (out_u8.stride(0), out_u8.stride(1)) if out_u8 is not None else (0, 0)
    check(lib.sg_clip_patchify_u8(x_u8.data_ptr(), x_u8.stride(0), x_u8.stride(1), N, h, w, Hr, Wr, top, left, m, s, S, ps, kpad,
                                  out.data_ptr(), _row_stride(out, "out"), _p(out_u8), *su, _p(hc), _p(hb), _p(vc), _p(vb), _stream()),
          "sg_clip_patchify_u8")
    return out


# SG_DTW_*: limits of sg_align_cost_f64 / sg_dtw_path_f64 (include/storygen_hip.h)
DTW_MAX_SHORT, DTW_MAX_SIDE = 2048, 65535


def _f64(t: torch.Tensor, name: str):
    if t.dtype != torch.float64 or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA/HIP float64 tensor, got {t.dtype} on {t.device}")


def _same_device(who: str, first: torch.Tensor, **others) -> None:
    """Every tensor of one launch lives on one device: a pointer of another GPU would be read as an address of this one."""
    for name, t in others.items():
        if t is not None and t.device != first.device:
            raise ValueError(f"{who}: {name} is on {t.device}, the first operand on {first.device}")


def check_align_sides(who: str, r: int, c: int, dtw: bool) -> None:
    if r < 1 or c < 1:
        raise ValueError(f"{who}: r = {r}, c = {c}: at least one frame and one sentence")
    if r > DTW_MAX_SIDE or c > DTW_MAX_SIDE or r * c >= 2 ** 31:
        raise ValueError(f"{who}: r = {r}, c = {c} exceed the limits (each side <= {DTW_MAX_SIDE}, r * c < 2^31)")
    if dtw and min(r, c) > DTW_MAX_SHORT:
        raise ValueError(f"{who}: the shorter side min({r}, {c}) exceeds {DTW_MAX_SHORT}")


def align_cost(frame_feats: torch.Tensor, sent_feats: torch.Tensor, frame_times: torch.Tensor, sent_times: torch.Tensor,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frame_feats fp32 [r, dim] (any row stride), sent_feats fp32 [c, dim] (contiguous), frame_times [r] and sent_times [c] float64 seconds
    -> cost float64 [r, c]: cosine distance 1 - f.s / (|f| |s| + 1e-9) in float64, plus floor(dt / 60) where the two times are more than
    60 s apart (sg_align_cost_f64; data_process/align.py:22-30,137-140).  `out`, when given, may be a window of a larger buffer."""
    _f32(frame_feats, "frame_feats"), _f32(sent_feats, "sent_feats"), _f64(frame_times, "frame_times"), _f64(sent_times, "sent_times")
    if frame_feats.dim() != 2 or sent_feats.dim() != 2 or frame_feats.shape[1] != sent_feats.shape[1]:
        raise ValueError(f"align_cost: features must be [r, dim] and [c, dim], got {tuple(frame_feats.shape)} and {tuple(sent_feats.shape)}")
    (r, dim), c = frame_feats.shape, sent_feats.shape[0]
    check_align_sides("align_cost", r, c, dtw=False)
    if dim < 1:
        raise ValueError("align_cost: dim must be at least 1")
    if tuple(frame_times.shape) != (r,) or tuple(sent_times.shape) != (c,):
        raise ValueError(f"align_cost: times must be [{r}] and [{c}], got {tuple(frame_times.shape)} and {tuple(sent_times.shape)}")
    if not (sent_feats.is_contiguous() and frame_times.is_contiguous() and sent_times.is_contiguous()):
        raise ValueError("align_cost: sent_feats, frame_times and sent_times must be contiguous")
    if out is None:
        out = torch.empty(r, c, dtype=torch.float64, device=frame_feats.device)
    _f64(out, "out")
    if tuple(out.shape) != (r, c):
        raise ValueError(f"align_cost: out must be [{r}, {c}], got {tuple(out.shape)}")
    _same_device("align_cost", frame_feats, sent_feats=sent_feats, frame_times=frame_times, sent_times=sent_times, out=out)
    check(lib.sg_align_cost_f64(frame_feats.data_ptr(), _row_stride(frame_feats, "frame_feats"), sent_feats.data_ptr(), frame_times.data_ptr(),
                                sent_times.data_ptr(), out.data_ptr(), _row_stride(out, "out"), r, c, dim, _stream()), "sg_align_cost_f64")
    return out


def dtw_path(cost: torch.Tensor, return_acc: bool = False, *, path: Optional[torch.Tensor] = None, path_len: Optional[torch.Tensor] = None,
             codes: Optional[torch.Tensor] = None, acc: Optional[torch.Tensor] = None):
    """cost float64 [r, c] (any row stride) -> (path int32 [r + c - 1, 2] of which the first path_len rows are written, path_len int32 [1],
    codes uint8 [r, c]), all on the device, plus the accumulated matrix acc float64 [r, c] with return_acc (sg_dtw_path_f64: the recurrence
    and the first-minimum backtrace of data_process/align.py:130-159, the path from (0, 0) to (r - 1, c - 1)).  Outputs are allocated when
    not given; a given acc may be a window of a larger buffer, the others are contiguous."""
    _f64(cost, "cost")
    if cost.dim() != 2:
        raise ValueError(f"dtw_path: cost must be [r, c], got {tuple(cost.shape)}")
    r, c = cost.shape
    check_align_sides("dtw_path", r, c, dtw=True)
    dev = cost.device
    path = torch.empty(r + c - 1, 2, dtype=torch.int32, device=dev) if path is None else path
    path_len = torch.empty(1, dtype=torch.int32, device=dev) if path_len is None else path_len
    codes = torch.empty(r, c, dtype=torch.uint8, device=dev) if codes is None else codes
    if acc is None and return_acc:
        acc = torch.empty(r, c, dtype=torch.float64, device=dev)
    for t, name, dtype, shape in ((path, "path", torch.int32, (r + c - 1, 2)), (path_len, "path_len", torch.int32, (1,)),
                                  (codes, "codes", torch.uint8, (r, c))):
        if t.dtype != dtype or not t.is_cuda:
            raise TypeError(f"{name}: expected a CUDA/HIP {dtype} tensor, got {t.dtype} on {t.device}")
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"dtw_path: {name} must be contiguous {shape}, got {tuple(t.shape)}")
    if acc is not None:
        _f64(acc, "acc")
        if tuple(acc.shape) != (r, c):
            raise ValueError(f"dtw_path: acc must be [{r}, {c}], got {tuple(acc.shape)}")
    _same_device("dtw_path", cost, path=path, path_len=path_len, codes=codes, acc=acc)
    check(lib.sg_dtw_path_f64(cost.data_ptr(), _row_stride(cost, "cost"), r, c, codes.data_ptr(), _p(acc),
                              0 if acc is None else _row_stride(acc, "acc"), path.data_ptr(), path_len.data_ptr(), _stream()), "sg_dtw_path_f64")
    return (path, path_len, codes, acc) if acc is not None else (path, path_len, codes)


# SG_DEDUP_*: limits of sg_adjacent_cosine_f64 (include/storygen_hip.h)
DEDUP_MAX_FRAMES, DEDUP_MAX_DIM = 1 << 20, 65536
DEDUP_IMAGE_MEAN = (0.485, 0.456, 0.406)                    # Normalize() of data_process/dup_remove.py:13 (the ImageNet constants)
DEDUP_IMAGE_STD = (0.229, 0.224, 0.225)


def dedup_u8_geometry(h: int, w: int, S: int, resize: int = 256) -> tuple:
    """(resized H, resized W, top, left) of dup_remove.py's Resize(resize) + CenterCrop(S) on an h x w image (host only): the shorter side
    becomes `resize`, the longer int(resize * long / short) (clip_resize_geometry(h, w, resize)'s resized sizes); the crop's offset per axis
    is int(round((size - S) / 2.0)), halves to the even integer (torchvision's CenterCrop).  A resized side below S is refused: the script
    would pad it."""
    Hr, Wr, _, _ = clip_resize_geometry(h, w, resize)
    if min(Hr, Wr) < S:
        raise ValueError(f"dedup_u8_geometry: a {h} x {w} frame resized to {Hr} x {Wr} is smaller than the {S} x {S} crop (padding is out of scope)")
    return Hr, Wr, int(round((Hr - S) / 2.0)), int(round((Wr - S) / 2.0))


def check_dedup_sides(who: str, N: int, dim: int) -> None:
    if N < 1 or N > DEDUP_MAX_FRAMES:
        raise ValueError(f"{who}: {N} frames are outside [1, {DEDUP_MAX_FRAMES}]")
    if dim < 1 or dim > DEDUP_MAX_DIM:
        raise ValueError(f"{who}: feature dim {dim} is outside [1, {DEDUP_MAX_DIM}]")


def adjacent_cosine(feats: torch.Tensor, threshold: float = 0.75, eps: float = 1e-8, sim: Optional[torch.Tensor] = None,
                    drop: Optional[torch.Tensor] = None) -> tuple:
    """feats fp32 [N, dim] (any row stride), frames in order -> (sim float64 [N], drop uint8 [N]) on the device: sim[0] = 0, sim[i] the
    float64 cosine similarity of frame i with frame i - 1 under torch.cosine_similarity's clamp of each norm at eps; drop[i] = 1 iff
    i + 1 < N and sim[i + 1] >= threshold — the files data_process/dup_remove.py:38-46 deletes (sg_adjacent_cosine_f64, one launch).
    sim and drop, when given, are contiguous [N] tensors and may be windows of larger buffers."""
    _f32(feats, "feats")
    if feats.dim() != 2:
        raise ValueError(f"adjacent_cosine: feats must be [N, dim], got {tuple(feats.shape)}")
    N, dim = feats.shape
    check_dedup_sides("adjacent_cosine", N, dim)
    eps, threshold = float(eps), float(threshold)
    if not eps >= 0.0:
        raise ValueError(f"adjacent_cosine: eps = {eps} must be a number >= 0")
    ldf = _row_stride(feats, "feats")
    if N == 1:
        ldf = max(ldf, dim)                                  # (the stride of a single row is never used)
    if ldf < dim:
        raise ValueError(f"adjacent_cosine: feats rows overlap (row stride {ldf} below dim {dim})")
    sim = torch.empty(N, dtype=torch.float64, device=feats.device) if sim is None else sim
    drop = torch.empty(N, dtype=torch.uint8, device=feats.device) if drop is None else drop
    _f64(sim, "sim")
    if drop.dtype != torch.uint8 or not drop.is_cuda:
        raise TypeError(f"drop: expected a CUDA/HIP uint8 tensor, got {drop.dtype} on {drop.device}")
    for t, name in ((sim, "sim"), (drop, "drop")):
        if tuple(t.shape) != (N,) or not t.is_contiguous():
            raise ValueError(f"adjacent_cosine: {name} must be contiguous [{N}], got {tuple(t.shape)}")
    _same_device("adjacent_cosine", feats, sim=sim, drop=drop)
    check(lib.sg_adjacent_cosine_f64(feats.data_ptr(), ldf, N, dim, eps, threshold, sim.data_ptr(), drop.data_ptr(), _stream()),
          "sg_adjacent_cosine_f64")
    return sim, drop


# SG_DET_* / SG_MASK_*: limits of sg_det_select / sg_det_nms / sg_box_mask_u8 (include/storygen_hip.h)
DET_MAX_BATCH, DET_MAX_ANCHORS, DET_MAX_NC, DET_MAX_NMS, DET_MAX_DET = 4096, 1 << 20, 1024, 30000, 1024
MASK_MAX_SIDE, MASK_MAX_TEXT = 16384, 1024


def _i32(t: torch.Tensor, name: str):
    if t.dtype != torch.int32 or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA/HIP int32 tensor, got {t.dtype} on {t.device}")


def _given(who: str, t: Optional[torch.Tensor], name: str, dtype, shape, device) -> torch.Tensor:
    """An output of a detection op: allocated when not given, else a contiguous tensor of that type and shape (a window of a larger
    buffer is fine)."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if t.dtype != dtype or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA/HIP {dtype} tensor, got {t.dtype} on {t.device}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous {tuple(shape)}, got {tuple(t.shape)}")
    return t


def check_det_sides(who: str, B: int, A: int, nc: int, max_nms: int, max_det: int) -> None:
    if B < 1 or B > DET_MAX_BATCH:
        raise ValueError(f"{who}: {B} images are outside [1, {DET_MAX_BATCH}]")
    if A < 1 or A > DET_MAX_ANCHORS:
        raise ValueError(f"{who}: {A} anchors are outside [1, {DET_MAX_ANCHORS}]")
    if nc < 1 or nc > DET_MAX_NC:
        raise ValueError(f"{who}: {nc} classes are outside [1, {DET_MAX_NC}]")
    if max_nms < 1 or max_nms > DET_MAX_NMS:
        raise ValueError(f"{who}: max_nms = {max_nms} is outside [1, {DET_MAX_NMS}]")
    if max_det < 1 or max_det > DET_MAX_DET:
        raise ValueError(f"{who}: max_det = {max_det} is outside [1, {DET_MAX_DET}]")


def check_mask_frame(who: str, h0: int, w0: int) -> None:
    if h0 < 1 or w0 < 1 or h0 > MASK_MAX_SIDE or w0 > MASK_MAX_SIDE:
        raise ValueError(f"{who}: a {h0} x {w0} frame is outside [1, {MASK_MAX_SIDE}] per side")


def det_select_workspace_bytes(B: int, A: int) -> int:
    return lib.sg_det_select_workspace_bytes(B, A)


def det_select(pred: torch.Tensor, conf_thres: float = 0.5, classes: tuple = (), max_nms: int = 30000, cand: Optional[torch.Tensor] = None,
               ncand: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> tuple:
    """pred fp32 or fp16 [B, A, 5 + nc] (any batch / row stride), rows (x, y, w, h, obj, cls ...) -> (cand fp32 [B, max_nms, 6], ncand int32
    [B]) on the device: per image the anchors with obj > conf_thres, conf = max_c cls_c * obj > conf_thres (first maximum; conf = obj at
    nc == 1) and the best class in `classes` (empty: all), as (x1, y1, x2, y2, conf, cls), ordered by conf descending with equal scores in
    anchor order, the first max_nms of them; ncand[b] rows are written (sg_det_select: non_max_suppression's filter, utils/general.py:
    617-679, in fp32).  workspace: uint8 of det_select_workspace_bytes(B, A), allocated when not given."""
    _act(pred, "pred")
    if pred.dim() != 3 or pred.shape[2] < 6:
        raise ValueError(f"det_select: pred must be [B, A, 5 + nc] with nc >= 1, got {tuple(pred.shape)}")
    B, A, nc = pred.shape[0], pred.shape[1], pred.shape[2] - 5
    max_nms = int(max_nms)
    check_det_sides("det_select", B, A, nc, max_nms, 1)
    conf_thres = float(conf_thres)
    if conf_thres != conf_thres:
        raise ValueError("det_select: conf_thres is NaN")
    classes = tuple(int(c) for c in classes)
    if any(c < 0 for c in classes) or len(classes) > DET_MAX_NC:
        raise ValueError(f"det_select: classes {classes} hold a negative id or more than {DET_MAX_NC} ids")
    if pred.stride(2) != 1:
        raise ValueError("det_select: innermost dimension must be contiguous")
    ldp = max(pred.stride(1), 5 + nc) if A == 1 else pred.stride(1)       # (the stride of a single row / image is never used)
    bsp = max(pred.stride(0), A * ldp) if B == 1 else pred.stride(0)
    if ldp < 5 + nc or bsp < A * ldp:
        raise ValueError(f"det_select: pred overlaps itself (row stride {ldp}, batch stride {bsp} for {A} rows of {5 + nc})")
    dev = pred.device
    cand = _given("det_select", cand, "cand", torch.float32, (B, max_nms, 6), dev)
    ncand = _given("det_select", ncand, "ncand", torch.int32, (B,), dev)
    need = det_select_workspace_bytes(B, A)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if workspace.dtype != torch.uint8 or not workspace.is_cuda:
        raise TypeError(f"workspace: expected a CUDA/HIP uint8 tensor, got {workspace.dtype} on {workspace.device}")
    if workspace.dim() != 1 or not workspace.is_contiguous() or workspace.numel() < need or workspace.data_ptr() % 4:
        raise ValueError(f"det_select: workspace must be contiguous, 4-byte aligned and hold {need} bytes, got {tuple(workspace.shape)}")
    _same_device("det_select", pred, cand=cand, ncand=ncand, workspace=workspace)
    cl = (C.c_int32 * max(1, len(classes)))(*classes)
    check(lib.sg_det_select(pred.data_ptr(), int(pred.dtype == torch.float16), bsp, ldp, B, A, nc, conf_thres, cl, len(classes), max_nms,
                            cand.data_ptr(), ncand.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream()), "sg_det_select")
    return cand, ncand


def det_nms(cand: torch.Tensor, ncand: torch.Tensor, geom: torch.Tensor, iou_thres: float = 0.6, agnostic: bool = False, max_det: int = 300,
            det: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None) -> tuple:
    """cand fp32 [B, max_nms, 6] and ncand int32 [B] as det_select leaves them, geom fp32 [B, 5] = (pad_x, pad_y, gain, w0, h0) per image
    -> (det fp32 [B, max_det, 6], count int32 [B]) on the device: greedy NMS by torchvision.ops.nms's definition on box + cls * 4096 (the
    plain box with agnostic), the first max_det kept rows in score order with their boxes taken to the frame as scale_coords and .round()
    do it: rint(clamp((v - pad) / gain, 0, size)) (sg_det_nms).  count[b] rows are written."""
    _f32(cand, "cand"), _i32(ncand, "ncand"), _f32(geom, "geom")
    if cand.dim() != 3 or cand.shape[2] != 6 or not cand.is_contiguous():
        raise ValueError(f"det_nms: cand must be contiguous [B, max_nms, 6], got {tuple(cand.shape)}")
    B, max_nms, max_det = cand.shape[0], cand.shape[1], int(max_det)
    check_det_sides("det_nms", B, 1, 1, max_nms, max_det)
    iou_thres = float(iou_thres)
    if iou_thres != iou_thres:
        raise ValueError("det_nms: iou_thres is NaN")
    if tuple(ncand.shape) != (B,) or not ncand.is_contiguous():
        raise ValueError(f"det_nms: ncand must be contiguous [{B}], got {tuple(ncand.shape)}")
    if tuple(geom.shape) != (B, 5) or not geom.is_contiguous():
        raise ValueError(f"det_nms: geom must be contiguous [{B}, 5], got {tuple(geom.shape)}")
    det = _given("det_nms", det, "det", torch.float32, (B, max_det, 6), cand.device)
    count = _given("det_nms", count, "count", torch.int32, (B,), cand.device)
    _same_device("det_nms", cand, ncand=ncand, geom=geom, det=det, count=count)
    check(lib.sg_det_nms(cand.data_ptr(), ncand.data_ptr(), B, max_nms, iou_thres, int(bool(agnostic)), max_det, geom.data_ptr(), det.data_ptr(),
                         count.data_ptr(), _stream()), "sg_det_nms")
    return det, count


def box_mask(h0: int, w0: int, det: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None, text: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, covered: Optional[torch.Tensor] = None) -> tuple:
    """-> (mask uint8 [h0, w0, 3] of 0 / 255, covered int32 [1]) on the device: mask[y1:y2, x1:x2] = 255 with NumPy's slice rules for the first
    count[0] rows of det (fp32 [max_det, 6], one image of det_nms's output; int() of its coordinates) and for every row of text (int32
    [T, 4], x1 y1 x2 y2); covered = the pixels under the det rectangles alone (sg_box_mask_u8; human_ocr_mask.py:41-70).  out, when given,
    is [h0, w0, 3] with contiguous pixels and any row stride.  At least one of det / text is given, or neither for an empty mask."""
    h0, w0 = int(h0), int(w0)
    check_mask_frame("box_mask", h0, w0)
    if (det is None) != (count is None):
        raise ValueError("box_mask: det and count go together")
    first = next((t for t in (det, text, out, covered) if t is not None), None)
    if first is None:
        raise ValueError("box_mask: no tensor names the device (give det, text, out or covered)")
    max_det = 0
    if det is not None:
        _f32(det, "det"), _i32(count, "count")
        if det.dim() != 2 or det.shape[1] != 6 or not det.is_contiguous() or not 1 <= det.shape[0] <= DET_MAX_DET:
            raise ValueError(f"box_mask: det must be contiguous [max_det <= {DET_MAX_DET}, 6], got {tuple(det.shape)}")
        if tuple(count.shape) != (1,):
            raise ValueError(f"box_mask: count must be [1], got {tuple(count.shape)}")
        max_det = det.shape[0]
    n_text = 0
    if text is not None:
        _i32(text, "text")
        if text.dim() != 2 or text.shape[1] != 4 or not text.is_contiguous() or text.shape[0] > MASK_MAX_TEXT:
            raise ValueError(f"box_mask: text must be contiguous [T <= {MASK_MAX_TEXT}, 4], got {tuple(text.shape)}")
        n_text = text.shape[0]
    dev = first.device
    if out is None:
        out = torch.empty(h0, w0, 3, dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or not out.is_cuda:
        raise TypeError(f"out: expected a CUDA/HIP uint8 tensor, got {out.dtype} on {out.device}")
    if tuple(out.shape) != (h0, w0, 3) or out.stride(2) != 1 or out.stride(1) != 3 or (h0 > 1 and out.stride(0) < 3 * w0):
        raise ValueError(f"box_mask: out must be [{h0}, {w0}, 3] with contiguous pixels and rows that do not overlap, got {tuple(out.shape)} "
                         f"with strides {tuple(out.stride())}")
    covered = _given("box_mask", covered, "covered", torch.int32, (1,), dev)
    _same_device("box_mask", first, det=det, count=count, text=text, out=out, covered=covered)
    ldm = max(out.stride(0), 3 * w0) if h0 == 1 else out.stride(0)
    check(lib.sg_box_mask_u8(out.data_ptr(), ldm, h0, w0, _p(det), _p(count), max_det, _p(text) if n_text else None, n_text, covered.data_ptr(),
                             _stream()), "sg_box_mask_u8")
    return out, covered


# ------------------------------------------------------------------------------------------------ backward pass (config 4)
# Validated on MI355X in round 2 (tests/test_backward_gpu.py).  Kernels: csrc/backward.hip, attention_bwd.hip; formulas: oracle/storygen_backward.py.
def layernorm_bwd(x: torch.Tensor, dy1: torch.Tensor, g1: torch.Tensor, out: torch.Tensor, eps: float = 1e-5,
                  dy2: Optional[torch.Tensor] = None, g2: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
                  res_scale: float = 1.0) -> torch.Tensor:
    """out[M,C] (fp32) = res_scale * res + dLayerNorm(x; dy1 * g1 (+ dy2 * g2)).  x, dy fp16 or fp32 (both dy alike)."""
    x_f32, dy_f32 = _act(x, "x"), _act(dy1, "dy1")
    _f32(out, "out"), _f16(g1, "g1")
    if dy2 is not None and _act(dy2, "dy2") != dy_f32:
        raise TypeError("layernorm_bwd: dy1 and dy2 must have the same dtype")
    if res is not None:
        _f32(res, "res")
    M, Cc = x.shape
    check(lib.sg_layernorm_bwd_f16(x.data_ptr(), _row_stride(x, "x"), int(x_f32), dy1.data_ptr(), _row_stride(dy1, "dy1"),
                                   g1.data_ptr(), _p(dy2), 0 if dy2 is None else _row_stride(dy2, "dy2"), _p(g2), int(dy_f32),
                                   _p(res), 0 if res is None else _row_stride(res, "res"), float(res_scale), out.data_ptr(),
                                   _row_stride(out, "out"), M, Cc, eps, _stream()), "sg_layernorm_bwd_f16")
    return out


def geglu_bwd(proj_il: torch.Tensor, du: torch.Tensor, dproj_il: torch.Tensor) -> torch.Tensor:
    """proj_il / dproj_il [M, N8] fp16 in the interleaved GEGLU column layout (repack.py), du [M, N8/2] fp16."""
    _f16(proj_il, "proj"), _f16(du, "du"), _f16(dproj_il, "dproj")
    M, N8 = proj_il.shape
    if tuple(du.shape) != (M, N8 // 2) or tuple(dproj_il.shape) != (M, N8):
        raise ValueError("geglu_bwd: shape mismatch")
    check(lib.sg_geglu_bwd_f16(proj_il.data_ptr(), _row_stride(proj_il, "proj"), du.data_ptr(), _row_stride(du, "du"),
                               dproj_il.data_ptr(), _row_stride(dproj_il, "dproj"), M, N8, _stream()), "sg_geglu_bwd_f16")
    return dproj_il


def groupnorm_bwd_workspace_bytes(B: int, groups: int) -> int:
    return lib.sg_groupnorm_bwd_workspace_bytes(B, groups)


def groupnorm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: torch.Tensor, groups: int,
                  eps: float, silu: bool, workspace: torch.Tensor, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x, dy [B, HW, C] (fp16 / fp32, row-strided views allowed).  out: fp32 [B, HW, C] (optionally + res, fp32 [B, HW, C]),
    fp16 [B, HW, C], or the zero-bordered fp16 image [B, H+2, W+2, C] (interior written)."""
    from ._lib import GroupNormBwdDesc
    x_f32, dy_f32 = _act(x, "x"), _act(dy, "dy")
    out_f32 = _act(out, "out")
    _f16(gamma, "gamma"), _f16(beta, "beta")
    B, HW, Cc = x.shape
    if tuple(dy.shape) != (B, HW, Cc) or x.stride(0) != HW * x.stride(1) or dy.stride(0) != HW * dy.stride(1):
        raise ValueError("groupnorm_bwd: x / dy must be [B, HW, C] with a single row stride")
    d = GroupNormBwdDesc()
    d.x, d.ldx, d.x_f32 = x.data_ptr(), x.stride(1), int(x_f32)
    d.dy, d.lddy, d.dy_f32 = dy.data_ptr(), dy.stride(1), int(dy_f32)
    d.gamma, d.beta = gamma.data_ptr(), beta.data_ptr()
    if res is not None:
        _f32(res, "res")
        if tuple(res.shape) != (B, HW, Cc) or res.stride(0) != HW * res.stride(1):
            raise ValueError("groupnorm_bwd: res must be [B, HW, C] with a single row stride")
        d.res, d.ldr = res.data_ptr(), res.stride(1)
    if out.dim() == 4:
        Hp, Wp = out.shape[1], out.shape[2]
        if out_f32 or (Hp - 2) * (Wp - 2) != HW or not out.is_contiguous():
            raise ValueError("groupnorm_bwd: a padded output must be a contiguous fp16 [B, H+2, W+2, C] image")
        d.out, d.ldo, d.out_f32, d.out_pad_w = out.data_ptr(), out.stride(2), 0, Wp - 2
    else:
        if tuple(out.shape) != (B, HW, Cc) or out.stride(0) != HW * out.stride(1):
            raise ValueError("groupnorm_bwd: out must be [B, HW, C] with a single row stride")
        d.out, d.ldo, d.out_f32, d.out_pad_w = out.data_ptr(), out.stride(1), int(out_f32), 0
    d.B, d.HW, d.C, d.groups, d.eps, d.silu = B, HW, Cc, groups, eps, int(silu)
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    check(lib.sg_groupnorm_bwd_nhwc_f16(C.byref(d), _stream()), "sg_groupnorm_bwd_nhwc_f16")
    return out


def transpose(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst [C, M] fp16 = src [M, C]^T (src fp16 or fp32)."""
    s32 = _act(src, "src")
    _f16(dst, "dst")
    M, Cc = src.shape
    if tuple(dst.shape) != (Cc, M):
        raise ValueError("transpose: dst must be [C, M]")
    check(lib.sg_transpose_f16(src.data_ptr(), _row_stride(src, "src"), int(s32), dst.data_ptr(), _row_stride(dst, "dst"), M, Cc,
                               _stream()), "sg_transpose_f16")
    return dst


def transpose_batched(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst [B, C, M] fp16 = src [B, M, C] transposed per batch row, ONE launch (src fp16 or fp32; row- and batch-strided views allowed)."""
    s32 = _act(src, "src")
    _f16(dst, "dst")
    B, M, Cc = src.shape
    if tuple(dst.shape) != (B, Cc, M) or src.stride(2) != 1 or dst.stride(2) != 1:
        raise ValueError("transpose_batched: dst must be [B, C, M], last dimensions contiguous")
    check(lib.sg_transpose_batched_f16(src.data_ptr(), src.stride(1), src.stride(0), int(s32), dst.data_ptr(), dst.stride(1), dst.stride(0),
                                       B, M, Cc, _stream()), "sg_transpose_batched_f16")
    return dst


def sum2x2(du: torch.Tensor, dx: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    """du [B, 2H, 2W, C] fp32 -> dx [B, H, W, C] fp32 (single pixel stride each)."""
    _f32(du, "du"), _f32(dx, "dx")
    B, H, W, Cc = dx.shape
    if tuple(du.shape) != (B, 2 * H, 2 * W, Cc) or du.stride(-1) != 1 or dx.stride(-1) != 1:
        raise ValueError("sum2x2: shape mismatch")
    for t, hh, ww in ((du, 2 * H, 2 * W), (dx, H, W)):
        if t.stride(1) != ww * t.stride(2) or t.stride(0) != hh * t.stride(1):
            raise ValueError("sum2x2: tensors must have a single pixel stride")
    check(lib.sg_sum2x2_f32(du.data_ptr(), du.stride(2), dx.data_ptr(), dx.stride(2), B, H, W, Cc, int(accumulate), _stream()),
          "sg_sum2x2_f32")
    return dx


def zero_stuff(dy: torch.Tensor, out_padded: torch.Tensor) -> torch.Tensor:
    """dy [B, Ho, Wo, C] (fp16 / fp32, single pixel stride) -> interior of the zero-bordered fp16 [B, 2Ho+2, 2Wo+2, C]."""
    d32 = _act(dy, "dy")
    _f16(out_padded, "out")
    B, Ho, Wo, Cc = dy.shape
    if tuple(out_padded.shape) != (B, 2 * Ho + 2, 2 * Wo + 2, Cc) or not out_padded.is_contiguous():
        raise ValueError("zero_stuff: out must be a contiguous [B, 2Ho+2, 2Wo+2, C]")
    if dy.stride(-1) != 1 or dy.stride(1) != Wo * dy.stride(2) or dy.stride(0) != Ho * dy.stride(1):
        raise ValueError("zero_stuff: dy must be [B, Ho, Wo, C] with a single pixel stride")
    check(lib.sg_zero_stuff_f16(dy.data_ptr(), dy.stride(2), int(d32), out_padded.data_ptr(), Cc, B, Ho, Wo, Cc, _stream()),
          "sg_zero_stuff_f16")
    return out_padded


def mse_grad(pred: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor, d_pred: torch.Tensor, loss: torch.Tensor) -> torch.Tensor:
    """loss[0] = mean(((pred - noise) * (1 - mask))^2), d_pred = its gradient; all fp32, contiguous, same shape."""
    for n, t in (("pred", pred), ("noise", noise), ("mask", mask), ("d_pred", d_pred), ("loss", loss)):
        _f32(t, n)
        if not t.is_contiguous():
            raise ValueError(f"mse_grad: {n} must be contiguous")
    check(lib.sg_mse_grad_f32(pred.data_ptr(), noise.data_ptr(), mask.data_ptr(), d_pred.data_ptr(), loss.data_ptr(),
                              pred.numel(), _stream()), "sg_mse_grad_f32")
    return d_pred


def _attn_desc(q, k, vt, out, heads, scale, nk):
    for n, t in (("q", q), ("k", k), ("vt", vt), ("out", out)):
        _f16(t, n)
        if t.dim() != 3 or t.stride(2) != 1:
            raise ValueError(f"attention: {n} must be 3-D with a contiguous last dimension")
    B, Nq, Cq = q.shape
    Bk = k.shape[0]
    Nk = k.shape[1] if nk is None else nk
    D = Cq // heads
    d = AttnDesc()
    d.q, d.ldq, d.bsq = q.data_ptr(), q.stride(1), q.stride(0)
    d.k, d.ldk, d.bsk = k.data_ptr(), k.stride(1), k.stride(0)
    d.vt, d.ldvt, d.bsvt = vt.data_ptr(), vt.stride(1), vt.stride(0)
    d.o, d.ldo, d.bso = out.data_ptr(), out.stride(1), out.stride(0)
    d.B, d.H, d.Nq, d.Nk, d.D, d.kv_batches, d.scale = B, heads, Nq, Nk, D, (0 if Bk == B else Bk), scale
    return d


def attention_lse(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, lse2: torch.Tensor, heads: int,
                  scale: float, nk: Optional[int] = None) -> torch.Tensor:
    """Training forward: `attention` that also stores lse2 [B, H, Nq] fp32 (log2-domain log-sum-exp rows)."""
    _f32(lse2, "lse2")
    if tuple(lse2.shape) != (q.shape[0], heads, q.shape[1]) or not lse2.is_contiguous():
        raise ValueError("attention_lse: lse2 must be a contiguous [B, H, Nq]")
    d = _attn_desc(q, k, vt, out, heads, scale, nk)
    with _timed(f"attention_d{d.D}", 4.0 * d.B * d.H * d.Nq * d.Nk * d.D, f"B{d.B} H{d.H} Nq{d.Nq} Nk{d.Nk} lse"):
        check(lib.sg_attn_fwd_lse_f16(C.byref(d), lse2.data_ptr(), _stream()), "sg_attn_fwd_lse_f16")
    return out


def attention_bwd_prep(o: torch.Tensor, dout: torch.Tensor, lse2: torch.Tensor, ld2: torch.Tensor, heads: int) -> torch.Tensor:
    """ld2 [B, H, Nq, 2] fp32 = (lse2, delta = rowsum_d(dO * O)) per (batch, head, query); o, dout [B, Nq, H*D] fp16."""
    _f16(o, "o"), _f16(dout, "dout"), _f32(lse2, "lse2"), _f32(ld2, "ld2")
    B, Nq, Cq = o.shape
    if tuple(ld2.shape) != (B, heads, Nq, 2) or not ld2.is_contiguous() or not lse2.is_contiguous():
        raise ValueError("attention_bwd_prep: ld2 must be a contiguous [B, H, Nq, 2], lse2 a contiguous [B, H, Nq]")
    check(lib.sg_attn_bwd_prep_f32(o.data_ptr(), o.stride(1), o.stride(0), dout.data_ptr(), dout.stride(1), dout.stride(0),
                                   lse2.data_ptr(), ld2.data_ptr(), B, heads, Nq, Cq // heads, _stream()), "sg_attn_bwd_prep_f32")
    return ld2


def _attn_bwd_desc(q, k, v, dout, ld2, heads, scale):
    from ._lib import AttnBwdDesc
    for n, t in (("q", q), ("k", k), ("v", v), ("dout", dout)):
        _f16(t, n)
        if t.dim() != 3 or t.stride(2) != 1:
            raise ValueError(f"attention_bwd: {n} must be [B, N, H*D] with a contiguous last dimension")
    _f32(ld2, "ld2")
    B, Nq, Cq = q.shape
    d = AttnBwdDesc()
    d.q, d.ldq, d.bsq = q.data_ptr(), q.stride(1), q.stride(0)
    d.k, d.ldk, d.bsk = k.data_ptr(), k.stride(1), k.stride(0)
    d.v, d.ldv, d.bsv = v.data_ptr(), v.stride(1), v.stride(0)
    d.dout, d.lddo, d.bsdo = dout.data_ptr(), dout.stride(1), dout.stride(0)
    d.ld2 = ld2.data_ptr()
    d.B, d.H, d.Nq, d.Nk, d.D, d.scale = B, heads, Nq, k.shape[1], Cq // heads, scale
    return d


def attention_bwd_dq(q: torch.Tensor, k: torch.Tensor, kt: torch.Tensor, v: torch.Tensor, dout: torch.Tensor, ld2: torch.Tensor,
                     dq: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """dq [B, Nq, H*D] = scale * dS K.  kt [B, H*D, Nk] = K transposed (keys contiguous)."""
    d = _attn_bwd_desc(q, k, v, dout, ld2, heads, scale)
    _f16(kt, "kt"), _f16(dq, "dq")
    d.kt, d.ldkt, d.bskt = kt.data_ptr(), kt.stride(1), kt.stride(0)
    d.dq, d.lddq, d.bsdq = dq.data_ptr(), dq.stride(1), dq.stride(0)
    with _timed("attention_bwd", 6.0 * d.B * d.H * d.Nq * d.Nk * d.D, f"dq B{d.B} H{d.H} Nq{d.Nq} Nk{d.Nk} D{d.D}"):     # S, dP, dQ: 1.5 x forward
        check(lib.sg_attn_bwd_dq_f16(C.byref(d), _stream()), "sg_attn_bwd_dq_f16")
    return dq


def attention_bwd_dkv(q: torch.Tensor, qt: torch.Tensor, k: torch.Tensor, v: torch.Tensor, dout: torch.Tensor, dot: torch.Tensor,
                      ld2: torch.Tensor, dkt: torch.Tensor, dvt: torch.Tensor, heads: int, scale: float):
    """dkt, dvt [B, H*D, Nk] (transposed: keys contiguous).  qt, dot [B, H*D, Nq] = Q, dO transposed."""
    d = _attn_bwd_desc(q, k, v, dout, ld2, heads, scale)
    for n, t in (("qt", qt), ("dot", dot), ("dkt", dkt), ("dvt", dvt)):
        _f16(t, n)
    d.qt, d.ldqt, d.bsqt = qt.data_ptr(), qt.stride(1), qt.stride(0)
    d.dot, d.lddot, d.bsdot = dot.data_ptr(), dot.stride(1), dot.stride(0)
    d.dkt, d.lddkt, d.bsdkt = dkt.data_ptr(), dkt.stride(1), dkt.stride(0)
    d.dvt, d.lddvt, d.bsdvt = dvt.data_ptr(), dvt.stride(1), dvt.stride(0)
    with _timed("attention_bwd", 8.0 * d.B * d.H * d.Nq * d.Nk * d.D, f"dkv B{d.B} H{d.H} Nq{d.Nq} Nk{d.Nk} D{d.D}"):    # S, dP, dK, dV: 2 x forward
        check(lib.sg_attn_bwd_dkv_f16(C.byref(d), _stream()), "sg_attn_bwd_dkv_f16")
    return dkt, dvt


def debug_set_tile(bm: int = 0, bn: int = 0, no_pipe: bool = False) -> None:
    """Test hook: force the GEMM/conv tile shape / kernel family (0, 0 = automatic)."""
    check(lib.sg_debug_set_tile(bm, bn, int(no_pipe)), "sg_debug_set_tile")


def debug_set_option(name: str, value: int) -> None:
    """Development option of the library (sg_debug_set_option; names in include/storygen_hip.h)."""
    check(lib.sg_debug_set_option(name.encode(), int(value)), "sg_debug_set_option")


# The development tools (tools/*.py, tests) historically selected kernel variants through SG_* environment variables.  The
# library no longer reads the environment: this maps the variables onto sg_debug_set_option, and only when a tool asks for it.
_ENV_OPTIONS = {"SG_NO_NMAJOR": "no_nmajor", "SG_NO_PIPE": "no_pipe", "SG_NO_SPLIT": "no_split",
                "SG_ATTN_D160": "attn_d160",
                "SG_FF_VARIANT": "ff_variant", "SG_PIPE_STAGES": "pipe_stages", "SG_GN_FUSED_NT": "gn_fused_nt", "SG_GN_CHUNKS": "gn_chunks", "SG_ATTN_LEAN": "attn_lean", "SG_ATTN_D40_GENERAL": "attn_d40_general", "SG_ATTN_D40_LOOP": "attn_d40_loop","SG_NO_GN_FUSED": "gn_no_fused", "SG_GN_WIDE": "gn_wide", "SG_GN_FUSED_MAX": "gn_fused_max",
                "SG_LAT_TILES": "lat_tiles", "SG_LAT_MIN_KT": "lat_min_kt", "SG_LAT_MAX_KT": "lat_max_kt", "SG_LAT_STAGES": "lat_stages", "SG_LAT_WIDE": "lat_wide", "SG_LAT_MASK": "lat_mask", "SG_LAT_WIDE_M": "lat_wide_m", "SG_FAT_M": "fat_m", "SG_BIG_M": "big_m", "SG_BIG_BM": "big_bm", "SG_BIG_BN": "big_bn"}


def apply_env_options() -> dict:
    """Development tools only (never called by the product path): SG_* variables -> sg_debug_set_option.  Returns what was set."""
    import os
    done = {}
    for var, name in _ENV_OPTIONS.items():
        if os.environ.get(var, "") != "":
            debug_set_option(name, int(os.environ[var]))
            done[name] = int(os.environ[var])
    if os.environ.get("SG_TILE"):
        bm, bn = (int(v) for v in os.environ["SG_TILE"].split(","))
        debug_set_option("tile_m", bm), debug_set_option("tile_n", bn)
        done["tile"] = (bm, bn)
    return done


def debug_mfma_f8(a_bytes: torch.Tensor, b_bytes: torch.Tensor, scale_a: int = 127, scale_b: int = 127) -> torch.Tensor:
    """a_bytes, b_bytes: uint8 [64, 32] (raw fp8 e4m3 operand bytes per lane) -> fp32 [64, 16] accumulator registers."""
    if a_bytes.dtype != torch.uint8 or tuple(a_bytes.shape) != (64, 32) or not a_bytes.is_cuda or not a_bytes.is_contiguous():
        raise TypeError("debug_mfma_f8: a must be a contiguous CUDA uint8 [64, 32]")
    if b_bytes.dtype != torch.uint8 or tuple(b_bytes.shape) != (64, 32) or not b_bytes.is_cuda or not b_bytes.is_contiguous():
        raise TypeError("debug_mfma_f8: b must be a contiguous CUDA uint8 [64, 32]")
    out = torch.empty(64, 16, dtype=torch.float32, device=a_bytes.device)
    check(lib.sg_debug_mfma_f8_32x32x64(a_bytes.data_ptr(), b_bytes.data_ptr(), out.data_ptr(), scale_a, scale_b, _stream()),
          "sg_debug_mfma_f8_32x32x64")
    return out


def debug_mfma(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    out = torch.empty(64, 16, dtype=torch.float32, device=a.device)
    check(lib.sg_debug_mfma_32x32x16(a.data_ptr(), b.data_ptr(), out.data_ptr(), _stream()), "sg_debug_mfma_32x32x16")
    return out
