"""TEST INFRASTRUCTURE — the conformance cases that tie the hand-written CPU stand-ins of storygen_amd.ops (tests/fake_ops.py,
tests/ops_emulation.py and, through it, tests/clip_ops_emulation.py and tests/pick_ops_emulation.py) to the real entry points.

One Case per (entry point, contract feature).  `build(gen)` draws CPU inputs from a seeded generator, already rounded to the dtype the
op takes, and returns a Call: the arguments, the outputs to compare and a float64 evaluation of the same expression.  Every output is
a view inside a wider NaN-prefilled buffer where ops.py accepts a view, else a contiguous tensor with NaN guards before and after it;
in-place operands start finite between the same guards.  tests/test_standin_conformance_gpu.py runs ops.<name> on device copies that
keep the view structure (mirror()) against each stand-in; tests/test_standin_signatures.py runs the stand-in side alone on the CPU.

Bars are the project's existing ones, imported from the suites that own them; the few fp32 outputs no suite names a constant for are
explained where they are set."""
import importlib
import math

import torch
import torch.nn.functional as F

from test_forward_edges_gpu import ATTN_SMALL_BAR, F32_L2, F32_MAX
from test_kernels_gpu import TOL_L2, TOL_MAX
from test_pick_score_gpu import ATTN_BAR

F16, F32 = torch.float16, torch.float32
NAN = float("nan")
FMIN = torch.finfo(torch.float32).min
LOG2E = 1.4426950408889634
EPI_GEGLU = 1
MODULES = ("fake_ops", "ops_emulation", "clip_ops_emulation", "pick_ops_emulation")

# ---------------------------------------------------------------------------------------------------------------- bars
EQUAL = ("equal",)
HALF = ("rel", TOL_L2, TOL_MAX)                 # fp16 outputs
FLOAT = ("rel", F32_L2, F32_MAX)                # fp32 outputs: elementwise fp32 arithmetic, or fp32 sums of exact fp16 products
ENC = ("rel", ATTN_BAR, ATTN_BAR)               # attention_enc (tests/test_pick_score_gpu.py holds rel-L2 and max-rel to one bar)
SMALL = ("rel", ATTN_SMALL_BAR, ATTN_SMALL_BAR)
# the attention training pipeline, as tests/test_attention_backward_edges_gpu.py::_assert_case and tests/test_backward_gpu.py state
# them (literals there): o at the forward bar, max |lse2 - exact| <= 2e-3, delta / dq / dk / dv aggregate rel-L2 <= 5e-3
LSE = ("abs", 2e-3)
ATTN_BWD = ("rel", 5e-3, None)
# groupnorm_bwd's fp32 output: tests/test_backward_gpu.py::test_groupnorm_bwd holds it to rel-L2 1e-4 (fp32 statistics over a group and
# the derivative of SiLU through the hardware exponential); the max-rel bar keeps F32_MAX / F32_L2 = 10 x the rel-L2 one
GN_BWD_F32 = ("rel", 1e-4, 1e-3)


class Call:
    """args / kwargs: what the op is called with (CPU).  outs: name -> the tensor to compare (an argument, or a view of one).  ref(): name ->
    float64 expectation of that tensor, NaN where the contract leaves the NaN prefill alone.  bars: name -> bar.  inplace: names whose tensor
    starts finite (the op reads it).  ret: index of the argument the op returns (None: returns None; a tuple: a tuple of arguments)."""

    def __init__(self, args, kwargs=None, outs=None, ref=None, bars=None, inplace=(), ret=None):
        self.args, self.kwargs, self.outs, self.ref, self.bars, self.inplace, self.ret = list(args), kwargs or {}, outs, ref, bars, set(inplace), ret


class Case:
    def __init__(self, name, op, modules, build):
        self.name, self.op, self.modules, self.build = name, op, tuple(modules), build

    def __repr__(self):
        return self.name


def standin(module, op):
    return getattr(importlib.import_module("tests." + module), op)


def gen_for(case):
    return torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(case.name)) % (2 ** 31))


# ---------------------------------------------------------------------------------------------------------------- tensors
def rnd(g, *shape, dtype=F16, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype)


def window(shape, dtype=F16, pad=8, fill=None, lead=8, tail=8):
    """A [.., rows, cols] view with row stride cols + pad (outer dimensions dense over it) inside a flat NaN buffer with `lead` elements in
    front and `tail` behind.  pad = 0: a contiguous tensor between the guards.  fill: finite contents copied into the view."""
    shape = tuple(shape)
    ld = shape[-1] + pad
    strides = [1] * len(shape)
    if len(shape) > 1:
        strides[-2] = ld
        for i in range(len(shape) - 3, -1, -1):
            strides[i] = strides[i + 1] * shape[i + 1]
    rows = 1
    for n in shape[:-1]:
        rows *= n
    flat = torch.full((lead + rows * ld + tail,), NAN, dtype=dtype)
    v = torch.as_strided(flat, shape, strides, lead)
    if fill is not None:
        v.copy_(fill.to(dtype))
    return v


def strided(t, pad=8):
    """t as a row-strided view of a NaN buffer: an INPUT whose surroundings must not be read."""
    return window(t.shape, t.dtype, pad, fill=t)


def backing(t):
    """The whole storage of t as a flat tensor of its dtype."""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())


def mirror(obj, dev, cache):
    """Device copy of a tensor / container that keeps the view structure: storages are copied once, views rebuilt by as_strided."""
    if isinstance(obj, torch.Tensor):
        key = obj.untyped_storage().data_ptr()
        if key not in cache:
            cache[key] = backing(obj).to(dev)
        return torch.as_strided(cache[key], obj.size(), obj.stride(), obj.storage_offset())
    if isinstance(obj, (list, tuple)):
        return type(obj)(mirror(o, dev, cache) for o in obj)
    if isinstance(obj, dict):
        return {k: mirror(v, dev, cache) for k, v in obj.items()}
    return obj


def measure(got, want, bar):
    """(ok, text): `got` against the float64 `want` on the elements `want` defines (not NaN)."""
    m = ~torch.isnan(want)
    a, b = got.double()[m], want[m]
    if bar[0] == "equal":
        ok = bool(torch.equal(a, b))
        return ok, "equal" if ok else f"NOT equal (max |d| {float((a - b).abs().max()):.2e})"
    if bar[0] == "abs":
        e = float((a - b).abs().max()) if a.numel() else 0.0
        return e <= bar[1], f"max-abs {e:.1e}"
    if not bool(torch.isfinite(a).all()):
        return False, "non-finite"
    e2 = float((a - b).norm() / b.norm().clamp_min(1e-30))
    em = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) if a.numel() else 0.0
    return e2 <= bar[1] and (bar[2] is None or em <= bar[2]), f"rel-L2 {e2:.1e} max-rel {em:.1e}"


def d(t):
    return t.double()


def rto(v, dtype):
    """float64 -> the op's output dtype -> float64: the expectation of an exact (copy / cast) op."""
    return v.to(dtype).double()


def covered(views):
    """Boolean mask over the shared backing buffer of `views`: the elements some view addresses."""
    b = backing(views[0])
    idx = torch.arange(b.numel())
    m = torch.zeros(b.numel(), dtype=torch.bool)
    for v in views:
        m[torch.as_strided(idx, v.size(), v.stride(), v.storage_offset()).reshape(-1)] = True
    return m


def by_storage(outs):
    """The output views grouped by the buffer they live in: [(names, views)]."""
    groups = {}
    for n, v in outs.items():
        groups.setdefault(v.untyped_storage().data_ptr(), ([], []))
        groups[v.untyped_storage().data_ptr()][0].append(n)
        groups[v.untyped_storage().data_ptr()][1].append(v)
    return list(groups.values())


def returned(ret, args):
    """What an op returned, as positions in its argument list (the Call.ret convention)."""
    pos = lambda t: next((i for i, a in enumerate(args) if a is t), "a tensor that is no argument")
    if ret is None:
        return None
    return tuple(pos(t) for t in ret) if isinstance(ret, tuple) else pos(ret)


def check_side(who, call, outs, want, ret):
    """One side (a stand-in, or the real op with its outputs copied to the CPU) against the float64 expectation: the elements written
    (NaN pattern inside every view, guards around the views untouched), the values within the bar, the returned object.  Returns
    (report lines, failures)."""
    lines, fails = [], []
    for names, views in by_storage(outs):
        b = backing(views[0])
        if not bool(torch.isnan(b[~covered(views)].float()).all()):
            fails.append(f"{who}: wrote outside {' / '.join(names)}")
    for n, v in outs.items():
        w = want[n]
        if tuple(v.shape) != tuple(w.shape):
            fails.append(f"{who}: {n} is {tuple(v.shape)}, the expectation {tuple(w.shape)}")
            continue
        if not torch.equal(torch.isnan(v.float()), torch.isnan(w)):
            fails.append(f"{who}: {n} has {int(torch.isnan(v.float()).sum())} NaN, the contract leaves {int(torch.isnan(w).sum())}")
            continue
        ok, text = measure(v, w, call.bars[n])
        lines.append(f"{who} vs float64 {n}: {text}")
        if not ok:
            fails.append(f"{who} vs float64: {n} {text} outside {call.bars[n]}")
    if ret != call.ret:
        fails.append(f"{who}: returned argument {ret}, expected {call.ret}")
    return lines, fails


CASES, REFUSED = [], []
BOTH = ("fake_ops", "ops_emulation")


def case(name, op, modules):
    def deco(fn):
        CASES.append(Case(name, op, modules, fn))
        return fn
    return deco


def refused(name, op, modules):
    def deco(fn):
        REFUSED.append(Case(name, op, modules, fn))
        return fn
    return deco


# ---------------------------------------------------------------------------------------------------------------- gemm
def _gemm_ref(a, w, bias=None, rowbias=None, rpb=1, res1=None, res2=None, geglu=False):
    v = d(a) @ d(w).t()
    M, N = v.shape
    if bias is not None:
        v = v + d(bias)
    if rowbias is not None:
        v = v + d(rowbias)[torch.arange(M) // rpb, :N]
    if geglu:
        v = v.view(M, N // 64, 2, 32)
        return (v[:, :, 0] * 0.5 * v[:, :, 1] * (1.0 + torch.erf(v[:, :, 1] / math.sqrt(2.0)))).reshape(M, N // 2)
    for r in (res1, res2):
        if r is not None:
            v = v + d(r)
    return v


@case("gemm[bias+res1+res2]", "gemm", BOTH)
def _(g):
    M, N, K = 72, 72, 64
    a, w, bias = rnd(g, M, K), rnd(g, N, K, scale=0.2), rnd(g, N)
    r1, r2, out = strided(rnd(g, M, N)), strided(rnd(g, M, N, dtype=F32)), window((M, N))
    return Call([a, w, out], dict(bias=bias, res1=r1, res2=r2), {"out": out}, lambda: {"out": _gemm_ref(a, w, bias, res1=r1, res2=r2)},
                {"out": HALF}, ret=2)


@case("gemm[out2, fp32 out]", "gemm", BOTH)
def _(g):
    M, N, K = 40, 24, 64
    a, w, out, out2 = rnd(g, M, K), rnd(g, N, K, scale=0.2), window((M, N), F32), window((M, N))
    return Call([a, w, out], dict(out2=out2), {"out": out, "out2": out2}, lambda: {"out": _gemm_ref(a, w), "out2": _gemm_ref(a, w)},
                {"out": FLOAT, "out2": HALF}, ret=2)


@case("gemm[geglu N=128]", "gemm", BOTH)
def _(g):
    M, N, K = 40, 128, 64
    a, w, bias, out = rnd(g, M, K), rnd(g, N, K, scale=0.2), rnd(g, N), window((M, N // 2))
    return Call([a, w, out], dict(bias=bias, epilogue=EPI_GEGLU), {"out": out}, lambda: {"out": _gemm_ref(a, w, bias, geglu=True)},
                {"out": HALF}, ret=2)


@case("gemm[row-strided a, w, out]", "gemm", BOTH)
def _(g):
    M, N, K = 24, 16, 72
    a, w, out = strided(rnd(g, M, K), 16), strided(rnd(g, N, K, scale=0.2), 8), window((M, N), F16, 24)
    return Call([a, w, out], {}, {"out": out}, lambda: {"out": _gemm_ref(a, w)}, {"out": HALF}, ret=2)


@case("gemm[rowbias, 36 rows per batch]", "gemm", BOTH)
def _(g):
    M, N, K = 72, 16, 64
    a, w, rb, out = rnd(g, M, K), rnd(g, N, K, scale=0.2), strided(rnd(g, 2, N, dtype=F32)), window((M, N))
    return Call([a, w, out], dict(rowbias=rb, rows_per_batch=36), {"out": out}, lambda: {"out": _gemm_ref(a, w, rowbias=rb, rpb=36)},
                {"out": HALF}, ret=2)


# ---------------------------------------------------------------------------------------------------------------- conv3x3
def _conv_ref(x, w, stride=1, bias=None, rowbias=None, res1=None, padding=1):
    v = F.conv2d(d(x).permute(0, 3, 1, 2), d(w).permute(0, 3, 1, 2), stride=stride, padding=padding).permute(0, 2, 3, 1)
    if bias is not None:
        v = v + d(bias)
    if rowbias is not None:
        v = v + d(rowbias)[:, None, None, :v.shape[3]]
    if res1 is not None:
        v = v + d(res1)
    return v


def _bordered(x):
    """The zero-bordered [B, H+2, W+2, C] image of x."""
    B, H, W, C = x.shape
    p = torch.zeros(B, H + 2, W + 2, C, dtype=x.dtype)
    p[:, 1:-1, 1:-1] = x
    return p


def _conv_case(name, H, W, Cin=64, Cout=16, out_dtype=F16, **feat):
    @case(f"conv3x3[{name}]", "conv3x3", BOTH)
    def _(g):
        B = 2
        x, w = rnd(g, B, H, W, Cin), rnd(g, Cout, 3, 3, Cin, scale=0.1)
        kw, stride, xin, xr, pad = {}, feat.get("stride", 1), x, x, 1
        if feat.get("upsample2x"):
            kw["upsample2x"] = True
            xr = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
        if feat.get("padded"):
            kw["x_padded"], xin = True, _bordered(x)
        if feat.get("vae"):
            # VaeEngine._pad: the same storage shifted by one padded row and one pixel; F.pad(x, (0, 1, 0, 1)) + stride 2, padding 0
            n, off = B * (H + 2) * (W + 2) * Cin, (W + 3) * Cin
            flat = torch.zeros(n + off, dtype=F16)
            flat[:n].view(B, H + 2, W + 2, Cin)[:, 1:-1, 1:-1] = x
            kw["x_padded"], xin = True, flat[off:off + n].view(B, H + 2, W + 2, Cin)
            xr, pad = F.pad(x, (0, 0, 0, 1, 0, 1)), 0
        if stride != 1:
            kw["stride"] = stride
        Ho, Wo = ((xr.shape[1] - 1) // stride + 1, (xr.shape[2] - 1) // stride + 1) if pad else (H // 2, W // 2)
        out = window((B, Ho, Wo, Cout), out_dtype)
        bias = rnd(g, Cout) if feat.get("bias", True) else None
        rb = strided(rnd(g, B, Cout, dtype=F32)) if feat.get("rowbias") else None
        r1 = strided(rnd(g, B, Ho, Wo, Cout, dtype=feat.get("res1"))) if feat.get("res1") else None
        for k, v in (("bias", bias), ("rowbias", rb), ("res1", r1)):
            if v is not None:
                kw[k] = v
        return Call([xin, w, out], kw, {"out": out}, lambda: {"out": _conv_ref(xr, w, stride, bias, rb, r1, pad)},
                    {"out": HALF if out_dtype == F16 else FLOAT}, ret=2)


_conv_case("unpadded", 6, 5)
_conv_case("unpadded stride 2, odd size", 7, 5, stride=2)
_conv_case("x_padded stride 1", 6, 5, padded=True)
_conv_case("x_padded stride 2, UNet form", 6, 8, padded=True, stride=2)
_conv_case("x_padded stride 2, VAE shifted view", 6, 8, vae=True, stride=2, out_dtype=F32)
_conv_case("upsample2x", 3, 4, padded=True, upsample2x=True)
_conv_case("rowbias", 6, 5, padded=True, rowbias=True)
_conv_case("res1 fp32, fp32 out", 6, 5, padded=True, res1=F32, out_dtype=F32)
_conv_case("res1 fp16, no bias", 6, 5, res1=F16, bias=False)
_conv_case("Cin 64 Cout 72", 6, 5, Cout=72, padded=True)


# ---------------------------------------------------------------------------------------------------------------- conv_in / conv_out
for _cin in (4, 3):
    for _dt in (F16, F32):
        @case(f"conv_in[Cin {_cin}, {'fp16' if _dt == F16 else 'fp32'} out]", "conv_in", BOTH)
        def _(g, cin=_cin, dt=_dt):
            B, H, W, Co = 2, 5, 7, 16
            x, w, bias, out = rnd(g, B, cin, H, W, dtype=F32), rnd(g, 9 * cin, Co, scale=0.3), rnd(g, Co), window((B, H, W, Co), dt)
            wt = d(w).view(3, 3, cin, Co).permute(3, 2, 0, 1)
            return Call([x, w, bias, out], {}, {"out": out}, lambda: {"out": F.conv2d(d(x), wt, d(bias), padding=1).permute(0, 2, 3, 1)},
                        {"out": HALF if dt == F16 else FLOAT}, ret=3)

for _co in (3, 4):
    @case(f"conv_out[Cout {_co}]", "conv_out", BOTH)
    def _(g, co=_co):
        B, H, W, Ci = 2, 5, 7, 16
        x, w, bias, out = strided(rnd(g, B, H, W, Ci)), rnd(g, co, 3, 3, Ci, scale=0.2), rnd(g, 8), window((B, co, H, W), F32, 0)
        return Call([x, w, bias, out], {}, {"out": out},
                    lambda: {"out": F.conv2d(d(x).permute(0, 3, 1, 2), d(w).permute(0, 3, 1, 2), d(bias)[:co], padding=1)}, {"out": FLOAT}, ret=3)


# ---------------------------------------------------------------------------------------------------------------- norms
def _gn64(x, gamma, beta, groups, eps, silu):
    B, HW, C = x.shape
    xg = d(x).view(B, HW, groups, C // groups)
    mean, var = xg.mean((1, 3), keepdim=True), xg.var((1, 3), unbiased=False, keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + eps)).view(B, HW, C) * d(gamma) + d(beta)
    return y * torch.sigmoid(y) if silu else y


def _interior(v, B, H, W, C):
    """v [B, H*W, C] inside a [B, H+2, W+2, C] frame of NaN: the border the op must leave alone."""
    p = torch.full((B, H + 2, W + 2, C), NAN, dtype=torch.float64)
    p[:, 1:-1, 1:-1] = v.reshape(B, H, W, C)
    return p


def _ws(nbytes):
    return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8)


def _gn_case(name, x_dtype, silu, padded=False, xcopy=False):
    @case(f"groupnorm[{name}]", "groupnorm", BOTH)
    def _(g):
        from storygen_amd import ops
        B, H, W, C, groups, eps = 2, 4, 6, 64, 4, 1e-5
        x = strided(rnd(g, B, H * W, C, dtype=x_dtype, shift=0.5))
        gamma, beta = rnd(g, C, shift=1.0, scale=0.2), rnd(g, C, scale=0.2)
        out = window((B, H + 2, W + 2, C) if padded else (B, H * W, C))
        outs, bars, kw = {"out": out}, {"out": HALF}, {}
        if xcopy:
            kw["xcopy"] = outs["xcopy"] = window((B, H * W, C))
            bars["xcopy"] = EQUAL

        def ref():
            y = _gn64(x, gamma, beta, groups, eps, silu)
            r = {"out": _interior(y, B, H, W, C) if padded else y}
            if xcopy:
                r["xcopy"] = rto(d(x), F16)
            return r
        return Call([x, gamma, beta, out, groups, eps, silu, _ws(ops.groupnorm_workspace_bytes(B, groups))], kw, outs, ref, bars, ret=3)


_gn_case("3-D out, silu, fp16 x", F16, True)
_gn_case("3-D out, no silu, fp32 x", F32, False)
_gn_case("4-D bordered out, silu, fp32 x", F32, True, padded=True)
_gn_case("4-D bordered out + xcopy, no silu, fp16 x", F16, False, padded=True, xcopy=True)
_gn_case("xcopy of fp32 x", F32, True, xcopy=True)


def _gn_bwd_case(name, x_dtype, dy_dtype, silu, form):
    @case(f"groupnorm_bwd[{name}]", "groupnorm_bwd", ("fake_ops",))
    def _(g):
        from storygen_amd import ops
        B, H, W, C, groups, eps = 2, 4, 6, 64, 4, 1e-5
        x, dy = strided(rnd(g, B, H * W, C, dtype=x_dtype, shift=0.5)), strided(rnd(g, B, H * W, C, dtype=dy_dtype))
        gamma, beta = rnd(g, C, shift=1.0, scale=0.2), rnd(g, C, scale=0.2)
        res = strided(rnd(g, B, H * W, C, dtype=F32)) if form == "f32res" else None
        out = {"f32res": lambda: window((B, H * W, C), F32), "f16": lambda: window((B, H * W, C)),
               "f16pad": lambda: window((B, H + 2, W + 2, C), F16, 0)}[form]()

        def ref():
            xr = d(x).clone().requires_grad_(True)
            with torch.enable_grad():
                (dx,) = torch.autograd.grad(_gn64(xr, gamma, beta, groups, eps, silu), xr, d(dy))
            if res is not None:
                dx = dx + d(res)
            return {"out": _interior(dx, B, H, W, C) if form == "f16pad" else dx}
        return Call([x, dy, gamma, beta, out, groups, eps, silu, _ws(ops.groupnorm_bwd_workspace_bytes(B, groups))],
                    {} if res is None else {"res": res}, {"out": out}, ref, {"out": GN_BWD_F32 if form == "f32res" else HALF}, ret=4)


_gn_bwd_case("fp32 out + res, silu, fp32 x, fp16 dy", F32, F16, True, "f32res")
_gn_bwd_case("fp16 out, no silu, fp16 x, fp32 dy", F16, F32, False, "f16")
_gn_bwd_case("bordered fp16 out, silu, fp16 x", F16, F16, True, "f16pad")


def _ln64(x, gamma, beta, eps):
    xd = d(x)
    return (xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + eps) * d(gamma) + d(beta)


for _dual, _xd in ((False, F32), (True, F32), (True, F16)):
    @case(f"layernorm[{'dual' if _dual else 'single'}, {'fp32' if _xd == F32 else 'fp16'} x]", "layernorm", BOTH)
    def _(g, dual=_dual, xd=_xd):
        M, C, eps = 9, 64, 1e-5
        x = strided(rnd(g, M, C, dtype=xd, shift=0.3))
        g1, b1, g2, b2 = rnd(g, C, shift=1.0, scale=0.2), rnd(g, C, scale=0.2), rnd(g, C, shift=1.0, scale=0.2), rnd(g, C, scale=0.2)
        y1, y2 = window((M, C)), window((M, C), F16, 16)
        if not dual:
            return Call([x, g1, b1, y1, eps], {}, {"y1": y1}, lambda: {"y1": _ln64(x, g1, b1, eps)}, {"y1": HALF})
        return Call([x, g1, b1, y1, eps], dict(g2=g2, b2=b2, y2=y2), {"y1": y1, "y2": y2},
                    lambda: {"y1": _ln64(x, g1, b1, eps), "y2": _ln64(x, g2, b2, eps)}, {"y1": HALF, "y2": HALF})

for _name, _two, _res in (("plain", False, False), ("dy2 / g2", True, False), ("res, res_scale 0.5", False, True), ("dy2 / g2 + res", True, True)):
    @case(f"layernorm_bwd[{_name}]", "layernorm_bwd", ("fake_ops",))
    def _(g, two=_two, with_res=_res):
        M, C, eps = 9, 64, 1e-5
        x, dy1, dy2 = strided(rnd(g, M, C, dtype=F32, shift=0.3)), strided(rnd(g, M, C)), strided(rnd(g, M, C))
        g1, g2, res, out = rnd(g, C, shift=1.0, scale=0.2), rnd(g, C, shift=1.0, scale=0.2), strided(rnd(g, M, C, dtype=F32)), window((M, C), F32)
        kw = {}
        if two:
            kw.update(dy2=dy2, g2=g2)
        if with_res:
            kw.update(res=res, res_scale=0.5)

        def ref():
            xr = d(x).clone().requires_grad_(True)
            with torch.enable_grad():
                xhat = (xr - xr.mean(-1, keepdim=True)) / torch.sqrt(xr.var(-1, unbiased=False, keepdim=True) + eps)
                (dx,) = torch.autograd.grad(xhat, xr, d(dy1) * d(g1) + (d(dy2) * d(g2) if two else 0.0))
            return {"out": dx + 0.5 * d(res) if with_res else dx}
        return Call([x, dy1, g1, out, eps], kw, {"out": out}, ref, {"out": FLOAT}, ret=3)


# ---------------------------------------------------------------------------------------------------------------- copies
for _xd in (F32, F16):
    @case(f"pad_cast[{'fp32' if _xd == F32 else 'fp16'} x]", "pad_cast", BOTH)
    def _(g, xd=_xd):
        B, H, W, C = 2, 3, 5, 16
        x, out = strided(rnd(g, B, H, W, C, dtype=xd)), window((B, H + 2, W + 2, C), F16, 0)
        return Call([x, out], {}, {"out": out}, lambda: {"out": _interior(rto(d(x), F16), B, H, W, C)}, {"out": EQUAL}, ret=1)

for _name, _sd, _dd in (("fp16 -> fp16", F16, F16), ("fp32 -> fp32", F32, F32), ("fp32 -> fp16", F32, F16)):
    @case(f"copy_rows[{_name}]", "copy_rows", BOTH)
    def _(g, sd=_sd, dd=_dd):
        src, dst = strided(rnd(g, 2, 5, 16, dtype=sd), 16), window((2, 5, 16), dd)
        return Call([dst, src], {}, {"dst": dst}, lambda: {"dst": rto(d(src), dd)}, {"dst": EQUAL}, ret=0)

for _sd in (F16, F32):
    @case(f"transpose[{'fp32' if _sd == F32 else 'fp16'} src]", "transpose", ("fake_ops",))
    def _(g, sd=_sd):
        src, dst = strided(rnd(g, 16, 24, dtype=sd)), window((24, 16))
        return Call([src, dst], {}, {"dst": dst}, lambda: {"dst": rto(d(src).t(), F16)}, {"dst": EQUAL}, ret=1)

    @case(f"transpose_batched[{'fp32' if _sd == F32 else 'fp16'} src]", "transpose_batched", ("fake_ops",))
    def _(g, sd=_sd):
        src, dst = strided(rnd(g, 2, 16, 24, dtype=sd)), window((2, 24, 16))
        return Call([src, dst], {}, {"dst": dst}, lambda: {"dst": rto(d(src).transpose(1, 2), F16)}, {"dst": EQUAL}, ret=1)

    @case(f"zero_stuff[{'fp32' if _sd == F32 else 'fp16'} dy]", "zero_stuff", ("fake_ops",))
    def _(g, sd=_sd):
        B, Ho, Wo, C = 2, 3, 4, 16
        dy, out = strided(rnd(g, B, Ho, Wo, C, dtype=sd)), window((B, 2 * Ho + 2, 2 * Wo + 2, C), F16, 0)

        def ref():
            inner = torch.zeros(B, 2 * Ho, 2 * Wo, C, dtype=torch.float64)
            inner[:, ::2, ::2] = rto(d(dy), F16)
            return {"out": _interior(inner, B, 2 * Ho, 2 * Wo, C)}
        return Call([dy, out], {}, {"out": out}, ref, {"out": EQUAL}, ret=1)

for _acc in (False, True):
    @case(f"sum2x2[accumulate={_acc}]", "sum2x2", ("fake_ops",))
    def _(g, acc=_acc):
        B, H, W, C = 2, 3, 4, 16
        du, old = strided(rnd(g, B, 2 * H, 2 * W, C, dtype=F32)), rnd(g, B, H, W, C, dtype=F32)
        dx = window((B, H, W, C), F32, fill=old if acc else None)
        return Call([du, dx], dict(accumulate=acc), {"dx": dx},
                    lambda: {"dx": d(du).reshape(B, H, 2, W, 2, C).sum(dim=(2, 4)) + (d(old) if acc else 0.0)}, {"dx": FLOAT},
                    inplace=("dx",) if acc else (), ret=1)


@case("geglu_bwd", "geglu_bwd", ("fake_ops",))
def _(g):
    M, N8 = 5, 128
    proj, du, dproj = strided(rnd(g, M, N8)), strided(rnd(g, M, N8 // 2)), window((M, N8))

    def ref():
        pr = d(proj).view(M, N8 // 64, 2, 32)
        val, gate, u = pr[:, :, 0], pr[:, :, 1], d(du).view(M, N8 // 64, 32)
        cdf, pdf = 0.5 * (1.0 + torch.erf(gate / math.sqrt(2.0))), torch.exp(-0.5 * gate * gate) / math.sqrt(2.0 * math.pi)
        return {"dproj": torch.stack([u * gate * cdf, u * val * (cdf + gate * pdf)], dim=2).reshape(M, N8)}
    return Call([proj, du, dproj], {}, {"dproj": dproj}, ref, {"dproj": HALF}, ret=2)


for _name in ("zeros", "ones", "mixed"):
    @case(f"mse_grad[mask of {_name}]", "mse_grad", ("fake_ops",))
    def _(g, kind=_name):
        shape = (2, 4, 8, 8)
        pred, noise = rnd(g, *shape, dtype=F32), rnd(g, *shape, dtype=F32)
        mask = {"zeros": torch.zeros(shape), "ones": torch.ones(shape),
                "mixed": torch.tensor([0.0, 1.0, 0.25, 0.0])[torch.randint(0, 4, shape, generator=g)]}[kind]
        d_pred, loss = window(shape, F32, 0), window((1,), F32, 0)

        def ref():
            keep = 1.0 - d(mask)
            e = (d(pred) - d(noise)) * keep
            return {"d_pred": 2.0 * e * keep / e.numel(), "loss": (e * e).mean().reshape(1)}
        return Call([pred, noise, mask, d_pred, loss], {}, {"d_pred": d_pred, "loss": loss}, ref, {"d_pred": FLOAT, "loss": FLOAT}, ret=3)

for _flip in (True, False):
    @case(f"timestep_embed[flip_sin_to_cos={_flip}]", "timestep_embed", ("fake_ops",))
    def _(g, flip=_flip):
        t, freqs, out = torch.tensor([0.0, 3.0, 12.0]), torch.exp(-math.log(1e4) * torch.arange(16, dtype=F32) / 16), window((3, 32), F32, 0)

        def ref():
            e = d(t)[:, None] * d(freqs)[None]
            return {"out": torch.cat([torch.cos(e), torch.sin(e)] if flip else [torch.sin(e), torch.cos(e)], -1)}
        return Call([t, freqs, out, flip], {}, {"out": out}, ref, {"out": FLOAT}, ret=2)

for _ai, _ao in ((True, False), (False, True)):
    @case(f"linear_rows[act_in={_ai}, act_out={_ao}]", "linear_rows", ("fake_ops",))
    def _(g, ai=_ai, ao=_ao):
        x, w, bias, out = strided(rnd(g, 3, 16, dtype=F32)), strided(rnd(g, 24, 16, scale=0.3)), rnd(g, 24), window((3, 24), F32)

        def ref():
            xi = d(x) * torch.sigmoid(d(x)) if ai else d(x)
            v = xi @ d(w).t() + d(bias)
            return {"out": v * torch.sigmoid(v) if ao else v}
        return Call([x, w, bias, out], dict(act_in=ai, act_out=ao), {"out": out}, ref, {"out": FLOAT}, ret=3)


# ---------------------------------------------------------------------------------------------------------------- encoder ops
@case("softmax_rows[N = 13 inside a wider probs]", "softmax_rows", ("ops_emulation",))
def _(g):
    M, N = 5, 13
    scores, probs = strided(rnd(g, M, N, dtype=F32, scale=3.0), 3), window((M, 16))

    def ref():
        p = torch.zeros(M, 16, dtype=torch.float64)         # columns [N, N rounded up to 8) are written as zeros
        p[:, :N] = torch.softmax(d(scores) * 0.7, -1)
        return {"probs": p}
    return Call([scores, probs], dict(scale=0.7), {"probs": probs}, ref, {"probs": HALF}, ret=1)


def _attn64(q, k, v, heads, scale, causal, key_bias):
    B, T, C = q.shape
    qh, kh, vh = (d(t).reshape(B, T, heads, C // heads).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) * scale
    if key_bias is not None:
        s = s + d(key_bias)[:, None, None, :]
    if causal:
        s = s + torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, T, C)


def _attn_case(op, modules, T, bar, name, causal, biased):
    @case(f"{op}[{name}]", op, modules)
    def _(g):
        B, H, D = 2, 2, 16
        C = H * D
        qkv = strided(rnd(g, B, T, 3 * C), 8)                   # q | k | v as column slices of one projection output
        q, k, v = qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
        out = window((B, T, C), F16, 16)                         # token stride H*D + 16
        kb = None
        if biased:                                               # a padding mask: the last keys of batch 1 at finfo.min
            kb = torch.zeros(B, T)
            kb[1, T - 3:] = FMIN
        scale = D ** -0.5
        return Call([q, k, v, out, H, scale, causal], {} if kb is None else {"key_bias": kb}, {"out": out},
                    lambda: {"out": _attn64(q, k, v, H, scale, causal, kb)}, {"out": bar}, ret=3)


for _name, _causal, _biased in (("causal", True, False), ("finfo.min key bias", False, True), ("causal + key bias", True, True)):
    _attn_case("attention_small", ("ops_emulation", "pick_ops_emulation"), 77, SMALL, _name, _causal, _biased)
    _attn_case("attention_enc", ("pick_ops_emulation",), 70, ENC, _name, _causal, _biased)

for _act in (0, 1):
    @case(f"act_rows[{('quick_gelu', 'gelu')[_act]}]", "act_rows", ("ops_emulation",))
    def _(g, act=_act):
        x0 = rnd(g, 5, 16, scale=2.0)
        x = window((5, 16), F16, fill=x0)
        return Call([x, act], {}, {"x": x},
                    lambda: {"x": d(x0) * torch.sigmoid(1.702 * d(x0)) if act == 0 else 0.5 * d(x0) * (1.0 + torch.erf(d(x0) / math.sqrt(2.0)))},
                    {"x": HALF}, inplace=("x",), ret=0)


@case("embed_tokens", "embed_tokens", ("ops_emulation",))
def _(g):
    T, C = 3, 16
    ids, tok, pos, out = torch.randint(0, 11, (6,), generator=g), rnd(g, 11, C, dtype=F32), rnd(g, 4, C, dtype=F32), window((6, C), F32)
    return Call([ids, tok, pos, out, T], {}, {"out": out}, lambda: {"out": rto(d(tok)[ids] + d(pos)[torch.arange(6) % T], F32)}, {"out": EQUAL}, ret=3)


for _noisy in (True, False):
    @case(f"gaussian_sample[{'noise' if _noisy else 'mode'}, logvar beyond both clamps]", "gaussian_sample", ("ops_emulation",))
    def _(g, noisy=_noisy):
        shape = (2, 4, 4, 4)
        mean, logvar, noise, out = rnd(g, *shape, dtype=F32), rnd(g, *shape, dtype=F32, scale=4.0), rnd(g, *shape, dtype=F32), window(shape, F32, 0)
        logvar.view(-1)[:4] = torch.tensor([-40.0, 30.0, -30.0, 20.0])
        return Call([mean, logvar, noise if noisy else None, out], dict(scale=0.18215), {"out": out},
                    lambda: {"out": (d(mean) + (torch.exp(0.5 * d(logvar).clamp(-30.0, 20.0)) * d(noise) if noisy else 0.0)) * 0.18215},
                    {"out": FLOAT}, ret=3)


def _patch64(x, S, ps, mean, std, in_scale, in_shift):
    from tests import clip_vision_reference as R
    RH, RW, top, left = R.resize_geometry(x.shape[2], x.shape[3], S)
    v = F.interpolate(d(x) * in_scale + in_shift, size=(RH, RW), mode="bicubic", antialias=True, align_corners=False)[:, :, top:top + S, left:left + S]
    v = (v - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    return R.patch_rows(v, ps)


CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


@case("clip_patchify[plain]", "clip_patchify", ("clip_ops_emulation", "pick_ops_emulation"))
def _(g):
    S, ps = 8, 4
    x, out = torch.rand(2, 3, 13, 16, generator=g), window((2 * 4, 48))
    return Call([x, out, S, ps, CLIP_MEAN, CLIP_STD], dict(in_scale=0.5, in_shift=0.25), {"out": out},
                lambda: {"out": _patch64(x, S, ps, CLIP_MEAN, CLIP_STD, 0.5, 0.25)}, {"out": HALF}, ret=1)


@case("clip_patchify[kpad 16 of 12 columns, out 24 wide]", "clip_patchify", ("pick_ops_emulation",))
def _(g):
    S, ps, K, kpad = 8, 2, 12, 16
    x, out = torch.rand(2, 3, 16, 11, generator=g), window((2 * 16, 24))

    def ref():
        r = torch.full((32, 24), NAN, dtype=torch.float64)      # columns beyond kpad are left alone
        r[:, :K], r[:, K:kpad] = _patch64(x, S, ps, CLIP_MEAN, CLIP_STD, 1.0, 0.0), 0.0
        return {"out": r}
    return Call([x, out, S, ps, CLIP_MEAN, CLIP_STD], dict(kpad=kpad), {"out": out}, ref, {"out": HALF}, ret=1)


@case("clip_embed_patches", "clip_embed_patches", ("clip_ops_emulation",))
def _(g):
    B, T, C = 2, 5, 16
    patches, cls, pos, out = strided(rnd(g, B * (T - 1), C, dtype=F32)), rnd(g, C, dtype=F32), rnd(g, T, C, dtype=F32), window((B * T, C), F32)

    def ref():
        v = torch.empty(B, T, C, dtype=torch.float64)
        v[:, 0], v[:, 1:] = d(cls) + d(pos)[0], d(patches).view(B, T - 1, C) + d(pos)[1:]
        return {"out": v.view(B * T, C)}
    return Call([patches, cls, pos, out, T], {}, {"out": out}, ref, {"out": FLOAT}, ret=3)


# ---------------------------------------------------------------------------------------------------------------- attention (training)
TB, TH, TD, TNQ, TNK = 2, 2, 40, 72, 77


def _heads(t):
    B, N, C = t.shape
    return d(t).reshape(B, N, TH, C // TH).transpose(1, 2)


def _merge(t):
    B, H, N, D = t.shape
    return t.transpose(1, 2).reshape(B, N, H * D)


def _transposed(x, extra=16):
    """[B, N, C] -> the [B, C, N rounded up to 8] operand (zero padded) as a view of a [B, C, N8 + extra] buffer of NaN."""
    B, N, C = x.shape
    N8 = (N + 7) & ~7
    t = torch.zeros(B, C, N8, dtype=F16)
    t[:, :, :N] = x.transpose(1, 2)
    return strided(t, extra)


def _train_inputs(g):
    C = TH * TD
    q, k, v, do = rnd(g, TB, TNQ, C), rnd(g, TB, TNK, C), rnd(g, TB, TNK, C), rnd(g, TB, TNQ, C, scale=0.5)
    scale = TD ** -0.5
    s = _heads(q) @ _heads(k).transpose(-1, -2) * scale
    lse = torch.logsumexp(s, -1)
    o = _merge(torch.exp(s - lse[..., None]) @ _heads(v))
    return q, k, v, do, scale, (lse * LOG2E).to(F32), o.to(F16)


def _bwd64(q, k, v, do, ld2, scale):
    qh, kh, vh, doh = (_heads(t) for t in (q, k, v, do))
    p = torch.exp2(qh @ kh.transpose(-1, -2) * (scale * LOG2E) - d(ld2)[..., 0][..., None])
    ds = p * (doh @ vh.transpose(-1, -2) - d(ld2)[..., 1][..., None])
    return _merge(ds @ kh * scale), _merge(ds.transpose(-1, -2) @ qh * scale), _merge(p.transpose(-1, -2) @ doh)


def _ld2_of(o, do, lse2):
    delta = (d(o) * d(do)).reshape(TB, TNQ, TH, TD).sum(-1).transpose(1, 2)
    return torch.stack([lse2, delta.to(F32)], -1).contiguous()


@case("attention_lse[D 40, nk 77 of 80 keys, vt wider than nk]", "attention_lse", ("fake_ops",))
def _(g):
    q, k, v, _, scale, lse2_ref, _ = _train_inputs(g)
    k80 = torch.cat([k, rnd(g, TB, 3, TH * TD)], 1)              # three more finite key rows that nk = 77 excludes
    vt, out, lse2 = _transposed(v), window((TB, TNQ, TH * TD)), window((TB, TH, TNQ), F32, 0)

    def ref():
        s = _heads(q) @ _heads(k).transpose(-1, -2) * scale
        lse = torch.logsumexp(s, -1)
        return {"out": _merge(torch.exp(s - lse[..., None]) @ _heads(v)), "lse2": lse * LOG2E}
    return Call([q, k80, vt, out, lse2, TH, scale], dict(nk=TNK), {"out": out, "lse2": lse2}, ref, {"out": HALF, "lse2": LSE}, ret=3)


@case("attention_bwd_prep", "attention_bwd_prep", ("fake_ops",))
def _(g):
    _, _, _, do, _, lse2, o = _train_inputs(g)
    o, do, ld2 = strided(o), strided(do), window((TB, TH, TNQ, 2), F32, 0)
    return Call([o, do, lse2, ld2, TH], {}, {"ld2[..., 0]": ld2[..., 0], "ld2[..., 1]": ld2[..., 1]},
                lambda: {"ld2[..., 0]": d(lse2), "ld2[..., 1]": (d(o) * d(do)).reshape(TB, TNQ, TH, TD).sum(-1).transpose(1, 2)},
                {"ld2[..., 0]": EQUAL, "ld2[..., 1]": ATTN_BWD}, ret=3)


@case("attention_bwd_dq[Nk 77, kt padded to 80 in a wider buffer]", "attention_bwd_dq", ("fake_ops",))
def _(g):
    q, k, v, do, scale, lse2, o = _train_inputs(g)
    ld2, dq = _ld2_of(o, do, lse2), window((TB, TNQ, TH * TD))
    return Call([q, k, _transposed(k), v, do, ld2, dq, TH, scale], {}, {"dq": dq}, lambda: {"dq": _bwd64(q, k, v, do, ld2, scale)[0]},
                {"dq": ATTN_BWD}, ret=6)


@case("attention_bwd_dkv[dkt / dvt rows of 77 in 88-wide buffers]", "attention_bwd_dkv", ("fake_ops",))
def _(g):
    q, k, v, do, scale, lse2, o = _train_inputs(g)
    ld2 = _ld2_of(o, do, lse2)
    dkt, dvt = window((TB, TH * TD, TNK), F16, 11), window((TB, TH * TD, TNK), F16, 11)

    def ref():
        _, dk, dv = _bwd64(q, k, v, do, ld2, scale)
        return {"dkt": dk.transpose(1, 2), "dvt": dv.transpose(1, 2)}
    return Call([q, _transposed(q), k, v, do, _transposed(do), ld2, dkt, dvt, TH, scale], {}, {"dkt": dkt, "dvt": dvt}, ref,
                {"dkt": ATTN_BWD, "dvt": ATTN_BWD}, ret=(7, 8))


# ---------------------------------------------------------------------------------------------------------------- cfg_*_step
LAT = (2, 4, 8, 8)


def _guided(eps3, c):
    eu, ei, ea = d(eps3)
    return eu + c[0] * (ei - eu) + c[1] * (ea - ei)


def _step_case(op, name, coef, build_extra, update, with_l3):
    """build_extra(g) -> (extra arguments between latents3 and coef, outs of the state, inplace names); update(e, x, c, extra) -> (new x,
    name -> float64 state expectations), all on float64 with c = the fp32 coefficients as float64."""
    @case(f"{op}[{name}, latents3 {'present' if with_l3 else 'absent'}]", op, ("fake_ops",))
    def _(g):
        eps3, x0 = rnd(g, 3, *LAT, dtype=F32), rnd(g, *LAT, dtype=F32)
        lat = window(LAT, F32, 0, fill=x0)
        l3 = window((3,) + LAT, F32, 0) if with_l3 else None
        cf = torch.tensor(coef, dtype=F32)
        extra, st_outs, st_inplace = build_extra(g)
        c = [float(v) for v in cf.double()]

        def ref():
            xn, state = update(_guided(eps3, c), d(x0), c[2:], extra)
            r = {"latents": xn, **state}
            if with_l3:
                r["latents3"] = xn.expand((3,) + LAT)
            return r
        outs = {"latents": lat, **st_outs}
        if with_l3:
            outs["latents3"] = l3
        return Call([eps3, lat, l3, *extra, cf], {}, outs, ref, {n: FLOAT for n in outs}, inplace=("latents", *st_inplace), ret=1)


for _l3 in (True, False):
    _step_case("cfg_ddim_step", "ddim", [7.5, 3.5, 0.8, 0.6, 0.85, 0.52], lambda g: ((), {}, ()),
               lambda e, x, c, extra: (c[2] * ((x - c[1] * e) / c[0]) + c[3] * e, {}), _l3)


def _var_case(clip, std, l3):
    def extra(g):
        return ((rnd(g, *LAT, dtype=F32),) if std else (None,)), {}, ()

    def update(e, x, c, ex):
        x0 = (x - c[1] * e) / c[0]
        xp = c[2] * (x0.clamp(-1, 1) if clip else x0) + c[3] * e
        return (xp + c[4] * d(ex[0]) if std else xp), {}
    _step_case("cfg_ddim_var_step", f"clip {'on' if clip else 'off'}, std {std:g}", [7.5, 3.5, 0.8, 0.6, 0.85, 0.4, std, float(clip)], extra, update, l3)


for _i, (_clip, _std) in enumerate(((0, 0.0), (0, 0.3), (1, 0.0), (1, 0.3))):
    _var_case(_clip, _std, _i % 2 == 0)


def _plms_case(name, w, slots, push, use_kept, keep, l3):
    def extra(g):
        hist0, kept0 = rnd(g, 4, *LAT, dtype=F32), rnd(g, *LAT, dtype=F32)
        hist, kept = window((4,) + LAT, F32, 0, fill=hist0), window(LAT, F32, 0, fill=kept0)
        return (hist, kept), {"history": hist, "kept": kept}, ("history", "kept")

    def update(e, x, c, ex):
        hist, kept = d(ex[0]).clone(), d(ex[1]).clone()          # (ref() runs before either side touches them)
        ep = c[2] * e + sum(c[2 + i] * hist[s] for i, s in ((1, slots[1]), (2, slots[2]), (3, slots[3])) if c[2 + i])
        if push:
            hist[slots[0]] = e
        xs = kept.clone() if use_kept else x
        if keep:
            kept = x.clone()
        return c[0] * xs - c[1] * ep, {"history": hist, "kept": kept}
    _step_case("cfg_plms_step", name, [7.5, 3.5, 1.02, 0.11, *w, *map(float, slots), float(push), float(use_kept), float(keep)], extra, update, l3)


_plms_case("first step: pushes and keeps", (1.0, 0.0, 0.0, 0.0), (0, 3, 2, 1), 1, 0, 1, True)
_plms_case("second visit: uses kept, keeps, no push", (0.5, 0.5, 0.0, 0.0), (1, 0, 3, 2), 0, 1, 1, False)
_plms_case("steady state: four weights live", (55 / 24, -59 / 24, 37 / 24, -9 / 24), (0, 3, 2, 1), 1, 0, 0, True)


def _dpm_case(order, l3):
    w = {1: (0.9, 0.0, 0.0), 2: (1.3, -0.4, 0.0), 3: (1.6, -0.9, 0.25)}[order]
    cur, s1, s2 = 0, 2, 1

    def extra(g):
        hist0 = rnd(g, 3, *LAT, dtype=F32)
        for i, (wi, s) in enumerate(((w[1], s1), (w[2], s2))):
            if not wi:
                hist0[s] = NAN                                   # a ring slot no step has written yet, under a zero weight
        hist = window((3,) + LAT, F32, 0, fill=hist0)
        return (hist,), {"history": hist}, ("history",)

    def update(e, x, c, ex):
        hist = d(ex[0]).clone()
        m = c[0] * x + c[1] * e
        xp = c[2] * x + c[3] * m + sum(c[4 + i] * hist[s] for i, s in ((0, s1), (1, s2)) if c[4 + i])
        hist[cur] = m
        return xp, {"history": hist}
    _step_case("cfg_dpm_step", f"order {order}", [7.5, 3.5, -0.3, 1.1, 0.97, *w, float(cur), float(s1), float(s2), 1.0], extra, update, l3)


for _order in (1, 2, 3):
    _dpm_case(_order, _order != 2)


# ---------------------------------------------------------------------------------------------------------------- refusals
# Argument sets a stand-in refuses by its own assert / raise: the real op must raise ValueError before any launch (the library checks
# shapes on the host: SG_EINVAL) and leave the output all NaN.  Each is outside a documented limit; none reaches a kernel.
def _refused_attn(op, modules, name, T, H, D, pad=16):
    @refused(f"{op}[{name}]", op, modules)
    def _(g):
        q, k, v = (rnd(g, 1, T, H * D) for _ in range(3))
        out = window((1, T, H * D), F16, pad)
        return Call([q, k, v, out, H, D ** -0.5, False], {}, {"out": out})


_refused_attn("attention_small", ("ops_emulation", "pick_ops_emulation"), "T = 129", 129, 1, 16)
_refused_attn("attention_small", ("ops_emulation", "pick_ops_emulation"), "D = 72", 8, 1, 72)
_refused_attn("attention_enc", ("pick_ops_emulation",), "T = 1025", 1025, 1, 8)
_refused_attn("attention_enc", ("pick_ops_emulation",), "D = 136", 8, 1, 136)
_refused_attn("attention_enc", ("pick_ops_emulation",), "D = 12", 8, 2, 12, pad=8)


@refused("conv_in[Cin = 9]", "conv_in", BOTH)
def _(g):
    out = window((1, 4, 4, 16))
    return Call([rnd(g, 1, 9, 4, 4, dtype=F32), rnd(g, 81, 16), rnd(g, 16), out], {}, {"out": out})


@refused("conv_out[Cout = 5]", "conv_out", BOTH)
def _(g):
    out = window((1, 5, 4, 4), F32, 0)
    return Call([rnd(g, 1, 4, 4, 16), rnd(g, 5, 3, 3, 16), rnd(g, 8), out], {}, {"out": out})


@refused("gemm[K = 12]", "gemm", BOTH)
def _(g):
    out = window((8, 16))
    return Call([rnd(g, 8, 12), rnd(g, 16, 12), out], {}, {"out": out})


@refused("gemm[geglu, N = 96]", "gemm", BOTH)
def _(g):
    out = window((8, 48))
    return Call([rnd(g, 8, 16), rnd(g, 96, 16), out], dict(epilogue=EPI_GEGLU), {"out": out})


@refused("conv3x3[Cin = 60]", "conv3x3", BOTH)
def _(g):
    out = window((1, 4, 4, 8))
    return Call([rnd(g, 1, 4, 4, 60), rnd(g, 8, 3, 3, 60), out], {}, {"out": out})


@refused("clip_patchify[3 * ps * ps = 27]", "clip_patchify", ("clip_ops_emulation", "pick_ops_emulation"))
def _(g):
    out = window((4, 27), F16, 5)
    return Call([torch.rand(1, 3, 8, 8, generator=g), out, 6, 3, CLIP_MEAN, CLIP_STD], {}, {"out": out})


@refused("clip_patchify[kpad = 12]", "clip_patchify", ("pick_ops_emulation",))
def _(g):
    out = window((16, 16))
    return Call([torch.rand(1, 3, 8, 8, generator=g), out, 8, 2, CLIP_MEAN, CLIP_STD], dict(kpad=12), {"out": out})
