"""UNetEngine — StoryGen's UNet forward on the HIP kernels (fp16 channels-last activations, fp32 accumulate).

Re-design of /root/reference/model/unet_2d_condition.py:338-485 (+ unet_2d_blocks.py forward paths and
attention.py:85-128,236-302) around what the MI355X wants rather than around nn.Module calls:

  * every activation is a channels-last matrix [B*H*W, C] — fp32 for the residual stream, fp16 for everything that
    feeds an MFMA; the transformer's token layout IS that matrix, so the reference's permute/reshape pairs
    (attention.py:103,117) disappear;
  * weights are repacked once and shared by every engine (EngineWeights): KRSC convs, fused q|k projections, V
    projections kept separate because they are computed TRANSPOSED (VT = Wv . X^T, the attention kernel's operand
    layout), [Wo2 | Wo3] for the single out-projection of the two cross-attentions, 32/32-interleaved GEGLU, all 22
    time_emb_proj stacked into one GEMV bundle whose output, plus the conv1 bias, becomes conv1's per-sample
    channel bias;
  * residual adds, biases, the `(a2+h)+(a3+h)` combine (attention.py:277,291-293) and GEGLU live in GEMM/conv
    epilogues; nearest-2x upsampling and stride-2 are folded into the conv gather; `torch.cat([h, skip])`
    costs nothing: the producer of h and the down-path producer of the skip both write their columns of the
    consuming resnet's concat buffer;
  * harvested features (attention.py:263) are written straight into slot r of the preallocated context buffers
    [B, R*HW, C] that the main pass cross-attends to (replaces the clones at unet_2d_condition.py:428-429,445,
    468-470 and the token-axis concat at pipeline.py:440-443);
  * all buffers are allocated up front, nothing allocates or synchronises inside `forward`, timestep values are
    read from device memory — so a whole pass (or a whole denoising step) can be captured in one hipGraph;
  * independent branches inside a pass (1x1 shortcut beside conv1 -> norm2, text attention beside image attention)
    can run on a side stream (`forward(side=...)`), and a reference pass can also run the attn3 K / V^T projections
    of each context it completes (HarvestPlan.kv), taking them off the main pass's critical path.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional

import torch

from . import ops
from .arch import BlockSpec, ResnetSpec, UNetArch, XfSpec, feature_shapes
from .repack import conv1x1_nk, conv3x3_krsc, conv_in_kn, ff_fused_pack, fold_layernorm, interleave_geglu, upsample_phase_pack

F16 = torch.float16
GN_EPILOGUE_STATS = True   # GroupNorm statistics from the producing conv / GEMM epilogues (False = every GroupNorm makes its own pass)
# Experiment, default off: the residual stream INSIDE a transformer block (h0: proj_in output, h1: after
# self-attention, h2/h3: after the cross-attentions) in fp16 instead of fp32; block inputs / outputs and the resnets stay fp32.  Halves
# the bytes of 3 GEMM outputs, 3 residual reads and 3 LayerNorm reads per block; costs fp16 rounding of the stream.  tools/exp_fp16_stream.py
FP16_BLOCK_STREAM = False
FP16_RESNET_STREAM = False   # same experiment for the rest of the stream: resnet / transformer / shortcut outputs and the skip-concat buffers
PAIR_GEMMS = True     # q|k + V^T, q2 + q3, k3 + v3^T as one launch each (sg_gemm_pair_f16); False = two launches (A/B switch)
# LayerNorm folded into the GEMM that consumes it (round 3; model/attention.py:250,268,283,298): the producers of h0 / h1 / h3 also
# write the raw fp16 copy and per-token partial statistics, the q|k / V^T / q2 / q3 / GEGLU projections run on the raw copy with
# gamma-scaled weights and normalise in their epilogues (sg_gemm_desc.ln_*).  No LayerNorm launch is left in a pass (-94 launches
# per step).  False = the separate layernorm kernel (A/B switch).
LN_FOLD = True
# Text and image cross-attention of a block in one launch (sg_attn_fwd_pair_f16).  Measured on the contract workload (r3c12: 14.69 /
# 14.70 ms paired vs 14.62 ms): the text attention already runs on the side stream beside the context K / V^T projections, and one
# grid after them gives that overlap up — so the default stays two launches (A/B: bench.py --attn-pair).
ATTN_PAIR = False
# Split-K convolutions at the 16x16 / 8x8 levels leave their second pass to the one-launch GroupNorm that consumes them (round 4;
# sg_conv3x3_desc.defer_reduce + sg_groupnorm_desc.split_*): conv1 -> norm2 of every ResnetBlock2D there, and conv2 -> Transformer2DModel.norm
# where a transformer follows.  Bit-identical values, one launch and one round trip of the tensor less per site.  False = separate
# splitk_reduce launches (A/B switch).
SPLITK_IN_GN = True
# GEGLU feed-forward of a transformer block as ONE launch where the kernel exists (C = 320, the 64x64 level: sg_ff_geglu_fused_f16;
# SURVEY 8(f) rank 2 — cross-layer fusion): norm3 -> Linear(C, 8C) -> a gelu(g) -> Linear(4C, C) -> + h with the [M, 4C] intermediate
# kept in registers.  False = LayerNorm-folded GEGLU GEMM + second GEMM (A/B switch: bench.py --no-ff-fused).
FF_FUSED = True
# Fused feed-forward launches of at most this many tokens split the hidden dimension over two workgroups per 128 tokens (round 5;
# sg_ff_desc.hidden_split): 12 288 tokens of the main pass are 96 workgroups on 256 CUs and the launch lasts as long as ONE wave's walk
# over the 40 hidden chunks.  The two partial sums land in the halves of an [M, 2C] buffer and proj_out contracts them with [W | W].
# 0 = never (A/B switch: bench.py --no-ff-split).
FF_SPLIT_MAX_TOKENS = 16384
# ff.net.2 and proj_out are two linear maps with nothing but a residual add between them (model/attention.py:300 `ff(norm3(h)) + h`, then
# :121-123 proj_out + the block's input): out = W_out (W_2 g + b_2 + h3) + b_out + x = [g | h3] [W_out W_2 | W_out]^T + (W_out b_2 + b_out) + x
# — ONE GEMM with K = 4C + C over the GEGLU output and the raw fp16 copy of h3 side by side in one buffer, the same FLOPs, one launch
# (and one fp16 rounding of an intermediate) less per transformer block at C = 640 / 1280 (round 6; the 64x64 level runs the fused
# feed-forward kernel instead).  False = the two GEMMs as written (A/B switch: bench.py --no-ff-proj-merge).
FF_PROJ_MERGE = True
# Upsample2D (nearest 2x + 3x3) as four 2x2 convolutions of the input-resolution image, one per output parity, on tap sums packed with
# the weights (repack.upsample_phase_pack; sg_conv3x3_desc.upsample2x = 2): 4/9 of the multiply-adds, one more fp16 rounding of the
# weights.  A launch the form does not fit (no row tile divides H W) keeps the 3x3 form.  False = the 3x3 form everywhere (A/B switch).
UPSAMPLE_PHASES = True
# ... from this many output rows (B * 2H * 2W) on.  Below, the launch is its weight stream and the pack is 16/9 of the 3x3 weights'
# bytes: the 8x8 -> 16x16 launch of the batch-3 main pass (768 rows, 52 MB of packed weights) measured 42.2 us against 41.6 us in the
# 3x3 form and stays there; the same level at batch 20 (5 120 rows) 150 against 168 us (profiles/r20b_per_shape.txt).
UPSAMPLE_PHASES_MIN_ROWS = 1024
LN_EPS = 1e-5         # torch.nn.LayerNorm default, as the reference constructs norm1..norm4 (model/attention.py:213-233)


def _pair(first, second):
    if PAIR_GEMMS:
        ops.gemm_pair(first, second)
    else:       # (the projections that are paired stay off the latency kernel either way: tile hint (0, 0, -1))
        for args, kw in (first, second):
            ops.gemm(*args, **{**kw, "tile": (0, 0, -1)})


class _Resnet:
    __slots__ = ("spec", "n1g", "n1b", "w1", "n2g", "n2b", "w2", "b2", "wsc", "bsc", "temb_off")


class _Xf:
    __slots__ = ("spec", "ng", "nb", "w_in", "b_in", "w_out", "b_out", "ln", "w_qk1", "w_v1", "w_o1", "b_o1", "w_q2", "w_k2",
                 "w_v2", "w_o2", "b_o2", "w_q3", "w_k3", "w_v3", "w_o3", "b_o3", "w_o23", "b_o23", "w_ff1", "b_ff1", "w_ff2", "b_ff2",
                 # LayerNorm-folded copies (repack.fold_layernorm): weight gamma (.) W in fp16, c / d in fp32
                 "w_qk1f", "c_qk1", "d_qk1", "w_v1f", "c_v1", "d_v1", "w_q2f", "c_q2", "d_q2", "w_q3f", "c_q3", "d_q3",
                 "w_ff1f", "c_ff1", "d_ff1",
                 "ff_pack",     # weight stream of the fused feed-forward kernel (repack.ff_fused_pack), or None
                 "w_out2",      # [W_out | W_out]: proj_out over the two partial sums of a hidden-split fused feed-forward
                 "w_ffo", "b_ffo")   # FF_PROJ_MERGE: [W_out W_ff2 | W_out] (fp32 product rounded once) and W_out b_ff2 + b_out, or None


class EngineWeights:
    """The checkpoint repacked once into the layouts the kernels consume (fp16, on the device).  Shared by every
    UNetEngine built on it (the reference-pass engine and the main-pass engine of the sampler use one copy)."""

    def __init__(self, arch: UNetArch, state_dict: Dict[str, torch.Tensor], device):
        self.arch, self.dev, self.cfg = arch, torch.device(device), arch.config
        self.version = 0                 # bumped by reload_(): anything derived from the weights and cached by an engine (time tables) is stale then
        self._load_weights(state_dict)

    def _w(self, sd, key) -> torch.Tensor:
        return sd[key].detach().to(device=self.dev, dtype=F16).contiguous()

    def _load_weights(self, sd):
        dev, arch = self.dev, self.arch
        g = lambda k: self._w(sd, k)  # noqa: E731
        self.w_conv_in = conv_in_kn(g("conv_in.weight"))
        self.b_conv_in = g("conv_in.bias")
        self.w_t1, self.b_t1 = g("time_embedding.linear_1.weight"), g("time_embedding.linear_1.bias")
        self.w_t2, self.b_t2 = g("time_embedding.linear_2.weight"), g("time_embedding.linear_2.bias")
        half = cfg_half = self.cfg["block_out_channels"][0] // 2
        # diffusers Timesteps: exp(-ln(1e4) * j / (half - shift)) computed in fp32 by torch, as the reference does
        self.freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32)
                               / (cfg_half - self.cfg["freq_shift"])).to(dev)
        self.resnets: Dict[str, _Resnet] = {}
        temb_w, temb_b, off = [], [], 0
        for r in arch.resnets:
            p = r.prefix
            o = _Resnet()
            o.spec = r
            o.n1g, o.n1b = g(f"{p}.norm1.weight"), g(f"{p}.norm1.bias")
            o.w1 = conv3x3_krsc(g(f"{p}.conv1.weight"))
            o.n2g, o.n2b = g(f"{p}.norm2.weight"), g(f"{p}.norm2.bias")
            o.w2, o.b2 = conv3x3_krsc(g(f"{p}.conv2.weight")), g(f"{p}.conv2.bias")
            if r.has_shortcut:
                o.wsc, o.bsc = conv1x1_nk(g(f"{p}.conv_shortcut.weight")), g(f"{p}.conv_shortcut.bias")
            else:
                o.wsc = o.bsc = None
            temb_w.append(g(f"{p}.time_emb_proj.weight"))
            # conv1 bias + time_emb_proj bias are both per-channel constants of the same add (resnet forward)
            temb_b.append((sd[f"{p}.time_emb_proj.bias"].float() + sd[f"{p}.conv1.bias"].float()).to(dev, F16))
            o.temb_off = off
            off += r.cout
            self.resnets[p] = o
        self.w_temb = torch.cat(temb_w, 0).contiguous()
        self.b_temb = torch.cat(temb_b, 0).contiguous()
        self.temb_total = off
        self.xfs: Dict[str, _Xf] = {}
        for blk in arch.blocks:
            for a in blk.attns:
                if a is None:
                    continue
                p, t = a.prefix, f"{a.prefix}.transformer_blocks.0"
                o = _Xf()
                o.spec = a
                o.ng, o.nb = g(f"{p}.norm.weight"), g(f"{p}.norm.bias")
                o.w_in, o.b_in = conv1x1_nk(g(f"{p}.proj_in.weight")), g(f"{p}.proj_in.bias")
                o.w_out, o.b_out = conv1x1_nk(g(f"{p}.proj_out.weight")), g(f"{p}.proj_out.bias")
                o.ln = {n: (g(f"{t}.{n}.weight"), g(f"{t}.{n}.bias")) for n in ("norm1", "norm2", "norm3", "norm4")}
                # q and k projections fused (one GEMM, token-major output); v separate: it is computed TRANSPOSED
                # (VT = Wv . X^T, the same GEMM with its operands swapped), the layout the attention kernel streams
                o.w_qk1 = torch.cat([g(f"{t}.attn1.to_q.weight"), g(f"{t}.attn1.to_k.weight")], 0).contiguous()
                o.w_v1 = g(f"{t}.attn1.to_v.weight")
                o.w_o1, o.b_o1 = g(f"{t}.attn1.to_out.0.weight"), g(f"{t}.attn1.to_out.0.bias")
                o.w_q2 = g(f"{t}.attn2.to_q.weight")
                o.w_k2, o.w_v2 = g(f"{t}.attn2.to_k.weight"), g(f"{t}.attn2.to_v.weight")
                o.w_o2, o.b_o2 = g(f"{t}.attn2.to_out.0.weight"), g(f"{t}.attn2.to_out.0.bias")
                o.w_q3 = g(f"{t}.attn3.to_q.weight")
                o.w_k3, o.w_v3 = g(f"{t}.attn3.to_k.weight"), g(f"{t}.attn3.to_v.weight")
                o.w_o3, o.b_o3 = g(f"{t}.attn3.to_out.0.weight"), g(f"{t}.attn3.to_out.0.bias")
                # main pass: (attn2.to_out(a2) + h) + (attn3.to_out(a3) + h) (attention.py:277,291-293) is ONE GEMM over the
                # concatenated heads [a2 | a3] with weights [Wo2 | Wo3] (K = 2C), bias b2 + b3 and the residual h twice
                o.w_o23 = torch.cat([o.w_o2, o.w_o3], dim=1).contiguous()
                o.b_o23 = (sd[f"{t}.attn2.to_out.0.bias"].float() + sd[f"{t}.attn3.to_out.0.bias"].float()).to(dev, F16)
                o.w_ff1, o.b_ff1 = interleave_geglu(g(f"{t}.ff.net.0.proj.weight"), g(f"{t}.ff.net.0.proj.bias"))
                o.w_ff2, o.b_ff2 = g(f"{t}.ff.net.2.weight"), g(f"{t}.ff.net.2.bias")
                for name, val in self._pack_folds(o).items():
                    setattr(o, name, val)
                o.ff_pack = ff_fused_pack(o.w_ff1f, o.d_ff1, o.w_ff2) if (ops.ff_fused_supported(a.channels) and dev.type == "cuda") else None
                o.w_out2 = torch.cat([o.w_out, o.w_out], dim=1).contiguous() if o.ff_pack is not None else None
                if o.ff_pack is None:         # ff.net.2 and proj_out as one K = 5C GEMM (FF_PROJ_MERGE)
                    wo32 = o.w_out.float()
                    o.w_ffo = torch.cat([(wo32 @ o.w_ff2.float()).to(F16), o.w_out], dim=1).contiguous()
                    o.b_ffo = (wo32 @ o.b_ff2.float() + o.b_out.float()).to(F16).contiguous()
                else:
                    o.w_ffo = o.b_ffo = None
                self.xfs[p] = o
        self.samplers = {}
        for blk in arch.down + arch.up:
            if blk.sampler_prefix:
                self.samplers[blk.sampler_prefix] = (conv3x3_krsc(g(f"{blk.sampler_prefix}.weight")),
                                                     g(f"{blk.sampler_prefix}.bias"))
        # Upsample2D convolutions as four 2x2 phase convolutions (UPSAMPLE_PHASES): tap sums per output parity, [4, Cout, 2, 2, Cin].  The
        # 3x3 weights above stay: a launch the phase form does not fit (ops.conv3x3_upsample) and the A/B switch run on them.
        self.sampler_phases = {blk.sampler_prefix: upsample_phase_pack(g(f"{blk.sampler_prefix}.weight"))
                               for blk in arch.up if blk.sampler_prefix}
        self.gn_out = (g("conv_norm_out.weight"), g("conv_norm_out.bias"))
        self.w_conv_out = conv3x3_krsc(g("conv_out.weight"))
        self.b_conv_out = g("conv_out.bias")

    @staticmethod
    def _pack_folds(xf: "_Xf", which=("qk1", "v1", "q2", "q3", "ff1")) -> Dict[str, torch.Tensor]:
        """LayerNorm-folded operand copies of the projections that follow norm1 (q|k, v), norm2 (q2), norm4 (q3) and norm3 (GEGLU):
        W' = gamma (.) W in fp16, c = row sums of W', d = W beta (+ bias)."""
        src = {"qk1": (xf.w_qk1, None, "norm1"), "v1": (xf.w_v1, None, "norm1"), "q2": (xf.w_q2, None, "norm2"),
               "q3": (xf.w_q3, None, "norm4"), "ff1": (xf.w_ff1, xf.b_ff1, "norm3")}
        out = {}
        for k in which:
            w, b, n = src[k]
            wf, c, d = fold_layernorm(w, b, *xf.ln[n])
            out[f"w_{k}f"], out[f"c_{k}"], out[f"d_{k}"] = wf.contiguous(), c.contiguous(), d.contiguous()
        return out

    # ---- in-place refresh: captured hipGraphs and engines hold the ADDRESSES of the repacked tensors, so new parameter
    # values are copied into the existing storage (same shapes) instead of re-allocating
    def _pack_attn3(self, sd, xf: "_Xf") -> Dict[str, torch.Tensor]:
        t = f"{xf.spec.prefix}.transformer_blocks.0"
        g = lambda k: self._w(sd, k)  # noqa: E731
        w_o3 = g(f"{t}.attn3.to_out.0.weight")
        return {"w_q3": g(f"{t}.attn3.to_q.weight"), "w_k3": g(f"{t}.attn3.to_k.weight"), "w_v3": g(f"{t}.attn3.to_v.weight"),
                "w_o3": w_o3, "b_o3": g(f"{t}.attn3.to_out.0.bias"), "w_o23": torch.cat([xf.w_o2, w_o3], dim=1),
                "b_o23": (sd[f"{t}.attn2.to_out.0.bias"].float() + sd[f"{t}.attn3.to_out.0.bias"].float()).to(self.dev, F16)}

    def refresh_attn3_(self, sd, prefixes=None):
        """Stage-2 training changes only the attn3 modules (train_StorySalon_stage2.py:170-177): re-pack those of the given
        Transformer2DModel prefixes (default: all) from `sd`, in place."""
        for p, xf in self.xfs.items():
            if prefixes is None or p in prefixes:
                for name, val in self._pack_attn3(sd, xf).items():
                    getattr(xf, name).copy_(val)
                for name, val in self._pack_folds(xf, ("q3",)).items():
                    getattr(xf, name).copy_(val)

    def _pack_attn1(self, sd, xf: "_Xf") -> Dict[str, torch.Tensor]:
        t = f"{xf.spec.prefix}.transformer_blocks.0"
        g = lambda k: self._w(sd, k)  # noqa: E731
        return {"w_qk1": torch.cat([g(f"{t}.attn1.to_q.weight"), g(f"{t}.attn1.to_k.weight")], 0), "w_v1": g(f"{t}.attn1.to_v.weight"),
                "w_o1": g(f"{t}.attn1.to_out.0.weight"), "b_o1": g(f"{t}.attn1.to_out.0.bias")}

    def refresh_attn1_(self, sd, prefixes=None):
        """Stage-1 training changes only the attn1 modules (train_StorySalon_stage1.py:175-179): the same in-place re-pack for them."""
        for p, xf in self.xfs.items():
            if prefixes is None or p in prefixes:
                for name, val in self._pack_attn1(sd, xf).items():
                    getattr(xf, name).copy_(val)
                for name, val in self._pack_folds(xf, ("qk1", "v1")).items():
                    getattr(xf, name).copy_(val)

    def reload_(self, sd):
        """Re-pack the whole checkpoint into the existing tensors (any parameter may have changed)."""
        fresh = EngineWeights.__new__(EngineWeights)
        fresh.arch, fresh.dev, fresh.cfg = self.arch, self.dev, self.cfg
        fresh._load_weights(sd)

        def walk(old, new):
            if torch.is_tensor(old):
                old.copy_(new)
            elif isinstance(old, dict):
                for k in old:
                    walk(old[k], new[k])
            elif isinstance(old, (tuple, list)):
                for a, b in zip(old, new):
                    walk(a, b)
            elif isinstance(old, (_Resnet, _Xf)):
                for k in old.__slots__:
                    if k != "spec" and getattr(old, k, None) is not None:
                        walk(getattr(old, k), getattr(new, k))
        for k, v in self.__dict__.items():
            if k not in ("arch", "dev", "cfg", "version"):
                walk(v, getattr(fresh, k))
        self.version += 1


class HarvestPlan:
    """Where a reference pass puts the features it harvests (attention.py:263).

    `ctx` are the context buffers of the engine that will consume them ([rows, R*HW, C] fp16 per feature key) and each
    op (src, src_step, dst_row, dst_slot, count) means: for j < count, slot dst_slot+j of ctx row dst_row <- the
    feature of sample src + j*src_step of this pass.  One strided copy per op (src_step = 0 broadcasts one sample
    into `count` frame slots)."""

    def __init__(self, ctx: Dict[str, torch.Tensor], ops_: List[tuple], kv: Optional[Dict[str, tuple]] = None,
                 src_offset: int = 0, short: int = 0, slots_per_row: Optional[int] = None, direct: bool = False,
                 identity: bool = False):
        # kv: feature key -> (K [rows*R*HW, C], VT [C, rows*R*HW]) buffers: when given, the reference pass also runs the
        # attn3 K / V^T projections of each finished context (they depend on nothing else), taking them off the main
        # pass's critical path.
        # src_offset: added to every op's `src` — a reference pass that batches the samples of several denoising steps
        # (sampler ref_ahead > 1) passes one plan per step, each pointing at that step's slice of the batch.
        # short / slots_per_row: layout of the DESTINATION buffers (UNetEngine ctx_short): the first `short` context rows hold one
        # frame slot, the others slots_per_row; flat slot of (row, slot) = row if row < short else short + (row - short) * R + slot.
        # direct: the pass's sample u belongs in flat slot u for every u (sampler._plan orders the batch that way), so the
        # producer of the feature writes its fp16 copy straight into the context buffer and no copy kernel runs.
        # identity: the CALLER guarantees that mapping for buffers it laid out itself — `ctx` / `kv` are flat [samples * HW, C]
        # matrices in the pass's sample order (the sampler's group schedule: the context sets of G steps end to end); no ops.
        self.ctx, self.ops, self.kv, self.src_offset = ctx, list(ops_), kv, int(src_offset)
        self.short, self.slots_per_row, self.direct = int(short), slots_per_row, bool(direct) or bool(identity)
        self.identity = bool(identity)
        if self.identity and (self.ops or self.src_offset):
            raise ValueError("an identity harvest plan has no copy ops and no source offset")

    def flat_slot(self, row: int, slot: int, R: int) -> int:
        return row if row < self.short else self.short + (row - self.short) * R + slot

    def is_direct(self, n_samples: int, R: int) -> bool:
        """True when this plan alone maps sample u -> flat slot u for all n_samples samples of the pass."""
        if self.identity:
            return all(c.dim() == 2 and c.shape[0] % n_samples == 0 for c in self.ctx.values())
        if not self.direct or self.src_offset:
            return False
        seen = {}
        for src, step, row, slot, cnt in self.ops:
            for j in range(cnt):
                seen[self.flat_slot(row, slot + j, R)] = src + j * step
        return seen == {u: u for u in range(n_samples)}


class _GnFeed(NamedTuple):
    """What a GroupNorm that reads a stream tensor needs to know beyond the tensor itself.  Every producer of a stream tensor returns
    this for its `out`, every consumer takes it for its `x`.  pstats: statistics the producers' epilogues wrote, one (buffer, rows per
    partial, channels) entry, or two in channel order for a concat [h | skip].  split: the tensor is still the K slices of a split-K
    convolution, which the GroupNorm must sum (the dict ops.groupnorm(split=...) takes).  Neither: it makes its own pass over x."""
    pstats: Optional[list] = None
    split: Optional[dict] = None

    @staticmethod
    def concat(h: "_GnFeed", skip: "_GnFeed", channels: int) -> "_GnFeed":
        """For cat = [h | skip] of `channels` columns: the statistics of both parts, when both have some and they cover the columns."""
        if h.pstats and skip.pstats and h.pstats[0][2] + skip.pstats[0][2] == channels:
            return _GnFeed(pstats=h.pstats + skip.pstats)
        return _NO_FEED


_NO_FEED = _GnFeed()


class _XfPass:
    """What one pass through a transformer derives from the module switches, the engine and its operands: made once per call (at call
    time: the switches are A/B knobs), read by every stage (UNetEngine._xf_*)."""

    def __init__(self, eng: "UNetEngine", xf: _Xf, x: torch.Tensor, x_gn: _GnFeed, out: Optional[torch.Tensor], lvl: int, consume: bool):
        L = self.L = eng.lv[lvl]
        self.xf, self.x, self.x_gn, self.out, self.lvl, self.consume, self.guard = xf, x, x_gn, out, lvl, consume, eng.ln_guard
        self.B, self.hw, self.M, self.C, self.heads = eng.B, eng.hw[lvl], x.shape[0], xf.spec.channels, xf.spec.heads
        self.scale = xf.spec.dim_head ** -0.5
        self.fold = LN_FOLD and self.C % 64 == 0 and self.C // 64 <= 20
        # fused feed-forward: needs the fp32 stream (it reads h3 itself: no raw copy, no LayerNorm partials from h3's producer)
        self.ff1 = FF_FUSED and xf.ff_pack is not None and L["h3"].dtype != F16
        # ff.net.2 + proj_out as one GEMM (FF_PROJ_MERGE): h3's raw copy lives beside the GEGLU output in L["ffo"]
        self.merge = FF_PROJ_MERGE and self.fold and not self.ff1 and xf.w_ffo is not None and L["h3"].dtype != F16 and out is not None
        self.h0r, self.h1r = self.raw(L["h0"], L["ln"]), self.raw(L["h1"], L["ln4"])
        self.h3raw = L["ffo"][:self.M, 4 * self.C:5 * self.C] if self.merge else L["ln"]

    @staticmethod
    def raw(t: torch.Tensor, buf: torch.Tensor) -> torch.Tensor:
        return t if t.dtype == F16 else buf                      # (fp16 stream: it IS the copy)

    def prod(self, t: torch.Tensor, buf: torch.Tensor, st: torch.Tensor) -> dict:
        """With the fold, the producer of a stream tensor also writes its raw fp16 copy and the LayerNorm partials of its rows."""
        return dict(out2=None if t.dtype == F16 else buf, ln_out=st, guard=self.guard) if self.fold else {}

    def prod3(self, h3: torch.Tensor) -> dict:
        return {} if self.ff1 else self.prod(h3, self.h3raw, self.L["lnst3"])


class UNetEngine:
    def __init__(self, arch: UNetArch, state_dict: Optional[Dict[str, torch.Tensor]], device, batch: int, height: int,
                 width: int, n_ref: int = 0, seq_len: int = 77, splitk_workspace_mb: int = 96,
                 weights: Optional[EngineWeights] = None, ctx_rows: Optional[int] = None,
                 attn3_groups: Optional[List[tuple]] = None, fp8_attention: bool = False, ctx_short: int = 0,
                 cfg_shared_head: bool = False, fp16_stream: Optional[tuple] = None):
        """fp16_stream = (block, resnet) or None (= the module switches FP16_BLOCK_STREAM / FP16_RESNET_STREAM): per ENGINE, which
        parts of the residual stream are stored as fp16 — block: the transformer state h0 / h1 (h2 / h3 stay fp32: they feed the fused
        feed-forward and the merged proj_out); resnet: block inputs / outputs, shortcut outputs, skip / concat buffers.
        batch = samples per UNet call; n_ref = R prior frames (sizes the context buffers; 0 = an engine that only
        harvests, into another engine's buffers).  ctx_rows = number of distinct context rows (default: one per
        sample); attn3_groups = [(q0, n, c0), ...]: samples [q0, q0+n) cross-attend to context rows [c0, c0+n) — lets
        samples whose prior-frame features are identical (the two image-conditioned CFG branches) share
        one copy of the context and of its K/V projection.  ctx_short = S > 0: the first S context rows hold ONE frame slot instead
        of R (the zero-image rows of `multi-image-condition`, whose R slots would be R copies of one feature map: softmax over R
        copies of the same keys is softmax over one); the context buffers are then flat [(S + (rows - S) R) HW, C] matrices.
        cfg_shared_head: the caller guarantees the classifier-free-guidance pattern of the loop's main pass (pipeline.py:448-453) with
        one story frame: batch 3 = the SAME latent and timestep three times, text rows [uncond, uncond, text], context rows [zero-image,
        frames, frames].  Until the first cross-attention the three samples are then the same computation, so forward(consume=True) runs
        conv_in, the first ResnetBlock2D and the first transformer's norm / proj_in / self-attention / to_out / query projections ONCE
        (batch 1), the text attention for (uncond, text) and the image attention for (zero-image, frames) only, and copies the results to
        the samples that share them — the same arithmetic on the same values (bit-exact redundancy removal)."""
        self.arch, self.dev = arch, torch.device(device)
        self.B, self.H, self.W, self.R, self.S = batch, height, width, n_ref, seq_len
        cfg = arch.config
        self.cfg = cfg
        nlev = len(cfg["block_out_channels"])
        if height % (1 << (nlev - 1)) or width % (1 << (nlev - 1)):
            raise ValueError(f"latent size {height}x{width} must be divisible by {1 << (nlev - 1)}")
        self.groups, self.eps = cfg["norm_num_groups"], cfg["norm_eps"]
        self.cad = cfg["cross_attention_dim"]
        self.hw = [(height >> l) * (width >> l) for l in range(nlev)]
        self.Sp = (seq_len + 7) & ~7          # text tokens padded with zero rows to a multiple of 8 (V^T row alignment)
        for k, lv in arch.feature_level.items():
            if self.hw[lv] % 8:
                raise ValueError(f"latent {height}x{width} leaves {self.hw[lv]} tokens at attention block {k}; the V^T layout "
                                 "needs a multiple of 8 (use a latent of at least 32x32 with the 4-level SD-1.5 UNet)")
        self.ctx_rows = batch if ctx_rows is None else ctx_rows
        self.attn3_groups = [(0, batch, 0)] if attn3_groups is None else list(attn3_groups)
        covered = sorted(q for q0, n, _ in self.attn3_groups for q in range(q0, q0 + n))
        if n_ref and (covered != list(range(batch)) or any(c0 + n > self.ctx_rows for _, n, c0 in self.attn3_groups)):
            raise ValueError(f"attn3_groups {self.attn3_groups} must cover samples 0..{batch - 1} once, within {self.ctx_rows} context rows")
        # the common sharing pattern maps onto the kernel's kv_batches argument (one launch instead of one per group)
        rows = self.ctx_rows
        share = sorted(self.attn3_groups) == ([(0, batch, 0)] if rows == batch else [(0, rows, 0), (rows, batch - rows, 2 * rows - batch)])
        self.attn3_share = rows if share else None
        self.ctx_short = int(ctx_short)
        if self.ctx_short and (not n_ref or self.attn3_share is None or self.ctx_short > rows):
            raise ValueError("ctx_short needs context buffers, at most ctx_rows short rows and the shared-row attn3 pattern")
        self.ctx_slots = self.ctx_short + (rows - self.ctx_short) * n_ref      # frame slots per feature key
        first = arch.down[0]
        self.cfg_shared_head = bool(cfg_shared_head)
        if self.cfg_shared_head and not (batch == 3 and n_ref and rows == 2 and self.attn3_share == 2 and self.ctx_short in (0, 1)
                                         and first.attns and first.attns[0] is not None and not fp8_attention):
            raise ValueError("cfg_shared_head needs batch 3 on 2 shared context rows (the CFG main pass of one story frame), a transformer "
                             "behind the first resnet and the fp16 attention path")
        self._head_checked = False
        self.fp16_block, self.fp16_resnet = (FP16_BLOCK_STREAM, FP16_RESNET_STREAM) if fp16_stream is None else map(bool, fp16_stream)
        self.wts = weights if weights is not None else EngineWeights(arch, state_dict, device)
        # BASELINE config 5: the head-dim-40 self / image attentions (the 46 080-key context of the 96x96 level) on the fp8 MFMA
        # path (sg_attn_fwd_f8_d40); text attention and the D = 80 / 160 levels stay fp16
        self.fp8_attention = bool(fp8_attention)
        # GroupNorm statistics as producer epilogues (north-star; HISTORY.md 5): a conv / GEMM whose output feeds a wide GroupNorm also
        # writes per-(row tile, channel) sums, and that GroupNorm skips its own statistics pass.  Per producer site: what its output
        # hands to a GroupNorm — its buffer with the cached answer of sg_*_stats_tile_rows, or nothing when that answer is 0 (this
        # launch cannot emit them -> the consumer makes its own pass).
        self.gn_epilogue_stats = GN_EPILOGUE_STATS
        self._stats_site: Dict[str, _GnFeed] = {}
        self._stats_want: Dict[tuple, bool] = {}
        self.text_cache: Dict[str, torch.Tensor] = {}
        # sticky flags of the LayerNorm fold's two assumptions (ops.LN_GUARD_*; include/storygen_hip.h): every producer / consumer of a
        # folded LayerNorm ORs into this word; check_ln_guard() reads it (one 4-byte D2H copy: call it where the host synchronises anyway)
        self.ln_guard = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._alloc(splitk_workspace_mb)

    def __getattr__(self, name):
        # repacked weights live in the shared EngineWeights object
        wts = self.__dict__.get("wts")
        if wts is not None and hasattr(wts, name):
            return getattr(wts, name)
        raise AttributeError(name)

    # ------------------------------------------------------------------------------------------ buffers
    def _buf(self, *shape, dtype=F16) -> torch.Tensor:
        return torch.empty(*shape, dtype=dtype, device=self.dev)

    def _alloc(self, splitk_mb: int):
        """Precision plan: the residual stream (block inputs/outputs, skips, concat buffers, the transformer's running
        state h0..h3, shortcut outputs) is fp32; every MFMA operand (norm outputs, q/k/v, attention outputs, FF inner,
        conv inputs) is fp16.  Conv inputs live in zero-bordered [B,H+2,W+2,C] buffers so padding needs no predicate."""
        B, arch = self.B, self.arch
        boc = self.cfg["block_out_channels"]
        nlev = len(boc)
        F32 = torch.float32
        self.x_in = self._buf(B, self.cfg["in_channels"], self.H, self.W, dtype=F32)
        self.t_in = self._buf(B, dtype=F32)
        self.text_pad = torch.zeros(B, self.Sp, self.cad, dtype=F16, device=self.dev)    # rows >= S stay zero
        self.text_in = self.text_pad[:, : self.S]
        self.eps_out = self._buf(B, self.cfg["out_channels"], self.H, self.W, dtype=F32)
        self.temb0 = self._buf(B, boc[0], dtype=F32)
        self.temb1 = self._buf(B, arch.temb_dim, dtype=F32)
        self.temb2 = self._buf(B, arch.temb_dim, dtype=F32)
        self.tproj = self._buf(B, self.temb_total, dtype=F32)
        self.time_table: Optional[tuple] = None                         # (timesteps [T], rows [T, temb_total]) — build_time_table()
        self.time_table_on = True                                       # False: forward() runs the chain itself (set_inputs); the buffers stay alive
        self.ws_split = ops.new_workspace(splitk_mb << 20, self.dev)      # split-K partial tiles (fp32, reduced by a second launch: no initialisation needed)
        self.ws_side = ops.new_workspace(splitk_mb << 20, self.dev)       # split-K scratch of the side-stream branches
        self.ws_pair = ops.new_workspace(splitk_mb << 20, self.dev)       # second problem of a paired GEMM launch
        self.side: Optional[torch.cuda.Stream] = None                   # set by forward(side=...)
        self.kv_ext: Optional[Dict[str, tuple]] = None                  # attn3 K / V^T computed by the reference pass
        self.ws_gn = self._buf(ops.groupnorm_workspace_bytes(B, self.groups), dtype=torch.uint8)
        self.f8_scratch = None
        if self.fp8_attention:
            heads = self.cfg["attention_head_dim"] if isinstance(self.cfg["attention_head_dim"], int) else self.cfg["attention_head_dim"][0]
            hw0 = self.hw[0]
            nk = max(hw0, self.R * hw0)
            kb = max(B, self.ctx_rows if self.R else B)
            need = (ops.attention_f8_bytes(B, heads, hw0, False) + ops.attention_f8_bytes(kb, heads, nk, False)
                    + ops.attention_f8_bytes(kb, heads, nk, True) + 4096)
            self.f8_scratch = self._buf(need, dtype=torch.uint8)
        # per level: widest resnet input (concat) and the level's channel count; every conv-input channel count
        cmax, cout = [0] * nlev, [0] * nlev
        conv_in_ch = [set() for _ in range(nlev)]
        for s in arch.schedule:
            r, l = s.resnet, s.level
            if r is None:                        # a sampler conv reads its block's output
                conv_in_ch[l].add(s.cout)
            else:
                cmax[l], cout[l] = max(cmax[l], r.cin), max(cout[l], r.cout)
                conv_in_ch[l].update((r.cin, r.cout))
        self.lv = []
        self.padded: Dict[tuple, torch.Tensor] = {}
        for l in range(nlev):
            M, C, Cw = B * self.hw[l], cout[l], max(cmax[l], cout[l])
            h, w = self.H >> l, self.W >> l
            for ch in conv_in_ch[l]:
                self.padded[(l, ch)] = torch.zeros(B, h + 2, w + 2, ch, dtype=F16, device=self.dev)
            f32 = lambda *sh: self._buf(*sh, dtype=F32)  # noqa: E731
            d = dict(
                # fp32 residual stream
                **{n: (self._buf(M, C) if self.fp16_resnet else f32(M, C)) for n in ("r", "t_out", "sc")},
                **{n: (self._buf(M, C) if self.fp16_block else f32(M, C)) for n in ("h0", "h1")},
                # h2 / h3 (the input of the feed-forward; in a reference pass h2 plays h3) stay fp32 unless the MODULE switch asks for
                # the round-2 experiment's all-fp16 block stream: the fused feed-forward kernel reads the fp32 stream
                **{n: (self._buf(M, C) if (self.fp16_block and FP16_BLOCK_STREAM) else f32(M, C)) for n in ("h2", "h3")},
                # fp16 MFMA operands
                gn=self._buf(M, C), x16=self._buf(M * Cw), c1=self._buf(M, C), h4=self._buf(M, C),
                ln=self._buf(M, C), ln4=self._buf(M, C), qk=self._buf(M, 2 * C),
                # LayerNorm fold: per-token (sum, M2) partials of h0 / h1 / h3 per 64-channel block
                **{n: torch.zeros(M, (C // 64 + 1) & ~1, 2, dtype=F32, device=self.dev) for n in ("lnst0", "lnst1", "lnst3")}, vt=self._buf(C, M), q=self._buf(M, C),
                att=self._buf(M, C), q2=self._buf(M, C), att23=self._buf(M, 2 * C), ffi=self._buf(M, 4 * C),
                ffo=self._buf(M, 5 * C),          # FF_PROJ_MERGE: [GEGLU output | raw fp16 copy of h3], the K = 5C operand of the merged GEMM
                kt=self._buf(B * self.Sp, C), vtt=self._buf(C, B * self.Sp),
                ki=self._buf(self.ctx_slots * self.hw[l], C) if self.R else None,
                vti=self._buf(C, self.ctx_slots * self.hw[l]) if self.R else None,
            )
            self.lv.append(d)
        # torch.cat([h, skip]) (unet_2d_blocks.py:609,626,716) without a copy: every up-path resnet owns its concat input
        # buffer [M, cin] (fp32); the producer of h writes columns [0, c_h) and the skip tensor (down_block_res_samples)
        # IS the column slice [c_h, cin) of the buffer of the resnet that will pop it — the down path writes it there.
        # up_cats[-1 - i] is the buffer of the resnet that pops skip tensor i (the pops run last in, first out)
        ups = [s for s in arch.schedule if s.pop is not None]
        assert [s.pop for s in ups] == list(range(len(ups) - 1, -1, -1))
        self.up_cats: List[torch.Tensor] = [self._buf(B * self.hw[s.level], s.resnet.cin, dtype=F16 if self.fp16_resnet else F32) for s in ups]
        self.skips: List[torch.Tensor] = [buf[:, s.resnet.cin - s.skip:] for s, buf in zip(reversed(ups), reversed(self.up_cats))]       # skips[i] = i-th tensor the down path produces
        self.skip_meta = arch.skips
        assert len(self.skips) == len(self.skip_meta)
        for sk, (l, c) in zip(self.skips, self.skip_meta):
            assert tuple(sk.shape) == (B * self.hw[l], c), (tuple(sk.shape), l, c)
        # context buffers: [ctx_rows, R*HW, C] fp16 per feature key (K/V projection operands of attn3); with short rows a flat
        # [ctx_slots * HW, C] matrix (short rows first)
        self.ctx: Dict[str, torch.Tensor] = {}
        if self.R:
            for k, (n, c) in feature_shapes(arch, self.H, self.W).items():
                self.ctx[k] = self._buf(self.ctx_slots * n, c) if self.ctx_short else self._buf(self.ctx_rows, self.R * n, c)

    # ------------------------------------------------------------------------------------------ layers
    def _img(self, x2d: torch.Tensor, lvl: int) -> torch.Tensor:
        h, w = self.H >> lvl, self.W >> lvl
        return x2d.unflatten(0, (self.B, h, w))

    def _fork(self) -> bool:
        """Start a side branch (independent kernels on the side stream) — inside a capture this becomes a parallel
        branch of the hipGraph.  Returns False when no side stream is configured (everything stays in order)."""
        if self.side is None:
            return False
        self.side.wait_stream(torch.cuda.current_stream(self.dev))
        return True

    def _join(self):
        torch.cuda.current_stream(self.dev).wait_stream(self.side)

    # ---- cfg_shared_head: run a stretch of the pass on the first n samples of every buffer
    def _enter_head(self, n: int):
        """Make self.B = n and point the level-0 buffers, the conv inputs and the time rows at their first n samples.  Returns the
        state _leave_head restores."""
        saved = (self.B, self.lv[0], self.padded, self.tproj)
        hw, B = self.hw[0], self.B
        cols = ("vt", "vtt", "vti")                          # transposed buffers [C, tokens]: the samples are column blocks
        head = {}
        for k, v in self.lv[0].items():
            if v is None:
                head[k] = None
            elif k in cols:
                head[k] = v[:, : v.shape[1] // B * n]
            else:
                head[k] = v[: v.shape[0] // B * n]
        self.B, self.lv[0] = n, head
        self.padded = {k: (v[:n] if k[0] == 0 else v) for k, v in saved[2].items()}
        self.tproj = saved[3][:n]
        return saved

    def _leave_head(self, saved):
        self.B, self.lv[0], self.padded, self.tproj = saved

    def _spread(self, t2d: torch.Tensor, n: int, copies: int):
        """Rows of samples [0, n) of a [B*hw, C] stream tensor (row-strided views allowed) -> the next `copies` groups of n samples."""
        rows = n * self.hw[0]
        src = t2d[:rows].unflatten(0, (1, rows)).expand(copies, rows, t2d.shape[1])
        ops.copy_rows(t2d[rows:(1 + copies) * rows].unflatten(0, (copies, rows)), src)

    # ---- GroupNorm statistics from producer epilogues
    def _stats_wanted(self, lvl: int, n_out: int) -> bool:
        """Does any GroupNorm that can read a tensor of n_out channels at this level take producer statistics?  Its own width, or the
        wider channel concats [h | skip] of the up blocks (unet_2d_blocks.py:600-601) — e.g. at 16x16 a 1280-channel GroupNorm is
        the one-launch kernel, the 2560- and 1920-channel concats are not.  (Statistics nobody reads cost the producer a few
        shuffles; a consumer that does not use them ignores them.)"""
        key = (lvl, n_out)
        if key not in self._stats_want:
            widths = [n_out] + sorted({r.cin for r in self.arch.resnets if r.cin > n_out})
            self._stats_want[key] = any(ops.groupnorm_uses_pstats(self.hw[lvl], c, self.groups) for c in widths)
        return self._stats_want[key]

    def _produce(self, site: str, lvl: int, n_out: int, launch, rows) -> _GnFeed:
        """A producer of a stream tensor [B*hw[lvl], n_out] that may emit GroupNorm statistics: launch(statistics buffer or None) runs
        it, rows(buf) -> rows per partial of exactly that launch (ops.*_stats_rows; 0 = it cannot emit them), asked once per site (the
        plan depends only on the shapes).  Returns what the tensor hands to the GroupNorm that reads it."""
        feed = _NO_FEED
        if self.gn_epilogue_stats and self._stats_wanted(lvl, n_out):
            feed = self._stats_site.get(site)
            if feed is None:
                M = self.B * self.hw[lvl]
                buf = torch.empty((M // 64) * 2 * n_out, dtype=torch.float32, device=self.dev)    # enough for any tile height >= 64
                # M < 64 (batch 1 on a 32-token level): no tile of >= 64 rows divides an image — and there is nothing to ask with: an
                # empty buffer has no address, which the query refuses as "no statistics requested"
                n = int(rows(buf)) if buf.numel() else 0
                feed = self._stats_site[site] = _GnFeed(pstats=[(buf, n, n_out)]) if n else _NO_FEED
        launch(feed.pstats[0][0] if feed.pstats else None)
        return feed

    def _defer_splits(self, site: str, lvl: int, cout: int, query) -> int:
        """K slices (> 1) of the convolution at `site` when it may leave its split-K reduction to the GroupNorm that consumes its
        [B*hw, cout] output (the one-launch variant sums the slices while loading its slab), else 0."""
        if not SPLITK_IN_GN or not ops.groupnorm_is_fused(self.hw[lvl], cout, self.groups):
            return 0
        # asked on every call: the plan is host-only arithmetic, but it depends on process state that can change after the first
        # forward (ops.load_tile_table, sg_debug_set_option) — and the GroupNorm must be told the slice count THIS launch uses
        n = int(query())
        return n if n > 1 else 0

    def _attention(self, q, k, vt, out, heads: int, scale: float, nk: Optional[int] = None, short: Optional[tuple] = None):
        """softmax(scale q k^T) v on the HIP kernels: fp16 MFMA, or e4m3 MFMA for the D = 40 image / self attentions when the
        engine was built with fp8_attention (text attention — 77 keys — and every other head dim stay fp16).
        short = (k2, vt2): leading K/V rows with their own key count (ops.attention)."""
        n_keys = k.shape[1] if nk is None else nk
        if self.fp8_attention and q.shape[2] == heads * 40 and n_keys >= 256:
            if short is not None:          # the fp8 kernel has one key count per launch: short rows first, then the others
                ns = short[0].shape[0]
                ops.attention_f8(q[:ns], short[0], short[1], out[:ns], heads, scale, self.f8_scratch)
                q, out = q[ns:], out[ns:]
            ops.attention_f8(q, k, vt, out, heads, scale, self.f8_scratch, nk=nk)
        else:
            ops.attention(q, k, vt, out, heads, scale, nk=nk, short=short)

    def _resnet(self, rn: _Resnet, x: torch.Tensor, x_gn: _GnFeed, out: torch.Tensor, lvl: int, defer_out: bool = False) -> _GnFeed:
        """diffusers ResnetBlock2D.  x fp32 [M,Cin] contiguous, x_gn what its producer handed over; out fp32 [M,Cout],
        possibly a column slice of a concat buffer.  defer_out: the only reader of `out` before anything else is the GroupNorm of the
        transformer that follows — a split-K conv2 may leave its reduction to it (SPLITK_IN_GN).  Returns the hand-off of `out`."""
        L, M, r, B, hw = self.lv[lvl], x.shape[0], rn.spec, self.B, self.hw[lvl]
        ws = self.ws_split
        p_in, p_mid = self.padded[(lvl, r.cin)], self.padded[(lvl, r.cout)]
        x16 = L["x16"][: M * r.cin].view(M, r.cin) if rn.wsc is not None else None
        ops.groupnorm(x.unflatten(0, (B, hw)), rn.n1g, rn.n1b, p_in, self.groups, self.eps, True, self.ws_gn,
                      xcopy=None if x16 is None else x16.unflatten(0, (B, hw)), pstats=x_gn.pstats)
        res, forked = x, False
        if rn.wsc is not None:                     # 1x1 shortcut: independent of conv1 -> norm2, runs beside them
            forked = self._fork()
            if forked:
                with torch.cuda.stream(self.side):
                    ops.gemm(x16, rn.wsc, L["sc"], bias=rn.bsc, workspace=self.ws_side)
            else:
                ops.gemm(x16, rn.wsc, L["sc"], bias=rn.bsc, workspace=ws)
            res = L["sc"]
        h1 = L["c1"]
        rb = self.tproj[:, rn.temb_off: rn.temb_off + r.cout]
        kw1 = dict(rowbias=rb, workspace=ws, x_padded=True)
        d1 = self._defer_splits(r.prefix + ".conv1", lvl, r.cout, lambda: ops.conv3x3_planned_splits(p_in, rn.w1, self._img(h1, lvl), **kw1))
        if d1:      # conv1 -> norm2: the GroupNorm sums the K slices itself; h1 is never stored (fp16 rounding kept: bit-identical)
            ops.conv3x3(p_in, rn.w1, self._img(h1, lvl), defer_reduce=True, **kw1)
            ops.groupnorm(h1.unflatten(0, (B, hw)), rn.n2g, rn.n2b, p_mid, self.groups, self.eps, True, self.ws_gn,
                          split=dict(ws=ws, splits=d1, rowbias=rb, store=False))
        else:
            h1_gn = self._produce(r.prefix + ".conv1", lvl, r.cout, lambda s: ops.conv3x3(p_in, rn.w1, self._img(h1, lvl), stats=s, **kw1),
                                  lambda buf: ops.conv3x3_stats_rows(p_in, rn.w1, self._img(h1, lvl), stats=buf, **kw1))
            ops.groupnorm(h1.unflatten(0, (B, hw)), rn.n2g, rn.n2b, p_mid, self.groups, self.eps, True, self.ws_gn, pstats=h1_gn.pstats)
        if forked:
            self._join()
        kw2 = dict(bias=rn.b2, res1=self._img(res, lvl), workspace=ws, x_padded=True)
        d2 = 0
        if defer_out:
            d2 = self._defer_splits(r.prefix + ".conv2", lvl, r.cout, lambda: ops.conv3x3_planned_splits(p_mid, rn.w2, self._img(out, lvl), **kw2))
        if d2:      # conv2 -> Transformer2DModel.norm: that GroupNorm reduces, and stores `out` (the residual of proj_out)
            ops.conv3x3(p_mid, rn.w2, self._img(out, lvl), defer_reduce=True, **kw2)
            return _GnFeed(split=dict(ws=ws, splits=d2, bias=rn.b2, res1=res.unflatten(0, (B, hw)), store=True))
        return self._produce(r.prefix + ".conv2", lvl, r.cout, lambda s: ops.conv3x3(p_mid, rn.w2, self._img(out, lvl), stats=s, **kw2),
                             lambda buf: ops.conv3x3_stats_rows(p_mid, rn.w2, self._img(out, lvl), stats=buf, **kw2))

    def _text_kv(self, xf: _Xf, lvl: int, use_cache: bool):
        """K and V^T projections of the text embeddings for attn2 (attention.py:192-199): timestep-invariant, so the
        sampler computes them once per prompt (cache_text_kv) instead of once per UNet call.  Returns (K [B,Sp,C],
        VT [B,C,Sp]) views; rows / columns >= S come from the zero padding tokens."""
        B, Sp, C = self.B, self.Sp, xf.spec.channels
        if use_cache:
            kt, vtt = self.text_cache[xf.spec.prefix]
        else:
            kt, vtt = self.lv[lvl]["kt"], self.lv[lvl]["vtt"]
            self._project_text(xf, kt, vtt)
        return kt.view(B, Sp, C), vtt.view(C, B, Sp).permute(1, 0, 2)

    def _project_text(self, xf: _Xf, kt: torch.Tensor, vtt: torch.Tensor):
        x = self.text_pad.view(self.B * self.Sp, self.cad)
        _pair(((x, xf.w_k2, kt), dict(workspace=self.ws_split)),
                      ((xf.w_v2, x, vtt), dict(workspace=self.ws_pair)))                   # VT = Wv . X^T

    def cache_text_kv(self):
        """Run every attn2 K / V^T projection on the current self.text_in and keep the results (use with
        forward(text_cache=True) while the prompts do not change)."""
        for blk in self.arch.blocks:
            for a in blk.attns:
                if a is None:
                    continue
                bufs = self.text_cache.get(a.prefix)
                if bufs is None:
                    bufs = self.text_cache[a.prefix] = (self._buf(self.B * self.Sp, a.channels),
                                                        self._buf(a.channels, self.B * self.Sp))
                self._project_text(self.xfs[a.prefix], *bufs)

    # ---- Transformer2DModel.forward (attention.py:85-128) + BasicTransformerBlock.forward (:236-302) as stages on one _XfPass: x, out,
    # h0..h3 are the fp32 stream, everything that feeds an MFMA is fp16
    def _transformer(self, xf: _Xf, x: torch.Tensor, x_gn: _GnFeed, out: Optional[torch.Tensor], lvl: int, text: Optional[torch.Tensor],
                     harvest: Optional[HarvestPlan], consume: bool, text_cache: bool = False) -> _GnFeed:
        st = _XfPass(self, xf, x, x_gn, out, lvl, consume)
        self._xf_to_harvest(st, harvest)
        self._xf_queries(st)
        return self._xf_back(st, text_cache)

    def _xf_to_harvest(self, st: _XfPass, harvest):
        """Everything up to and including the harvested feature (a harvest_only pass needs nothing behind it)."""
        plans = () if harvest is None else (tuple(harvest) if isinstance(harvest, (list, tuple)) else (harvest,))
        self._xf_entry(st)
        self._self_projections(st, st.L["h0"], st.h0r, st.L["qk"], st.L["vt"])
        self._xf_harvest(st, plans, self._xf_self_attention(st, plans))

    def _xf_back(self, st: _XfPass, text_cache: bool, shared: bool = False) -> _GnFeed:
        """From the cross-attentions on: everything that depends on more than the hidden states (cfg_shared_head runs what comes before
        once for the three CFG samples; shared = their ONE query tensor is still the only one).  Returns the hand-off of st.out."""
        h3 = self._xf_cross_consume(st, text_cache, shared) if st.consume else self._xf_cross_text(st, text_cache)
        return self._xf_feed_forward(st, h3)

    def _xf_entry(self, st: _XfPass):
        L, xf, x = st.L, st.xf, st.x
        ops.groupnorm(x.unflatten(0, (st.B, st.hw)), xf.ng, xf.nb, L["gn"].unflatten(0, (st.B, st.hw)), self.groups, 1e-6, False,
                      self.ws_gn, pstats=st.x_gn.pstats, split=st.x_gn.split)   # :99 (eps 1e-6, :55)
        ops.gemm(L["gn"], xf.w_in, L["h0"], bias=xf.b_in, workspace=self.ws_split, **st.prod(L["h0"], L["ln"], L["lnst0"]))   # proj_in :101

    def _self_projections(self, st: _XfPass, h0: torch.Tensor, h0r: torch.Tensor, qk: torch.Tensor, vt: torch.Tensor):
        """Self-attention projections :250-262: q|k (token-major) and V^T = Wv . X^T (the attention kernel's operand layout), two GEMMs on
        one LayerNorm output, one launch.  Reads h0 — folded: its raw copy h0r and the partials L["lnst0"] — and writes qk and vt.
        (tools/exp_determinism.py puts its instrumented variant in this method's place.)"""
        xf, L = st.xf, st.L
        if st.fold:
            _pair(((h0r, xf.w_qk1f, qk), dict(ln=(1, L["lnst0"], xf.c_qk1, xf.d_qk1, LN_EPS), guard=st.guard)),
                  ((xf.w_v1f, h0r, vt), dict(ln=(2, L["lnst0"], xf.c_v1, xf.d_v1, LN_EPS), guard=st.guard)))
        else:
            ops.layernorm(h0, *xf.ln["norm1"], L["ln"])
            _pair(((L["ln"], xf.w_qk1, qk), dict(workspace=self.ws_split)), ((xf.w_v1, L["ln"], vt), dict(workspace=self.ws_pair)))

    def _xf_self_attention(self, st: _XfPass, plans: tuple) -> Optional[torch.Tensor]:
        """Self-attention and its out-projection + residual -> h1, the feature :263.  A plan whose sample order is the context's slot
        order (HarvestPlan.direct) gets the feature as the second, fp16 output of that GEMM — written straight into the context buffer,
        which then also serves as the raw copy of h1 that the folded query projections read.  Returns that buffer, or None: any other
        plan is served by strided copies (_xf_harvest)."""
        xf, L, B, hw, C = st.xf, st.L, st.B, st.hw, st.C
        qk3 = L["qk"].view(B, hw, 2 * C)
        self._attention(qk3[:, :, :C], qk3[:, :, C:], L["vt"].view(C, B, hw).permute(1, 0, 2), L["att"].view(B, hw, C), st.heads, st.scale)
        direct = None
        if len(plans) == 1 and plans[0].is_direct(B, plans[0].slots_per_row or self.R):
            c = plans[0].ctx[xf.spec.feature_key]
            direct = c if c.dim() == 2 else c.view(-1, C)
            assert direct.shape[0] == st.M, (direct.shape, st.M)
        kw1 = st.prod(L["h1"], L["ln4"], L["lnst1"])
        if direct is not None:
            kw1["out2"] = st.h1r = direct
        ops.gemm(L["att"], xf.w_o1, L["h1"], bias=xf.b_o1, res1=L["h0"], workspace=self.ws_split, **kw1)
        return direct

    def _xf_harvest(self, st: _XfPass, plans: tuple, direct: Optional[torch.Tensor]):
        """h1 into the context buffers of the plans that did not get it directly (one strided copy per op), and the attn3 K / V^T of
        each context this finishes (HarvestPlan.kv; attention.py:215-223)."""
        xf, hw, C = st.xf, st.hw, st.C
        h1b = st.L["h1"].view(st.B, hw, C)
        for plan in plans:
            ctx = plan.ctx[xf.spec.feature_key]
            c2d = ctx if ctx.dim() == 2 else ctx.view(-1, C)
            if direct is None:
                Rp = plan.slots_per_row or (ctx.shape[1] // hw)
                for src, step, row, slot, cnt in plan.ops:
                    t0 = plan.flat_slot(row, slot, Rp) * hw
                    dst = c2d[t0:t0 + cnt * hw].view(cnt, hw, C)
                    ops.copy_rows(dst, h1b[plan.src_offset + src:].as_strided((cnt, hw, C), (step * hw * C, C, 1)))
            if plan.kv is not None:
                ki, vti = plan.kv[xf.spec.feature_key]
                _pair(((c2d, xf.w_k3, ki), dict(workspace=self.ws_split)), ((xf.w_v3, c2d, vti), dict(workspace=self.ws_pair)))   # VT[C, slots*hw]

    def _xf_queries(self, st: _XfPass):
        """Query projections of the text cross-attention :266-277 (norm2) and, in a main pass, the image cross-attention :281-291
        (norm4): they share statistics, and both in one launch."""
        xf, L, h1, h1r, gd, ws = st.xf, st.L, st.L["h1"], st.h1r, st.guard, self.ws_split
        if st.consume and st.fold:
            _pair(((h1r, xf.w_q2f, L["q2"]), dict(ln=(1, L["lnst1"], xf.c_q2, xf.d_q2, LN_EPS), guard=gd)),
                  ((h1r, xf.w_q3f, L["q"]), dict(ln=(1, L["lnst1"], xf.c_q3, xf.d_q3, LN_EPS), guard=gd)))
        elif st.consume:
            ops.layernorm(h1, *xf.ln["norm2"], L["ln"], 1e-5, *xf.ln["norm4"], L["ln4"])
            _pair(((L["ln"], xf.w_q2, L["q2"]), dict(workspace=ws)), ((L["ln4"], xf.w_q3, L["q"]), dict(workspace=self.ws_pair)))
        elif st.fold:
            ops.gemm(h1r, xf.w_q2f, L["q"], ln=(1, L["lnst1"], xf.c_q2, xf.d_q2, LN_EPS), guard=gd)
        else:
            ops.layernorm(h1, *xf.ln["norm2"], L["ln"])
            ops.gemm(L["ln"], xf.w_q2, L["q"], workspace=ws)

    def _ctx_kv(self, st: _XfPass):
        """attn3's K / V^T of the image context — projected here unless a reference pass left them (kv_ext) — as (K [rows - ns, R hw, C],
        VT [rows - ns, C, R hw], short): `ns` short rows (hw keys each, `short` = their (K, VT) or None) in front of the long ones."""
        xf, L, hw, C = st.xf, st.L, st.hw, st.C
        if self.kv_ext is not None:
            ki, vti = self.kv_ext[xf.spec.feature_key]
        else:
            ctx = self.ctx[xf.spec.feature_key]
            c2d = ctx if ctx.dim() == 2 else ctx.view(-1, C)
            ki, vti = L["ki"], L["vti"]
            _pair(((c2d, xf.w_k3, ki), dict(workspace=self.ws_split)), ((xf.w_v3, c2d, vti), dict(workspace=self.ws_pair)))   # VT[C, slots*hw]
        ns, rows, nk = self.ctx_short, self.ctx_rows, self.R * hw
        short = (ki[: ns * hw].view(ns, hw, C), vti[:, : ns * hw].unflatten(1, (ns, hw)).permute(1, 0, 2)) if ns else None
        return ki[ns * hw:].view(rows - ns, nk, C), vti[:, ns * hw:].unflatten(1, (rows - ns, nk)).permute(1, 0, 2), short

    def _xf_cross_consume(self, st: _XfPass, text_cache: bool, shared: bool) -> torch.Tensor:
        """Main pass: the text branch (q2 -> attn2, :266-276) and the image branch (q3 -> attn3, :281-290) write the two halves of one
        [M, 2C] buffer; their out-projections, biases and both residual adds (:277,291-293) are one GEMM -> h3."""
        xf, L, B, hw, C, heads, scale, S = st.xf, st.L, st.B, st.hw, st.C, st.heads, st.scale, self.S
        kt3, vtt3 = self._text_kv(xf, st.lvl, text_cache)
        att23, h1, h3 = L["att23"], L["h1"], L["h3"]
        a2v, a3v = att23[:, :C].unflatten(0, (B, hw)), att23[:, C:].unflatten(0, (B, hw))
        if shared:      # cfg_shared_head, first transformer: ONE query tensor for the three CFG samples
            q2q = L["q2"][:hw].view(1, hw, C).expand(2, hw, C)
            q3 = L["q"][:hw].view(1, hw, C).expand(2, hw, C)
            kt3, vtt3, a2o, a3o = kt3[::2], vtt3[::2], a2v[::2], a3v[:2]       # text rows (uncond, text) -> samples 0 and 2
        else:
            q2q, q3, a2o, a3o = L["q2"].view(B, hw, C), L["q"].view(B, hw, C), a2v, a3v
        # text + image attention as one launch when the image attention is one fp16 launch itself (else the text attention runs
        # beside the context projections on the side stream)
        paired = (ATTN_PAIR and self.attn3_share is not None and not self.ctx_short and not shared
                  and not (self.fp8_attention and C == heads * 40))
        forked = False if paired else self._fork()
        if forked:
            with torch.cuda.stream(self.side):
                ops.attention(q2q, kt3, vtt3, a2o, heads, scale, nk=S)
        elif not paired:
            ops.attention(q2q, kt3, vtt3, a2o, heads, scale, nk=S)
        ki3, vti3, short = self._ctx_kv(st)
        if paired:
            ops.attention_pair((q3, ki3, vti3, a3v, None), (q2q, kt3, vtt3, a2v, S), heads, scale)
        elif self.attn3_share is not None:    # one launch: batch b reads context row b (b < rows) or b - (B - rows)
            self._attention(q3, ki3, vti3, a3o, heads, scale, short=short)
        else:
            for q0, n, c0 in self.attn3_groups:
                self._attention(q3[q0:q0 + n], ki3[c0:c0 + n], vti3[c0:c0 + n], a3v[q0:q0 + n], heads, scale)
        if forked:
            self._join()
        if shared:      # sample 1 = (uncond text, frames): its text attention is sample 0's, its image attention sample 2 shares
            ops.copy_rows(a2v[1:2], a2v[0:1])
            ops.copy_rows(a3v[2:3], a3v[1:2])
        ops.gemm(att23, xf.w_o23, h3, bias=xf.b_o23, res1=h1, res2=h1, workspace=self.ws_split, **st.prod3(h3))  # (a2 + h) + (a3 + h)
        return h3

    def _xf_cross_text(self, st: _XfPass, text_cache: bool) -> torch.Tensor:
        """Reference pass: text cross-attention only (:266-277); h2 plays h3."""
        xf, L, B, hw, C = st.xf, st.L, st.B, st.hw, st.C
        kt3, vtt3 = self._text_kv(xf, st.lvl, text_cache)
        ops.attention(L["q"].view(B, hw, C), kt3, vtt3, L["att"].view(B, hw, C), st.heads, st.scale, nk=self.S)
        h3 = L["h2"]
        ops.gemm(L["att"], xf.w_o2, h3, bias=xf.b_o2, res1=L["h1"], workspace=self.ws_split, **st.prod3(h3))   # :277,295
        return h3

    def _xf_feed_forward(self, st: _XfPass, h3: torch.Tensor) -> _GnFeed:
        """Feed-forward :298-300 and proj_out + the block's residual :121-123.  Returns the hand-off of st.out."""
        xf, L, M, C, gd, ws, x, out = st.xf, st.L, st.M, st.C, st.guard, self.ws_split, st.x, st.out
        h4, w_out = L["h4"], xf.w_out
        if st.ff1 and M <= FF_SPLIT_MAX_TOKENS:      # small launch: two workgroups per 128 tokens, partial sums side by side
            # L["att23"] as scratch: its only reader, the w_o23 / w_o2 GEMM above, is behind us on this stream, and the next writer (the
            # cross-attentions of the next block at this level) comes after proj_out below has consumed the partial sums (advisor r5).
            # The two halves are rounded to fp16 separately and re-added by proj_out's K = 2C contraction: one more rounding than the
            # unsplit kernel's single fp16 output, covered by the full-depth parity tests on the default (split) schedule.
            h4, w_out = L["att23"], xf.w_out2
            ops.ff_fused(h3, xf.ff_pack, xf.b_ff2, h4, LN_EPS, split=True)
        elif st.ff1:    # one launch: LayerNorm in registers, GEGLU intermediate never materialised (h4 is fp16: it only feeds proj_out)
            ops.ff_fused(h3, xf.ff_pack, xf.b_ff2, L["h4"], LN_EPS)
        elif st.merge:      # GEGLU into columns [0, 4C) of the buffer whose columns [4C, 5C) hold h3's raw copy; ff.net.2 happens inside proj_out's GEMM
            ops.gemm(st.h3raw, xf.w_ff1f, L["ffo"][:M, :4 * C], epilogue=ops.EPI_GEGLU, ln=(1, L["lnst3"], xf.c_ff1, xf.d_ff1, LN_EPS), guard=gd)
            h4, w_out = L["ffo"][:M], xf.w_ffo
        elif st.fold:
            ops.gemm(st.raw(h3, L["ln"]), xf.w_ff1f, L["ffi"], epilogue=ops.EPI_GEGLU, ln=(1, L["lnst3"], xf.c_ff1, xf.d_ff1, LN_EPS), guard=gd)
        else:
            ops.layernorm(h3, *xf.ln["norm3"], L["ln"])
            ops.gemm(L["ln"], xf.w_ff1, L["ffi"], bias=xf.b_ff1, epilogue=ops.EPI_GEGLU, workspace=ws)
        if not st.ff1 and not st.merge:
            ops.gemm(L["ffi"], xf.w_ff2, L["h4"], bias=xf.b_ff2, res1=h3, workspace=ws)   # fp16: only feeds proj_out
        kwo = dict(bias=xf.b_ffo if st.merge else xf.b_out, res1=x, workspace=ws)
        return self._produce(xf.spec.prefix + ".proj_out", st.lvl, C,
                             lambda s: ops.gemm(h4, w_out, out, stats=None if s is None else (s, st.hw), **kwo),
                             lambda buf: ops.gemm_stats_rows(h4, w_out, out, stats=(buf, st.hw), **kwo))

    def _sampler_conv(self, prefix: str, h: torch.Tensor, out: torch.Tensor, lvl: int, out_lvl: int, down: bool) -> _GnFeed:
        """Downsample2D (3x3 stride 2) / Upsample2D (nearest 2x + 3x3): the fp32 stream tensor is cast into the
        zero-bordered fp16 conv input first.  Returns the hand-off of `out`."""
        w, b = self.samplers[prefix]
        pbuf = self.padded[(lvl, h.shape[1])]
        ops.pad_cast(self._img(h, lvl), pbuf)
        kw = dict(stride=2 if down else 1, upsample2x=not down, bias=b, workspace=self.ws_split, x_padded=True)
        # Upsample2D as four 2x2 phase convolutions where that form has a launch for this batch and level (asked on every call, like
        # _defer_splits: host-only arithmetic that depends on process state); its statistics site is its own — the rows per partial
        # are those of ITS plan
        if not down and UPSAMPLE_PHASES and self.dev.type == "cuda" and out.shape[0] >= UPSAMPLE_PHASES_MIN_ROWS:
            kwp = dict(kw, upsample2x=2)
            wp = self.sampler_phases[prefix]
            if ops.conv3x3_phases_fit(pbuf, wp, self._img(out, out_lvl), **kwp):
                w, kw, prefix = wp, kwp, prefix + "#phases"
        return self._produce(prefix, out_lvl, out.shape[1], lambda s: ops.conv3x3(pbuf, w, self._img(out, out_lvl), stats=s, **kw),
                             lambda buf: ops.conv3x3_stats_rows(pbuf, w, self._img(out, out_lvl), stats=buf, **kw))

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, harvest_slot: Optional[int] = None, consume: bool = False, harvest: Optional[HarvestPlan] = None,
                harvest_only: bool = False, text_cache: bool = False,
                side: Optional[torch.cuda.Stream] = None) -> Optional[torch.Tensor]:
        """One UNet call on the static inputs (self.x_in fp32 NCHW, self.t_in fp32 [B], self.text_in fp16).

        harvest_slot=r : reference pass — no image context; sample b's features go to slot r of row b of self.ctx.
        harvest=plan   : reference pass writing into another engine's context buffers (HarvestPlan, or a list of them:
                         one per slice of the batch, HarvestPlan.src_offset).
        harvest_only   : stop right after the last feature is harvested (the rest of the pass — text attention and FF
                         of the last block, conv_out — only produces an epsilon the loop discards, pipeline.py:433-435);
                         returns None.
        consume=True   : main pass — attn3 cross-attends to self.ctx.
        text_cache     : use the attn2 K/V projections stored by cache_text_kv().
        side           : a second stream for the pass's independent branches (1x1 shortcuts beside conv1/norm2, the text
                         attention beside the image attention); in a capture they become parallel graph branches.
        Returns self.eps_out (fp32 NCHW)."""
        if harvest_slot is not None:
            if harvest is not None or self.ctx_rows != self.B:
                raise ValueError("harvest_slot needs one context row per sample and no explicit plan")
            if not self.R:
                raise ValueError("engine was built without context buffers (n_ref=0)")
            if self.ctx_short:
                raise ValueError("harvest_slot: this engine's context rows have different slot counts (ctx_short); pass a HarvestPlan")
            harvest = HarvestPlan(self.ctx, [(b, 0, b, harvest_slot, 1) for b in range(self.B)])
        if harvest is not None and consume:
            raise ValueError("a pass either harvests features or consumes them")
        if consume and not self.R:
            raise ValueError("engine was built without context buffers (n_ref=0)")
        if harvest_only and harvest is None:
            raise ValueError("harvest_only needs a harvest plan")
        self.side = side
        arch, text, skips = self.arch, self.text_in, self.skips
        steps = list(zip(arch.schedule, arch.schedule[1:] + [None]))       # (layer, the one after it)
        last_xf = [s.xf for s in arch.schedule if s.xf is not None][-1].prefix if harvest_only else None
        tk = dict(text_cache=text_cache)
        skip_gn: List[_GnFeed] = [_NO_FEED]      # parallel to skips: what each skip tensor hands to a GroupNorm (conv_in: nothing)
        # --- time embedding :392-398, then all 22 time_emb_proj(silu(emb)) in one GEMV bundle.  emb is only ever consumed through
        # silu (resnet.py time_emb_proj), so the second linear writes silu(emb) once instead of every wave of the bundle redoing it
        if self.time_table is not None and self.time_table_on:       # the loop's timesteps were tabulated at prepare() time: one row lookup instead of the chain
            ops.lookup_rows(self.t_in, self.time_table[0], self.time_table[1], self.tproj)
        else:
            self._time_chain(self.t_in, self.temb0, self.temb1, self.temb2, self.tproj)
        shared = self.cfg_shared_head and consume
        if shared and not self._head_checked and not torch.cuda.is_current_stream_capturing():
            # the caller's guarantee, verified on the first eager pass (the sampler's warm-up before capture): one latent, one timestep,
            # text rows 0 and 1 alike.  (One host synchronisation, once per engine.)
            self._head_checked = True
            if not (torch.equal(self.x_in[0], self.x_in[1]) and torch.equal(self.x_in[0], self.x_in[2])
                    and bool((self.t_in == self.t_in[0]).all()) and torch.equal(self.text_in[0], self.text_in[1])):
                raise ValueError("cfg_shared_head: the three samples must be the same latent at the same timestep with text rows "
                                 "[uncond, uncond, text] (the CFG main pass of one story frame, pipeline.py:448-453)")
        if shared:
            # CFG main pass of one story frame: the three samples are ONE computation up to the first cross-attention — conv_in :411,
            # the first ResnetBlock2D and the first transformer's front half run on sample 0 only, their results are copied to the
            # other two, and the cross-attentions of that transformer run once per DISTINCT (query, context) pair
            blk0 = arch.down[0]
            r0, xf0 = self.resnets[blk0.resnets[0].prefix], self.xfs[blk0.attns[0].prefix]
            # (conv_in at batch 3: a 0.2 GFLOP launch costs the same at either batch, and the skip tensor it writes is needed per sample)
            ops.conv_in(self.x_in, self.w_conv_in, self.b_conv_in, self._img(skips[0], 0))
            saved = self._enter_head(1)
            try:
                sk0 = skips[0][: self.hw[0]]
                r_gn = self._resnet(r0, sk0, _NO_FEED, self.lv[0]["r"], 0, defer_out=True)
                st = _XfPass(self, xf0, self.lv[0]["r"], r_gn, None, 0, True)
                self._xf_to_harvest(st, None)
                self._xf_queries(st)
            finally:
                self._leave_head(saved)
            for t2d in (self.lv[0]["r"], self.lv[0]["h1"]):                # proj_out's residual, the attentions' residual
                self._spread(t2d, 1, 2)
            h_gn = self._xf_back(_XfPass(self, xf0, self.lv[0]["r"], r_gn, skips[1], 0, True), text_cache, shared=True)
            skip_gn.append(h_gn)
            h, steps = skips[1], steps[1:]
        else:
            # --- conv_in :411
            ops.conv_in(self.x_in, self.w_conv_in, self.b_conv_in, self._img(skips[0], 0))
            h, h_gn = skips[0], _NO_FEED
        # --- down :417-433, mid :436-445, up :448-475
        for s, nxt in steps:
            lvl, L = s.level, self.lv[s.level]
            if s.push is not None:                        # every down-path output is a skip tensor: written straight into its skip buffer
                out = skips[s.push]
            elif nxt is not None and nxt.pop is not None:     # the h columns of the next layer's [h | skip] (the down path wrote the skip)
                out = self.up_cats[-1 - nxt.pop][:, : nxt.resnet.cin - nxt.skip]
            else:
                out = L["t_out"]
            if s.resnet is None:                          # Downsample2D / Upsample2D :656-658,730-732
                h_gn = self._sampler_conv(s.sampler, h, out, lvl, s.out_level, down=s.out_level > lvl)
            else:
                rn = self.resnets[s.resnet.prefix]
                if s.pop is not None:
                    h, h_gn = self.up_cats[-1 - s.pop], _GnFeed.concat(h_gn, skip_gn[s.pop], s.resnet.cin)
                if s.xf is None:
                    h_gn = self._resnet(rn, h, h_gn, out, lvl)
                else:
                    r_gn = self._resnet(rn, h, h_gn, L["r"], lvl, defer_out=True)
                    if s.xf.prefix == last_xf:      # harvest_only: the pass ends with its last feature (before that block's text projections)
                        self._xf_to_harvest(_XfPass(self, self.xfs[s.xf.prefix], L["r"], r_gn, None, lvl, consume), harvest)
                        return None
                    h_gn = self._transformer(self.xfs[s.xf.prefix], L["r"], r_gn, out, lvl, text, harvest, consume, **tk)
            if s.push is not None:
                skip_gn.append(h_gn)
            h = out
        # --- out :477-480
        L = self.lv[0]
        ops.groupnorm(h.unflatten(0, (self.B, self.hw[0])), *self.gn_out, L["gn"].unflatten(0, (self.B, self.hw[0])),
                      self.groups, self.eps, True, self.ws_gn, pstats=h_gn.pstats)
        ops.conv_out(self._img(L["gn"], 0), self.w_conv_out, self.b_conv_out, self.eps_out)
        return self.eps_out

    def check_ln_guard(self, clear: bool = True) -> int:
        """Flags raised by the folded LayerNorms since the last check (0 = both assumptions held; synchronises on a 4-byte copy).
        Raises when one did not: the pass that set it must be rerun with engine.LN_FOLD = False (the LayerNorm launch on the fp32
        stream, as the reference computes it)."""
        flags = int(self.ln_guard.item())
        if clear and flags:
            self.ln_guard.zero_()
        if flags:
            why = []
            if flags & ops.LN_GUARD_RANGE:
                why.append("a stream tensor reached |x| >= 65504 (its fp16 copy was saturated)")
            if flags & ops.LN_GUARD_OFFSET:
                why.append(f"a token had |mean| / sigma > {ops.LN_GUARD_RATIO:g} (fp16 rounding of the raw copy no longer negligible)")
            raise FloatingPointError("LayerNorm fold outside its range: " + "; ".join(why) + " — rerun with storygen_amd.engine.LN_FOLD = False")
        return flags

    # ------------------------------------------------------------------------------------------ convenience
    def _time_chain(self, t, e0, e1, e2, out):
        """Timesteps -> TimestepEmbedding -> all time_emb_proj(silu(emb)) rows (unet_2d_condition.py:392-398, ResnetBlock2D)."""
        ops.timestep_embed(t, self.freqs, e0, self.cfg["flip_sin_to_cos"])
        ops.linear_rows(e0, self.w_t1, self.b_t1, e1, act_out=True)
        ops.linear_rows(e1, self.w_t2, self.b_t2, e2, act_out=True)
        ops.linear_rows(e2, self.w_temb, self.b_temb, out)

    def build_time_table(self, timesteps, capacity: int = 256) -> bool:
        """Tabulate the time-embedding chain for every distinct value in `timesteps` (a sampler knows them all at prepare() time:
        pipeline.py:410-415).  forward() then reads the rows of self.t_in with ops.lookup_rows — one launch of a few microseconds instead
        of four (the last one streams the 22 stacked time_emb_proj matrices, ~45 MB, per UNet call) — and gets NaN rows, not stale ones,
        for a timestep that is not in the table.  Rows are computed by the same kernels four at a time, exactly as forward() would.
        The table lives in buffers of `capacity` rows (unused keys are NaN, which matches nothing) that later calls refill IN PLACE, so a
        captured graph stays valid; returns True when the buffers were (re)allocated — or dropped — i.e. when graphs captured before
        the call must be captured again.  Pass None to drop the table (training, set_inputs() with arbitrary timesteps)."""
        self.time_table_on = True
        if timesteps is None:
            had = self.time_table is not None
            self.time_table = None
            self._time_keys = None
            return had
        keys = sorted({float(t) for t in timesteps})
        if not keys:
            raise ValueError("build_time_table: no timesteps")
        tag = (keys, getattr(self.wts, "version", 0))
        if self.time_table is not None and getattr(self, "_time_keys", None) == tag:
            return False                          # the same schedule on the same weights as the last call (a pipeline called again): the rows are already there
        F32, dev, T = torch.float32, self.dev, len(keys)
        fresh = self.time_table is None or self.time_table[0].numel() < T
        if fresh:
            cap = max(int(capacity), T)
            self.time_table = (torch.empty(cap, dtype=F32, device=dev), torch.empty(cap, self.temb_total, dtype=F32, device=dev))
        tk, tab = self.time_table
        tk.fill_(float("nan"))
        tk[:T].copy_(torch.tensor(keys, dtype=F32))
        e0 = torch.empty(4, self.temb0.shape[1], dtype=F32, device=dev)
        e1, e2 = (torch.empty(4, self.arch.temb_dim, dtype=F32, device=dev) for _ in range(2))
        for i in range(0, T, 4):
            n = min(4, T - i)
            self._time_chain(tk[i:i + n], e0[:n], e1[:n], e2[:n], tab[i:i + n])
        self._time_keys = tag
        return fresh

    def set_inputs(self, sample: torch.Tensor, timestep, text: torch.Tensor):
        self.x_in.copy_(sample.to(self.dev, torch.float32))
        # arbitrary timesteps: the chain itself, not a sampler's table.  The table's buffers are kept (a hipGraph captured while it was
        # in use still reads them; build_time_table() switches it back on and refills them in place)
        self.time_table_on = False
        t = timestep if torch.is_tensor(timestep) else torch.tensor([float(timestep)])
        self.t_in.copy_(t.to(self.dev, torch.float32).reshape(-1).expand(self.B))
        self.text_in.copy_(text.to(self.dev, F16))

    def features(self, slot: int = 0) -> Dict[str, torch.Tensor]:  # fp16 views
        """The 16 harvested [B, HW, C] features of slot r, as views into the context buffers."""
        if self.ctx_short:
            raise ValueError("features(): this engine's context rows have different slot counts (ctx_short)")
        out = {}
        for k, (n, _) in feature_shapes(self.arch, self.H, self.W).items():
            out[k] = self.ctx[k][:, slot * n:(slot + 1) * n, :]
        return out
