"""TEST INFRASTRUCTURE — float64 restatement of one optimizer step as storygen_amd.optim performs it: gradient unscale, optional
global-norm clip over every tensor that has a gradient, AdamW with a PER-PARAMETER step number (torch.optim.AdamW and bitsandbytes
keep state["step"] per parameter, created when the parameter first has a gradient).  tests/test_optim_reference.py pins it to
torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ and to oracle/optim_oracle.py without a GPU; tests/test_optim_edges_gpu.py
measures the kernels against it.  The 8-bit step only scales and clips the gradient here and delegates the block algorithm to
oracle.optim_oracle.adamw8bit_step."""
import math
from typing import List, Optional, Sequence, Tuple

import torch

from oracle import optim_oracle as oo

F64 = torch.float64
REFERENCE_HP = dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)     # the reference's optimizer arguments


def ulp32(x: float) -> float:
    """Spacing of fp32 numbers at |x| (x != 0)."""
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23) if x else 2.0 ** -149


def total_norm64(grads: Sequence[Optional[torch.Tensor]], grad_scale: float = 1.0) -> float:
    """2-norm of the UNSCALED gradients (grad_scale * g) over every tensor that has one."""
    return float(grad_scale) * math.sqrt(sum(float((g.to(F64) ** 2).sum()) for g in grads if g is not None))


def grad_factor64(grads: Sequence[Optional[torch.Tensor]], grad_scale: float = 1.0, max_norm: Optional[float] = None) -> Tuple[float, float]:
    """(factor every gradient is multiplied by, total norm): clip AFTER unscale, torch.nn.utils.clip_grad_norm_'s coefficient
    min(1, max_norm / (norm + 1e-6))."""
    norm = total_norm64(grads, grad_scale)
    if max_norm is None:
        return float(grad_scale), norm
    return float(grad_scale) * min(1.0, float(max_norm) / (norm + 1e-6)), norm


def adamw_step64(p, g, m, v, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, factor: float = 1.0):
    """In place on the float64 tensors p, m, v; g is multiplied by `factor` first.  torch.optim.AdamW's formula, every operation
    in float64 (no fused or reordered step: this is the value, not an implementation)."""
    b1, b2 = betas
    g = g.to(F64) * factor
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).add_(g * g, alpha=1 - b2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p.mul_(1 - lr * weight_decay)
    p.sub_((lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps))


class AdamW64:
    """A list of tensors stepped in float64.  `step(grads)`: grads[i] is None for a tensor without a gradient — it is not updated,
    does not enter the clip norm and its step number does not advance.  Returns the total norm of the unscaled gradients."""

    def __init__(self, params: Sequence[torch.Tensor], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        self.p = [x.detach().cpu().to(F64).flatten().clone() for x in params]
        self.m = [torch.zeros_like(x) for x in self.p]
        self.v = [torch.zeros_like(x) for x in self.p]
        self.steps = [0] * len(self.p)
        self.hp = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)

    def step(self, grads: Sequence[Optional[torch.Tensor]], grad_scale: float = 1.0, max_norm: Optional[float] = None) -> float:
        grads = [None if g is None else g.detach().cpu().flatten() for g in grads]
        factor, norm = grad_factor64(grads, grad_scale, max_norm)
        for i, g in enumerate(grads):
            if g is not None:
                self.steps[i] += 1
                adamw_step64(self.p[i], g, self.m[i], self.v[i], self.steps[i], factor=factor, **self.hp)
        return norm


def adamw8bit_step_scaled(p, g, c1, c2, a1, a2, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                          factor: float = 1.0):
    """oo.adamw8bit_step on the gradient g * factor (factor from grad_factor64, rounded to fp32 as the kernel holds it).  In place on
    p (flat fp32), c1 / c2 (uint8 codes), a1 / a2 (per-block absmax)."""
    gs = g if factor == 1.0 else g * torch.tensor(factor, dtype=torch.float32)
    oo.adamw8bit_step(p, gs, c1, c2, a1, a2, step, lr, betas, eps, weight_decay)


def adamw8bit_step_f64_moments(p, g, c1, c2, a1, a2, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2):
    """The variant the seed check of tests/test_optim_reference.py compares oo.adamw8bit_step with: the same step with the moments,
    their block maxima and the normalised values formed in float64, rounded to fp32 only where the code book is searched.  Where the
    two pick different codes, an fp32 rounding decided the bin — that is the room two correct fp32 implementations have.  Returns the
    updated parameter in float64 (p receives it rounded)."""
    b1, b2 = betas
    code1, code2 = oo.dynamic_map(True), oo.dynamic_map(False)
    n, nb = p.numel(), a1.numel()
    blk = torch.arange(n) // oo.BLOCK
    g = g.to(F64)
    m = b1 * (code1[c1.long()].to(F64) * a1.to(F64)[blk]) + (1 - b1) * g
    v = b2 * (code2[c2.long()].to(F64) * a2.to(F64)[blk]) + (1 - b2) * g * g
    bc1, sbc2 = 1 - b1 ** step, math.sqrt(1 - b2 ** step)
    p64 = p.to(F64)
    p64 = p64 - lr * weight_decay * p64
    p64 = p64 - (lr * sbc2 / bc1) * (m / (v.sqrt() + eps * sbc2))
    p.copy_(p64.float())
    pad = torch.zeros(nb * oo.BLOCK - n, dtype=F64)
    mx1 = torch.cat([m.abs(), pad]).view(nb, oo.BLOCK).amax(1)
    mx2 = torch.cat([v, pad]).view(nb, oo.BLOCK).amax(1)
    a1.copy_(mx1.float()), a2.copy_(mx2.float())
    r1 = torch.where(mx1 > 0, 1.0 / mx1, torch.zeros_like(mx1))[blk]
    r2 = torch.where(mx2 > 0, 1.0 / mx2, torch.zeros_like(mx2))[blk]
    c1.copy_(oo.nearest_code(code1, (m * r1).float())), c2.copy_(oo.nearest_code(code2, (v * r2).float()))
    return p64


# ---------------------------------------------------------------------------------------------------- 8-bit test inputs
# Shared by the CPU seed check (tests/test_optim_reference.py) and the GPU comparison (tests/test_optim_edges_gpu.py): the inputs
# the kernel is measured on are exactly the ones the CPU test has shown to be well inside the 1 % cap.
EIGHT_BIT_SIZES = (4096, 4097, 2 * 2048, 3 * 2048 - 1, 5 * 2048 + 1)
EIGHT_BIT_STEPS = 3
HP_8BIT = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)         # tests/test_optim_gpu.py's set
# The outlier pushes the second moment of every other element of its block below the code book (1e-8 of the block maximum), so their
# next update divides by sqrt((1 - beta2) g^2) alone: at lr = 1e-2 parameters reach the hundreds, where one fp32 ulp is 3e-5 and no
# two fp32 implementations agree to 1e-5.  A tenth of the rate and gradients of one scale keep them O(1).
HP_OUTLIER = dict(HP_8BIT, lr=1e-3)
# name -> (n, content, hyper-parameters, grad_scale, max_norm, elements of a second tensor in the same optimizer or 0)
EIGHT_BIT_CASES = {f"n{n}": (n, "normal", HP_8BIT, 1.0, None, 0) for n in EIGHT_BIT_SIZES}
EIGHT_BIT_CASES.update({
    "zero_block": (3 * 2048 - 1, "zero_block", HP_8BIT, 1.0, None, 0),
    "outlier": (3 * 2048 - 1, "outlier", HP_OUTLIER, 1.0, None, 0),
    "lr1e-5": (5 * 2048 + 1, "normal", REFERENCE_HP, 1.0, None, 0),
    "clip_scale_mixed": (4097, "normal", HP_8BIT, 0.25, 1.0, 4095),
})


def eight_bit_case(n: int, content: str, seed: int = 11) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """(initial parameter, gradients of steps 1..3) on the CPU.
      normal      N(0, 1) gradients whose scale changes by decades from step to step
      zero_block  block 0 has a zero gradient on every step (absmax 0 -> reciprocal 0 at step 1; it stays zero while block 1 moves)
      outlier     one element of block 1 is 1e4 times the rest (N(0, 1) on every step): everything else falls into the lowest decades
                  of the signed code book and below the unsigned one"""
    gen = torch.Generator().manual_seed(seed + n)
    p = torch.randn(n, generator=gen)
    grads = []
    for step in range(1, EIGHT_BIT_STEPS + 1):
        g = torch.randn(n, generator=gen) * (1.0 if content == "outlier" else 10.0 ** -(step % 3))
        if content == "zero_block":
            g[:oo.BLOCK] = 0.0
        elif content == "outlier":
            g[oo.BLOCK + 5] = 1e4
        elif content != "normal":
            raise ValueError(content)
        grads.append(g)
    return p, grads


def eight_bit_inputs(name: str):
    """EIGHT_BIT_CASES[name] as ([initial parameters], [per step: the RAW gradient of each tensor], hp, grad_scale, max_norm).  Raw
    gradients are the case's gradients divided by grad_scale (they still carry the loss scale); the first tensor is the 8-bit one."""
    n, content, hp, grad_scale, max_norm, n_small = EIGHT_BIT_CASES[name]
    p, grads = eight_bit_case(n, content)
    params, per_step = [p], [[g / grad_scale] for g in grads]
    if n_small:
        ps, gs = eight_bit_case(n_small, "normal")
        params.append(ps)
        for row, g in zip(per_step, gs):
            row.append(g / grad_scale)
    return params, per_step, hp, grad_scale, max_norm
