"""Times the near-duplicate pass over 64 keyframes of 1280 x 720 at dino_vitb8's geometry (12 layers, width 768, 785 tokens; random weights),
on the GPU: KeyframeDeduper.dedup end to end — upload of the 8-bit frames, sg_clip_patchify_u8, the tower, sg_adjacent_cosine_f64, the two
small copies back — beside the same network written in torch ops on the same device (fp16 and fp32) on pixels that are already
transformed and uploaded, followed by torch.cosine_similarity, alternating in one process; the kernel alone on 4096 features; and, once,
what the script's PIL transform costs per frame on this host.  Asserts nothing; prints how far the decisions agree.

    python tools/bench_dedup.py [--out FILE] [--rounds N] [--frames N]

An untimed pass first; device figures are medians over rounds of device-event time, host figures medians of perf_counter."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

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


def torch_tower(sd, px, heads, chunk=16):
    """DINO's forward in torch ops on the device and dtype of `sd`, `chunk` images at a time."""
    wp = sd["patch_embed.proj.weight"]
    C = wp.shape[0]
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    out = []
    for lo in range(0, px.shape[0], chunk):
        x = F.conv2d(px[lo:lo + chunk], wp, sd["patch_embed.proj.bias"], stride=wp.shape[2]).flatten(2).transpose(1, 2)
        B = x.shape[0]
        x = torch.cat([sd["cls_token"].expand(B, 1, C), x], 1) + sd["pos_embed"]
        T, D = x.shape[1], C // heads
        for i in range(depth):
            p = f"blocks.{i}."
            h = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
            qkv = F.linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).view(B, T, 3, heads, D).permute(2, 0, 3, 1, 4)
            a = torch.softmax((qkv[0] * D ** -0.5) @ qkv[1].transpose(-1, -2), -1) @ qkv[2]
            x = x + F.linear(a.transpose(1, 2).reshape(B, T, C), sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
            h = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
            x = x + F.linear(F.gelu(F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        out.append(F.layer_norm(x[:, 0], (C,), sd["norm.weight"], sd["norm.bias"], 1e-6))
    return torch.cat(out)


def torch_decisions(feats, threshold):
    f = feats.float()
    sim = torch.cat([torch.zeros(1, device=f.device), torch.cosine_similarity(f[1:], f[:-1], dim=1)])
    return sim, torch.cat([sim[1:] >= threshold, torch.zeros(1, dtype=torch.bool, device=f.device)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dedup: needs the GPU (no CPU path)")
    from storygen_amd import ops
    from storygen_amd.dedup import KeyframeDeduper
    from tests import dedup_reference as D
    dev = torch.device("cuda:0")
    N, thr = args.frames, 0.75
    sd = D.tiny_state(0, table_scale=1.0, embed_dim=768, depth=12, img_size=224)
    shots = [D.block_image(s, 720, 1280, cells=9) for s in range(N // 4 + 1)]
    frames = np.stack([shots[i // 4] if i % 4 == 0 else D.near_copy(shots[i // 4], i) for i in range(N)])      # shots of four keyframes
    dd = KeyframeDeduper(sd, device=dev, threshold=thr)
    t0 = time.perf_counter()
    px8 = D.pixel_values(list(frames[:8]))
    pil_ms = (time.perf_counter() - t0) * 1e3 / 8
    out = dd.dedup(frames)
    px = torch.cat([D.pixel_values(list(frames[lo:lo + 8])) for lo in range(0, N, 8)]).to(dev)
    assert torch.equal(px[:8].cpu(), px8)
    sds = {dt: {k: v.to(dev, dt) for k, v in sd.items()} for dt in (torch.float16, torch.float32)}
    pxs = {dt: px.to(dt) for dt in sds}
    with torch.no_grad():
        ref = {dt: torch_decisions(torch_tower(sds[dt], pxs[dt], 12), thr) for dt in sds}
    big = torch.randn(4096, 768, device=dev)
    sim_o, drop_o = ops.adjacent_cosine(big)
    torch.cuda.synchronize()
    t = {"ours": [], "ours_dev": [], "t16": [], "t32": [], "kernel": [], "cos": []}
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        dd.dedup(frames)
        t["ours"].append((time.perf_counter() - t0) * 1e3)
        up = torch.from_numpy(frames).to(dev)
        t["ours_dev"].append(timed(lambda: ops.adjacent_cosine(dd.engine(up), thr), 1))
        with torch.no_grad():
            t["t16"].append(timed(lambda: torch_decisions(torch_tower(sds[torch.float16], pxs[torch.float16], 12), thr), 1))
            t["t32"].append(timed(lambda: torch_decisions(torch_tower(sds[torch.float32], pxs[torch.float32], 12), thr), 1))
        t["kernel"].append(timed(lambda: ops.adjacent_cosine(big, thr, sim=sim_o, drop=drop_o), 50))
        t["cos"].append(timed(lambda: torch_decisions(big, thr), 50))
    med = {k: statistics.median(v) for k, v in t.items()}
    agree = {dt: int((ref[dt][1].cpu().numpy() == out.drop).sum()) for dt in sds}
    dsim = {dt: float(np.abs(ref[dt][0].double().cpu().numpy() - out.similarity).max()) for dt in sds}
    lines = [f"{N} uint8 frames of 1280 x 720, dino_vitb8 geometry (12 layers, 768 wide, 785 tokens, random weights), threshold {thr}; "
             f"{args.rounds} alternating rounds",
             f"  KeyframeDeduper.dedup: upload + patchify + tower + decision + copies back    median {med['ours']:9.2f} ms wall (min {min(t['ours']):.2f}, max {max(t['ours']):.2f})",
             f"    of which on the device, frames already uploaded (patchify + tower + kernel) median {med['ours_dev']:9.2f} ms",
             f"  torch ops fp16, pixels already transformed and on the device + cosine          median {med['t16']:9.2f} ms",
             f"  torch ops fp32, the same                                                      median {med['t32']:9.2f} ms",
             f"  the script's PIL transform (Resize 256 + CenterCrop 224 + Normalize), this host      {pil_ms:9.2f} ms per frame (8 frames, once)",
             f"  sg_adjacent_cosine_f64 alone, 4096 x 768                                      median {med['kernel'] * 1e3:9.1f} us",
             f"  torch.cosine_similarity + compare (fp32), 4096 x 768                          median {med['cos'] * 1e3:9.1f} us",
             f"  decisions: {int(out.drop.sum())} of {N} dropped; equal to torch fp16 on {agree[torch.float16]} / {N}, to torch fp32 on {agree[torch.float32]} / {N}; "
             f"largest similarity difference {dsim[torch.float16]:.2e} (fp16), {dsim[torch.float32]:.2e} (fp32)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
