"""Times the human / text mask of one frame at the script's real geometry, on the GPU: pred fp16 [1, 25200, 85] (a 640 x 640 detector input,
80 classes), person only, a 1280 x 720 frame, 20 text boxes — HumanTextMasker.mask end to end (two small uploads, sg_det_select,
sg_det_nms, sg_box_mask_u8, one readback) and each launch alone, beside the fp32 restatement of tests/mask_reference.py on this host's
CPU.  Asserts nothing; prints whether detections, ratio and mask equal the restatement's.

    python tools/bench_mask.py [--out FILE] [--rounds N]

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


def scene(A=25200, nc=80, people=5, seed=0):
    """Mostly background (obj ~ rand^6), plus `people` clusters of 60 anchors that agree on a person box to within a few pixels."""
    rng = np.random.default_rng(seed)
    p = np.zeros((A, 5 + nc), np.float32)
    p[:, 0], p[:, 1] = rng.random(A) * 640, rng.random(A) * 640
    p[:, 2], p[:, 3] = 10 + rng.random(A) * 200, 10 + rng.random(A) * 200
    p[:, 4] = rng.random(A) ** 6
    p[:, 5:] = rng.random((A, nc)) * 0.6
    for k in range(people):
        idx = rng.choice(A, 60, replace=False)
        cx, cy, w, h = 80 + 110 * k, 300 + 10 * k, 30 + 4 * k, 90 + 6 * k
        p[idx, :4] = np.array([cx, cy, w, h]) + rng.normal(0, 1.0, (60, 4))
        p[idx, 4] = 0.7 + 0.3 * rng.random(60)
        p[idx, 5] = 0.8 + 0.2 * rng.random(60)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask: needs the GPU (no CPU path)")
    from storygen_amd import ops
    from storygen_amd.mask import HumanTextMasker, letterbox_shape, scale_geometry
    from tests import mask_reference as R
    dev = torch.device("cuda:0")
    frame = (720, 1280)
    input_shape = (640, 640)                                          # 25200 anchors are the 640 x 640 input's; letterbox_shape gives (384, 640)
    rng = np.random.default_rng(1)
    text = [(int(x), int(y), int(x) + 120, int(y) + 30) for x, y in zip(rng.integers(-30, 1250, 20), rng.integers(-10, 700, 20))]
    p16 = torch.from_numpy(scene()).to(torch.float16)
    pred = p16[None].to(dev)
    m = HumanTextMasker()
    got = m.mask(pred, input_shape, [frame], [text])[0]
    t0 = time.perf_counter()
    wm, wdet, wratio, wrem = R.human_text_mask(p16.float().numpy(), input_shape, frame, text)
    cpu = [(time.perf_counter() - t0) * 1e3]
    same = (got.removed == wrem and got.human_ratio == wratio and got.detections.cpu().numpy().tobytes() == wdet.tobytes()
            and (wrem or bool((got.mask.cpu().numpy() == wm).all())))
    geom = torch.tensor([[*scale_geometry(input_shape, frame), frame[1], frame[0]]], dtype=torch.float64).float().to(dev)
    tx = torch.tensor(text, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.det_select_workspace_bytes(1, pred.shape[1]), dtype=torch.uint8, device=dev)
    cand, ncand = ops.det_select(pred, 0.5, (0,), 30000, workspace=ws)
    det, count = ops.det_nms(cand, ncand, geom)
    out, cov = ops.box_mask(*frame, det[0], count, tx)
    torch.cuda.synchronize()
    t = {"wall": [], "select": [], "nms": [], "paint": []}
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        m.mask(pred, input_shape, [frame], [text])
        t["wall"].append((time.perf_counter() - t0) * 1e3)
        t["select"].append(timed(lambda: ops.det_select(pred, 0.5, (0,), 30000, cand=cand, ncand=ncand, workspace=ws), 20))
        t["nms"].append(timed(lambda: ops.det_nms(cand, ncand, geom, det=det, count=count), 20))
        t["paint"].append(timed(lambda: ops.box_mask(*frame, det[0], count, tx, out=out, covered=cov), 20))
    for _ in range(2):
        t0 = time.perf_counter()
        R.human_text_mask(p16.float().numpy(), input_shape, frame, text)
        cpu.append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"pred fp16 [1, 25200, 85], classes (0,), conf 0.5, iou 0.6, frame 1280 x 720, 20 text boxes; {args.rounds} rounds "
             f"(letterbox_shape(720, 1280) = {letterbox_shape(720, 1280)}; the 25200 anchors are a 640 x 640 input's)",
             f"  candidates after the filter {int(ncand[0])}, detections {int(count[0])}, human ratio {got.human_ratio:.4f}, removed {got.removed}",
             f"  HumanTextMasker.mask end to end (uploads, 3 ops, readback)   median {med['wall']:9.3f} ms wall (min {min(t['wall']):.3f}, max {max(t['wall']):.3f})",
             f"  sg_det_select (2 launches)                                    median {med['select'] * 1e3:9.1f} us",
             f"  sg_det_nms                                                    median {med['nms'] * 1e3:9.1f} us",
             f"  sg_box_mask_u8 (memset + 1 launch, 2.76 MB written)           median {med['paint'] * 1e3:9.1f} us",
             f"  the fp32 restatement on this host's CPU (NumPy / torch loops) median {statistics.median(cpu):9.1f} ms (3 runs)",
             f"  detections, ratio, decision and mask equal the restatement's: {same}"]
    text_out = "\n".join(lines)
    print(text_out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text_out + "\n")


if __name__ == "__main__":
    main()
