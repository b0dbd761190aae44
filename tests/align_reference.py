"""TEST INFRASTRUCTURE — what the reference's data_process/align.py computes once it has features, restated in NumPy float64: the `H-M-S-ms`
timestamps, the cost matrix (cosine distance plus a penalty of one per whole minute beyond the first), the dynamic-time-warping
recurrence, the first-minimum backtrace and the grouping of the path by frame.  Written from the description of that arithmetic, cell by
cell; `accumulate` fills the same recurrence one anti-diagonal at a time (the same one add and two comparisons per cell on the same
operands, so the same bits) because the GPU tests need matrices of millions of cells, and tests/test_align_host.py holds it to the plain
double loop.  The script's fp16 features and fp16 cosine are not restated: features are fp32, everything after them float64.
Nothing in the product imports this file."""
import numpy as np

DIAGONAL, UP, LEFT = 0, 1, 2


def timestamp_seconds(stamp: str) -> float:
    """`H-M-S-ms` -> seconds as the script's time_dist sees them.  The script parses the stamp with a "0" appended, so the fourth field
    arrives as ten times its value and is scaled by 0.0001; the three integer fields are added first, as integers."""
    h, m, s, ms = (int(v) for v in stamp.split("-"))
    whole = h * 3600 + m * 60 + s
    return whole + int(str(ms) + "0") * 0.0001


def cosine_distance(a: np.ndarray, b: np.ndarray) -> float:
    a, b = a.astype(np.float64), b.astype(np.float64)
    return 1.0 - np.dot(a, b) / (np.sqrt(np.dot(a, a)) * np.sqrt(np.dot(b, b)) + 1e-9)


def cost_matrix(frame_feats, sent_feats, frame_times, sent_times) -> np.ndarray:
    """float64 [r, c]: cosine distance, plus floor(dt / 60) where the two times lie more than 60 s apart."""
    f, s = np.asarray(frame_feats, np.float64), np.asarray(sent_feats, np.float64)
    tf, ts = np.asarray(frame_times, np.float64), np.asarray(sent_times, np.float64)
    M = np.empty((f.shape[0], s.shape[0]), np.float64)
    for i in range(f.shape[0]):
        for j in range(s.shape[0]):
            dt = abs(tf[i] - ts[j])
            cd = cosine_distance(f[i], s[j])
            M[i, j] = cd if dt <= 60 else np.floor(dt / 60) + cd
    return M


def _first_min(dg, up, lf):
    """(minimum, code) of the triple in the order diagonal, up, left; the first minimum wins."""
    m, code = dg, DIAGONAL
    if up < m:
        m, code = up, UP
    if lf < m:
        m, code = lf, LEFT
    return m, code


def accumulate_loops(M: np.ndarray):
    """The recurrence as a plain double loop: (acc float64 [r, c], codes uint8 [r, c]).  Outside the matrix acc[-1, -1] = 0 and every other
    cell is +inf.  codes[i, j] is the move the backtrace makes from (i, j); row 0 can only go left and column 0 only up, which is also what
    the first minimum says whenever the costs are finite."""
    r, c = M.shape
    D = np.full((r + 1, c + 1), np.inf)
    D[0, 0] = 0.0
    codes = np.zeros((r, c), np.uint8)
    for i in range(r):
        for j in range(c):
            m, code = _first_min(D[i, j], D[i, j + 1], D[i + 1, j])
            D[i + 1, j + 1] = M[i, j] + m
            codes[i, j] = code if i > 0 and j > 0 else (LEFT if j > 0 else (UP if i > 0 else DIAGONAL))
    return D[1:, 1:].copy(), codes


def accumulate(M: np.ndarray):
    """accumulate_loops, one anti-diagonal i + j = d at a time."""
    r, c = M.shape
    D = np.full((r + 1, c + 1), np.inf)
    D[0, 0] = 0.0
    codes = np.zeros((r, c), np.uint8)
    with np.errstate(invalid="ignore"):
        for d in range(r + c - 1):
            i = np.arange(max(0, d - (c - 1)), min(r - 1, d) + 1)
            j = d - i
            m, code = D[i, j].copy(), np.zeros(len(i), np.uint8)
            for value, name in ((D[i, j + 1], UP), (D[i + 1, j], LEFT)):
                take = value < m
                m[take], code[take] = value[take], name
            D[i + 1, j + 1] = M[i, j] + m
            code[i == 0] = LEFT
            code[j == 0] = UP
            code[(i == 0) & (j == 0)] = DIAGONAL
            codes[i, j] = code
    return D[1:, 1:].copy(), codes


def backtrace(codes: np.ndarray):
    """From (r - 1, c - 1) while i > 0 or j > 0, following the codes; returned from (0, 0) on."""
    i, j = codes.shape[0] - 1, codes.shape[1] - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        code = codes[i, j]
        if code == DIAGONAL:
            i, j = i - 1, j - 1
        elif code == UP:
            i -= 1
        else:
            j -= 1
        assert i >= 0 and j >= 0
        path.append((i, j))
    return path[::-1]


def backtrace_values(acc: np.ndarray):
    """The backtrace as the script runs it: on the accumulated VALUES, argmin of (diagonal, up, left), first minimum.  For finite costs it
    is `backtrace(codes)`; tests/test_align_host.py checks that."""
    r, c = acc.shape
    D = np.full((r + 1, c + 1), np.inf)
    D[0, 0] = 0.0
    D[1:, 1:] = acc
    i, j = r - 1, c - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        tb = int(np.argmin((D[i, j], D[i, j + 1], D[i + 1, j])))
        if tb == 0:
            i, j = i - 1, j - 1
        elif tb == 1:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return path[::-1]


def dtw(M: np.ndarray):
    """(path, acc, codes) of a cost matrix."""
    acc, codes = accumulate(np.asarray(M, np.float64))
    return backtrace(codes), acc, codes


def groups(path):
    """Consecutive path entries with one frame index -> [(frame, [sentences in order])]."""
    out = []
    for i, j in path:
        if not out or out[-1][0] != i:
            out.append((i, []))
        out[-1][1].append(j)
    return out


def decision_margin(acc: np.ndarray) -> float:
    """The smallest gap between the best and the second-best predecessor over the interior cells (i, j > 0), where the move is a choice."""
    r, c = acc.shape
    if r < 2 or c < 2:
        return float("inf")
    t = np.sort(np.stack([acc[:-1, :-1], acc[:-1, 1:], acc[1:, :-1]]), axis=0)
    return float((t[1] - t[0]).min())


# ------------------------------------------------------------------------------------------------- fixtures shared by the align tests
STORY_SEED = 10       # weights and inputs of the end-to-end tests: tests/test_align_host.py asserts the decision margin this seed leaves


def b16_config(image: int = 64, vision_hidden: int = 128, text_hidden: int = 128, layers: int = 2, proj: int = 32) -> dict:
    """A CLIPConfig-shaped dict with ViT-B/16's features at a small size: patch 16, heads of 64 in both towers, quick_gelu, 77 positions."""
    from tests import pick_score_reference as P
    cfg = P.tiny_config(vision_hidden=vision_hidden, vision_heads=vision_hidden // 64, image=image, patch=16, text_hidden=text_hidden,
                        text_heads=text_hidden // 64, proj=proj, layers=layers)
    cfg["vision_config"]["hidden_act"] = cfg["text_config"]["hidden_act"] = "quick_gelu"
    return cfg


def story_inputs(seed: int, sizes=((70, 90), (64, 64), (70, 90), (100, 66), (64, 80)), sentences: int = 7, T: int = 20, vocab: int = 96):
    """(frames: uint8 [h,w,3] arrays of mixed sizes, frame stamps, sentence ids [c, T], sentence stamps, ocr_ids with two entries set).
    Every id row starts with 0, holds the EOS id — the largest — once and pad id 1 after it.  The stamps step by 25 s and 20 s, so cells
    with no, one and two minutes of penalty all occur."""
    from tests import clip_u8_reference as U
    rng = np.random.default_rng(seed)
    frames = [U.content("random", h, w, seed=seed + i) for i, (h, w) in enumerate(sizes)]

    def ids(n):
        out = rng.integers(2, vocab - 1, (n, T))
        out[:, 0] = 0
        for row, e in zip(out, rng.integers(3, T - 1, n)):
            row[e], row[e + 1:] = vocab - 1, 1
        return out

    sent_ids, ocr_rows = ids(sentences), ids(2)
    ocr = [None] * len(sizes)
    ocr[1], ocr[3] = ocr_rows[0], ocr_rows[1]
    frame_stamps = ["0-%d-%d-%d" % ((25 * i) // 60, (25 * i) % 60, 40 * i) for i in range(len(sizes))]
    sent_stamps = ["0-%d-%d-%d" % ((20 * j + 7) // 60, (20 * j + 7) % 60, 5 * j) for j in range(sentences)]
    return frames, frame_stamps, sent_ids, sent_stamps, ocr


def story_features(sd, cfg, frames, sent_ids, ocr, round_operands: bool = False):
    """(frame features [r, dim], sentence features [c, dim]) of the restatement, fp32 NumPy: an OCR frame is its text's feature."""
    import torch
    from tests import clip_u8_reference as U
    from tests import pick_score_reference as P
    px = U.pixel_values(frames, cfg["vision_config"]["image_size"], "torchvision")
    f = P.image_features(sd, cfg, px, round_operands).clone()
    for i, o in enumerate(ocr):
        if o is not None:
            f[i] = P.text_features(sd, cfg, torch.as_tensor(o)[None], round_operands=round_operands)[0]
    s = P.text_features(sd, cfg, torch.as_tensor(sent_ids), round_operands=round_operands)
    return f.numpy(), s.numpy()
