"""Frame / narration alignment on the host (no GPU): the NumPy restatement of tests/align_reference.py against hand-worked cases, the
one-minute boundaries of the time penalty, the timestamp parsing, the path's invariants on 200 random shapes, the host-side rejections of
sg_align_cost_f64 / sg_dtw_path_f64 and their ops wrappers, FrameAligner's host logic over the emulated ops of
tests/align_ops_emulation.py, and the restatement of the two towers at a small ViT-B/16-shaped config pinned to transformers."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from tests import align_reference as A
from tests import pick_score_reference as P
from tests.align_ops_emulation import patched_align_ops

INF = float("inf")


# ------------------------------------------------------------------------------------------------- the restatement, worked by hand
def test_two_by_two_by_hand():
    path, acc, codes = A.dtw(np.array([[1.0, 2.0], [3.0, 1.0]]))
    assert acc.tolist() == [[1.0, 3.0], [4.0, 2.0]]                 # (1,1): 1 + min(1, 3, 4)
    assert codes.tolist() == [[0, 2], [1, 0]]
    assert path == [(0, 0), (1, 1)] and A.groups(path) == [(0, [0]), (1, [1])]


def test_three_by_two_with_a_three_way_tie_by_hand():
    """(2,1) sees diagonal acc[1,0] = 2, up acc[1,1] = 2 and left acc[2,0] = 2: the diagonal, first in the order, wins."""
    M = np.array([[1.0, 1.0], [1.0, 1.0], [0.0, 5.0]])
    path, acc, codes = A.dtw(M)
    assert acc.tolist() == [[1.0, 2.0], [2.0, 2.0], [2.0, 7.0]]
    assert (acc[1, 0], acc[1, 1], acc[2, 0]) == (2.0, 2.0, 2.0)
    assert codes.tolist() == [[0, 2], [1, 0], [1, 0]]
    assert path == [(0, 0), (1, 0), (2, 1)] and A.groups(path) == [(0, [0]), (1, [0]), (2, [1])]


def test_up_wins_a_tie_with_left_by_hand():
    """Negative costs make up = left = 0 < diagonal = 1 at (1,1): up, second in the order, wins; frame 0 then owns both sentences."""
    path, acc, codes = A.dtw(np.array([[1.0, -1.0], [-1.0, 4.0]]))
    assert acc.tolist() == [[1.0, 0.0], [0.0, 4.0]] and codes[1, 1] == A.UP
    assert path == [(0, 0), (0, 1), (1, 1)] and A.groups(path) == [(0, [0, 1]), (1, [1])]


def test_single_row_and_single_column():
    p, acc, codes = A.dtw(np.array([[1.0, 2.0, 3.0]]))
    assert p == [(0, 0), (0, 1), (0, 2)] and acc.tolist() == [[1.0, 3.0, 6.0]] and codes.tolist() == [[0, 2, 2]]
    p, acc, codes = A.dtw(np.array([[1.0], [2.0], [3.0]]))
    assert p == [(0, 0), (1, 0), (2, 0)] and acc.tolist() == [[1.0], [3.0], [6.0]] and codes.tolist() == [[0], [1], [1]]


def test_sixty_second_boundaries():
    """dt = 60 no penalty, 60.001 one, 119.9 one, 120 two; the cosine distance of a vector with itself is the 1e-9 of the denominator."""
    f = np.array([[3.0, 4.0]], np.float32)
    times = [60.0, 60.001, 119.9, 120.0, 0.0, 59.999, 180.0, 3600.5]
    M = A.cost_matrix(f, np.repeat(f, len(times), 0), [0.0], times)
    cd = A.cosine_distance(f[0], f[0])
    assert 0.0 < cd < 2e-9
    assert (M[0] - cd).tolist() == [0.0, 1.0, 1.0, 2.0, 0.0, 0.0, 3.0, 60.0]
    # the distance is symmetric in the two times, and a zero feature row keeps the quotient finite: cd = 1 - 0 / 1e-9
    assert A.cost_matrix(f, f, [200.0], [79.0])[0, 0] - cd == 2.0
    assert A.cost_matrix(np.zeros((1, 2), np.float32), f, [0.0], [0.0])[0, 0] == 1.0
    # orthogonal and opposite vectors
    g = np.array([[-4.0, 3.0], [-3.0, -4.0]], np.float32)
    assert np.allclose(A.cost_matrix(f, g, [0.0], [0.0, 0.0])[0], [1.0, 2.0], atol=1e-9, rtol=0)


STAMPS = [("0-1-23-456", 83.456), ("0-0-0-0", 0.0), ("1-0-0-5", 3600.005), ("2-59-59-999", 10799.999), ("0-0-7-50", 7.05),
          ("10-10-10-10", 36610.01), ("0-0-59-1000", 60.0)]


@pytest.mark.parametrize("stamp,want", STAMPS)
def test_timestamp_seconds(stamp, want):
    """h * 3600 + m * 60 + s as integers, then + (10 * ms) * 0.0001 in float64: "0-1-23-456" is 83 + 4560 * 0.0001."""
    from storygen_amd.align import timestamp_seconds
    h, m, s, ms = (int(v) for v in stamp.split("-"))
    by_hand = (h * 3600 + m * 60 + s) + (ms * 10) * 0.0001
    assert timestamp_seconds(stamp) == A.timestamp_seconds(stamp) == by_hand
    assert abs(by_hand - want) < 1e-9
    assert isinstance(timestamp_seconds(stamp), float)


def test_timestamp_seconds_by_hand():
    """Worked on paper, the last field as tenths of a millisecond times 0.0001: 456 -> 4560 * 0.0001 = 0.456; 50 -> 500 * 0.0001 = 0.05
    (not 0.5: the field is a count, not a decimal fraction); 1000 -> 1 s.  Leading zeros count for nothing."""
    from storygen_amd.align import timestamp_seconds
    assert timestamp_seconds("0-1-23-456") == 83 + 4560 * 0.0001 and abs(timestamp_seconds("0-1-23-456") - 83.456) < 1e-12
    assert timestamp_seconds("0-0-7-50") == 7 + 500 * 0.0001 and timestamp_seconds("0-0-7-050") == 7 + 500 * 0.0001
    assert abs(timestamp_seconds("0-0-7-50") - 7.05) < 1e-12
    assert timestamp_seconds("1-1-1-0") == 3661.0 and timestamp_seconds("01-01-01-000") == 3661.0
    assert timestamp_seconds("0-0-59-1000") == 60.0
    assert timestamp_seconds("0-2-0-0") - timestamp_seconds("0-1-0-0") == 60.0


@pytest.mark.parametrize("bad", ["1-2-3", "1-2-3-4-5", "a-b-c-d", "", "1:2:3.4", 12.0, None, "0-0--1-0", " 0-0-1-0", "0-0-1-0\n", "0-0-1.5-0"])
def test_timestamp_seconds_refuses_other_forms(bad):
    from storygen_amd.align import timestamp_seconds
    with pytest.raises(ValueError, match="H-M-S-ms"):
        timestamp_seconds(bad)


# ------------------------------------------------------------------------------------------------- invariants
def test_path_invariants_on_200_random_shapes():
    rng = np.random.default_rng(0)
    for n in range(200):
        r, c = (int(v) for v in rng.integers(1, 41, 2))
        M = rng.integers(0, 4, (r, c)).astype(np.float64) if n % 2 else rng.random((r, c))
        path, acc, codes = A.dtw(M)
        assert path[0] == (0, 0) and path[-1] == (r - 1, c - 1) and max(r, c) <= len(path) <= r + c - 1
        steps = {(b[0] - a[0], b[1] - a[1]) for a, b in zip(path, path[1:])}
        assert steps <= {(1, 1), (1, 0), (0, 1)}, steps
        # the diagonal-at-a-time fill is the double loop, and following the codes is the script's argmin over the values
        acc2, codes2 = A.accumulate_loops(M)
        assert np.array_equal(acc, acc2) and np.array_equal(codes, codes2)
        assert A.backtrace_values(acc) == path
        assert acc[-1, -1] == sum(M[i, j] for i, j in path) or abs(acc[-1, -1] - sum(M[i, j] for i, j in path)) < 1e-9
        g = A.groups(path)
        assert [i for i, _ in g] == sorted({i for i, _ in path}) and sum(len(s) for _, s in g) == len(path)


def test_all_equal_matrix_goes_down_the_diagonal_first():
    for r, c in ((5, 5), (3, 7), (7, 3)):
        path, _, _ = A.dtw(np.ones((r, c)))
        n = min(r, c)
        assert path[-n:] == [(r - n + k, c - n + k) for k in range(n)]            # the walk leaves (r-1, c-1) diagonally ...
        assert all(i == 0 or j == 0 for i, j in path[:len(path) - n + 1])          # ... and finishes along a border


def test_decision_margin():
    acc = A.dtw(np.array([[1.0, 1.0], [1.0, 1.0], [0.0, 5.0]]))[1]
    assert A.decision_margin(acc) == 0.0                                            # the three-way tie
    assert A.decision_margin(A.dtw(np.array([[1.0, 2.0], [3.5, 1.0]]))[1]) == 2.0   # (1,1): 1, 3, 4.5
    assert A.decision_margin(np.ones((1, 5))) == INF


# ------------------------------------------------------------------------------------------------- host-side rejections
@pytest.fixture(scope="module")
def lib():
    from storygen_amd import _lib
    from storygen_amd.build import build
    build(force=False, verbose=False)
    return _lib.load()


def test_entry_points_reject_before_launch(lib):
    """Fake pointers, no device: every refusal is SG_EINVAL with a message, and nothing is enqueued."""
    P_ = 0x10000

    def cost(frames=P_, ldf=8, sents=P_ * 2, ft=P_ * 3, st=P_ * 4, out=P_ * 5, ldo=7, r=5, c=7, dim=8):
        return lib.sg_align_cost_f64(frames, ldf, sents, ft, st, out, ldo, r, c, dim, None)

    def dtw(cost_=P_, ldc=7, r=5, c=7, codes=P_ * 2, acc=None, lda=0, path=P_ * 3, plen=P_ * 4):
        return lib.sg_dtw_path_f64(cost_, ldc, r, c, codes, acc, lda, path, plen, None)

    for kw, msg in ((dict(frames=None), b"null"), (dict(sents=None), b"null"), (dict(ft=None), b"null"), (dict(st=None), b"null"),
                    (dict(out=None), b"null"), (dict(r=0), b"at least 1"), (dict(c=0), b"at least 1"), (dict(r=-3), b"at least 1"),
                    (dict(r=65536, ldo=7), b"exceed 65535"), (dict(c=65536, ldo=65536), b"exceed 65535"),
                    (dict(r=65535, c=32769, ldo=32769), b"2^31"), (dict(dim=0), b"dim = 0"), (dict(ldf=7), b"below dim"), (dict(ldo=6), b"below c")):
        assert cost(**kw) == -1, kw
        assert msg in lib.sg_last_error(), (kw, lib.sg_last_error())
    for kw, msg in ((dict(cost_=None), b"null"), (dict(codes=None), b"null"), (dict(path=None), b"null"), (dict(plen=None), b"null"),
                    (dict(r=0), b"at least 1"), (dict(c=-1), b"at least 1"), (dict(r=65536), b"exceed 65535"),
                    (dict(c=65536, ldc=65536), b"exceed 65535"), (dict(r=2049, c=2049, ldc=2049), b"shorter side"),
                    (dict(r=65535, c=32769, ldc=32769), b"2^31"), (dict(ldc=6), b"cost row stride"),
                    (dict(acc=P_ * 6, lda=6), b"acc row stride")):
        assert dtw(**kw) == -1, kw
        assert msg in lib.sg_last_error(), (kw, lib.sg_last_error())


def test_ops_wrappers_validate():
    from storygen_amd import ops
    assert (ops.DTW_MAX_SHORT, ops.DTW_MAX_SIDE) == (2048, 65535)
    header = open(__file__.replace("tests/test_align_host.py", "include/storygen_hip.h")).read()
    for name, value in (("SG_DTW_MAX_SHORT", 2048), ("SG_DTW_MAX_SIDE", 65535), ("SG_DTW_THREADS", 256)):
        assert f"#define {name} {value}\n" in header
    f, s, t = torch.zeros(3, 8), torch.zeros(4, 8), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(TypeError, match="CUDA/HIP float32"):
        ops.align_cost(f, s, t, torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError, match="CUDA/HIP float32"):
        ops.align_cost(f.double(), s, t, t)
    with pytest.raises(TypeError, match="CUDA/HIP float64"):
        ops.dtw_path(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(TypeError, match="CUDA/HIP float64"):
        ops.dtw_path(torch.zeros(3, 4))
    # every tensor of a launch on one device (a second GPU is not needed to see the refusal: the meta device stands in for it)
    ops._same_device("x", f, a=s, b=None)
    with pytest.raises(ValueError, match="sent_times is on meta"):
        ops._same_device("x", f, sent_feats=s, sent_times=torch.zeros(4, dtype=torch.float64, device="meta"))
    ops.check_align_sides("x", 2048, 65535 // 2, dtw=True)
    ops.check_align_sides("x", 65535, 2048, dtw=True)
    ops.check_align_sides("x", 30000, 30000, dtw=False)
    for r, c, dtw in ((0, 3, False), (3, 0, True), (65536, 1, False), (1, 65536, True), (2049, 2049, True), (65535, 32769, False),
                      (46341, 46341, False)):
        with pytest.raises(ValueError):
            ops.check_align_sides("x", r, c, dtw=dtw)


# ------------------------------------------------------------------------------------------------- FrameAligner's host logic
SEED = A.STORY_SEED


@pytest.fixture(scope="module")
def story():
    cfg = A.b16_config()
    return cfg, P.tiny_state(SEED, cfg), A.story_inputs(SEED)


def test_aligner_host_logic(story):
    from PIL import Image
    from storygen_amd.align import Alignment, FrameAligner, align_features
    cfg, sd, (frames, fstamps, ids, sstamps, ocr) = story
    with patched_align_ops() as calls:
        al = FrameAligner(sd, cfg, device="cpu")
        assert al.crop == "torchvision" and al.vision.wide and (al.vision.T, al.vision.ps, al.vision.heads, al.text.heads) == (17, 16, 2, 2)
        mixed = [frames[0], Image.fromarray(frames[1]), torch.from_numpy(frames[2]), frames[3], Image.fromarray(frames[4])]
        out = al.align(mixed, fstamps, torch.from_numpy(ids), sstamps, ocr_ids=ocr)
        assert isinstance(out, Alignment) and calls == [("align_cost", (5, 32), (7, 32)), ("dtw_path", (5, 7))]
        # the frame features: the text feature of the OCR ids where given, the image feature of the frame elsewhere, in the frames' order
        feats = al.frame_features(frames, ocr)
        img, txt = al.image_features(frames), al.text_features(torch.from_numpy(np.stack([ocr[1], ocr[3]])))
        assert torch.equal(feats[[0, 2, 4]], img[[0, 2, 4]]) and torch.equal(feats[[1, 3]], txt)
        assert torch.equal(al.frame_features(frames), img) and torch.equal(al.frame_features(frames, [None] * 5), img)
        sent = al.text_features(torch.from_numpy(ids))
        ft, st = [A.timestamp_seconds(s) for s in fstamps], [A.timestamp_seconds(s) for s in sstamps]
        want_M = A.cost_matrix(feats.numpy(), sent.numpy(), ft, st)
        want_path = A.dtw(want_M)[0]
        assert np.array_equal(out.cost.numpy(), want_M) and out.path == want_path and out.groups == A.groups(want_path)
        assert {int(v) for v in np.floor(want_M).flatten()} >= {0, 1, 2}                  # no, one and two minutes of penalty occur
        # times as floats, arrays or tensors are the stamps' seconds; features in hand take the same route
        for tf, ts in ((ft, st), (np.array(ft), torch.tensor(st, dtype=torch.float64))):
            assert al.align(frames, tf, ids, ts, ocr).path == want_path
        assert align_features(feats, sent, fstamps, st).path == want_path
        # refusals
        with pytest.raises(ValueError, match="ocr_ids"):
            al.align(frames, fstamps, ids, sstamps, ocr_ids=ocr[:4])
        with pytest.raises(ValueError, match="one length"):
            al.frame_features(frames, [None, ocr[1], None, ocr[3][:5], None])
        with pytest.raises(ValueError, match="4 times for 5"):
            al.align(frames, fstamps[:4], ids, sstamps)
        with pytest.raises(ValueError, match="8 times for 7"):
            al.align(frames, fstamps, ids, sstamps + ["0-9-0-0"])
        with pytest.raises(ValueError, match="sentence_ids"):
            al.align(frames, fstamps, ids[0], sstamps)
        with pytest.raises(ValueError, match="H-M-S-ms"):
            al.align(frames, ["0:0:1.5"] * 5, ids, sstamps)
        with pytest.raises(TypeError, match="8-bit"):
            al.align(torch.rand(5, 3, 64, 64), fstamps, ids, sstamps)
        with pytest.raises(ValueError, match="shorter side"):
            align_features(torch.zeros(2049, 8), torch.zeros(2049, 8), np.zeros(2049), np.zeros(2049))
        with pytest.raises(ValueError):
            align_features(torch.zeros(0, 8), sent, [], st)


def test_aligner_refuses_what_the_kernels_cannot_run(story):
    from storygen_amd.align import FrameAligner
    cfg, sd, _ = story
    with patched_align_ops():
        for side, key, value in (("vision_config", "hidden_act", "relu"), ("text_config", "hidden_act", "silu"),
                                 ("vision_config", "image_size", 70), ("text_config", "num_attention_heads", 1)):
            bad = {**cfg, side: {**cfg[side], key: value}}
            with pytest.raises(ValueError):
                FrameAligner(sd, bad, device="cpu")
        with pytest.raises(KeyError, match="text tower"):
            FrameAligner({k: v for k, v in sd.items() if not k.startswith("text_")}, cfg, device="cpu")
        with pytest.raises(KeyError, match="image tower"):
            FrameAligner({k: v for k, v in sd.items() if not k.startswith("vis")}, cfg, device="cpu")
        with pytest.raises(KeyError, match="vision_config"):
            FrameAligner(sd, cfg["vision_config"], device="cpu")
        # the real model's geometry passes the host checks: ViT-B/16, 197 tokens, 12 heads of 64; text 8 heads of 64
        from storygen_amd.pick_score import check_pick_config
        check_pick_config(dict(hidden_size=768, num_attention_heads=12, image_size=224, patch_size=16),
                          dict(hidden_size=512, num_attention_heads=8, max_position_embeddings=77), "FrameAligner")


# ------------------------------------------------------------------------------------------------- the towers, pinned
def test_tower_restatement_matches_transformers_at_a_b16_shape(story):
    """tests/pick_score_reference.py at the aligner's kind of model — patch 16, heads of 64, quick_gelu, no attention mask (the `clip`
    package's encode_text has none) — against transformers' CLIPModel: 1e-5 rel-L2, the fp32 bar of tests/test_pick_score_reference.py.
    Then the aligner's engines over the emulated ops against that restatement, as tests/test_pick_score_host.py holds PickScorer's."""
    transformers = pytest.importorskip("transformers")
    from storygen_amd.align import FrameAligner
    from tests import clip_u8_reference as U
    cfg, sd, (frames, _, ids, _, ocr) = story
    conf = transformers.CLIPConfig(text_config=cfg["text_config"], vision_config=cfg["vision_config"], projection_dim=cfg["projection_dim"],
                                   logit_scale_init_value=cfg["logit_scale_init_value"])
    model = transformers.CLIPModel(conf).eval().float()
    own = {k: v for k, v in model.state_dict().items() if not k.endswith("position_ids")}
    assert set(own) == set(sd), sorted(set(own) ^ set(sd))[:6]
    model.load_state_dict(sd, strict=False)
    px = U.pixel_values(frames, 64, "torchvision")
    tids = torch.from_numpy(ids)
    with torch.no_grad():
        wi, wt = model.get_image_features(pixel_values=px), model.get_text_features(input_ids=tids)
        wi, wt = (getattr(t, "pooler_output", t) for t in (wi, wt))
    gi, gt = P.image_features(sd, cfg, px), P.text_features(sd, cfg, tids)
    print(f"ViT-B/16-shaped restatement vs transformers: image features rel-L2 {rel_l2(gi, wi):.2e}, text features {rel_l2(gt, wt):.2e}")
    assert tuple(gi.shape) == (5, 32) and tuple(gt.shape) == (7, 32)
    assert rel_l2(gi, wi) < 1e-5 and rel_l2(gt, wt) < 1e-5
    f, s = A.story_features(sd, cfg, frames, ids, ocr)
    assert np.array_equal(s, gt.numpy()) and np.array_equal(f[[0, 2, 4]], gi.numpy()[[0, 2, 4]]) and not np.array_equal(f[1], gi.numpy()[1])
    with patched_align_ops():
        al = FrameAligner(sd, cfg, device="cpu")
        ei, et = al.image_features(frames), al.text_features(tids)
    ri, rt = P.image_features(sd, cfg, px, round_operands=True), P.text_features(sd, cfg, tids, round_operands=True)
    print(f"engines over emulated ops: image {rel_l2(ei, gi):.2e} (fp16-rounded restatement {rel_l2(ri, gi):.2e}), text {rel_l2(et, gt):.2e} "
          f"(fp16-rounded restatement {rel_l2(rt, gt):.2e})")
    assert rel_l2(ei, gi) < 2e-3 and rel_l2(et, gt) < 2e-3                              # the bars of tests/test_pick_score_host.py
    assert rel_l2(ei, ri) < 5e-4 and rel_l2(et, rt) < 5e-4


def test_gpu_seed_leaves_every_decision_a_margin(story):
    """The end-to-end GPU test compares paths: on the restatement's own cost matrix the best and second-best predecessor of every cell
    differ by far more than the engines' fp16-level deviation can move a cost."""
    cfg, sd, (frames, fstamps, ids, sstamps, ocr) = story
    f, s = A.story_features(sd, cfg, frames, ids, ocr)
    fr, sr = A.story_features(sd, cfg, frames, ids, ocr, round_operands=True)
    ft, st = [A.timestamp_seconds(v) for v in fstamps], [A.timestamp_seconds(v) for v in sstamps]
    M, Mr = A.cost_matrix(f, s, ft, st), A.cost_matrix(fr, sr, ft, st)
    path, acc, _ = A.dtw(M)
    margin, moved = A.decision_margin(acc), float(np.abs(Mr - M).max())
    print(f"decision margin {margin:.3e}; fp16-rounded towers move a cost by at most {moved:.3e}; path {path}")
    assert margin > 1e-6
    assert margin > 4 * (5 + 7 - 1) * moved          # an accumulated value sums at most r + c - 1 costs; two of them are compared
    assert A.dtw(Mr)[0] == path
