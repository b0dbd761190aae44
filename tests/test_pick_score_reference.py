"""Pins tests/pick_score_reference.py (the fp32 restatement the GPU tests of PickScore are judged against) to transformers' CLIPModel on a tiny
two-tower model with PickScore's features: head dim 80, patch size 14, gelu, EOS as the largest token id.  Bar: 1e-5 rel-L2, the fp32 bar of
SURVEY §8c.  Also asserts, for the seeds tests/test_pick_score_gpu.py uses, that the best and the second-best score are further apart than
4 x the score bar of that test, so that its argmax assertion cannot hinge on rounding."""
import pytest
import torch

from conftest import rel_l2
from tests import pick_score_reference as P


def test_restatement_matches_transformers_clip_model():
    transformers = pytest.importorskip("transformers")
    cfg = P.tiny_config()
    sd = P.tiny_state(4, cfg)
    conf = transformers.CLIPConfig(text_config=cfg["text_config"], vision_config=cfg["vision_config"], projection_dim=cfg["projection_dim"],
                                   logit_scale_init_value=cfg["logit_scale_init_value"])
    model = transformers.CLIPModel(conf).eval().float()
    own = {k: v for k, v in model.state_dict().items() if not k.endswith("position_ids")}
    assert set(own) == set(sd), sorted(set(own) ^ set(sd))[:6]
    model.load_state_dict(sd, strict=False)
    frames, ids = P.tiny_inputs(21, n_images=3)
    ids = torch.cat([ids, P.tiny_inputs(22, eos_at=17)[1]])
    px = P.preprocess_frames(frames, cfg["vision_config"]["image_size"])
    mask = (ids != 1).long()
    with torch.no_grad():
        wi = model.get_image_features(pixel_values=px)
        wt = model.get_text_features(input_ids=ids, attention_mask=mask)
        wi, wt = (getattr(t, "pooler_output", t) for t in (wi, wt))
        ws = model.logit_scale.exp() * (wt / wt.norm(dim=-1, keepdim=True)) @ (wi / wi.norm(dim=-1, keepdim=True)).t()
    gi, gt = P.image_features(sd, cfg, px), P.text_features(sd, cfg, ids, mask)
    print(f"image features rel-L2 {rel_l2(gi, wi):.2e}, text features {rel_l2(gt, wt):.2e}")
    assert rel_l2(gi, wi) < 1e-5 and rel_l2(gt, wt) < 1e-5
    assert rel_l2(P.scores(sd, cfg, ids, px, mask), ws) < 1e-5
    assert abs(float(model.logit_scale.detach().exp()) - 100.0) < 1e-3
    p = P.probs(sd, cfg, ids, px, mask)
    assert tuple(p.shape) == (2, 3) and float((p.sum(-1) - 1).abs().max()) < 1e-6
    idx, p0 = P.best_of(sd, cfg, ids[:1], px, mask[:1])
    assert idx == int(ws[0].argmax()) and torch.allclose(p0, p[0], atol=1e-6)


def test_rounded_restatement_stays_close_and_differs():
    cfg = P.tiny_config()
    sd = P.tiny_state(2, cfg)
    frames, ids = P.tiny_inputs(13)
    px = P.preprocess_frames(frames, 126)
    for fn, args in ((P.image_features, (px,)), (P.text_features, (ids,))):
        a, b = fn(sd, cfg, *args), fn(sd, cfg, *args, round_operands=True)
        assert 1e-5 < rel_l2(b, a) < 1e-3


def test_gpu_test_seeds_leave_a_clear_winner():
    from tests.test_pick_score_gpu import COSINE_DEV, SCORER_SEEDS, cosine_bar
    cfg = P.tiny_config()
    sd = P.tiny_state(SCORER_SEEDS[0], cfg)
    frames, ids = P.tiny_inputs(SCORER_SEEDS[1])
    px = P.preprocess_frames(frames, cfg["vision_config"]["image_size"])
    s = P.scores(sd, cfg, ids, px)[0]
    top = s.sort(descending=True).values
    score_bar = float(sd["logit_scale"].exp()) * cosine_bar()
    # the first entry of COSINE_DEV is this machine-independent figure: the fp16-rounded restatement against the fp32 one
    t, i = P.text_features(sd, cfg, ids), P.image_features(sd, cfg, px)
    tr, ir = P.text_features(sd, cfg, ids, round_operands=True), P.image_features(sd, cfg, px, round_operands=True)
    dev = float((P.cosines(tr, ir) - P.cosines(t, i)).abs().max())
    print(f"scores {s.tolist()}: gap {float(top[0] - top[1]):.3f}, score bar {score_bar:.3f}; fp16-rounded cosine deviation {dev:.3e}")
    assert abs(dev - COSINE_DEV[0]) < 0.05 * COSINE_DEV[0]
    assert float(top[0] - top[1]) > 4 * score_bar
