"""TEST INFRASTRUCTURE — fp32 restatement, on the CPU, of what storygen_amd.pick_score computes on the GPU: transformers' CLIPModel as the
reference's evaluation/calc_Pickscore.py and inference_COCO_val.py use it.

  image side   tests/clip_vision_reference.vision_forward(..., hidden_act=...) on the `clip` preprocessing (CLIPImageProcessor's for ViT-H/14)
  text side    oracle/encoders_oracle.clip_text_forward(..., hidden_act=...) followed by text_projection
  scores       exp(logit_scale) * t^ . i^T; probs = softmax over the images; best_of = argmax for one prompt

tests/test_pick_score_reference.py pins it to transformers.  With `round_operands=True` both towers round to fp16 exactly where the engines do
(every MFMA operand, the LayerNorm outputs, the q|k|v rows, the activation): the distance of that run from the fp32 one is the deviation the
number formats alone account for; tests/test_pick_score_gpu.py derives its bars for the embedding, the cosine and the score from it.  Nothing
in the product imports this file."""
import math

import torch
import torch.nn.functional as F

from oracle import encoders_oracle as eo
from tests import clip_vision_reference as R

TINY = dict(vision_hidden=160, vision_heads=2, image=126, patch=14, text_hidden=64, text_heads=2, vocab=96, proj=32, layers=2)


def tiny_config(**over) -> dict:
    """A CLIPConfig-shaped dict of the tiny PickScore-like model: vision hidden 160 in 2 heads (head dim 80), patch 14, image 126 (82 tokens),
    text hidden 64 in 2 heads, vocabulary 96 with EOS = 95 (the largest id), gelu in both towers as in ViT-H/14."""
    c = dict(TINY, **over)
    return dict(projection_dim=c["proj"], logit_scale_init_value=math.log(100.0),
                vision_config=dict(hidden_size=c["vision_hidden"], intermediate_size=2 * c["vision_hidden"], num_hidden_layers=c["layers"],
                                   num_attention_heads=c["vision_heads"], image_size=c["image"], patch_size=c["patch"], hidden_act="gelu",
                                   layer_norm_eps=1e-5, projection_dim=c["proj"]),
                text_config=dict(vocab_size=c["vocab"], hidden_size=c["text_hidden"], intermediate_size=2 * c["text_hidden"],
                                 num_hidden_layers=c["layers"], num_attention_heads=c["text_heads"], max_position_embeddings=77,
                                 hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=c["proj"], eos_token_id=c["vocab"] - 1, bos_token_id=0,
                                 pad_token_id=1))


def tiny_state(seed: int = 0, config=None) -> dict:
    """fp16-representable CLIPModel state dict for `config` with non-trivial LayerNorms and embeddings of a trained model's order."""
    from storygen_amd.encoders import clip_text_param_shapes, clip_vision_param_shapes, init_state
    cfg = config or tiny_config()
    vc, tc = cfg["vision_config"], cfg["text_config"]
    shapes = clip_vision_param_shapes(vc["hidden_size"], vc["intermediate_size"], vc["num_hidden_layers"], vc["image_size"], vc["patch_size"],
                                      cfg["projection_dim"])
    tshapes = clip_text_param_shapes(tc["vocab_size"], tc["hidden_size"], tc["intermediate_size"], tc["num_hidden_layers"],
                                     tc["max_position_embeddings"])
    tshapes["text_projection.weight"] = (cfg["projection_dim"], tc["hidden_size"])
    sd = {**init_state(shapes, seed), **init_state(tshapes, seed + 1)}
    g = torch.Generator().manual_seed(seed + 2)
    for k in sd:
        if "norm" in k:
            sd[k] = sd[k] + 0.2 * torch.randn(sd[k].shape, generator=g)
        if "embedding" in k:
            sd[k] = sd[k] * 10
        sd[k] = sd[k].half().float()
    sd["logit_scale"] = torch.tensor(cfg["logit_scale_init_value"], dtype=torch.float32)
    return sd


def tiny_inputs(seed: int, n_images: int = 5, hw=(150, 170), T: int = 24, eos_at: int = 10, vocab: int = 96):
    """(frames float [N, H, W, 3] numpy in [0, 1], input_ids [1, T] with the EOS id — the largest — at position eos_at)."""
    g = torch.Generator().manual_seed(seed)
    frames = torch.rand(n_images, hw[0], hw[1], 3, generator=g).numpy()
    ids = torch.randint(2, vocab - 1, (1, T), generator=g)
    ids[:, 0] = 0
    ids[:, eos_at] = vocab - 1
    ids[:, eos_at + 1:] = 1
    return frames, ids


def _r(t, on):
    return t.half().float() if on else t


def image_features(sd, config, pixels: torch.Tensor, round_operands: bool = False) -> torch.Tensor:
    """get_image_features on preprocessed pixels [N, 3, S, S] -> [N, projection_dim]."""
    vc = config["vision_config"]
    return R.vision_forward(sd, pixels, vc["num_attention_heads"], vc.get("layer_norm_eps", 1e-5), vc.get("hidden_act", "quick_gelu"),
                            round_operands)[0]


def image_hidden(sd, config, pixels: torch.Tensor, round_operands: bool = False) -> torch.Tensor:
    vc = config["vision_config"]
    return R.vision_forward(sd, pixels, vc["num_attention_heads"], vc.get("layer_norm_eps", 1e-5), vc.get("hidden_act", "quick_gelu"),
                            round_operands)[1]


def _text_pooled_rounded(sd, ids, heads, eps, hidden_act, attention_mask):
    """clip_text_forward with ClipTextEngine's fp16 rounding points: fp32 residual stream; LayerNorm outputs, q|k|v, the attention output, the
    activation's input and output and every GEMM operand fp16."""
    sd = {k: v.float() for k, v in eo.clip_text_state(sd).items()}
    r = lambda t: t.half().float()   # noqa: E731
    B, T = ids.shape
    x = sd["embeddings.token_embedding.weight"][ids] + sd["embeddings.position_embedding.weight"][:T][None]
    C = x.shape[-1]
    D = C // heads
    mask = torch.full((T, T), float("-inf")).triu(1)[None, None]
    if attention_mask is not None:
        mask = mask + (1.0 - attention_mask[:, None, None, :].float()) * torch.finfo(torch.float32).min
    act = eo.quick_gelu if hidden_act == "quick_gelu" else F.gelu
    i = 0
    while f"encoder.layers.{i}.layer_norm1.weight" in sd:
        p = f"encoder.layers.{i}."
        lin = lambda t, n: r(t) @ r(sd[p + n + ".weight"]).t() + r(sd[p + n + ".bias"])   # noqa: E731
        h = F.layer_norm(x, (C,), r(sd[p + "layer_norm1.weight"]), r(sd[p + "layer_norm1.bias"]), eps)
        q, k, v = (r(lin(h, "self_attn." + n)).view(B, T, heads, D).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        a = torch.softmax((q * D ** -0.5) @ k.transpose(-1, -2) + mask, -1) @ v
        x = x + lin(a.transpose(1, 2).reshape(B, T, C), "self_attn.out_proj")
        h = F.layer_norm(x, (C,), r(sd[p + "layer_norm2.weight"]), r(sd[p + "layer_norm2.bias"]), eps)
        x = x + lin(act(r(lin(h, "mlp.fc1"))), "mlp.fc2")
        i += 1
    x = r(F.layer_norm(x, (C,), r(sd["final_layer_norm.weight"]), r(sd["final_layer_norm.bias"]), eps))
    return x[torch.arange(B), ids.argmax(dim=-1)]


def text_features(sd, config, input_ids: torch.Tensor, attention_mask=None, round_operands: bool = False) -> torch.Tensor:
    """get_text_features -> [P, projection_dim]."""
    tc = config["text_config"]
    heads, eps, act = tc["num_attention_heads"], tc.get("layer_norm_eps", 1e-5), tc.get("hidden_act", "quick_gelu")
    tsd = {k: v for k, v in sd.items() if k.startswith("text_model.")}
    if round_operands:
        pooled = _text_pooled_rounded(tsd, input_ids, heads, eps, act, attention_mask)
    else:
        pooled = eo.clip_text_forward(tsd, input_ids, heads, eps, act, attention_mask)[1]
    return _r(pooled, round_operands) @ _r(sd["text_projection.weight"].float(), round_operands).t()


def cosines(t: torch.Tensor, i: torch.Tensor) -> torch.Tensor:
    return (t / t.norm(dim=-1, keepdim=True)) @ (i / i.norm(dim=-1, keepdim=True)).t()


def scores(sd, config, input_ids, pixels, attention_mask=None, round_operands: bool = False) -> torch.Tensor:
    """exp(logit_scale) * t^ . i^T, [P, N] (calc_Pickscore.py:21 is row 0 with one image)."""
    t = text_features(sd, config, input_ids, attention_mask, round_operands)
    i = image_features(sd, config, pixels, round_operands)
    return sd["logit_scale"].float().exp() * cosines(t, i)


def probs(sd, config, input_ids, pixels, attention_mask=None, round_operands: bool = False) -> torch.Tensor:
    return torch.softmax(scores(sd, config, input_ids, pixels, attention_mask, round_operands), dim=-1)


def best_of(sd, config, input_ids, pixels, attention_mask=None, round_operands: bool = False):
    assert input_ids.shape[0] == 1
    p = probs(sd, config, input_ids, pixels, attention_mask, round_operands)[0]
    return int(p.argmax()), p


def preprocess_frames(frames, S: int) -> torch.Tensor:
    """numpy [N, H, W, 3] in [0, 1] -> preprocessed pixels [N, 3, S, S]."""
    return R.preprocess(torch.as_tensor(frames).float().permute(0, 3, 1, 2), S)
