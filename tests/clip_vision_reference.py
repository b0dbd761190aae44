"""TEST INFRASTRUCTURE — fp32 restatements, on the CPU, of what storygen_amd.clip_score computes on the GPU:

  * the `clip` package's image preprocessing (torchvision Resize(S, BICUBIC) + CenterCrop(S) + Normalize) on float images, resampling through
    torch.nn.functional.interpolate(mode="bicubic", antialias=True);
  * transformers' CLIPVisionTransformer + visual_projection.

tests/test_clip_vision_reference.py pins the geometry to hand-computed numbers and the tower to transformers.  With `round_operands=True`
the tower rounds to fp16 exactly where ClipVisionEngine does (every MFMA operand, the LayerNorm outputs, the activation): the distance
between that run and the fp32 one is the deviation the number formats alone account for (tests/test_clip_score_gpu.py derives its bars
for the projected embedding and the cosine from it).  Nothing in the product imports this file."""
import torch
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def resize_geometry(H: int, W: int, S: int):
    """(resized H, resized W, top, left): the shorter side becomes S, the longer int(S * long / short); CenterCrop's offset is
    int(round((size - S) / 2.0)) — Python's round, halves to the even integer — per axis."""
    short, long_ = (W, H) if W <= H else (H, W)
    new_long = int(S * long_ / short)
    RH, RW = (new_long, S) if W <= H else (S, new_long)
    return RH, RW, int(round((RH - S) / 2.0)), int(round((RW - S) / 2.0))


def preprocess(x: torch.Tensor, S: int, in_scale: float = 1.0, in_shift: float = 0.0, mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """x float [B,3,H,W] -> normalised fp32 [B,3,S,S]."""
    B, _, H, W = x.shape
    RH, RW, top, left = resize_geometry(H, W, S)
    v = x.float() * in_scale + in_shift
    v = F.interpolate(v, size=(RH, RW), mode="bicubic", antialias=True, align_corners=False)
    v = v[:, :, top:top + S, left:left + S]
    m, s = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1), torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return (v - m) / s


def patch_rows(pixels: torch.Tensor, ps: int) -> torch.Tensor:
    """[B,3,S,S] -> [B * (S/ps)^2, 3*ps*ps]: row-major patches, columns (c, dy, dx) — the rows a stride-ps convolution multiplies with
    weight.view(C, 3*ps*ps)."""
    B, Cc, S, _ = pixels.shape
    G = S // ps
    return pixels.reshape(B, Cc, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, Cc * ps * ps)


def _r(t: torch.Tensor, on: bool) -> torch.Tensor:
    return t.half().float() if on else t


def vision_forward(sd, pixels: torch.Tensor, heads: int, eps: float = 1e-5, hidden_act: str = "quick_gelu", round_operands: bool = False):
    """transformers CLIPVisionModelWithProjection.forward on preprocessed pixels [B,3,S,S] with the state dict `sd` (transformers names):
    (image_embeds [B, projection_dim], last_hidden_state [B,T,C]), fp32."""
    g = lambda n: sd[n].float()   # noqa: E731
    r = lambda t: _r(t, round_operands)   # noqa: E731
    wp = g("vision_model.embeddings.patch_embedding.weight")
    C, ps = wp.shape[0], wp.shape[2]
    B = pixels.shape[0]
    pe = r(patch_rows(pixels.float(), ps)) @ r(wp.reshape(C, -1)).t()                          # = conv2d(pixels, wp, stride=ps)
    P = pe.shape[0] // B
    x = torch.cat([g("vision_model.embeddings.class_embedding").expand(B, 1, C), pe.view(B, P, C)], 1)
    x = x + g("vision_model.embeddings.position_embedding.weight")[None]
    T = P + 1
    x = r(F.layer_norm(x, (C,), g("vision_model.pre_layrnorm.weight"), g("vision_model.pre_layrnorm.bias"), eps))
    D = C // heads
    i = 0
    while f"vision_model.encoder.layers.{i}.layer_norm1.weight" in sd:
        p = f"vision_model.encoder.layers.{i}."
        lin = lambda t, n: r(t) @ r(g(p + n + ".weight")).t() + g(p + n + ".bias")   # noqa: E731
        h = F.layer_norm(x, (C,), g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias"), eps)
        q, k, v = (r(lin(h, "self_attn." + n)).view(B, T, heads, D).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        a = torch.softmax((q * D ** -0.5) @ k.transpose(-1, -2), -1) @ v
        x = x + lin(a.transpose(1, 2).reshape(B, T, C), "self_attn.out_proj")
        h = F.layer_norm(x, (C,), g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias"), eps)
        u = r(lin(h, "mlp.fc1"))
        u = u * torch.sigmoid(1.702 * u) if hidden_act == "quick_gelu" else F.gelu(u)
        x = x + lin(u, "mlp.fc2")
        i += 1
    pooled = F.layer_norm(x[:, 0], (C,), g("vision_model.post_layernorm.weight"), g("vision_model.post_layernorm.bias"), eps)
    return r(pooled) @ r(g("visual_projection.weight")).t(), x


def cosine(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))
