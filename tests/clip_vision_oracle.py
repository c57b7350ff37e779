"""Plain-torch fp32 restatement of the CLIP image-similarity reward (edit_ppo/reward_model.py:128-134, 512-552): test infrastructure, not a fallback.

* ``PROCESSOR``        -- the ``openai/clip-vit-large-patch14`` processor constants (shortest edge 224, PIL BICUBIC, center crop 224, rescale 1/255, CLIP mean /
  std); the PIL-exact integer resize, the crop and the normalisation are tests/vit_oracle.py's, which take the constants as an argument;
* ``ClipVisionOracle`` -- ``transformers.CLIPVisionModelWithProjection(pixel_values).image_embeds`` (bias-free patch conv, class embedding, learned position
  table, ``pre_layrnorm``, pre-LN blocks with quick-GELU, ``post_layernorm`` of the CLS row, bias-free ``visual_projection``) in a dtype of choice (fp32: the
  oracle; bf16: the class comparator);
* ``clip_reward``      -- F.normalize -> F.cosine_similarity -> (cos + 1) * 50 (the tail the dino reward has).

Checked against the installed transformers / PIL through the committed fixture (tests/test_clip_reward_oracle.py); needs neither at run time.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import vit_oracle as vo
from tests.vit_oracle import to_uint8_hwc, synthetic_image          # noqa: F401  (re-exported: the tests take both from here)

CLIP_VIT_L14 = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
                    projection_dim=768, layer_norm_eps=1e-5)
PROCESSOR = dict(shortest_edge=224, crop_size=224, rescale_factor=1 / 255, image_mean=(0.48145466, 0.4578275, 0.40821073),
                 image_std=(0.26862954, 0.26130258, 0.27577711))


def crop_uint8(img_u8):
    return vo.crop_uint8(img_u8, PROCESSOR)


def preprocess(images):
    """[B,3,H,W] float tensor in [0,1] -> (uint8 crops [B,3,224,224] numpy, pixel_values [B,3,224,224] fp32 tensor)"""
    return vo.preprocess(images, PROCESSOR)


def clip_manifest(cfg=None):
    """names and shapes of ``CLIPVisionModelWithProjection.state_dict()``, in its order (a full ``CLIPModel`` holds the same tensors under the same names)"""
    c = dict(CLIP_VIT_L14)
    c.update(cfg or {})
    D, I, P = c["hidden_size"], c["intermediate_size"], c["patch_size"]
    n = (c["image_size"] // P) ** 2
    v = "vision_model."
    out = [(v + "embeddings.class_embedding", (D,)), (v + "embeddings.patch_embedding.weight", (D, 3, P, P)),
           (v + "embeddings.position_embedding.weight", (n + 1, D)), (v + "pre_layrnorm.weight", (D,)), (v + "pre_layrnorm.bias", (D,))]
    for l in range(c["num_hidden_layers"]):
        p = f"{v}encoder.layers.{l}"
        for q in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out += [(f"{p}.self_attn.{q}.weight", (D, D)), (f"{p}.self_attn.{q}.bias", (D,))]
        out += [(f"{p}.layer_norm1.weight", (D,)), (f"{p}.layer_norm1.bias", (D,)), (f"{p}.mlp.fc1.weight", (I, D)), (f"{p}.mlp.fc1.bias", (I,)),
                (f"{p}.mlp.fc2.weight", (D, I)), (f"{p}.mlp.fc2.bias", (D,)), (f"{p}.layer_norm2.weight", (D,)), (f"{p}.layer_norm2.bias", (D,))]
    out += [(v + "post_layernorm.weight", (D,)), (v + "post_layernorm.bias", (D,)), ("visual_projection.weight", (c["projection_dim"], D))]
    return out


def config_flops(cfg=None, batch=1):
    """multiply-adds x 2 of one forward, from the config alone: patch projection + the pre-LN stack (4 D^2 + 2 D I per token and layer, plus the two
    attention products) + the projection of the CLS row"""
    c = dict(CLIP_VIT_L14)
    c.update(cfg or {})
    D, I, P = c["hidden_size"], c["intermediate_size"], c["patch_size"]
    NP = (c["image_size"] // P) ** 2
    T = NP + 1
    layers = c["num_hidden_layers"] * (2.0 * batch * T * D * (4 * D + 2 * I) + 4.0 * batch * T * T * D)
    return 2.0 * batch * NP * 3 * P * P * D + layers + 2.0 * batch * D * c["projection_dim"]


class ClipVisionOracle:
    def __init__(self, sd, cfg=None, dtype=torch.float32):
        c = dict(CLIP_VIT_L14)
        c.update(cfg or {})
        self.cfg, self.dtype = c, dtype
        self.sd = {k: v.detach().to(torch.float32) for k, v in sd.items()}

    def embeddings(self, pixel_values):
        """the token matrix after ``pre_layrnorm`` [B, T, D]"""
        c, dt = self.cfg, self.dtype
        W = lambda k: self.sd["vision_model." + k].to(dt)
        D, P, eps = c["hidden_size"], c["patch_size"], c["layer_norm_eps"]
        x = F.conv2d(pixel_values.to(dt), W("embeddings.patch_embedding.weight"), None, stride=P).flatten(2).transpose(1, 2)
        x = torch.cat([W("embeddings.class_embedding").expand(x.shape[0], 1, -1), x], 1) + W("embeddings.position_embedding.weight")
        return F.layer_norm(x, (D,), W("pre_layrnorm.weight"), W("pre_layrnorm.bias"), eps)

    @torch.no_grad()
    def __call__(self, pixel_values):
        """pixel_values [B,3,S,S] -> image_embeds [B, projection_dim]"""
        c, dt = self.cfg, self.dtype
        W = lambda k: self.sd["vision_model." + k].to(dt)
        D, H, eps = c["hidden_size"], c["num_attention_heads"], c["layer_norm_eps"]
        x = self.embeddings(pixel_values)
        B, N, _ = x.shape
        for l in range(c["num_hidden_layers"]):
            p = f"encoder.layers.{l}"
            n = F.layer_norm(x, (D,), W(f"{p}.layer_norm1.weight"), W(f"{p}.layer_norm1.bias"), eps)
            q, k, v = (F.linear(n, W(f"{p}.self_attn.{t}_proj.weight"), W(f"{p}.self_attn.{t}_proj.bias")).view(B, N, H, D // H).transpose(1, 2) for t in "qkv")
            a = torch.softmax((q @ k.transpose(-1, -2)) * (D // H) ** -0.5, -1) @ v
            x = x + F.linear(a.transpose(1, 2).reshape(B, N, D), W(f"{p}.self_attn.out_proj.weight"), W(f"{p}.self_attn.out_proj.bias"))
            n = F.layer_norm(x, (D,), W(f"{p}.layer_norm2.weight"), W(f"{p}.layer_norm2.bias"), eps)
            h = F.linear(n, W(f"{p}.mlp.fc1.weight"), W(f"{p}.mlp.fc1.bias"))
            x = x + F.linear(h * torch.sigmoid(1.702 * h), W(f"{p}.mlp.fc2.weight"), W(f"{p}.mlp.fc2.bias"))
        pooled = F.layer_norm(x[:, 0], (D,), W("post_layernorm.weight"), W("post_layernorm.bias"), eps)
        return F.linear(pooled, self.sd["visual_projection.weight"].to(dt))


def clip_reward(pred_embeds, target_embeds):
    """the tail of calculate_clip_reward: image_embeds [B,P] x2 -> rewards [B,1] fp32"""
    a = F.normalize(pred_embeds, p=2, dim=-1)
    b = F.normalize(target_embeds, p=2, dim=-1)
    return ((F.cosine_similarity(a.float(), b.float(), dim=1) + 1.0) * 50.0).unsqueeze(1)
