"""Plain-torch fp32 restatement of the DINOv2 image-similarity reward (edit_ppo/reward_model.py:217-257): test infrastructure, not a fallback.

* ``to_uint8_hwc``     -- torchvision ``ToPILImage`` on a float tensor: ``x.mul(255).byte()`` (multiply in the tensor's dtype, truncation);
* ``pil_bicubic_resize`` -- ``PIL.Image.resize(..., BICUBIC)`` on uint8: two fixed-point passes (horizontal, then vertical, rounded to uint8 in between),
  Keys cubic a = -0.5 with support 2 * scale, coefficients normalised in double and converted as int(+-0.5 + k 2^22), accumulator 2^21, shift 22, clip to 8 bits;
* ``preprocess``       -- the ``facebook/dinov2-base`` processor: shortest edge 256, center crop 224, rescale 1/255, normalise;
* ``Dinov2Oracle``     -- ``transformers.Dinov2Model`` (patch conv, CLS, bicubically interpolated position table, pre-LN blocks with LayerScale, exact GELU);
* ``dino_reward``      -- F.normalize -> F.cosine_similarity -> (cos + 1) * 50.

Checked against the installed transformers / PIL in tests/test_dino_oracle.py; needs neither at run time.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

DINOV2_BASE = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, mlp_ratio=4, image_size=518, patch_size=14, layer_norm_eps=1e-6)
PROCESSOR = dict(shortest_edge=256, crop_size=224, rescale_factor=1 / 255, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225))
PRECISION_BITS = 22


def to_uint8_hwc(x):
    """[3,H,W] float tensor in [0,1] (any float dtype) -> uint8 [H,W,3] numpy, as ToPILImage does"""
    return x.detach().cpu().mul(255).byte().permute(1, 2, 0).contiguous().numpy()


def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_coeffs(in_size, out_size):
    """-> (xmin [out] int, count [out] int, kk [out][ksize] int32): the fixed-point taps of one pass"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ww = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_cubic((x + xmin - center + 0.5) * ww) for x in range(xmax)]
        tot = sum(w)
        for x in range(xmax):
            k = w[x] / tot if tot != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds[:, 0], bounds[:, 1], kk


def _pass(img, out_size, axis):
    """one integer pass along ``axis`` of a uint8 array"""
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    xmin, cnt, kk = resize_coeffs(img.shape[0], out_size)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    for xx in range(out_size):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(cnt[xx]):
            acc += img[xmin[xx] + x] * int(kk[xx, x])
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def pil_bicubic_resize(img, out_h, out_w):
    """uint8 [H,W,C] -> uint8 [out_h,out_w,C]; a pass whose size does not change is skipped, as PIL does"""
    if img.shape[1] != out_w:
        img = _pass(img, out_w, 1)
    if img.shape[0] != out_h:
        img = _pass(img, out_h, 0)
    return img


def resize_output_size(h, w, shortest_edge=256):
    """transformers get_resize_output_image_size(default_to_square=False): the short side becomes ``shortest_edge``, the long side int(edge * long / short)"""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = shortest_edge, int(shortest_edge * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def crop_uint8(img_u8, proc=PROCESSOR):
    """uint8 [H,W,3] -> resized, center-cropped uint8 [3, crop, crop]"""
    h, w = img_u8.shape[:2]
    nh, nw = resize_output_size(h, w, proc["shortest_edge"])
    r = pil_bicubic_resize(img_u8, nh, nw)
    c = proc["crop_size"]
    top, left = (nh - c) // 2, (nw - c) // 2
    return np.ascontiguousarray(r[top:top + c, left:left + c].transpose(2, 0, 1))


def normalize_uint8(crop_u8, proc=PROCESSOR):
    """uint8 [3,h,w] -> fp32 pixel_values, in the processor's own order of operations (rescale in double rounded to fp32, then (x - mean) / std in fp32)"""
    x = (crop_u8.astype(np.float64) * proc["rescale_factor"]).astype(np.float32)
    mean = np.array(proc["image_mean"], dtype=np.float32)[:, None, None]
    std = np.array(proc["image_std"], dtype=np.float32)[:, None, None]
    return (x - mean) / std


def preprocess(images, proc=PROCESSOR):
    """[B,3,H,W] float tensor in [0,1] -> (uint8 crops [B,3,224,224] numpy, pixel_values [B,3,224,224] fp32 tensor)"""
    crops = np.stack([crop_uint8(to_uint8_hwc(im), proc) for im in images])
    return crops, torch.from_numpy(np.stack([normalize_uint8(c, proc) for c in crops]))


def dinov2_manifest(cfg=None):
    c = dict(DINOV2_BASE)
    c.update(cfg or {})
    D, I, P = c["hidden_size"], c["hidden_size"] * c["mlp_ratio"], c["patch_size"]
    n = (c["image_size"] // P) ** 2
    out = [("embeddings.cls_token", (1, 1, D)), ("embeddings.mask_token", (1, D)), ("embeddings.position_embeddings", (1, n + 1, D)),
           ("embeddings.patch_embeddings.projection.weight", (D, 3, P, P)), ("embeddings.patch_embeddings.projection.bias", (D,))]
    for l in range(c["num_hidden_layers"]):
        p = f"encoder.layer.{l}"
        out += [(f"{p}.norm1.weight", (D,)), (f"{p}.norm1.bias", (D,))]
        for q in ("query", "key", "value"):
            out += [(f"{p}.attention.attention.{q}.weight", (D, D)), (f"{p}.attention.attention.{q}.bias", (D,))]
        out += [(f"{p}.attention.output.dense.weight", (D, D)), (f"{p}.attention.output.dense.bias", (D,)), (f"{p}.layer_scale1.lambda1", (D,)),
                (f"{p}.norm2.weight", (D,)), (f"{p}.norm2.bias", (D,)), (f"{p}.mlp.fc1.weight", (I, D)), (f"{p}.mlp.fc1.bias", (I,)),
                (f"{p}.mlp.fc2.weight", (D, I)), (f"{p}.mlp.fc2.bias", (D,)), (f"{p}.layer_scale2.lambda1", (D,))]
    out += [("layernorm.weight", (D,)), ("layernorm.bias", (D,))]
    return out


class Dinov2Oracle:
    """``Dinov2Model(pixel_values).last_hidden_state`` in ``dtype`` (fp32: the oracle; bf16: the class comparator)"""

    def __init__(self, sd, cfg=None, dtype=torch.float32):
        c = dict(DINOV2_BASE)
        c.update(cfg or {})
        self.cfg, self.dtype = c, dtype
        self.sd = {k: v.detach().to(torch.float32) for k, v in sd.items()}

    def position_table(self, gh, gw):
        pos = self.sd["embeddings.position_embeddings"]
        n = pos.shape[1] - 1
        s = int(n ** 0.5)
        if gh * gw == n and gh == gw:
            return pos
        D = pos.shape[-1]
        pp = pos[:, 1:].reshape(1, s, s, D).permute(0, 3, 1, 2)
        pp = F.interpolate(pp.float(), size=(gh, gw), mode="bicubic", align_corners=False)
        return torch.cat([pos[:, :1], pp.permute(0, 2, 3, 1).reshape(1, -1, D)], 1)

    @torch.no_grad()
    def __call__(self, pixel_values):
        c, sd, dt = self.cfg, self.sd, self.dtype
        W = lambda k: sd[k].to(dt)
        D, H, P, eps = c["hidden_size"], c["num_attention_heads"], c["patch_size"], c["layer_norm_eps"]
        x = pixel_values.to(dt)
        B, _, h, w = x.shape
        x = F.conv2d(x, W("embeddings.patch_embeddings.projection.weight"), W("embeddings.patch_embeddings.projection.bias"), stride=P)
        x = x.flatten(2).transpose(1, 2)
        x = torch.cat([W("embeddings.cls_token").expand(B, -1, -1), x], 1) + self.position_table(h // P, w // P).to(dt)
        N = x.shape[1]
        for l in range(c["num_hidden_layers"]):
            p = f"encoder.layer.{l}"
            n = F.layer_norm(x, (D,), W(f"{p}.norm1.weight"), W(f"{p}.norm1.bias"), eps)
            q, k, v = (F.linear(n, W(f"{p}.attention.attention.{t}.weight"), W(f"{p}.attention.attention.{t}.bias")).view(B, N, H, D // H).transpose(1, 2)
                       for t in ("query", "key", "value"))
            a = torch.softmax((q @ k.transpose(-1, -2)) * (D // H) ** -0.5, -1) @ v
            a = F.linear(a.transpose(1, 2).reshape(B, N, D), W(f"{p}.attention.output.dense.weight"), W(f"{p}.attention.output.dense.bias"))
            x = a * W(f"{p}.layer_scale1.lambda1") + x
            n = F.layer_norm(x, (D,), W(f"{p}.norm2.weight"), W(f"{p}.norm2.bias"), eps)
            m = F.linear(F.gelu(F.linear(n, W(f"{p}.mlp.fc1.weight"), W(f"{p}.mlp.fc1.bias"))), W(f"{p}.mlp.fc2.weight"), W(f"{p}.mlp.fc2.bias"))
            x = m * W(f"{p}.layer_scale2.lambda1") + x
        return F.layer_norm(x, (D,), W("layernorm.weight"), W("layernorm.bias"), eps)

    def cls(self, pixel_values):
        return self(pixel_values)[:, 0]


def dino_reward(pred_cls, target_cls):
    """the tail of calculate_dino_reward: CLS features [B,D] x2 -> rewards [B,1] fp32"""
    a = F.normalize(pred_cls, p=2, dim=-1)
    b = F.normalize(target_cls, p=2, dim=-1)
    return ((F.cosine_similarity(a.float(), b.float(), dim=1) + 1.0) * 50.0).unsqueeze(1)


def synthetic_image(seed, h, w, dtype=torch.float32):
    """a smooth image plus mild noise in [0,1], [3,h,w]: seeded, so fixtures store results and not inputs"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    ph = torch.rand(3, 4, generator=g) * 6.28
    fr = 1 + torch.rand(3, 4, generator=g) * 9
    img = torch.stack([0.5 + 0.22 * torch.sin(fr[c, 0] * xx * 6.28 + ph[c, 0]) * torch.cos(fr[c, 1] * yy * 6.28 + ph[c, 1])
                       + 0.2 * torch.sin(fr[c, 2] * (xx + yy) * 6.28 + ph[c, 2]) + 0.1 * torch.cos(fr[c, 3] * (xx - yy) * 12.56 + ph[c, 3]) for c in range(3)])
    img = img + 0.06 * torch.randn(3, h, w, generator=g)
    return img.clamp(0, 1).to(dtype)
