"""Plain-torch fp32 restatement of the SegFormer mask-agreement reward (edit_ppo/reward_model.py:110-117, 425-481): test infrastructure, not a fallback.

* ``preprocess``       -- ``ToPILImage`` + the Segformer image processor of ``nvidia/segformer-b4-finetuned-ade-512-512`` for a SQUARE input: PIL BILINEAR
  resize to ``size`` x ``size`` (PIL's fixed-point triangle filter; a pass whose size does not change is skipped), rescale 1/255, ImageNet mean / std;
* ``SegformerOracle``  -- ``transformers.SegformerForSemanticSegmentation``: four stages of overlapped patch embedding (7x7 / 4, then 3x3 / 2) + LayerNorm,
  blocks of efficient self-attention (keys / values from ``LayerNorm(conv(kernel = stride = sr))``) and Mix-FFN (dense, depthwise 3x3, erf-GELU, dense), a
  LayerNorm per stage; the all-MLP head (per-stage linear, bilinear align_corners=False to the stage-1 grid, concat in reversed stage order, bias-free 1x1 fuse,
  BatchNorm in eval mode, ReLU, 1x1 classifier).  Every LayerNorm and the BatchNorm use eps = 1e-5 (torch's defaults);
* ``masks`` / ``seg_reward`` -- argmax over the classes (a tie to the lowest index) and 100 * mean(mask_pred == mask_target).

Checked against the installed transformers / PIL in tests/test_segmentation_reward_oracle.py (through the fixture tools/make_segformer_golden.py writes); needs
neither at run time.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import vit_oracle as vo

SEGFORMER_B4 = dict(hidden_sizes=(64, 128, 320, 512), depths=(3, 8, 27, 3), num_attention_heads=(1, 2, 5, 8), sr_ratios=(8, 4, 2, 1), mlp_ratio=4,
                    decoder_hidden_size=768, num_labels=150, image_size=512)
# the reduced shape of the committed fixture (tools/make_segformer_golden.py); image_size is the processor's size of the case (128 or 160)
REDUCED = dict(depths=(1, 1, 2, 1), decoder_hidden_size=256)
PROCESSOR = dict(rescale_factor=1 / 255, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225))
EPS = 1e-5
BITS = 22


def bilinear_coeffs(in_size, out_size):
    """PIL ImagingResample's taps of one BILINEAR pass: (first input index [out], count [out], fixed-point taps [out][ksize])"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    lo, cnt, kk = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64), np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(n)]
        tot = sum(w)
        for x in range(n):
            k = w[x] / tot if tot != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * (1 << BITS)) if k < 0 else int(0.5 + k * (1 << BITS))
        lo[xx], cnt[xx] = xmin, n
    return lo, cnt, kk


def _pass(img, out_size, axis):
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    lo, cnt, kk = bilinear_coeffs(img.shape[0], out_size)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    for xx in range(out_size):
        acc = np.full(img.shape[1:], 1 << (BITS - 1), np.int64)
        for x in range(cnt[xx]):
            acc += img[lo[xx] + x] * int(kk[xx, x])
        out[xx] = np.clip(acc >> BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def pil_bilinear_resize(img, out_h, out_w):
    """uint8 [H,W,C] -> uint8 [out_h,out_w,C]: horizontal pass, then vertical; a pass whose size does not change is skipped, as PIL does"""
    if img.shape[1] != out_w:
        img = _pass(img, out_w, 1)
    if img.shape[0] != out_h:
        img = _pass(img, out_h, 0)
    return img


def resized_uint8(img_u8, size):
    h, w = img_u8.shape[:2]
    if h != w:
        raise ValueError("only square inputs are restated (and built)")
    return np.ascontiguousarray(pil_bilinear_resize(img_u8, size, size).transpose(2, 0, 1))


def preprocess(images, size):
    """[B,3,H,H] float tensor in [0,1] -> (uint8 [B,3,size,size] numpy, pixel_values [B,3,size,size] fp32 tensor)"""
    u8 = np.stack([resized_uint8(vo.to_uint8_hwc(im), size) for im in images])
    return u8, torch.from_numpy(np.stack([vo.normalize_uint8(c, PROCESSOR) for c in u8]))


def _cfg(cfg):
    c = dict(SEGFORMER_B4)
    c.update(cfg or {})
    return c


def manifest(cfg=None):
    """[(name, shape)] of ``SegformerForSemanticSegmentation(cfg).state_dict()``, in its order"""
    c = _cfg(cfg)
    out = []
    wb = lambda p, shape: [(p + ".weight", tuple(shape)), (p + ".bias", (shape[0],))]
    for i, (C, depth, sr) in enumerate(zip(c["hidden_sizes"], c["depths"], c["sr_ratios"])):
        s, I = f"segformer.stages.{i}", C * c["mlp_ratio"]
        out += wb(s + ".patch_embeddings.proj", (C, 3, 7, 7) if i == 0 else (C, c["hidden_sizes"][i - 1], 3, 3)) + wb(s + ".patch_embeddings.layer_norm", (C,))
        for l in range(depth):
            p = f"{s}.blocks.{l}"
            out += wb(p + ".layernorm_before", (C,))
            for q in ("q_proj", "k_proj", "v_proj", "o_proj"):
                out += wb(f"{p}.attention.{q}", (C, C))
            if sr > 1:
                out += wb(p + ".attention.sequence_reduction.sequence_reduction", (C, C, sr, sr)) + wb(p + ".attention.sequence_reduction.layer_norm", (C,))
            out += wb(p + ".layernorm_after", (C,)) + wb(p + ".mlp.fc1", (I, C)) + wb(p + ".mlp.dwconv.dwconv", (I, 1, 3, 3)) + wb(p + ".mlp.fc2", (C, I))
        out += wb(s + ".layer_norm", (C,))
    Dd = c["decoder_hidden_size"]
    for i, C in enumerate(c["hidden_sizes"]):
        out += wb(f"decode_head.linear_projections.{i}.proj", (Dd, C))
    out += [("decode_head.linear_fuse.weight", (Dd, 4 * Dd, 1, 1))] + wb("decode_head.batch_norm", (Dd,))
    out += [("decode_head.batch_norm.running_mean", (Dd,)), ("decode_head.batch_norm.running_var", (Dd,)), ("decode_head.batch_norm.num_batches_tracked", ())]
    return out + wb("decode_head.classifier", (c["num_labels"], Dd, 1, 1))


def config_flops(cfg=None):
    """multiply-adds x 2 of one image through every matrix product, the attention and the depthwise conv (what cs_seg_flops counts)"""
    c = _cfg(cfg)
    Dd, f = c["decoder_hidden_size"], 0.0
    for i, (C, depth, sr) in enumerate(zip(c["hidden_sizes"], c["depths"], c["sr_ratios"])):
        g = c["image_size"] >> (2 + i)
        R, Nk, I = g * g, (g // sr) ** 2, C * c["mlp_ratio"]
        f += 2.0 * R * (147 if i == 0 else 9 * c["hidden_sizes"][i - 1]) * C
        blk = 2.0 * R * C * C * 2 + 2.0 * Nk * C * 2 * C + 4.0 * R * Nk * C + 4.0 * R * C * I + 18.0 * R * I + (2.0 * Nk * sr * sr * C * C if sr > 1 else 0.0)
        f += depth * blk + 2.0 * R * C * Dd
    R0 = (c["image_size"] // 4) ** 2
    return f + 2.0 * R0 * 4 * Dd * Dd + 2.0 * R0 * Dd * c["num_labels"]


class SegformerOracle:
    """``SegformerForSemanticSegmentation(pixel_values).logits`` in ``dtype`` (fp32: the oracle; bf16: the class comparator)"""

    def __init__(self, sd, cfg=None, dtype=torch.float32):
        self.cfg, self.dtype = _cfg(cfg), dtype
        self.sd = {k: v.detach().to(torch.float32) for k, v in sd.items()}

    def _ln(self, x, p):
        return F.layer_norm(x, (x.shape[-1],), self.sd[p + ".weight"].to(self.dtype), self.sd[p + ".bias"].to(self.dtype), EPS)

    def _lin(self, x, p):
        return F.linear(x, self.sd[p + ".weight"].to(self.dtype), self.sd[p + ".bias"].to(self.dtype))

    def stages(self, pixel_values):
        """the four stage outputs [B, C_i, g_i, g_i]"""
        c, dt = self.cfg, self.dtype
        W = lambda k: self.sd[k].to(dt)
        x = pixel_values.to(dt)
        B = x.shape[0]
        out = []
        for i, (C, depth, heads, sr) in enumerate(zip(c["hidden_sizes"], c["depths"], c["num_attention_heads"], c["sr_ratios"])):
            s = f"segformer.stages.{i}"
            k, st = (7, 4) if i == 0 else (3, 2)
            x = F.conv2d(x, W(s + ".patch_embeddings.proj.weight"), W(s + ".patch_embeddings.proj.bias"), stride=st, padding=k // 2)
            h, w = x.shape[2:]
            x = self._ln(x.flatten(2).transpose(1, 2), s + ".patch_embeddings.layer_norm")
            N = h * w
            for l in range(depth):
                p = f"{s}.blocks.{l}"
                n = self._ln(x, p + ".layernorm_before")
                q = self._lin(n, p + ".attention.q_proj").view(B, N, heads, C // heads).transpose(1, 2)
                kv = n
                if sr > 1:
                    r = p + ".attention.sequence_reduction"
                    kv = F.conv2d(n.transpose(1, 2).reshape(B, C, h, w), W(r + ".sequence_reduction.weight"), W(r + ".sequence_reduction.bias"), stride=sr)
                    kv = self._ln(kv.reshape(B, C, -1).transpose(1, 2), r + ".layer_norm")
                kk = self._lin(kv, p + ".attention.k_proj").view(B, -1, heads, C // heads).transpose(1, 2)
                vv = self._lin(kv, p + ".attention.v_proj").view(B, -1, heads, C // heads).transpose(1, 2)
                a = torch.softmax((q @ kk.transpose(2, 3)) * (C // heads) ** -0.5, -1, dtype=torch.float32).to(dt) @ vv
                x = x + self._lin(a.transpose(1, 2).reshape(B, N, C), p + ".attention.o_proj")
                n = self._lin(self._ln(x, p + ".layernorm_after"), p + ".mlp.fc1")
                I = n.shape[-1]
                n = F.conv2d(n.transpose(1, 2).reshape(B, I, h, w), W(p + ".mlp.dwconv.dwconv.weight"), W(p + ".mlp.dwconv.dwconv.bias"), padding=1, groups=I)
                x = x + self._lin(F.gelu(n.flatten(2).transpose(1, 2)), p + ".mlp.fc2")
            x = self._ln(x, s + ".layer_norm").reshape(B, h, w, C).permute(0, 3, 1, 2).contiguous()
            out.append(x)
        return out

    @torch.no_grad()
    def __call__(self, pixel_values):
        dt = self.dtype
        W = lambda k: self.sd[k].to(dt)
        feats = self.stages(pixel_values)
        size = feats[0].shape[2:]
        ups = []
        for i, f in enumerate(feats):
            B, C, h, w = f.shape
            y = self._lin(f.flatten(2).transpose(1, 2), f"decode_head.linear_projections.{i}.proj").transpose(1, 2).reshape(B, -1, h, w)
            ups.append(F.interpolate(y, size=size, mode="bilinear", align_corners=False))
        y = F.conv2d(torch.cat(ups[::-1], 1), W("decode_head.linear_fuse.weight"))
        b = "decode_head.batch_norm."
        y = F.relu(F.batch_norm(y, W(b + "running_mean"), W(b + "running_var"), W(b + "weight"), W(b + "bias"), False, 0.0, EPS))
        return F.conv2d(y, W("decode_head.classifier.weight"), W("decode_head.classifier.bias"))


def masks(logits):
    """[B,NL,h,w] -> [B,h,w] int64 (on the CPU a tie goes to the lowest class)"""
    return logits.float().argmax(1)


def seg_reward(pred_masks, target_masks):
    """class masks [B,h,w] x2 -> rewards [B,1] fp32: the reference's "dice", the share of equal pixels, times 100"""
    return (pred_masks == target_masks).float().mean((1, 2)).unsqueeze(1) * 100


def top2_margin(logits):
    """[B,NL,h,w] -> [B,h,w]: the gap between the largest and the second largest logit"""
    t = logits.float().topk(2, dim=1).values
    return t[:, 0] - t[:, 1]
