"""Plain-torch fp32 restatement of the Depth Anything depth-PSNR reward (edit_ppo/reward_model.py:92-96, 359-422): test infrastructure, not a fallback.

* ``preprocess``        -- ``ToPILImage`` + the DPT image processor of ``depth-anything/Depth-Anything-V2-Small-hf`` for a SQUARE input: PIL bicubic resize to
  ``size`` x ``size`` (``keep_aspect_ratio`` with ``ensure_multiple_of = 14`` gives exactly that for a square image), rescale 1/255, ImageNet mean / std;
* ``DepthAnythingOracle`` -- ``transformers.DepthAnythingForDepthEstimation``: the DINOv2 backbone with the final LayerNorm applied to the hidden states after
  ``out_indices`` layers, the reassemble stage (1x1 projection, then ConvTranspose 4x4/4, ConvTranspose 2x2/2, identity, 3x3 stride-2 conv), the bias-free 3x3
  neck convs, four fusion layers (pre-activation residual units, bilinear align_corners=True upsample, 1x1 projection), the head (3x3, bilinear to the input
  size, 3x3 + ReLU, 1x1 + ReLU, x max_depth);
* ``normalized_maps``   -- ``post_process_depth_estimation`` (torch bicubic, align_corners=False) to the images' size and (d - min) / (max - min + 1e-8) per map;
* ``depth_reward``      -- 10 log10(1 / (mse + 1e-8)) clamped below at 0.

Checked against the installed transformers / PIL in tests/test_depth_reward_oracle.py (through the fixture tools/make_depth_golden.py writes); needs neither at run time.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import vit_oracle as vo

DEPTH_ANYTHING_V2_SMALL = dict(hidden_size=384, num_hidden_layers=12, num_attention_heads=6, mlp_ratio=4, image_size=518, patch_size=14, layer_norm_eps=1e-6,
                               out_indices=(3, 6, 9, 12), neck_hidden_sizes=(48, 96, 192, 384), fusion_hidden_size=64, head_hidden_size=32, max_depth=1.0)
# the reduced shape of the committed fixture (tools/make_depth_golden.py); image_size is the processor's size of the case (126 or 70)
REDUCED = dict(hidden_size=128, num_hidden_layers=4, num_attention_heads=2, out_indices=(1, 2, 3, 4))
PROCESSOR = dict(rescale_factor=1 / 255, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225))


def resized_uint8(img_u8, size):
    """uint8 [H,H,3] -> uint8 [3,size,size]: the DPT processor's resize of a square image"""
    h, w = img_u8.shape[:2]
    if h != w:
        raise ValueError("only square inputs are restated (and built)")
    return np.ascontiguousarray(vo.pil_bicubic_resize(img_u8, size, size).transpose(2, 0, 1))


def preprocess(images, size):
    """[B,3,H,H] float tensor in [0,1] -> (uint8 [B,3,size,size] numpy, pixel_values [B,3,size,size] fp32 tensor)"""
    u8 = np.stack([resized_uint8(vo.to_uint8_hwc(im), size) for im in images])
    return u8, torch.from_numpy(np.stack([vo.normalize_uint8(c, PROCESSOR) for c in u8]))


def manifest(cfg=None):
    """[(name, shape)] of ``DepthAnythingForDepthEstimation(cfg).state_dict()``, in its order"""
    c = dict(DEPTH_ANYTHING_V2_SMALL)
    c.update(cfg or {})
    D, Fh, Hh = c["hidden_size"], c["fusion_hidden_size"], c["head_hidden_size"]
    out = [("backbone." + n, s) for n, s in vo.dinov2_manifest({k: c[k] for k in vo.DINOV2_BASE})]
    for i, (C, k) in enumerate(zip(c["neck_hidden_sizes"], (4, 2, 0, 3))):
        p = f"neck.reassemble_stage.layers.{i}"
        out += [(f"{p}.projection.weight", (C, D, 1, 1)), (f"{p}.projection.bias", (C,))]
        if k:
            out += [(f"{p}.resize.weight", (C, C, k, k)), (f"{p}.resize.bias", (C,))]
    out += [(f"neck.convs.{i}.weight", (Fh, C, 3, 3)) for i, C in enumerate(c["neck_hidden_sizes"])]
    for i in range(4):
        p = f"neck.fusion_stage.layers.{i}"
        out += [(f"{p}.projection.weight", (Fh, Fh, 1, 1)), (f"{p}.projection.bias", (Fh,))]
        for r in ("residual_layer1", "residual_layer2"):
            for q in ("convolution1", "convolution2"):
                out += [(f"{p}.{r}.{q}.weight", (Fh, Fh, 3, 3)), (f"{p}.{r}.{q}.bias", (Fh,))]
    out += [("head.conv1.weight", (Fh // 2, Fh, 3, 3)), ("head.conv1.bias", (Fh // 2,)), ("head.conv2.weight", (Hh, Fh // 2, 3, 3)), ("head.conv2.bias", (Hh,)),
            ("head.conv3.weight", (1, Hh, 1, 1)), ("head.conv3.bias", (1,))]
    return out


class DepthAnythingOracle:
    """``DepthAnythingForDepthEstimation(pixel_values).predicted_depth`` in ``dtype`` (fp32: the oracle; bf16: the class comparator)"""

    def __init__(self, sd, cfg=None, dtype=torch.float32):
        c = dict(DEPTH_ANYTHING_V2_SMALL)
        c.update(cfg or {})
        self.cfg, self.dtype = c, dtype
        self.sd = {k: v.detach().to(torch.float32) for k, v in sd.items()}

    def taps(self, pixel_values):
        """the backbone's feature maps: the hidden states after ``out_indices`` layers, final LayerNorm applied, CLS row included"""
        c, sd, dt = self.cfg, self.sd, self.dtype
        W = lambda k: sd["backbone." + k].to(dt)
        D, H, P, eps = c["hidden_size"], c["num_attention_heads"], c["patch_size"], c["layer_norm_eps"]
        x = pixel_values.to(dt)
        B = x.shape[0]
        x = F.conv2d(x, W("embeddings.patch_embeddings.projection.weight"), W("embeddings.patch_embeddings.projection.bias"), stride=P)
        x = x.flatten(2).transpose(1, 2)
        pos = W("embeddings.position_embeddings")
        assert pos.shape[1] == x.shape[1] + 1, "the position table is used as it is: the input grid must be the training grid"
        x = torch.cat([W("embeddings.cls_token").expand(B, -1, -1), x], 1) + pos
        N = x.shape[1]
        out = []
        for l in range(max(c["out_indices"])):
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
            if l + 1 in c["out_indices"]:
                out.append(F.layer_norm(x, (D,), W("layernorm.weight"), W("layernorm.bias"), eps))
        return out

    def _rcu(self, x, p):
        W = lambda k: self.sd[k].to(self.dtype)
        h = F.conv2d(F.relu(x), W(f"{p}.convolution1.weight"), W(f"{p}.convolution1.bias"), padding=1)
        h = F.conv2d(F.relu(h), W(f"{p}.convolution2.weight"), W(f"{p}.convolution2.bias"), padding=1)
        return h + x

    @torch.no_grad()
    def __call__(self, pixel_values):
        c, dt = self.cfg, self.dtype
        W = lambda k: self.sd[k].to(dt)
        B, _, h, w = pixel_values.shape
        gh, gw = h // c["patch_size"], w // c["patch_size"]
        feats = []
        for i, t in enumerate(self.taps(pixel_values)):
            p = f"neck.reassemble_stage.layers.{i}"
            x = t[:, 1:].reshape(B, gh, gw, -1).permute(0, 3, 1, 2)
            x = F.conv2d(x, W(f"{p}.projection.weight"), W(f"{p}.projection.bias"))
            if i == 0:
                x = F.conv_transpose2d(x, W(f"{p}.resize.weight"), W(f"{p}.resize.bias"), stride=4)
            elif i == 1:
                x = F.conv_transpose2d(x, W(f"{p}.resize.weight"), W(f"{p}.resize.bias"), stride=2)
            elif i == 3:
                x = F.conv2d(x, W(f"{p}.resize.weight"), W(f"{p}.resize.bias"), stride=2, padding=1)
            feats.append(F.conv2d(x, W(f"neck.convs.{i}.weight"), None, padding=1))
        feats = feats[::-1]
        fused = None
        for l, f in enumerate(feats):
            p = f"neck.fusion_stage.layers.{l}"
            x = f if fused is None else fused + self._rcu(f, f"{p}.residual_layer1")
            x = self._rcu(x, f"{p}.residual_layer2")
            if l + 1 < len(feats):
                x = F.interpolate(x, size=feats[l + 1].shape[2:], mode="bilinear", align_corners=True)
            else:
                x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
            fused = F.conv2d(x, W(f"{p}.projection.weight"), W(f"{p}.projection.bias"))
        x = F.conv2d(fused, W("head.conv1.weight"), W("head.conv1.bias"), padding=1)
        x = F.interpolate(x, (gh * c["patch_size"], gw * c["patch_size"]), mode="bilinear", align_corners=True)
        x = F.relu(F.conv2d(x, W("head.conv2.weight"), W("head.conv2.bias"), padding=1))
        x = F.relu(F.conv2d(x, W("head.conv3.weight"), W("head.conv3.bias"))) * c["max_depth"]
        return x[:, 0]


def normalized_maps(predicted_depth, height, width):
    """[B,S,S] -> [B,height,width] fp32: post_process_depth_estimation per image, then the reward's min / max normalisation"""
    d = F.interpolate(predicted_depth.float()[:, None], size=(height, width), mode="bicubic", align_corners=False)[:, 0]
    mn, mx = d.amin((1, 2), keepdim=True), d.amax((1, 2), keepdim=True)
    return (d - mn) / (mx - mn + 1e-8)


def depth_reward(pred_maps, target_maps):
    """normalised maps [B,H,W] x2 -> rewards [B,1] fp32"""
    mse = ((pred_maps.float() - target_maps.float()) ** 2).mean((1, 2))
    return torch.clamp(10 * torch.log10(1.0 / (mse + 1e-8)), min=0).unsqueeze(1)
