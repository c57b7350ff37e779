"""Plain-torch restatement of the Inception-v3 logit-cosine reward (edit_ppo/reward_model.py:98-108, 319-356): test infrastructure, not a fallback.

* ``preprocess``        -- ``ToPILImage`` + torchvision's ``Resize(size, BICUBIC)`` (shortest edge -> size, long side int(size * long / short); PIL's fixed-point
  bicubic, restated in tests/vit_oracle.py) + ``CenterCrop(size)`` (window at ``int(round((n - size) / 2.0))``: Python's round half to even) + ``ToTensor``
  + ``Normalize`` with the ImageNet mean / std;
* ``InceptionOracle``   -- torchvision ``inception_v3(aux_logits=True, transform_input=False).eval()``, evaluated in float64 on the fp32 weights by default
  (see the class): the wiring is restated here (``walk``), the building blocks are ``F.conv2d`` / ``F.batch_norm`` (eps 1e-3) / ``F.max_pool2d`` / ``F.avg_pool2d`` / ``F.linear`` themselves.  AuxLogits is never evaluated and
  dropout is the identity in eval mode.  The output is the [B, 1000] logits of ``fc``;
* ``inception_reward``  -- (F.cosine_similarity(pred_logits, target_logits) + 1) * 50;
* ``calibrate_batch_norm`` -- sets every BatchNorm's running statistics to the batch statistics of the given images (one forward pass in training-mode
  normalisation).  With the plain synthetic recipe (running_var in [0.5, 1.5]) 94 ReLU layers build up a constant component that the statistics do not
  remove and the logits barely depend on the image: the reward of ANY pair is above 99.9, so a reward test on such weights passes with broken wiring.

torchvision is not installed and there are no checkpoint weights: the wiring is pinned by the published parameter counts (23,834,568 without AuxLogits,
27,161,264 with it) in tests/test_inception_reward_oracle.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import vit_oracle as vo

PROCESSOR = dict(rescale_factor=1 / 255, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225))
BN_EPS = 1e-3
AUX_PARAMS = 3_326_696          # AuxLogits: conv0 768 -> 128 1x1, conv1 128 -> 768 5x5 (each + BatchNorm), fc 768 -> 1000


def walk(ops, x):
    """torchvision Inception3._forward up to the last Mixed block, over an ``ops`` object: conv(name, x, cout, (kh, kw), stride, (ph, pw)), maxpool(x),
    avgpool(x), cat([...])"""
    c = ops.conv

    def a(x, p, pf):
        b1 = c(p + ".branch1x1", x, 64, (1, 1), 1, (0, 0))
        b5 = c(p + ".branch5x5_2", c(p + ".branch5x5_1", x, 48, (1, 1), 1, (0, 0)), 64, (5, 5), 1, (2, 2))
        b3 = c(p + ".branch3x3dbl_1", x, 64, (1, 1), 1, (0, 0))
        b3 = c(p + ".branch3x3dbl_3", c(p + ".branch3x3dbl_2", b3, 96, (3, 3), 1, (1, 1)), 96, (3, 3), 1, (1, 1))
        bp = c(p + ".branch_pool", ops.avgpool(x), pf, (1, 1), 1, (0, 0))
        return ops.cat([b1, b5, b3, bp])

    def b(x, p):
        b3 = c(p + ".branch3x3", x, 384, (3, 3), 2, (0, 0))
        bd = c(p + ".branch3x3dbl_2", c(p + ".branch3x3dbl_1", x, 64, (1, 1), 1, (0, 0)), 96, (3, 3), 1, (1, 1))
        bd = c(p + ".branch3x3dbl_3", bd, 96, (3, 3), 2, (0, 0))
        return ops.cat([b3, bd, ops.maxpool(x)])

    def cc(x, p, c7):
        b1 = c(p + ".branch1x1", x, 192, (1, 1), 1, (0, 0))
        b7 = c(p + ".branch7x7_1", x, c7, (1, 1), 1, (0, 0))
        b7 = c(p + ".branch7x7_2", b7, c7, (1, 7), 1, (0, 3))
        b7 = c(p + ".branch7x7_3", b7, 192, (7, 1), 1, (3, 0))
        bd = c(p + ".branch7x7dbl_1", x, c7, (1, 1), 1, (0, 0))
        bd = c(p + ".branch7x7dbl_2", bd, c7, (7, 1), 1, (3, 0))
        bd = c(p + ".branch7x7dbl_3", bd, c7, (1, 7), 1, (0, 3))
        bd = c(p + ".branch7x7dbl_4", bd, c7, (7, 1), 1, (3, 0))
        bd = c(p + ".branch7x7dbl_5", bd, 192, (1, 7), 1, (0, 3))
        bp = c(p + ".branch_pool", ops.avgpool(x), 192, (1, 1), 1, (0, 0))
        return ops.cat([b1, b7, bd, bp])

    def d(x, p):
        b3 = c(p + ".branch3x3_2", c(p + ".branch3x3_1", x, 192, (1, 1), 1, (0, 0)), 320, (3, 3), 2, (0, 0))
        b7 = c(p + ".branch7x7x3_1", x, 192, (1, 1), 1, (0, 0))
        b7 = c(p + ".branch7x7x3_2", b7, 192, (1, 7), 1, (0, 3))
        b7 = c(p + ".branch7x7x3_3", b7, 192, (7, 1), 1, (3, 0))
        b7 = c(p + ".branch7x7x3_4", b7, 192, (3, 3), 2, (0, 0))
        return ops.cat([b3, b7, ops.maxpool(x)])

    def e(x, p):
        b1 = c(p + ".branch1x1", x, 320, (1, 1), 1, (0, 0))
        b3 = c(p + ".branch3x3_1", x, 384, (1, 1), 1, (0, 0))
        b3 = ops.cat([c(p + ".branch3x3_2a", b3, 384, (1, 3), 1, (0, 1)), c(p + ".branch3x3_2b", b3, 384, (3, 1), 1, (1, 0))])
        bd = c(p + ".branch3x3dbl_2", c(p + ".branch3x3dbl_1", x, 448, (1, 1), 1, (0, 0)), 384, (3, 3), 1, (1, 1))
        bd = ops.cat([c(p + ".branch3x3dbl_3a", bd, 384, (1, 3), 1, (0, 1)), c(p + ".branch3x3dbl_3b", bd, 384, (3, 1), 1, (1, 0))])
        bp = c(p + ".branch_pool", ops.avgpool(x), 192, (1, 1), 1, (0, 0))
        return ops.cat([b1, b3, bd, bp])

    x = c("Conv2d_1a_3x3", x, 32, (3, 3), 2, (0, 0))
    x = c("Conv2d_2a_3x3", x, 32, (3, 3), 1, (0, 0))
    x = c("Conv2d_2b_3x3", x, 64, (3, 3), 1, (1, 1))
    x = ops.maxpool(x)
    x = c("Conv2d_3b_1x1", x, 80, (1, 1), 1, (0, 0))
    x = c("Conv2d_4a_3x3", x, 192, (3, 3), 1, (0, 0))
    x = ops.maxpool(x)
    x = a(x, "Mixed_5b", 32)
    x = a(x, "Mixed_5c", 64)
    x = a(x, "Mixed_5d", 64)
    x = b(x, "Mixed_6a")
    x = cc(x, "Mixed_6b", 128)
    x = cc(x, "Mixed_6c", 160)
    x = cc(x, "Mixed_6d", 160)
    x = cc(x, "Mixed_6e", 192)
    x = d(x, "Mixed_7a")
    x = e(x, "Mixed_7b")
    return e(x, "Mixed_7c")


class _Tracer:
    """shapes only: x is (C, H, W); collects the manifest and the multiply-adds"""

    def __init__(self):
        self.tensors, self.macs = [], 0

    def conv(self, name, x, cout, k, stride, pad):
        cin, h, w = x
        ho, wo = (h + 2 * pad[0] - k[0]) // stride + 1, (w + 2 * pad[1] - k[1]) // stride + 1
        self.tensors.append((name + ".conv.weight", (cout, cin, k[0], k[1])))
        self.tensors += [(name + ".bn." + q, (cout,)) for q in ("weight", "bias", "running_mean", "running_var")]
        self.tensors.append((name + ".bn.num_batches_tracked", ()))
        self.macs += ho * wo * cout * cin * k[0] * k[1]
        return (cout, ho, wo)

    def maxpool(self, x):
        return (x[0], (x[1] - 3) // 2 + 1, (x[2] - 3) // 2 + 1)

    def avgpool(self, x):
        return x

    def cat(self, xs):
        return (sum(x[0] for x in xs),) + xs[0][1:]


def _trace(size, num_classes=1000):
    t = _Tracer()
    c, h, w = walk(t, (3, size, size))
    assert c == 2048 and h >= 1 and w >= 1
    t.tensors += [("fc.weight", (num_classes, 2048)), ("fc.bias", (num_classes,))]
    t.macs += 2048 * num_classes
    return t


def manifest(num_classes=1000):
    """[(name, shape)] in torchvision's state-dict order, without AuxLogits (never evaluated): 94 BasicConv2d x 6 + fc = 566 entries"""
    return _trace(299, num_classes).tensors


def param_count(num_classes=1000):
    """trainable parameters of the evaluated network (no BatchNorm buffers): 23,834,568; with AUX_PARAMS torchvision's published 27,161,264"""
    return sum(int(np.prod(s)) for k, s in manifest(num_classes) if "running_" not in k and "num_batches" not in k)


def config_flops(size=299, num_classes=1000):
    """2 x multiply-adds of the convolutions and fc, per image"""
    return 2.0 * _trace(size, num_classes).macs


def crop_offset(n, size):
    """torchvision CenterCrop: int(round((n - size) / 2.0)), Python's round half to even"""
    return int(round((n - size) / 2.0))


def crop_uint8(img_u8, size):
    """uint8 [H,W,3] -> resized, center-cropped uint8 [3, size, size]"""
    h, w = img_u8.shape[:2]
    nh, nw = vo.resize_output_size(h, w, size)
    if nh < size or nw < size:
        raise ValueError("the resized image is smaller than the crop (CenterCrop would pad)")
    r = vo.pil_bicubic_resize(img_u8, nh, nw)
    top, left = crop_offset(nh, size), crop_offset(nw, size)
    return np.ascontiguousarray(r[top:top + size, left:left + size].transpose(2, 0, 1))


def normalize_uint8(crop_u8):
    """uint8 [3,h,w] -> fp32 pixel_values: ToTensor (uint8 / 255 in fp32), then (x - mean) / std in fp32"""
    x = torch.from_numpy(crop_u8).to(torch.float32).div(255)
    mean = torch.tensor(PROCESSOR["image_mean"], dtype=torch.float32)[:, None, None]
    std = torch.tensor(PROCESSOR["image_std"], dtype=torch.float32)[:, None, None]
    return (x - mean) / std


def preprocess(images, size=299):
    """[B,3,H,W] float tensor in [0,1] -> (uint8 crops [B,3,size,size] numpy, pixel_values [B,3,size,size] fp32 tensor)"""
    crops = np.stack([crop_uint8(vo.to_uint8_hwc(im), size) for im in images])
    return crops, torch.stack([normalize_uint8(c) for c in crops])


class InceptionOracle:
    """``dtype``: the arithmetic of the evaluation.  The default is float64 (weights and inputs are the fp32 values, exactly): the calibrated random network
    amplifies a perturbation so much that an fp32 evaluation changes by 4e-5 with the host's thread count (another summation order); the float64 one gives
    the same fp32 figures everywhere.  Against the fp16 path's 1e-2 the difference between the two is nothing.  bfloat16: the comparator of the GPU tests."""

    def __init__(self, sd, dtype=torch.float64):
        self.dtype = dtype
        self.sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items() if not k.startswith("AuxLogits.")}

    def bn(self, name, y):
        sd = self.sd
        return F.batch_norm(y, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"], sd[name + ".bn.bias"], False, 0.0, BN_EPS)

    def conv(self, name, x, cout, k, stride, pad):
        w = self.sd[name + ".conv.weight"]
        assert tuple(w.shape) == (cout, x.shape[1], k[0], k[1]), name
        return F.relu(self.bn(name, F.conv2d(x, w, None, stride, pad)))

    def maxpool(self, x):
        return F.max_pool2d(x, 3, 2)

    def avgpool(self, x):
        return F.avg_pool2d(x, 3, 1, 1)

    def cat(self, xs):
        return torch.cat(xs, 1)

    @torch.no_grad()
    def __call__(self, pixel_values):
        """pixel_values [B,3,size,size] -> the logits of fc [B, num_classes] in fp32"""
        x = walk(self, pixel_values.to(self.dtype))
        x = F.adaptive_avg_pool2d(x, 1).flatten(1)
        return F.linear(x, self.sd["fc.weight"], self.sd["fc.bias"]).float()


class _Calibrator(InceptionOracle):
    def bn(self, name, y):
        var, mean = torch.var_mean(y, dim=(0, 2, 3), unbiased=False)
        mean, var = mean.float(), var.float().clamp_min(1e-6)          # what the state dict stores; the pass goes on with exactly these
        self.sd[name + ".bn.running_mean"], self.sd[name + ".bn.running_var"] = mean.double(), var.double()
        return super().bn(name, y)


@torch.no_grad()
def calibrate_batch_norm(sd, pixel_values):
    """-> a copy of ``sd`` whose BatchNorm running statistics are the batch statistics of ``pixel_values`` [N,3,size,size], layer by layer in one pass"""
    c = _Calibrator(sd)
    walk(c, pixel_values.double())
    out = dict(sd)
    out.update({k: v.float() for k, v in c.sd.items() if "running_" in k})
    return out


def calibration_images(size, n=16, seed=77):
    """n varied synthetic images [n,3,size,size] in [0,1]: smooth random fields, flipped, rolled and with noise of growing amplitude"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        low = torch.rand(1, 3, 4 + i % 5, 5 + i % 3, generator=g)
        im = F.interpolate(low, size=(size, size), mode="bicubic", align_corners=False)[0]
        if i % 2:
            im = im.flip(2)
        if i % 3 == 0:
            im = im.roll(size // 3, 1)
        im = im + (0.02 + 0.03 * i) * torch.randn(3, size, size, generator=g)
        out.append(im.clamp(0, 1))
    return torch.stack(out)


def inception_reward(pred_logits, target_logits):
    """[B,N] x ([B,N] or [1,N]) -> [B,1] fp32"""
    return ((F.cosine_similarity(pred_logits.float(), target_logits.float(), dim=1) + 1) * 50).unsqueeze(1)
