"""Plain-torch fp32 restatement of the Depth Anything depth-PSNR reward for images of ANY aspect ratio: what tests/depth_oracle.py leaves out.  Test
infrastructure, not a fallback.

* ``output_size``       -- the DPT processor's size rule with ``keep_aspect_ratio`` and ``ensure_multiple_of``: ``scale_h = size / H``, ``scale_w = size / W``, the
  scale closer to 1 for both axes, each side ``round(scale * side / multiple) * multiple`` (Python's round: half to even; 105 / 14 = 7.5 -> 8);
* ``resized_uint8`` / ``preprocess`` -- ``ToPILImage`` + PIL's bicubic resize straight to that size, the two axes on independent scales (tests/vit_oracle.py's
  fixed-point passes), rescale 1/255, ImageNet mean / std;
* ``interpolated_positions`` -- transformers' ``Dinov2Embeddings.interpolate_pos_encoding``: the trained [s][s][D] grid through
  ``F.interpolate(mode="bicubic", align_corners=False, size=(gh, gw))`` in fp32, the class row kept; the training grid itself is returned as it is;
* ``DepthAnythingOracleHW`` -- ``DepthAnythingForDepthEstimation`` at any patch grid: tests/depth_oracle.py's graph (which is written over gh x gw already) on a
  state dict whose position table is the interpolated one.

``normalized_maps`` and ``depth_reward`` of tests/depth_oracle.py take any size and are used as they are.  Checked against the installed transformers / PIL in
tests/test_reward_any_aspect_oracle.py (through the fixture tools/make_depth_hw_golden.py writes); needs neither at run time.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import depth_oracle as do
from tests import vit_oracle as vo

normalized_maps, depth_reward = do.normalized_maps, do.depth_reward


def output_size(height, width, size, multiple=14):
    scale_h, scale_w = size / height, size / width
    if abs(1 - scale_w) < abs(1 - scale_h):
        scale_h = scale_w
    else:
        scale_w = scale_h
    return round(scale_h * height / multiple) * multiple, round(scale_w * width / multiple) * multiple


def resized_uint8(img_u8, size):
    """uint8 [H,W,3] -> uint8 [3,out_h,out_w]: the DPT processor's resize"""
    oh, ow = output_size(img_u8.shape[0], img_u8.shape[1], size)
    return np.ascontiguousarray(vo.pil_bicubic_resize(img_u8, oh, ow).transpose(2, 0, 1))


def preprocess(images, size):
    """[B,3,H,W] float tensor in [0,1] -> (uint8 [B,3,out_h,out_w] numpy, pixel_values [B,3,out_h,out_w] fp32 tensor)"""
    u8 = np.stack([resized_uint8(vo.to_uint8_hwc(im), size) for im in images])
    return u8, torch.from_numpy(np.stack([vo.normalize_uint8(c, do.PROCESSOR) for c in u8]))


def interpolated_positions(position_embeddings, gh, gw):
    """[1, 1 + s s, D] -> [1, 1 + gh gw, D] fp32"""
    pos = position_embeddings.detach().to(torch.float32)
    s = int(round((pos.shape[1] - 1) ** 0.5))
    assert s * s == pos.shape[1] - 1
    if (gh, gw) == (s, s):
        return pos
    grid = pos[:, 1:].reshape(1, s, s, -1).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(gh, gw), mode="bicubic", align_corners=False)
    return torch.cat([pos[:, :1], grid.permute(0, 2, 3, 1).reshape(1, gh * gw, -1)], 1)


class DepthAnythingOracleHW:
    """``DepthAnythingForDepthEstimation(pixel_values).predicted_depth`` in ``dtype`` for pixel_values [B,3,h,w], h and w multiples of the patch size"""

    def __init__(self, sd, cfg=None, dtype=torch.float32):
        self.sd, self.cfg, self.dtype = sd, cfg, dtype
        self._by_grid = {}

    def __call__(self, pixel_values):
        P = dict(do.DEPTH_ANYTHING_V2_SMALL, **(self.cfg or {}))["patch_size"]
        grid = (pixel_values.shape[-2] // P, pixel_values.shape[-1] // P)
        if grid not in self._by_grid:
            sd = dict(self.sd)
            sd["backbone.embeddings.position_embeddings"] = interpolated_positions(sd["backbone.embeddings.position_embeddings"], *grid)
            self._by_grid[grid] = do.DepthAnythingOracle(sd, self.cfg, self.dtype)
        return self._by_grid[grid](pixel_values)
