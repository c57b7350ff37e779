"""DINOv2 and CLIP image-similarity rewards and the Depth Anything depth-PSNR reward on the HIP library (``--reward_type="dino"``, edit_ppo/run_ppo.sh:30; ``"clip"``, compute_reward.sh:5).

Mirror of edit_ppo/reward_model.py by name:

* ``load_reward_model("dino")`` (:25-57, :59-64) -> ``(model, processor)``: a ``HipDinov2Model`` of the ``facebook/dinov2-base`` shape and a
  ``DinoImageProcessor`` holding that checkpoint's published preprocessing constants.  No hub access: weights are loaded by the caller with
  ``model.load_state_dict`` under their ``transformers.Dinov2Model`` names.
* ``calculate_dino_reward(reward_model, reward_model_processor, model_pred, target, device)`` (:217-257) -> rewards ``[B,1]`` fp32 in [0, 100].

What the reference does per image on the host -- ``ToPILImage`` (``x.mul(255).byte()``: product in the tensor's dtype, truncation), PIL's fixed-point
bicubic resize to shortest edge 256, center crop 224, rescale, normalise -- runs here as two HIP kernels on the whole batch, bit-identical on the uint8
image; the encoder runs in fp16 with fp32 accumulation (cs_vit_forward) and returns the CLS features in fp32; the tail (normalize, cosine, (cos + 1) * 50)
is one kernel.  Inputs are clamped to [0, 1] unconditionally (the reference clamps when ``min < 0``; ``decode_latents`` never leaves [0, 1]).
There is no CPU fallback; the fp32 restatement lives in tests/vit_oracle.py.

``clip`` has the same shape (:128-134, :512-552): ``load_reward_model("clip")`` -> a ``HipCLIPVisionModel`` of the ``openai/clip-vit-large-patch14`` vision
tower + ``visual_projection`` and a ``ClipImageProcessor``; ``calculate_clip_reward`` runs the same front end with CLIP's constants (shortest edge 224), the
tower (cs_clipv_forward: embeddings + pre_layrnorm in one kernel, the shared pre-LN layer loop with quick-GELU, post_layernorm + projection in one kernel)
and the same tail on ``image_embeds``.  Weights load under their ``transformers.CLIPModel`` names (a full CLIPModel state dict or a
CLIPVisionModelWithProjection one).  The fp32 restatement lives in tests/clip_vision_oracle.py.

``depth`` (:92-96, :359-422; the reward the reference trains with by default): ``load_depth_reward()`` -> a ``HipDepthAnythingModel`` of the
``depth-anything/Depth-Anything-V2-Small-hf`` shape and a ``DepthImageProcessor``; ``calculate_depth_reward`` runs the front end (PIL bicubic resize to the
DPT processor's size for the image's aspect ratio -- 518 x 518 for a square, 518 x 700 for 880 x 1184 --, bit-identical on the uint8 image), the DINOv2-small backbone tapped at four depths, the DPT neck and head (cs_depth_forward),
torch's bicubic resize back to the images' size with the per-map min / max normalisation (cs_depth_normalized_maps) and the PSNR tail
(``ppo.depth_psnr_tail``).  Weights load under their ``transformers.DepthAnythingForDepthEstimation`` names.  The fp32 restatement lives in
tests/depth_oracle.py.

``segmentation`` (:110-117, :425-481): ``load_segmentation_reward()`` -> a ``HipSegformerModel`` of the ``nvidia/segformer-b4-finetuned-ade-512-512`` shape
and a ``SegImageProcessor``; ``calculate_segmentation_reward`` runs the front end (PIL BILINEAR resize of the image, whatever its aspect ratio, to 512 x 512,
bit-identical on the uint8 image), the MiT-B4 encoder and the all-MLP head (cs_seg_forward), the class argmax at a quarter of the processor's size (cs_seg_masks) and the
agreement tail 100 * mean(mask_pred == mask_target) (cs_seg_agreement).  Weights load under their ``transformers.SegformerForSemanticSegmentation`` names.
The fp32 restatement lives in tests/segformer_oracle.py.

``inception`` (:98-108, :319-356): ``load_inception_reward()`` -> a ``HipInceptionV3`` (torchvision ``inception_v3`` in eval mode; AuxLogits is never
evaluated) and an ``InceptionImageProcessor``; ``calculate_inception_reward`` runs the front end (torchvision's ``Resize(299, BICUBIC)`` +
``CenterCrop(299)`` with its round-half-even offset, any aspect ratio, bit-identical on the uint8 image), the 94 BatchNorm-folded convolutions on one
implicit-GEMM MFMA kernel with the pools and the fp32 head (cs_incep_forward) and the cosine tail on the [B,1000] logits of ``fc``.  Weights load under
their torchvision names.  The fp32 restatement lives in tests/inception_oracle.py.
"""
import ctypes as C

import torch

from . import _lib as L

DINOV2_BASE_CONFIG = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, mlp_ratio=4, image_size=518, patch_size=14,
                          layer_norm_eps=1e-6)
CLIP_VIT_L14_CONFIG = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
                           projection_dim=768, layer_norm_eps=1e-5)
# depth-anything/Depth-Anything-V2-Small-hf (its config.json, from memory: no hub access here): a DINOv2-small backbone tapped after ``out_indices`` layers
# (the final LayerNorm applied to every tap), the DPT neck and head.  ``out_indices`` is a config key: a checkpoint with other taps passes its own.
DEPTH_ANYTHING_V2_SMALL_CONFIG = dict(hidden_size=384, num_hidden_layers=12, num_attention_heads=6, mlp_ratio=4, image_size=518, patch_size=14,
                                      layer_norm_eps=1e-6, out_indices=(3, 6, 9, 12), neck_hidden_sizes=(48, 96, 192, 384), fusion_hidden_size=64,
                                      head_hidden_size=32, max_depth=1.0)
# nvidia/segformer-b4-finetuned-ade-512-512 (its config.json, from memory: no hub access here): MiT-B4 + the all-MLP head over the 150 ADE20K classes
SEGFORMER_B4_ADE_CONFIG = dict(hidden_sizes=(64, 128, 320, 512), depths=(3, 8, 27, 3), num_attention_heads=(1, 2, 5, 8), sr_ratios=(8, 4, 2, 1), mlp_ratio=4,
                               decoder_hidden_size=768, num_labels=150, image_size=512)
# torchvision inception_v3 (the widths are the architecture's); image_size is the reference's Resize / CenterCrop edge
INCEPTION_V3_CONFIG = dict(image_size=299, num_classes=1000)
_DT = {torch.float32: L.CS_F32, torch.float16: L.CS_F16}


class DinoImageProcessor:
    """The preprocessing constants of ``facebook/dinov2-base`` (its preprocessor_config.json): resize to shortest edge 256 with PIL BICUBIC, center crop
    224, rescale 1/255, normalise with the ImageNet mean / std.  A plain holder: the arithmetic runs in ``HipDinov2Model.preprocess``."""
    do_resize = do_center_crop = do_rescale = do_normalize = True
    resample = 3                                   # PIL.Image.BICUBIC

    def __init__(self, size=None, crop_size=None, rescale_factor=1 / 255, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225)):
        self.size = dict(size or {"shortest_edge": 256})
        self.crop_size = dict(crop_size or {"height": 224, "width": 224})
        if set(self.size) != {"shortest_edge"} or self.crop_size["height"] != self.crop_size["width"]:
            raise ValueError("the HIP front end implements the shortest-edge resize and a square center crop")
        self.rescale_factor, self.image_mean, self.image_std = float(rescale_factor), tuple(image_mean), tuple(image_std)

    def constants(self):
        return (self.size["shortest_edge"], self.crop_size["height"], self.rescale_factor, self.image_mean, self.image_std)


class _VitOutput(tuple):
    """(last_hidden_state, pooler_output).  Only the CLS row is materialised: ``last_hidden_state`` is ``[B, 1, hidden]`` so that the reference's
    ``outputs.last_hidden_state[:, 0, :]`` reads the CLS features; ``pooler_output`` is the same ``[B, hidden]`` tensor (as in transformers)."""
    last_hidden_state = property(lambda self: self[0])
    pooler_output = property(lambda self: self[1])


class _HipImageModel:
    """What the image-reward models share (csrc/image_tower.h on the C side): a handle of the C ABI family ``cs_<_prefix>_*`` (create / weights / preprocess /
    forward), the front end, and the chunked forward call.  Subclasses create the handle from their config struct."""
    is_consolver_hip = True
    dtype = torch.float16
    max_batch = 64             # images per encoder call (bounds the workspace)
    _prefix = None

    def _init_handle(self, h, crop, patch):
        self._h = h
        self._ws = None
        self._pws = None
        self._finalized = False
        self.crop, self.patch = crop, patch
        self.patch_cols, self.num_tokens = int(self._fn("patch_cols")(h)), int(self._fn("num_tokens")(h))

    def _fn(self, name):
        return getattr(L.lib(), f"cs_{self._prefix}_{name}")

    def __del__(self):
        try:
            L.destroy(self._prefix, self)
        except Exception:          # interpreter shutdown: the module's globals may be gone
            pass

    # reference call sites: reward_model.eval(); reward_model.to(device)
    def eval(self):
        return self

    def to(self, device=None, *args, **kwargs):
        if device is not None:
            d = torch.device(device)
            if d.type == "cuda" and d.index is None:
                d = torch.device("cuda", self.device.index if self.device.type == "cuda" else torch.cuda.current_device())
            if d != self.device:
                raise RuntimeError(f"{type(self).__name__} lives on {self.device} (its weights are packed there); cannot move it to {d}")
        return self

    def manifest(self):
        return L.manifest(self._prefix, self._h)

    def load_state_dict(self, sd, strict=True):
        L.load_float_weights(self._prefix, self._h, sd, self.device)
        self._finalized = True
        return self

    def flops(self, batch):
        return float(self._fn("flops")(self._h, batch))

    # ---- front end ------------------------------------------------------------------------------------------------
    def preprocess(self, images, return_crop=False):
        """[B,3,H,W] fp16 / fp32 in [0,1] -> patch rows [B * (crop/patch)^2, patch_cols] fp16 (the encoder's input) and, with ``return_crop``, the resized
        and center-cropped uint8 image [B,3,crop,crop] (what PIL hands the processor's rescale)."""
        L.require_cuda(images, "images")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"images must be [B,3,H,W], got {tuple(images.shape)}")
        if images.dtype not in _DT:
            # ToPILImage multiplies in the tensor's own dtype: a bf16 / fp64 image quantises differently from its fp32 copy, so no silent conversion
            raise TypeError(f"images must be float16 or float32 (the two quantisation paths that are built), got {images.dtype}")
        images = images.contiguous()
        B, _, H, W = images.shape
        g = self.crop // self.patch
        patches = torch.empty(B * g * g, self.patch_cols, dtype=torch.float16, device=images.device)
        crop = torch.empty(B, 3, self.crop, self.crop, dtype=torch.uint8, device=images.device) if return_crop else None
        if B:
            need = int(self._fn("preprocess_workspace_bytes")(self._h, B, H, W))
            if self._pws is None or self._pws.numel() < need or self._pws.device != images.device:
                self._pws = torch.empty(need, dtype=torch.uint8, device=images.device)
            with torch.cuda.device(images.device):          # the resize tables of a new image size are allocated on the current device
                L.check(self._fn("preprocess")(self._h, L.ptr(images), _DT[images.dtype], B, H, W, L.ptr(patches), L.ptr(crop), L.ptr(self._pws),
                                                self._pws.numel(), L.stream_ptr(images.device)))
        return (patches, crop) if return_crop else patches

    def patches_to_pixel_values(self, patches):
        """the patch rows back in the processor's layout: ``pixel_values`` [B,3,crop,crop] fp16"""
        g, P = self.crop // self.patch, self.patch
        B = patches.shape[0] // (g * g)
        return patches[:, :3 * P * P].reshape(B, g, g, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, g * P, g * P)

    def pixel_values_to_patches(self, pixel_values):
        g, P = self.crop // self.patch, self.patch
        B = pixel_values.shape[0]
        if tuple(pixel_values.shape[1:]) != (3, g * P, g * P):
            raise ValueError(f"pixel_values must be [B,3,{g * P},{g * P}] (the processor's crop), got {tuple(pixel_values.shape)}")
        rows = pixel_values.to(torch.float16).reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * P * P)
        out = rows.new_zeros(B * g * g, self.patch_cols)
        out[:, :3 * P * P] = rows
        return out

    # ---- model --------------------------------------------------------------------------------------------------
    def _forward(self, patches, *out_shape):
        """patch rows -> cs_<_prefix>_forward's fp32 output [B, *out_shape], ``max_batch`` images per call"""
        if not self._finalized:
            raise RuntimeError("weights not loaded")
        L.require_cuda(patches, "patches")
        g = self.crop // self.patch
        B = patches.shape[0] // (g * g)
        out = torch.empty(B, *out_shape, dtype=torch.float32, device=patches.device)
        for s in range(0, B, self.max_batch):
            n = min(self.max_batch, B - s)
            need = int(self._fn("workspace_bytes")(self._h, n))
            if self._ws is None or self._ws.numel() < need or self._ws.device != patches.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=patches.device)
            L.check(self._fn("forward")(self._h, L.ptr(patches[s * g * g:]), n, L.ptr(out[s:]), L.ptr(self._ws), self._ws.numel(),
                                        L.stream_ptr(patches.device)))
        return out


class _HipImageEncoder(_HipImageModel):
    """The models whose forward gives one feature vector per image; subclasses name its width (``_feature_dim``)."""

    def encode_patches(self, patches):
        """patch rows -> features [B, _feature_dim] fp32 (dino: ``last_hidden_state[:, 0]`` after the final LayerNorm; clip: ``image_embeds``)"""
        return self._forward(patches, self._feature_dim)

    def image_features(self, images):
        """[B,3,H,W] in [0,1] -> features [B, _feature_dim] fp32: the whole per-image path of the reward up to F.normalize"""
        return self.encode_patches(self.preprocess(images))


class HipDinov2Model(_HipImageEncoder):
    max_batch = 64             # 7.6 MB of workspace per image at the base size
    _prefix = "vit"

    def __init__(self, config=None, device="cuda:0", processor=None):
        cfg = dict(DINOV2_BASE_CONFIG)
        cfg.update(config or {})
        self.config = cfg
        self.device = torch.device(device)
        self.processor = processor or DinoImageProcessor()
        edge, crop, rescale, mean, std = self.processor.constants()
        c = L.CsVitConfig(cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["mlp_ratio"], cfg["image_size"], cfg["patch_size"],
                          cfg["layer_norm_eps"], edge, crop, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), rescale)
        h = C.c_void_p()
        L.check(L.lib().cs_vit_create(C.byref(c), C.byref(h)))
        self._init_handle(h, crop, cfg["patch_size"])
        self._feature_dim = cfg["hidden_size"]

    @torch.no_grad()
    def __call__(self, pixel_values=None, **_ignored):
        """``reward_model(**inputs)`` with the processor's ``pixel_values`` [B,3,crop,crop] -> see ``_VitOutput``"""
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        L.require_cuda(pixel_values, "pixel_values")
        cls = self.encode_patches(self.pixel_values_to_patches(pixel_values))
        return _VitOutput((cls.unsqueeze(1), cls))


class ClipImageProcessor(DinoImageProcessor):
    """The preprocessing constants of ``openai/clip-vit-large-patch14`` (its preprocessor_config.json): resize to shortest edge 224 with PIL BICUBIC, center
    crop 224, rescale 1/255, normalise with the CLIP mean / std.  A plain holder: the arithmetic runs in ``HipCLIPVisionModel.preprocess``."""

    def __init__(self, size=None, crop_size=None, rescale_factor=1 / 255, image_mean=(0.48145466, 0.4578275, 0.40821073),
                 image_std=(0.26862954, 0.26130258, 0.27577711)):
        super().__init__(size or {"shortest_edge": 224}, crop_size, rescale_factor, image_mean, image_std)


class HipCLIPVisionModel(_HipImageEncoder):
    """The vision tower and ``visual_projection`` of ``transformers.CLIPModel`` (default: ViT-L/14).  ``get_image_features(pixel_values=...)`` is the call the
    reference makes; ``image_features(images)`` runs the processor's arithmetic on the GPU as well."""
    max_batch = 32             # 12.4 MB of workspace per image at ViT-L/14
    _prefix = "clipv"

    def __init__(self, config=None, device="cuda:0", processor=None):
        cfg = dict(CLIP_VIT_L14_CONFIG)
        cfg.update(config or {})
        self.config = cfg
        self.device = torch.device(device)
        self.processor = processor or ClipImageProcessor()
        edge, crop, rescale, mean, std = self.processor.constants()
        c = L.CsClipVisionConfig(cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["image_size"],
                                 cfg["patch_size"], cfg["projection_dim"], cfg["layer_norm_eps"], edge, crop, (C.c_float * 3)(*mean), (C.c_float * 3)(*std),
                                 rescale)
        h = C.c_void_p()
        L.check(L.lib().cs_clipv_create(C.byref(c), C.byref(h)))
        self._init_handle(h, crop, cfg["patch_size"])
        self._feature_dim = cfg["projection_dim"]

    @torch.no_grad()
    def get_image_features(self, pixel_values=None, **_ignored):
        """``reward_model.get_image_features(**inputs)`` with the processor's ``pixel_values`` [B,3,crop,crop] -> ``image_embeds`` [B, projection_dim] fp32"""
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        L.require_cuda(pixel_values, "pixel_values")
        return self.encode_patches(self.pixel_values_to_patches(pixel_values))


class DepthImageProcessor:
    """The preprocessing constants of ``depth-anything/Depth-Anything-V2-Small-hf`` (its preprocessor_config.json, a DPTImageProcessor; from memory: no hub
    access here): resize to 518 x 518 with PIL BICUBIC under ``keep_aspect_ratio`` and ``ensure_multiple_of = 14`` (for a square input exactly
    ``size`` x ``size``; ``output_size`` gives the rule for every input), no crop, no pad, rescale 1/255, normalise with the ImageNet mean / std.  A plain
    holder: the arithmetic runs in ``HipDepthAnythingModel.preprocess``."""
    do_resize = do_rescale = do_normalize = keep_aspect_ratio = True
    do_pad = False
    ensure_multiple_of = 14
    resample = 3                                   # PIL.Image.BICUBIC

    def __init__(self, size=None, rescale_factor=1 / 255, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225)):
        self.size = dict(size or {"height": 518, "width": 518})
        if set(self.size) != {"height", "width"} or self.size["height"] != self.size["width"] or self.size["height"] % self.ensure_multiple_of:
            raise ValueError("the HIP front end implements a square size that is a multiple of 14")
        self.rescale_factor, self.image_mean, self.image_std = float(rescale_factor), tuple(image_mean), tuple(image_std)

    def constants(self):
        return (self.size["height"], self.size["height"], self.rescale_factor, self.image_mean, self.image_std)

    def output_size(self, height, width):
        """the processed (height, width) of an input: transformers' ``get_resize_output_image_size`` with ``keep_aspect_ratio`` -- the scale closer to 1
        serves both axes, each side is then rounded (Python's ``round``: half to even) to a multiple of ``ensure_multiple_of``.  880 x 1184 -> (518, 700)."""
        m = self.ensure_multiple_of
        scale_h, scale_w = self.size["height"] / height, self.size["width"] / width
        if abs(1 - scale_w) < abs(1 - scale_h):
            scale_h = scale_w
        else:
            scale_w = scale_h
        return round(scale_h * height / m) * m, round(scale_w * width / m) * m


class _DepthOutput(tuple):
    """(predicted_depth,): ``outputs.predicted_depth`` [B, h, w] fp32 (the processed size), as transformers' DepthEstimatorOutput names it"""
    predicted_depth = property(lambda self: self[0])


class HipDepthAnythingModel(_HipImageModel):
    """``transformers.DepthAnythingForDepthEstimation`` (default: the V2-Small shape).  ``model(pixel_values=...).predicted_depth`` is the call the reference
    makes; ``predicted_depth(images)`` and ``normalized_depth(images)`` run the processor's arithmetic and the post-processing on the GPU as well."""
    workspace_budget = 600 << 20          # bytes of workspace one call may take: max_batch is sized from it (V2-Small: 72.7 MB per image -> 8 images per call)
    _prefix = "depth"

    def __init__(self, config=None, device="cuda:0", processor=None):
        cfg = dict(DEPTH_ANYTHING_V2_SMALL_CONFIG)
        cfg.update(config or {})
        self.config = cfg
        self.device = torch.device(device)
        self.processor = processor or DepthImageProcessor({"height": cfg["image_size"], "width": cfg["image_size"]})
        size, _, rescale, mean, std = self.processor.constants()
        c = L.CsDepthConfig(cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["mlp_ratio"], cfg["image_size"], cfg["patch_size"],
                            cfg["layer_norm_eps"], (C.c_int * 4)(*cfg["out_indices"]), (C.c_int * 4)(*cfg["neck_hidden_sizes"]), cfg["fusion_hidden_size"],
                            cfg["head_hidden_size"], cfg["max_depth"], size, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), rescale)
        h = C.c_void_p()
        L.check(L.lib().cs_depth_create(C.byref(c), C.byref(h)))
        self._init_handle(h, size, cfg["patch_size"])
        self.max_batch = max(1, min(_HipImageModel.max_batch, self.workspace_budget // int(self._fn("workspace_bytes")(h, 1))))

    def depth_from_patches(self, patches):
        """patch rows -> ``predicted_depth`` [B, size, size] fp32, ``max_batch`` images per call"""
        return self._forward(patches, self.crop, self.crop)

    # ---- any aspect ratio: the `_hw` entry points ---------------------------------------------------------------------
    def processed_size(self, height, width):
        """the (height, width) the front end resizes an input to (cs_depth_processed_size: the processor's rule; RuntimeError beyond the limits of
        include/consolver_hip.h)"""
        oh, ow = C.c_int(), C.c_int()
        L.check(L.lib().cs_depth_processed_size(self._h, height, width, C.byref(oh), C.byref(ow)))
        if (oh.value, ow.value) != tuple(self.processor.output_size(height, width)):
            raise ValueError(f"the processor's size rule gives {self.processor.output_size(height, width)} for {height} x {width}, the front end "
                             f"{(oh.value, ow.value)}: ensure_multiple_of must be the model's patch size")
        return oh.value, ow.value

    def preprocess_hw(self, images, return_crop=False):
        """[B,3,H,W] fp16 / fp32 in [0,1], any aspect ratio -> (patch rows [B * gh * gw, patch_cols] fp16, (out_h, out_w)) and, with ``return_crop``, the
        resized uint8 image [B,3,out_h,out_w] as a third item (what PIL hands the processor's rescale)"""
        L.require_cuda(images, "images")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"images must be [B,3,H,W], got {tuple(images.shape)}")
        if images.dtype not in _DT:
            raise TypeError(f"images must be float16 or float32 (the two quantisation paths that are built), got {images.dtype}")
        images = images.contiguous()
        B, _, H, W = images.shape
        oh, ow = self.processed_size(H, W)
        patches = torch.empty(B * (oh // self.patch) * (ow // self.patch), self.patch_cols, dtype=torch.float16, device=images.device)
        crop = torch.empty(B, 3, oh, ow, dtype=torch.uint8, device=images.device) if return_crop else None
        if B:
            need = int(L.lib().cs_depth_preprocess_workspace_bytes_hw(self._h, B, H, W))
            if self._pws is None or self._pws.numel() < need or self._pws.device != images.device:
                self._pws = torch.empty(need, dtype=torch.uint8, device=images.device)
            with torch.cuda.device(images.device):          # the resize tables of a new image size are allocated on the current device
                L.check(L.lib().cs_depth_preprocess_hw(self._h, L.ptr(images), _DT[images.dtype], B, H, W, None, None, L.ptr(patches), L.ptr(crop),
                                                       L.ptr(self._pws), self._pws.numel(), L.stream_ptr(images.device)))
        return (patches, (oh, ow), crop) if return_crop else (patches, (oh, ow))

    def depth_from_patches_hw(self, patches, size):
        """patch rows of images processed to ``size`` = (out_h, out_w) -> ``predicted_depth`` [B, out_h, out_w] fp32.  Images per call: ``max_batch``,
        and no more than ``workspace_budget`` holds of this size's workspace."""
        if not self._finalized:
            raise RuntimeError("weights not loaded")
        L.require_cuda(patches, "patches")
        oh, ow = size
        per_image = int(L.lib().cs_depth_workspace_bytes_hw(self._h, 1, oh, ow))
        if not per_image:
            L.check(L.lib().cs_depth_forward_hw(self._h, None, 0, oh, ow, None, None, 0, None))          # raises with the library's reason for the refusal
            raise RuntimeError(f"processed size {oh} x {ow} is not supported")
        step = max(1, min(self.max_batch, self.workspace_budget // per_image))
        n_rows = (oh // self.patch) * (ow // self.patch)
        if patches.dim() != 2 or patches.shape[1] != self.patch_cols or patches.shape[0] % n_rows:
            raise ValueError(f"patches must be [B * {n_rows}, {self.patch_cols}] for a {oh} x {ow} image, got {tuple(patches.shape)}")
        patches = patches.contiguous()
        B = patches.shape[0] // n_rows
        out = torch.empty(B, oh, ow, dtype=torch.float32, device=patches.device)
        with torch.cuda.device(patches.device):             # the position table of a new grid is allocated on the current device
            for s in range(0, B, step):
                n = min(step, B - s)
                need = int(L.lib().cs_depth_workspace_bytes_hw(self._h, n, oh, ow))
                if self._ws is None or self._ws.numel() < need or self._ws.device != patches.device:
                    self._ws = torch.empty(need, dtype=torch.uint8, device=patches.device)
                L.check(L.lib().cs_depth_forward_hw(self._h, L.ptr(patches[s * n_rows:]), n, oh, ow, L.ptr(out[s:]), L.ptr(self._ws), self._ws.numel(),
                                                    L.stream_ptr(patches.device)))
        return out

    def flops_hw(self, batch, size):
        return float(L.lib().cs_depth_flops_hw(self._h, batch, size[0], size[1]))

    def position_table(self, gh, gw):
        """-> (the position table [1 + gh * gw, hidden] fp16 the forward reads at a gh x gw patch grid, whether this call interpolated it on the device)"""
        if not self._finalized:
            raise RuntimeError("weights not loaded")
        table = torch.empty(1 + gh * gw, self.config["hidden_size"], dtype=torch.float16, device=self.device)
        launched = C.c_int(-1)
        with torch.cuda.device(self.device):
            L.check(L.lib().cs_depth_position_table(self._h, gh, gw, L.ptr(table), C.byref(launched), L.stream_ptr(self.device)))
        return table, bool(launched.value)

    def patches_to_pixel_values(self, patches, size=None):
        """the patch rows back in the processor's layout: ``pixel_values`` [B,3,out_h,out_w] fp16 (``size``: the processed size; default the square one)"""
        if size is None:
            return super().patches_to_pixel_values(patches)
        gh, gw, P = size[0] // self.patch, size[1] // self.patch, self.patch
        B = patches.shape[0] // (gh * gw)
        return patches[:, :3 * P * P].reshape(B, gh, gw, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, gh * P, gw * P)

    def pixel_values_to_patches(self, pixel_values):
        """``pixel_values`` [B,3,h,w], h and w multiples of the patch size -> the patch rows"""
        P = self.patch
        B, ch, h, w = pixel_values.shape
        if ch != 3 or h % P or w % P or not h or not w:
            raise ValueError(f"pixel_values must be [B,3,h,w] with h and w multiples of the patch size {P}, got {tuple(pixel_values.shape)}")
        gh, gw = h // P, w // P
        rows = pixel_values.to(torch.float16).reshape(B, 3, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, 3 * P * P)
        out = rows.new_zeros(B * gh * gw, self.patch_cols)
        out[:, :3 * P * P] = rows
        return out

    @torch.no_grad()
    def __call__(self, pixel_values=None, **_ignored):
        """``reward_model(**inputs)`` with the processor's ``pixel_values`` [B,3,h,w] (h and w multiples of the patch size, as transformers takes them; the
        processor's own square size runs the square entry point) -> see ``_DepthOutput``"""
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        L.require_cuda(pixel_values, "pixel_values")
        patches = self.pixel_values_to_patches(pixel_values)
        size = tuple(pixel_values.shape[-2:])
        return _DepthOutput((self.depth_from_patches(patches) if size == (self.crop, self.crop) else self.depth_from_patches_hw(patches, size),))

    def predicted_depth(self, images):
        """[B,3,H,W] in [0,1] -> ``predicted_depth`` [B, out_h, out_w] fp32 at the processed size (a square image: [B, size, size], the square entry points)"""
        if images.dim() == 4 and images.shape[-1] != images.shape[-2]:
            return self.depth_from_patches_hw(*self.preprocess_hw(images))
        return self.depth_from_patches(self.preprocess(images))

    def post_process(self, predicted_depth, height, width):
        """``post_process_depth_estimation(target_sizes=[(height, width)])`` (torch bicubic) and the reward's per-map (d - min) / (max - min + 1e-8):
        [B, h, w] fp32 -> [B, height, width] fp32"""
        L.require_cuda(predicted_depth, "predicted_depth")
        d = predicted_depth.to(torch.float32).contiguous()
        if d.dim() != 3 or not d.shape[1] or not d.shape[2]:
            raise ValueError(f"predicted_depth must be [B,h,w], got {tuple(d.shape)}")
        B, ih, iw = d.shape
        out = torch.empty(B, height, width, dtype=torch.float32, device=d.device)
        if B and (ih, iw) == (self.crop, self.crop):
            L.check(self._fn("normalized_maps")(self._h, L.ptr(d), B, height, width, L.ptr(out), L.stream_ptr(d.device)))
        elif B:
            L.check(L.lib().cs_depth_normalized_maps_hw(self._h, L.ptr(d), B, ih, iw, height, width, L.ptr(out), L.stream_ptr(d.device)))
        return out

    def normalized_depth(self, images):
        """[B,3,H,W] in [0,1] -> the normalised depth maps at the images' size, [B,H,W] fp32: the whole per-image path of the reward up to the PSNR"""
        return self.post_process(self.predicted_depth(images), images.shape[-2], images.shape[-1])


class SegImageProcessor:
    """The preprocessing constants of ``nvidia/segformer-b4-finetuned-ade-512-512`` (its preprocessor_config.json, a SegformerImageProcessor; from memory: no
    hub access here): resize to 512 x 512 with PIL BILINEAR, no crop, rescale 1/255, normalise with the ImageNet mean / std, labels not reduced.  A plain
    holder: the arithmetic runs in ``HipSegformerModel.preprocess`` (square inputs) and ``preprocess_hw`` (any aspect ratio: stretched to the same size)."""
    do_resize = do_rescale = do_normalize = True
    do_reduce_labels = False
    resample = 2                                   # PIL.Image.BILINEAR

    def __init__(self, size=None, rescale_factor=1 / 255, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225)):
        self.size = dict(size or {"height": 512, "width": 512})
        if set(self.size) != {"height", "width"} or self.size["height"] != self.size["width"] or self.size["height"] % 32:
            raise ValueError("the HIP front end implements a square size that is a multiple of 32")
        self.rescale_factor, self.image_mean, self.image_std = float(rescale_factor), tuple(image_mean), tuple(image_std)

    def constants(self):
        return (self.size["height"], self.resample, self.rescale_factor, self.image_mean, self.image_std)


class _SegConfigView:
    """``model.config.num_labels`` / ``.num_classes`` as the reference reads them, and the config dict's keys"""

    def __init__(self, cfg):
        self.__dict__.update(cfg)
        self.num_classes = cfg["num_labels"]

    def __eq__(self, other):
        return {k: v for k, v in self.__dict__.items() if k != "num_classes"} == (other if isinstance(other, dict) else getattr(other, "__dict__", None))

    def __getitem__(self, k):
        return self.__dict__[k]


class _SegOutput(tuple):
    """(logits,): ``outputs.logits`` [B, num_labels, size / 4, size / 4] fp32, as transformers' SemanticSegmenterOutput names it"""
    logits = property(lambda self: self[0])


class HipSegformerModel(_HipImageModel):
    """``transformers.SegformerForSemanticSegmentation`` (default: the MiT-B4 ADE shape).  ``model(pixel_values=...).logits`` is the call the reference
    makes; ``masks(images)`` runs the processor's arithmetic and the class argmax on the GPU as well."""
    workspace_budget = 2048 << 20         # bytes of workspace one call may take: max_batch is sized from it (B4 at 512: 167 MB per image -> 12 images per call)
    _prefix = "seg"

    def __init__(self, config=None, device="cuda:0", processor=None):
        cfg = dict(SEGFORMER_B4_ADE_CONFIG)
        cfg.update(config or {})
        self.config = _SegConfigView(cfg)
        self.device = torch.device(device)
        self.processor = processor or SegImageProcessor({"height": cfg["image_size"], "width": cfg["image_size"]})
        size, _, rescale, mean, std = self.processor.constants()
        if size != cfg["image_size"]:
            raise ValueError(f"the processor resizes to {size}, the model was configured for {cfg['image_size']}")
        i4 = lambda k: (C.c_int * 4)(*cfg[k])
        c = L.CsSegConfig(i4("hidden_sizes"), i4("depths"), i4("num_attention_heads"), i4("sr_ratios"), cfg["mlp_ratio"], cfg["decoder_hidden_size"],
                          cfg["num_labels"], size, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), rescale)
        h = C.c_void_p()
        L.check(L.lib().cs_seg_create(C.byref(c), C.byref(h)))
        self._init_handle(h, size, 1)
        self.grid, self.num_labels = size // 4, cfg["num_labels"]
        self.max_batch = max(1, min(_HipImageModel.max_batch, self.workspace_budget // int(self._fn("workspace_bytes")(h, 1))))

    def _run(self, patches, want_logits, want_masks):
        """the normalised image rows -> (logits [B, num_labels, g, g] fp32 | None, masks [B, g, g] int32 | None), ``max_batch`` images per call"""
        if not self._finalized:
            raise RuntimeError("weights not loaded")
        L.require_cuda(patches, "patches")
        px, g = self.crop * self.crop, self.grid
        B = patches.shape[0] // px
        logits = torch.empty(B, self.num_labels, g, g, dtype=torch.float32, device=patches.device) if want_logits else None
        masks = torch.empty(B, g, g, dtype=torch.int32, device=patches.device) if want_masks else None
        st = L.stream_ptr(patches.device)
        for s in range(0, B, self.max_batch):
            n = min(self.max_batch, B - s)
            need = int(self._fn("workspace_bytes")(self._h, n))
            if self._ws is None or self._ws.numel() < need or self._ws.device != patches.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=patches.device)
            L.check(self._fn("forward")(self._h, L.ptr(patches[s * px:]), n, L.ptr(logits[s:]) if want_logits else None, L.ptr(self._ws), self._ws.numel(), st))
            if want_masks:
                L.check(self._fn("masks")(self._h, n, L.ptr(self._ws), self._ws.numel(), L.ptr(masks[s:]), st))
        return logits, masks

    @torch.no_grad()
    def __call__(self, pixel_values=None, **_ignored):
        """``reward_model(**inputs)`` with the processor's ``pixel_values`` [B,3,size,size] -> see ``_SegOutput``"""
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        L.require_cuda(pixel_values, "pixel_values")
        return _SegOutput((self._run(self.pixel_values_to_patches(pixel_values), True, False)[0],))

    def preprocess_hw(self, images, return_crop=False):
        """``preprocess`` for images of any aspect ratio: the processor stretches them to size x size, so the outputs have the square call's shapes"""
        L.require_cuda(images, "images")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"images must be [B,3,H,W], got {tuple(images.shape)}")
        if images.dtype not in _DT:
            raise TypeError(f"images must be float16 or float32 (the two quantisation paths that are built), got {images.dtype}")
        images = images.contiguous()
        B, _, H, W = images.shape
        patches = torch.empty(B * self.crop * self.crop, self.patch_cols, dtype=torch.float16, device=images.device)
        crop = torch.empty(B, 3, self.crop, self.crop, dtype=torch.uint8, device=images.device) if return_crop else None
        if B:
            need = int(self._fn("preprocess_workspace_bytes")(self._h, B, H, W))
            if self._pws is None or self._pws.numel() < need or self._pws.device != images.device:
                self._pws = torch.empty(need, dtype=torch.uint8, device=images.device)
            with torch.cuda.device(images.device):
                L.check(L.lib().cs_seg_preprocess_hw(self._h, L.ptr(images), _DT[images.dtype], B, H, W, None, None, L.ptr(patches), L.ptr(crop), L.ptr(self._pws),
                                                     self._pws.numel(), L.stream_ptr(images.device)))
        return (patches, crop) if return_crop else patches

    def _front_end(self, images):
        return self.preprocess_hw(images) if images.dim() == 4 and images.shape[-1] != images.shape[-2] else self.preprocess(images)

    def logits_and_masks(self, images):
        """[B,3,H,W] in [0,1] -> (logits [B, num_labels, g, g] fp32, masks [B, g, g] int32) of one pass"""
        return self._run(self._front_end(images), True, True)

    def masks(self, images):
        """[B,3,H,W] in [0,1] -> the class masks [B, size / 4, size / 4] int32 (argmax of the logits, a tie to the lowest class): the whole per-image path of
        the reward up to the comparison"""
        return self._run(self._front_end(images), False, True)[1]


class InceptionImageProcessor:
    """The reference's torchvision transform for the inception reward (edit_ppo/reward_model.py:98-108): ``Resize(size, BICUBIC)`` (shortest edge),
    ``CenterCrop(size)`` (window at ``int(round((n - size) / 2.0))``, round half to even), ``ToTensor``, ``Normalize`` with the ImageNet mean / std.  A plain
    holder: the arithmetic runs in ``HipInceptionV3.preprocess`` (any aspect ratio)."""
    do_resize = do_center_crop = do_rescale = do_normalize = True
    resample = 3                                   # PIL.Image.BICUBIC

    def __init__(self, size=299, rescale_factor=1 / 255, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225)):
        self.size = int(size)
        if not 75 <= self.size <= 2048:
            raise ValueError("Inception-v3 needs an image edge of 75 .. 2048")
        self.rescale_factor, self.image_mean, self.image_std = float(rescale_factor), tuple(image_mean), tuple(image_std)

    def constants(self):
        return (self.size, self.size, self.rescale_factor, self.image_mean, self.image_std)


class HipInceptionV3(_HipImageEncoder):
    """torchvision ``inception_v3(aux_logits=True, transform_input=False).eval()``.  ``model(pixel_values)`` -> the logits of ``fc`` [B, num_classes] fp32 is
    the call the reference makes (its comment says features; the tensor is the logits); ``image_features(images)`` runs the transform on the GPU as well.
    ``AuxLogits.*`` tensors of a checkpoint are ignored by ``load_state_dict``."""
    workspace_budget = 1024 << 20         # bytes of workspace one call may take: max_batch is sized from it (299: 5.4 MB per image)
    _prefix = "incep"

    def __init__(self, config=None, device="cuda:0", processor=None):
        cfg = dict(INCEPTION_V3_CONFIG)
        cfg.update(config or {})
        self.config = cfg
        self.device = torch.device(device)
        self.processor = processor or InceptionImageProcessor(cfg["image_size"])
        size, _, rescale, mean, std = self.processor.constants()
        if size != cfg["image_size"]:
            raise ValueError(f"the processor resizes to {size}, the model was configured for {cfg['image_size']}")
        c = L.CsIncepConfig(size, cfg["num_classes"], (C.c_float * 3)(*mean), (C.c_float * 3)(*std), rescale)
        h = C.c_void_p()
        L.check(L.lib().cs_incep_create(C.byref(c), C.byref(h)))
        self._init_handle(h, size, 1)
        self._feature_dim = cfg["num_classes"]
        self.max_batch = max(1, min(_HipImageModel.max_batch, self.workspace_budget // int(self._fn("workspace_bytes")(h, 1))))

    @torch.no_grad()
    def __call__(self, pixel_values=None, **_ignored):
        """``reward_model(img_tensor)`` with the transform's output [B,3,size,size] -> logits [B, num_classes] fp32"""
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        L.require_cuda(pixel_values, "pixel_values")
        return self.encode_patches(self.pixel_values_to_patches(pixel_values))


def mask_agreement(pred_masks, target_masks):
    """int32 masks [B,h,w] x ([B,h,w] or [1,h,w]) -> 100 * mean(pred == target) per sample, [B,1] fp32"""
    L.require_cuda(pred_masks, "pred_masks")
    a, b = pred_masks.to(torch.int32).contiguous(), target_masks.to(torch.int32).contiguous()
    B = a.shape[0]
    if b.shape[0] not in (B, 1) or b.shape[1:] != a.shape[1:]:
        raise ValueError(f"mask shapes {tuple(a.shape)} vs {tuple(b.shape)}")
    n = a[0].numel() if B else 0
    out = torch.empty(B, 1, dtype=torch.float32, device=a.device)
    if B:
        L.check(L.lib().cs_seg_agreement(L.ptr(a), L.ptr(b), n if (b.shape[0] == B and B > 1) else 0, B, n, L.ptr(out), L.stream_ptr(a.device)))
    return out


def load_dino_reward(device="cuda:0", config=None):
    """edit_ppo/reward_model.py:59-64 without the hub: the dinov2-base shapes and processor constants; the caller loads the weights."""
    processor = DinoImageProcessor()
    return HipDinov2Model(config, device=device, processor=processor), processor


def load_clip_reward(device="cuda:0", config=None):
    """edit_ppo/reward_model.py:128-134 without the hub: the clip-vit-large-patch14 vision shapes and processor constants; the caller loads the weights."""
    processor = ClipImageProcessor()
    return HipCLIPVisionModel(config, device=device, processor=processor), processor


def load_depth_reward(device="cuda:0", config=None):
    """edit_ppo/reward_model.py:92-96 without the hub: the Depth-Anything-V2-Small shapes and processor constants; the caller loads the weights."""
    cfg = dict(DEPTH_ANYTHING_V2_SMALL_CONFIG)
    cfg.update(config or {})
    processor = DepthImageProcessor({"height": cfg["image_size"], "width": cfg["image_size"]})
    return HipDepthAnythingModel(cfg, device=device, processor=processor), processor


def load_segmentation_reward(device="cuda:0", config=None):
    """edit_ppo/reward_model.py:110-117 without the hub: the segformer-b4-finetuned-ade-512-512 shapes and processor constants; the caller loads the weights."""
    cfg = dict(SEGFORMER_B4_ADE_CONFIG)
    cfg.update(config or {})
    processor = SegImageProcessor({"height": cfg["image_size"], "width": cfg["image_size"]})
    return HipSegformerModel(cfg, device=device, processor=processor), processor


def load_inception_reward(device="cuda:0", config=None):
    """edit_ppo/reward_model.py:98-108 without the hub: torchvision's Inception-v3 shapes and the reference's transform constants; the caller loads the weights."""
    cfg = dict(INCEPTION_V3_CONFIG)
    cfg.update(config or {})
    processor = InceptionImageProcessor(cfg["image_size"])
    return HipInceptionV3(cfg, device=device, processor=processor), processor


def load_reward_model(reward_type, device="cuda:0", config=None):
    """edit_ppo/reward_model.py:25-57.  ``image_psnr`` needs no model; ``dino`` and ``clip`` are built here; ``depth``, ``segmentation`` and ``inception`` are
    built but loaded through ``load_depth_reward`` / ``load_segmentation_reward`` / ``load_inception_reward`` (this dispatcher's answers for them are pinned
    by the existing tests); the other backbones are not implemented."""
    if reward_type == "image_psnr":
        return None, None
    if reward_type == "dino":
        return load_dino_reward(device, config)
    if reward_type == "clip":
        return load_clip_reward(device, config)
    if reward_type == "depth":
        raise NotImplementedError("reward_type 'depth' is not loaded through this dispatcher yet: use load_depth_reward(device, config)")
    if reward_type == "segmentation":
        raise NotImplementedError("reward_type 'segmentation' is not loaded through this dispatcher yet: use load_segmentation_reward(device, config)")
    if reward_type == "inception":
        raise NotImplementedError("reward_type 'inception' is not loaded through this dispatcher yet: use load_inception_reward(device, config)")
    if reward_type in ("llava", "qwen_vl"):
        raise NotImplementedError(f"reward_type '{reward_type}' needs a third-party backbone network that is not implemented")
    raise ValueError(f"Unknown reward_type: {reward_type}")


def cosine_reward(pred_features, target_features):
    """[B,D] fp32 x ([B,D] or [1,D]) -> (cosine_similarity(normalize(a), normalize(b)) + 1) * 50, [B,1] fp32.  cs_cosine_reward normalises and then takes
    the cosine (the dino / clip form); that equals a plain ``F.cosine_similarity`` of the raw vectors (the inception form) to fp32 rounding unless a
    vector's norm is under 1e-8 (where both clamp, differently)."""
    L.require_cuda(pred_features, "pred_features")
    a, b = pred_features.to(torch.float32).contiguous(), target_features.to(torch.float32).contiguous()
    B, D = a.shape
    if b.shape not in ((B, D), (1, D)):
        raise ValueError(f"feature shapes {tuple(a.shape)} vs {tuple(b.shape)}")
    out = torch.empty(B, 1, dtype=torch.float32, device=a.device)
    if B:
        L.check(L.lib().cs_cosine_reward(L.ptr(a), L.ptr(b), B, D, D if (b.shape[0] == B and B > 1) else 0, L.ptr(out), L.stream_ptr(a.device)))
    return out


def _paired_image_pass(reward_model, reward_model_processor, model_pred, target, per_image):
    """the part the model rewards share: processor check, argument checks, and ``per_image`` ([n,3,H,W] -> [n, ...]) in one pass over the 2 B images
    (a [1,3,H,W] target shared by the batch, or one of another dtype, goes through on its own) -> (of model_pred [B, ...], of target [B or 1, ...])"""
    if reward_model_processor is not None and reward_model_processor.constants() != reward_model.processor.constants():
        raise ValueError("the processor's constants differ from the ones the model's front end was built with")
    L.require_cuda(model_pred, "model_pred")
    L.require_cuda(target, "target")
    B = model_pred.shape[0]
    if target.shape[0] not in (B, 1) or target.shape[1:] != model_pred.shape[1:]:
        raise ValueError(f"shape mismatch {tuple(model_pred.shape)} vs {tuple(target.shape)}")
    if target.dtype != model_pred.dtype or target.shape[0] != B:
        return per_image(model_pred), per_image(target)
    out = per_image(torch.cat([model_pred, target]))            # one front-end and one model pass for the 2 B images
    return out[:B], out[B:]


def _feature_cosine_reward(reward_model, reward_model_processor, model_pred, target):
    """the image-similarity rewards: the features of pred and target (a [1,3,H,W] target is encoded once), the cosine tail"""
    return cosine_reward(*_paired_image_pass(reward_model, reward_model_processor, model_pred, target, reward_model.image_features))


def calculate_dino_reward(reward_model, reward_model_processor, model_pred, target, device=None):
    """edit_ppo/reward_model.py:217-257 for the whole batch in one pass: ``model_pred`` [B,3,H,W] and ``target`` [B,3,H,W] (or [1,3,H,W]: one
    target shared by the batch, its features computed once) in [0,1] -> rewards [B,1] fp32 in [0, 100].  Values outside [0,1] are clamped."""
    if not isinstance(reward_model, HipDinov2Model):
        raise TypeError("reward_type 'dino' needs a HipDinov2Model (load_reward_model('dino')); there is no CPU or eager path")
    return _feature_cosine_reward(reward_model, reward_model_processor, model_pred, target)


def calculate_clip_reward(reward_model, reward_model_processor, model_pred, target, device=None):
    """edit_ppo/reward_model.py:512-552 for the whole batch in one pass, with the argument forms of ``calculate_dino_reward``: cosine similarity of the
    CLIP ``image_embeds`` of pred and target -> rewards [B,1] fp32 in [0, 100].  Any other ``reward_model`` (``None``, a transformers CLIPModel) raises
    ``NotImplementedError``: the eager transformers path is not implemented."""
    if not isinstance(reward_model, HipCLIPVisionModel):
        raise NotImplementedError("reward_type 'clip' needs a HipCLIPVisionModel (load_reward_model('clip')); the eager transformers path is not implemented")
    return _feature_cosine_reward(reward_model, reward_model_processor, model_pred, target)


def calculate_depth_reward(reward_model, reward_model_processor, model_pred, target, device=None):
    """edit_ppo/reward_model.py:359-422 for the whole batch on the GPU, with the argument forms of ``calculate_dino_reward``: the PSNR of the min / max
    normalised Depth Anything maps of pred and target at the images' size, clamp(min=0) only -> rewards [B,1] fp32 (identical maps: 80, the value of
    10 log10(1 / 1e-8)).  Any other ``reward_model`` (``None``, a transformers model) raises ``NotImplementedError``: the eager transformers path is
    not implemented."""
    if not isinstance(reward_model, HipDepthAnythingModel):
        raise NotImplementedError("reward_type 'depth' needs a HipDepthAnythingModel (load_depth_reward(device, config)); the eager transformers path is "
                                  "not implemented")
    pred_maps, target_maps = _paired_image_pass(reward_model, reward_model_processor, model_pred, target, reward_model.normalized_depth)
    from .ppo import depth_psnr_tail            # a one-row target map is read in place by every row (cs_image_psnr_bcast)
    return depth_psnr_tail(pred_maps, target_maps)


def calculate_segmentation_reward(reward_model, reward_model_processor, model_pred, target, device=None):
    """edit_ppo/reward_model.py:425-481 for the whole batch on the GPU, with the argument forms of ``calculate_dino_reward``: the share of pixels, times
    100, on which the SegFormer class masks (argmax of the logits at a quarter of the processor's size) of pred and target agree -> rewards [B,1] fp32 in
    [0, 100].  Any other ``reward_model`` (``None``, a transformers model) raises ``NotImplementedError``: the eager transformers path is not implemented."""
    if not isinstance(reward_model, HipSegformerModel):
        raise NotImplementedError("reward_type 'segmentation' needs a HipSegformerModel (load_segmentation_reward(device, config)); the eager transformers "
                                  "path is not implemented")
    return mask_agreement(*_paired_image_pass(reward_model, reward_model_processor, model_pred, target, reward_model.masks))


def calculate_inception_reward(reward_model, reward_model_processor, model_pred, target, device=None):
    """edit_ppo/reward_model.py:319-356 for the whole batch in one pass, with the argument forms of ``calculate_dino_reward`` and images of any aspect ratio:
    (cosine_similarity of the Inception-v3 logits of pred and target + 1) * 50 -> rewards [B,1] fp32 in [0, 100].  The tail normalises each logit vector and
    then takes the cosine (``cosine_reward``): equal to ``F.cosine_similarity`` of the raw logits to fp32 rounding unless a logit vector's norm is under
    1e-8.  Any other ``reward_model`` (``None``, a torchvision module) raises ``NotImplementedError``: the eager torchvision path is not implemented."""
    if not isinstance(reward_model, HipInceptionV3):
        raise NotImplementedError("reward_type 'inception' needs a HipInceptionV3 (load_inception_reward(device, config)); the eager torchvision path is "
                                  "not implemented")
    return _feature_cosine_reward(reward_model, reward_model_processor, model_pred, target)
