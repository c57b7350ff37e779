"""Seeded synthetic weights of the exact SD1.5 shapes (no checkpoints exist offline).

conv / linear weights ~ N(0, 1/fan_in), norm gamma = 1 + small noise, beta small noise, biases small:
activations stay O(1) through the GroupNorms so fp16 neither overflows nor underflows.
"""
import torch


def synthetic_unet_state_dict(manifest, seed=20251226, device="cpu"):
    """``device``: where the values are drawn (the CPU and the GPU generators give different streams for one seed: the tests and their committed numbers use the
    CPU stream, bench.py draws on each rank's own GPU)."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, shape in manifest:
        if name.endswith(".weight") and len(shape) >= 2:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            w = torch.randn(shape, generator=g, device=device) * (1.0 / fan_in) ** 0.5
        elif ("norm" in name) and name.endswith(".weight"):
            w = 1.0 + 0.1 * torch.randn(shape, generator=g, device=device)
        else:
            w = 0.05 * torch.randn(shape, generator=g, device=device)
        sd[name] = w
    return sd


def synthetic_vae_state_dict(manifest, seed=20251227):
    """Same recipe for the AutoencoderKL decoder; conv_out is scaled so images land inside [-1, 1] with some clipping."""
    return synthetic_unet_state_dict(manifest, seed)


def synthetic_clip_state_dict(manifest, seed=20251228):
    """CLIP text tower: embeddings ~ N(0, 0.02^2)-like scale kept O(1) after the first LayerNorm, linears ~ N(0, 1/fan_in)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in manifest:
        if "embedding" in name:
            w = 0.5 * torch.randn(shape, generator=g)
        elif name.endswith(".weight") and len(shape) == 2:
            w = torch.randn(shape, generator=g) * (1.0 / shape[1]) ** 0.5
        elif "layer_norm" in name and name.endswith(".weight"):
            w = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            w = 0.05 * torch.randn(shape, generator=g)
        sd[name] = w
    return sd


def synthetic_dinov2_state_dict(manifest, seed=20251229):
    """DINOv2 encoder: matrices (the patch projection included) ~ N(0, 1/fan_in), biases and the mask token 0.05 N, LayerScale lambda uniform in
    [0.05, 1] (trained checkpoints spread over that range; the init value 1.0 would hide a LayerScale that is dropped), CLS token and position
    table 0.5 N, norm gains 1 + 0.1 N."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in manifest:
        if name.endswith("lambda1"):
            w = 0.05 + 0.95 * torch.rand(shape, generator=g)
        elif name.endswith("cls_token") or name.endswith("position_embeddings"):
            w = 0.5 * torch.randn(shape, generator=g)
        elif name.endswith(".weight") and len(shape) >= 2:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            w = torch.randn(shape, generator=g) * (1.0 / fan_in) ** 0.5
        elif "norm" in name and name.endswith(".weight"):
            w = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            w = 0.05 * torch.randn(shape, generator=g)
        sd[name] = w
    return sd


def synthetic_depth_anything_state_dict(manifest, seed=20251231):
    """Depth Anything (``HipDepthAnythingModel.manifest()``): the ``backbone.*`` tensors from ``synthetic_dinov2_state_dict``; neck and head matrices
    ~ N(0, 1/fan_in), where the two transposed convs of the reassemble stage (kernel = stride: ONE tap per output pixel, weight [in, out, k, k]) count
    fan_in = input channels; biases 0.05 N.  With torch's default init the head's ReLU output is ~1e-5 everywhere and the reward's min / max normalisation
    would turn rounding noise into the whole signal; this scaling keeps every layer's activations of order one, so the depth map has a range of order one."""
    bb = "backbone."
    sd = {bb + k: v for k, v in synthetic_dinov2_state_dict([(n[len(bb):], s) for n, s in manifest if n.startswith(bb)], seed=seed).items()}
    g = torch.Generator().manual_seed(seed + 1)
    for name, shape in manifest:
        if name.startswith(bb):
            continue
        if name.endswith(".weight"):
            transposed = ".resize." in name and shape[2] != 3
            fan_in = shape[0] if transposed else shape[1] * shape[2] * shape[3]
            sd[name] = torch.randn(shape, generator=g) * (1.0 / fan_in) ** 0.5
        else:
            sd[name] = 0.05 * torch.randn(shape, generator=g)
    return sd


def synthetic_segformer_state_dict(manifest, seed=20260101):
    """SegFormer (``HipSegformerModel.manifest()``): matrices and conv filters ~ N(0, 1/fan_in) (a depthwise 3x3 filter: fan_in 9), LayerNorm / BatchNorm
    gains 1 + 0.1 N, biases 0.05 N, the BatchNorm's running_mean 0.1 N and running_var uniform in [0.5, 1.5] (the init values 0 and 1 would hide a fold that
    drops them), ``num_batches_tracked`` an int64 zero as in a state dict."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in manifest:
        if name.endswith("num_batches_tracked"):
            w = torch.zeros(shape, dtype=torch.int64)
        elif name.endswith("running_var"):
            w = 0.5 + torch.rand(shape, generator=g)
        elif name.endswith("running_mean"):
            w = 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".weight") and len(shape) >= 2:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            w = torch.randn(shape, generator=g) * (1.0 / fan_in) ** 0.5
        elif "norm" in name and name.endswith(".weight"):
            w = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            w = 0.05 * torch.randn(shape, generator=g)
        sd[name] = w
    return sd


def synthetic_inception_state_dict(manifest, seed=20260102):
    """Inception-v3 (``HipInceptionV3.manifest()``), the SegFormer recipe: conv filters and ``fc.weight`` ~ N(0, 1/fan_in), BatchNorm gains 1 + 0.1 N, biases
    0.05 N, running_mean 0.1 N, running_var uniform in [0.5, 1.5], ``num_batches_tracked`` an int64 zero.  With these running statistics 94 ReLU layers
    build up a constant component and the logits hardly depend on the image: tests calibrate the statistics on a batch first
    (tests/inception_oracle.py ``calibrate_batch_norm``)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in manifest:
        if name.endswith("num_batches_tracked"):
            w = torch.zeros(shape, dtype=torch.int64)
        elif name.endswith("running_var"):
            w = 0.5 + torch.rand(shape, generator=g)
        elif name.endswith("running_mean"):
            w = 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".weight") and len(shape) >= 2:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            w = torch.randn(shape, generator=g) * (1.0 / fan_in) ** 0.5
        elif ".bn." in name and name.endswith(".weight"):
            w = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            w = 0.05 * torch.randn(shape, generator=g)
        sd[name] = w
    return sd


def synthetic_clip_vision_state_dict(manifest, seed=20251230):
    """CLIP vision tower + projection: matrices (the patch projection included) ~ N(0, 1/fan_in), class and position embeddings 0.5 N, norm gains
    1 + 0.1 N (``pre_layrnorm`` / ``post_layernorm`` / ``layer_norm1|2``), biases 0.05 N."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in manifest:
        if name.endswith("class_embedding") or name.endswith("position_embedding.weight"):
            w = 0.5 * torch.randn(shape, generator=g)
        elif name.endswith(".weight") and len(shape) >= 2:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            w = torch.randn(shape, generator=g) * (1.0 / fan_in) ** 0.5
        elif "norm" in name and name.endswith(".weight"):
            w = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            w = 0.05 * torch.randn(shape, generator=g)
        sd[name] = w
    return sd


def synthetic_prompt_embeds(batch, ctx_len=77, dim=768, seed=1001):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, ctx_len, dim, generator=g)
    return torch.nn.functional.layer_norm(x, (dim,))


def synthetic_flux_state_dict(manifest, seed=20251226, device="cpu", dtype=torch.float32):
    """seeded FLUX-DiT weights: linear ~ N(0, 1/fan_in), norm weights ~ 1, modulation linears small so that
    gates stay O(0.1-1) (an untrained adaLN-Zero would gate every block off)."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, shape in manifest:
        if name.endswith("norm_q.weight") or name.endswith("norm_k.weight") or name.endswith("norm_added_q.weight") or name.endswith("norm_added_k.weight"):
            w = 1.0 + 0.1 * torch.randn(shape, generator=g, device=device)
        elif name.endswith(".weight"):
            w = torch.randn(shape, generator=g, device=device) * (1.0 / shape[1]) ** 0.5
            if ".norm" in name and name.endswith("linear.weight"):
                w = w * 0.5
        else:
            w = 0.05 * torch.randn(shape, generator=g, device=device)
            if ".norm" in name and name.endswith("linear.bias"):
                w = w + 0.3
        sd[name] = w.to(dtype)
    return sd


def synthetic_fid_inception_state_dict(manifest, seed=20260103):
    """The FID Inception-v3 (``HipFIDInception.manifest()``: the inception manifest without ``fc``): the recipe of ``synthetic_inception_state_dict``; tests
    calibrate the BatchNorm statistics on a batch first, as they do for the classifier."""
    return synthetic_inception_state_dict(manifest, seed)
