"""CPU checks behind the CLIP image-similarity reward (reward_type "clip"): tests/clip_vision_oracle.py against the committed transformers / PIL fixture,
the weight manifest against the published ViT-L/14 parameter count, the loaders and the host-side rejections of cs_clipv_create / load_state_dict."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import clip_vision_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCED = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, projection_dim=64)
SMALL = dict(hidden_size=128, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, projection_dim=8)


def _generator():
    spec = importlib.util.spec_from_file_location("make_clip_reward_golden", os.path.join(ROOT, "tools", "make_clip_reward_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_oracle_reproduces_the_fixture_without_transformers(golden):
    """what the GPU suite relies on: seeded images and weights + tests/clip_vision_oracle.py give the fixture's crops, pixel_values, image_embeds and rewards
    (two fp32 evaluations: rtol / atol 1e-5 on the features, 1e-4 on the reward, as for the dino oracle)"""
    from consolver_amd.synth import synthetic_clip_vision_state_dict
    gen = _generator()
    g = golden["clip_reward"]
    assert [int(v) for v in g["cfg"]] == [gen.REDUCED[k] for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size",
                                                                   "patch_size", "projection_dim")]
    sd = synthetic_clip_vision_state_dict(co.clip_manifest(REDUCED), seed=int(g["weight_seed"]))
    orc = co.ClipVisionOracle(sd, REDUCED)
    assert [c[0] for c in gen.CASES] == [str(c) for c in g["cases"]] and len(gen.CASES) == 4
    for i, (name, h, w, dtype) in enumerate(gen.CASES):
        crops, pv = co.preprocess(torch.stack(gen.case_images(i, h, w, dtype)))
        assert crops.dtype == np.uint8 and np.array_equal(crops[0], g[f"{name}_crop"]), name
        if i == 0:
            assert np.array_equal(pv[0].numpy(), g[f"{name}_pixel_values"])
        assert float(pv.abs().max()) < 4.0                       # the magnitude bound the fp16 front-end tolerance (2^-10) rests on
        emb = orc(pv)
        np.testing.assert_allclose(emb.numpy(), g[f"{name}_embeds"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(co.clip_reward(emb[:1], emb[1:]).numpy(), g[f"{name}_reward"], rtol=0, atol=1e-4)


def test_manifest_loaders_and_create_rejections():
    """cs_clipv_create is host code: no GPU is touched.  303,966,208 = transformers' CLIPVisionModelWithProjection at the ViT-L/14 config (392 tensors)."""
    from consolver_amd.reward_model import (HipCLIPVisionModel, ClipImageProcessor, HipDinov2Model, DinoImageProcessor, load_reward_model, load_clip_reward)
    m = HipCLIPVisionModel(device="cpu")
    man = m.manifest()
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "clip_vit_l14_vision_manifest.json")))
    assert [[k, list(s)] for k, s in man] == want["tensors"] and len(man) == 392
    assert sum(int(np.prod(s)) for _, s in man) == want["params"] == 303966208
    assert man == co.clip_manifest()
    assert ("vision_model.pre_layrnorm.weight", (1024,)) in man and man[-1] == ("visual_projection.weight", (768, 1024))
    assert m.patch_cols == 640 and m.num_tokens == 257
    assert abs(m.flops(1) / co.config_flops() - 1.0) < 0.01 and 150e9 < m.flops(1) < 170e9
    assert m.flops(3) == pytest.approx(3 * m.flops(1), rel=1e-12)
    model, proc = load_reward_model("clip", device="cpu")
    assert isinstance(model, HipCLIPVisionModel) and isinstance(proc, ClipImageProcessor)
    assert isinstance(load_clip_reward("cpu")[0], HipCLIPVisionModel)
    assert proc.constants() == (224, 224, 1 / 255, (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
    assert proc.resample == 3 and co.PROCESSOR == dict(shortest_edge=224, crop_size=224, rescale_factor=1 / 255, image_mean=proc.image_mean, image_std=proc.image_std)
    # the dino pair is what it was
    dm, dp = load_reward_model("dino", device="cpu")
    assert isinstance(dm, HipDinov2Model) and type(dp) is DinoImageProcessor and dp.constants()[0] == 256
    for rt in ("depth", "inception", "segmentation", "llava", "qwen_vl"):
        with pytest.raises(NotImplementedError):
            load_reward_model(rt)
    with pytest.raises(RuntimeError, match="dim 64"):
        HipCLIPVisionModel(dict(hidden_size=128, num_attention_heads=4), device="cpu")                       # heads of 64 only
    with pytest.raises(RuntimeError, match="image_size"):
        HipCLIPVisionModel(dict(image_size=336), device="cpu")                                               # crop 224 != image 336: no position interpolation
    with pytest.raises(RuntimeError, match="multiples of 128"):
        HipCLIPVisionModel(dict(hidden_size=192, num_attention_heads=3), device="cpu")
    with pytest.raises(RuntimeError, match="multiples of 128"):
        HipCLIPVisionModel(dict(intermediate_size=4000), device="cpu")
    with pytest.raises(RuntimeError, match="image_std"):
        HipCLIPVisionModel(device="cpu", processor=ClipImageProcessor(image_std=(0.2, 0.0, 0.2)))
    assert HipCLIPVisionModel(SMALL, device="cpu").manifest() == co.clip_manifest(SMALL)


def test_load_state_dict_rejects_missing_and_misshapen_tensors():
    from consolver_amd.reward_model import HipCLIPVisionModel
    from consolver_amd.synth import synthetic_clip_vision_state_dict
    m = HipCLIPVisionModel(SMALL, device="cpu")
    sd = synthetic_clip_vision_state_dict(m.manifest(), seed=1)
    missing = dict(sd)
    del missing["vision_model.pre_layrnorm.bias"]
    with pytest.raises(KeyError):
        m.load_state_dict(missing)
    bad = dict(sd)
    bad["visual_projection.weight"] = torch.zeros(128, 8)               # transposed
    with pytest.raises(ValueError):
        m.load_state_dict(bad)
    bad = dict(sd)
    bad["vision_model.embeddings.position_embedding.weight"] = torch.zeros(1, 257, 128)        # the dino layout
    with pytest.raises(ValueError):
        m.load_state_dict(bad)


def test_full_clip_model_state_dict_passes_the_name_and_shape_checks():
    """a CLIPModel state dict (text tower, text projection, logit scale and position_ids buffers next to the vision part): every tensor of the manifest is
    found and accepted by cs_clipv_set_weight, the extra keys are ignored.  Host only: up to (not including) cs_clipv_finalize, which uploads."""
    import ctypes as C
    from consolver_amd import _lib as L
    from consolver_amd.reward_model import HipCLIPVisionModel
    from consolver_amd.synth import synthetic_clip_vision_state_dict
    m = HipCLIPVisionModel(SMALL, device="cpu")
    sd = synthetic_clip_vision_state_dict(m.manifest(), seed=2)
    sd.update({"logit_scale": torch.tensor(2.6592), "text_projection.weight": torch.zeros(8, 64), "text_model.embeddings.token_embedding.weight": torch.zeros(50, 64),
               "text_model.embeddings.position_ids": torch.arange(77)[None], "vision_model.embeddings.position_ids": torch.arange(257)[None],
               "text_model.final_layer_norm.weight": torch.ones(64)})
    want = dict(m.manifest())
    assert not [k for k in want if k not in sd]
    lib = L.lib()
    for name, shape in want.items():
        t = sd[name].detach().to(torch.float32).contiguous()
        assert tuple(t.shape) == shape, name
        L.check(lib.cs_clipv_set_weight(m._h, name.encode(), C.c_void_p(t.data_ptr()), (C.c_int64 * len(shape))(*shape), len(shape)))
    # a name outside the manifest is an error of the C ABI (the Python loader never sends one)
    t = sd["text_projection.weight"]
    assert lib.cs_clipv_set_weight(m._h, b"text_projection.weight", C.c_void_p(t.data_ptr()), (C.c_int64 * 2)(8, 64), 2) != 0
    assert int(lib.cs_clipv_num_weights(m._h)) == len(want) == 5 + 16 + 3


def test_dispatchers_reject_what_is_not_built():
    """host-side argument checks of the dispatcher (no GPU): the eager transformers path is not implemented; the other backbones still raise"""
    from consolver_amd import ppo
    from consolver_amd.reward_model import calculate_clip_reward
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError):
        ppo.calculate_reward("clip", None, None, x, x, "cpu")
    with pytest.raises(NotImplementedError):
        calculate_clip_reward(object(), None, x, x, "cpu")
    for rt in ("depth", "inception", "segmentation", "llava", "qwen_vl"):
        with pytest.raises(NotImplementedError):
            ppo.calculate_reward(rt, None, None, x, x, "cpu")


def test_synthetic_weights_follow_the_recipe():
    from consolver_amd.synth import synthetic_clip_vision_state_dict
    sd = synthetic_clip_vision_state_dict(co.clip_manifest(dict(REDUCED, num_hidden_layers=1)), seed=3)
    assert abs(float(sd["vision_model.encoder.layers.0.mlp.fc2.weight"].std()) - 512 ** -0.5) < 0.1 * 512 ** -0.5
    assert abs(float(sd["vision_model.embeddings.patch_embedding.weight"].std()) - 588 ** -0.5) < 0.1 * 588 ** -0.5
    assert abs(float(sd["vision_model.embeddings.position_embedding.weight"].std()) - 0.5) < 0.05
    assert abs(float(sd["vision_model.pre_layrnorm.weight"].mean()) - 1.0) < 0.05 and abs(float(sd["vision_model.post_layernorm.weight"].mean()) - 1.0) < 0.05
    assert float(sd["vision_model.encoder.layers.0.self_attn.q_proj.bias"].abs().max()) < 0.3
    again = synthetic_clip_vision_state_dict(co.clip_manifest(dict(REDUCED, num_hidden_layers=1)), seed=3)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
