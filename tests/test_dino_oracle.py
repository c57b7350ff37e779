"""CPU checks behind the DINOv2 reward (reward_type "dino"): tests/vit_oracle.py against the installed PIL / transformers, the committed fixture against
its generator, the weight manifest against the published parameter count, and the compiler's output for the new kernels (no scratch)."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import vit_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
REDUCED = dict(hidden_size=128, num_hidden_layers=3, num_attention_heads=2)


def _generator():
    spec = importlib.util.spec_from_file_location("make_dino_golden", os.path.join(ROOT, "tools", "make_dino_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("h,w,dtype", [(512, 512, torch.float16), (512, 512, torch.float32), (1024, 1024, torch.float16), (1024, 1024, torch.float32),
                                       (512, 768, torch.float32), (700, 512, torch.float16), (128, 128, torch.float16)])
def test_integer_resize_is_pil_and_pixel_values_are_the_processors(h, w, dtype):
    """fixture sizes (512^2, 1024^2), two non-square sizes (the processor's output-size rule) and an upscale (the reduced VAE's 128^2 images)"""
    Image = pytest.importorskip("PIL.Image")
    pytest.importorskip("transformers")
    u8 = vo.to_uint8_hwc(vo.synthetic_image(h * 3 + w, h, w, dtype))
    nh, nw = vo.resize_output_size(h, w)
    assert np.array_equal(vo.pil_bicubic_resize(u8, nh, nw), np.asarray(Image.fromarray(u8).resize((nw, nh), Image.BICUBIC)))
    gen = _generator()
    pil = Image.fromarray(u8)
    want = gen.hf_processor()(images=[pil], return_tensors="pt")["pixel_values"][0].numpy()
    want_u8 = gen.hf_processor()(images=[pil], return_tensors="pt", do_rescale=False, do_normalize=False)["pixel_values"][0].numpy()
    crop = vo.crop_uint8(u8)
    assert crop.dtype == np.uint8 and np.array_equal(crop, want_u8)
    got = vo.normalize_uint8(crop)
    assert got.dtype == np.float32 and float(np.abs(got - want).max()) == 0.0
    assert float(np.abs(got).max()) < 2.65              # the magnitude bound the fp16 front-end tolerance (2^-10) rests on


def test_to_uint8_truncates_in_the_tensors_dtype():
    x = torch.tensor([0.0, 0.5, 0.999, 1.0, 0.1234, 0.7071]).view(1, 1, 6).expand(3, 1, 6)
    for dt in (torch.float16, torch.float32):
        got = vo.to_uint8_hwc(x.to(dt))[0, :, 0]
        want = [int(float((torch.tensor(v, dtype=dt) * 255))) for v in x[0, 0].to(dt).tolist()]
        assert got.tolist() == want
    assert vo.to_uint8_hwc(torch.full((3, 1, 1), 0.999, dtype=torch.float16))[0, 0, 0] == 254       # fp16: 0.999 -> 0.9990234 * 255 = 254.75 -> 254


def test_encoder_oracle_matches_transformers_dinov2():
    pytest.importorskip("transformers")
    from consolver_amd.synth import synthetic_dinov2_state_dict
    gen = _generator()
    sd = synthetic_dinov2_state_dict(vo.dinov2_manifest(REDUCED), seed=5)
    model = gen.hf_model(dict(gen.REDUCED), sd)
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == vo.dinov2_manifest(REDUCED)
    x = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = model(pixel_values=x).last_hidden_state
    got = vo.Dinov2Oracle(sd, REDUCED)(x)
    assert torch.allclose(got[:, 0], want[:, 0], rtol=1e-5, atol=1e-5)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-4)
    # 518-pixel input: the position table as is (no interpolation), as transformers does
    x = torch.randn(1, 3, 518, 518, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = model(pixel_values=x).last_hidden_state[:, 0]
    assert torch.allclose(vo.Dinov2Oracle(sd, REDUCED).cls(x), want, rtol=1e-5, atol=1e-5)


def test_fixture_regenerates(golden):
    """integers and the processor's fp32 output exactly; results of fp32 matmuls to round-off (the BLAS blocking may differ between hosts); the bf16
    comparator within two bf16 ulps of its largest value"""
    pytest.importorskip("transformers")
    pytest.importorskip("PIL.Image")
    g = golden["dino_reward"]
    fx = _generator().build_fixture()
    assert sorted(fx) == sorted(g.files)
    for k in g.files:
        a, b = np.asarray(fx[k]), np.asarray(g[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k.endswith("_bf16"):
            assert float(np.abs(a - b).max()) <= 2 * 2.0 ** -8 * float(np.abs(b).max()), k
        elif a.dtype == np.float32 and not k.endswith("_pixel_values"):
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-5, err_msg=k)
        else:
            assert np.array_equal(a, b), k


def test_oracle_reproduces_the_fixture_without_transformers(golden):
    """what the GPU suite relies on: seeded images and weights + tests/vit_oracle.py give the fixture's crops, features and rewards"""
    from consolver_amd.synth import synthetic_dinov2_state_dict
    gen = _generator()
    g = golden["dino_reward"]
    sd = synthetic_dinov2_state_dict(vo.dinov2_manifest(REDUCED), seed=int(g["weight_seed"]))
    orc = vo.Dinov2Oracle(sd, REDUCED)
    for i, (name, h, w, dtype) in enumerate(gen.CASES):
        crops, pv = vo.preprocess(torch.stack(gen.case_images(i, h, w, dtype)))
        assert np.array_equal(crops[0], g[f"{name}_crop"])
        if f"{name}_pixel_values" in g.files:
            assert np.array_equal(pv[0].numpy(), g[f"{name}_pixel_values"])
        cls = orc.cls(pv)
        np.testing.assert_allclose(cls.numpy(), g[f"{name}_cls"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(vo.dino_reward(cls[:1], cls[1:]).numpy(), g[f"{name}_reward"], rtol=0, atol=1e-4)


def test_manifest_is_the_published_dinov2_base():
    """cs_vit_create is host code: no GPU is touched.  86,580,480 = the published facebook/dinov2-base parameter count (mask_token included)."""
    from consolver_amd.reward_model import HipDinov2Model, load_reward_model, DinoImageProcessor
    m = HipDinov2Model(device="cpu")
    man = m.manifest()
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "dinov2_base_manifest.json")))
    assert [[k, list(s)] for k, s in man] == want["tensors"]
    assert sum(int(np.prod(s)) for _, s in man) == want["params"] == 86580480
    assert man == vo.dinov2_manifest()
    assert ("embeddings.mask_token", (1, 768)) in man
    assert m.patch_cols == 640 and m.num_tokens == 257
    assert abs(m.flops(1) / 1e9 - 46.3) < 0.5                   # 46 GFLOP per image
    model, proc = load_reward_model("dino", device="cpu")
    assert isinstance(model, HipDinov2Model) and isinstance(proc, DinoImageProcessor)
    assert proc.constants() == (256, 224, 1 / 255, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    assert load_reward_model("image_psnr") == (None, None)
    with pytest.raises(NotImplementedError):
        load_reward_model("depth")
    with pytest.raises(ValueError):
        load_reward_model("nope")
    with pytest.raises(RuntimeError):
        HipDinov2Model(dict(hidden_size=100, num_attention_heads=2), device="cpu")           # heads of 64 only


def test_vit_kernels_do_not_spill(tmp_path):
    """every kernel of vit_ops.hip: 0 bytes of scratch on the cross-compiled assembly"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "vit_ops.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-x", "hip", os.path.join(ROOT, "consolver_amd", "csrc", "vit_ops.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    names = set()
    for b in blocks:
        name = b.split("\n")[0].split()[0]
        names.add(name)
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
    for k in ("vit_hresize_kernel", "vit_vresize_patch_kernel", "vit_tokens_kernel", "gelu_erf_kernel", "vit_cls_layer_norm_kernel", "cosine_reward_kernel"):
        assert any(k in n for n in names), (k, names)
    assert len(names) >= 7                                       # the horizontal pass is built for fp16 and fp32 inputs


def test_unmasked_head64_attention_does_not_spill(tmp_path):
    """the attention instantiation the encoder adds (attn_kernel<f16, 64, 2>, no mask, no bias): 0 bytes of scratch, two workgroups per CU (launch_bounds(256, 2))"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "attention.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-x", "hip", os.path.join(ROOT, "consolver_amd", "csrc", "attention.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:] if "attn_kernelIDF16_Li64ELi2ELb0ELb0ELb0E" in b.split("\n")[0]]
    assert len(blocks) == 1, [b.split("\n")[0] for b in blocks]
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blocks[0]).group(1))
    occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blocks[0]).group(1))
    assert scratch == 0 and occ >= 2, (scratch, occ)
