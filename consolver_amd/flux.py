"""HIP-backed FLUX.1-Kontext DiT (``FluxTransformer2DModel`` stand-in) + the latent layout helpers and
the edit sampling loop of the FLUX side of the hot path.

Mirrors what the reference drives (edit_ppo/pipeline.py:1074-1140, edit_ppo/denoise_diffusion.py:96-160):

    x_in = cat([latents, image_latents], dim=1)
    v    = transformer(hidden_states=x_in, timestep=t/1000, guidance=g, pooled_projections=pooled,
                       encoder_hidden_states=t5, txt_ids=txt_ids, img_ids=ids, return_dict=False)[0][:, :L]
    latents = scheduler.step(v, t, latents, return_dict=False)[0]

Weights load by their diffusers state-dict names.  There is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .tables import calculate_shift

FLUX_KONTEXT_CONFIG = dict(in_channels=64, num_layers=19, num_single_layers=38, num_heads=24, head_dim=128,
                           joint_attention_dim=4096, pooled_projection_dim=768, guidance_embeds=True,
                           axes_dims_rope=(16, 56, 56), dtype=torch.bfloat16)


class _Config(dict):
    """dict with attribute access (``pipe.transformer.config.in_channels``, edit_ppo/denoise_diffusion.py:50,69)"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


# ---- layout helpers (pure index shuffles, edit_ppo/pipeline.py:574-611) ------------------------------------------
def prepare_latent_image_ids(height, width, first=0.0):
    ids = np.zeros((height, width, 3), np.float32)
    ids[..., 0] = first
    ids[..., 1] += np.arange(height, dtype=np.float32)[:, None]
    ids[..., 2] += np.arange(width, dtype=np.float32)[None, :]
    return ids.reshape(height * width, 3)


def pack_latents(latents):
    """[B, C, H, W] -> [B, (H/2)(W/2), 4C] (2x2 patches)."""
    B, Cc, H, W = latents.shape
    x = latents.view(B, Cc, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(B, (H // 2) * (W // 2), Cc * 4)


def unpack_latents(latents, height, width, vae_scale_factor=8):
    B, _, ch = latents.shape
    h = 2 * (int(height) // (vae_scale_factor * 2))
    w = 2 * (int(width) // (vae_scale_factor * 2))
    x = latents.view(B, h // 2, w // 2, ch // 4, 2, 2).permute(0, 3, 1, 4, 2, 5)
    return x.reshape(B, ch // 4, h, w)


def rope_tables(ids, axes_dims, theta=10000.0):
    """cos/sin [S, head_dim/2] fp32 of the 3-axis rotary embedding (float64 angles like diffusers)."""
    cos, sin = [], []
    ids = np.asarray(ids, np.float64)
    for i, d in enumerate(axes_dims):
        freqs = 1.0 / (theta ** (np.arange(0, d, 2, dtype=np.float64)[: d // 2] / d))
        ang = np.outer(ids[:, i], freqs)
        cos.append(np.cos(ang)); sin.append(np.sin(ang))
    return np.concatenate(cos, 1).astype(np.float32), np.concatenate(sin, 1).astype(np.float32)


class HipFluxTransformer2DModel:
    is_consolver_hip = True
    broadcasts_latent_rows = True        # __call__ takes R latent rows beside G * R text rows (cs_flux_forward_joint_rows)

    RESIDUAL_MODES = {"plain": 0, "bf16": 0, "f16": 0, "split": 1, "bf16x2": 1, "f16x2": 1}

    def __init__(self, config=None, device="cuda:0", residual="split"):
        """``residual``: storage of the hidden-state stream between kernels (include/consolver_hip.h, cs_flux_set_residual_precision): ``"split"`` (default: hi + lo
        planes of the model dtype, fp32-class adds along the 57-block stream) or ``"plain"`` (one plane: the reference bf16 pipeline's own arithmetic class)."""
        cfg = _Config(FLUX_KONTEXT_CONFIG)
        cfg.update(config or {})
        self.config = cfg
        self.dtype = cfg["dtype"]
        self.device = torch.device(device)
        c = L.CsFluxConfig()
        c.in_channels, c.num_layers, c.num_single_layers = cfg["in_channels"], cfg["num_layers"], cfg["num_single_layers"]
        c.num_heads, c.head_dim = cfg["num_heads"], cfg["head_dim"]
        c.joint_attention_dim, c.pooled_projection_dim = cfg["joint_attention_dim"], cfg["pooled_projection_dim"]
        c.guidance_embeds = int(cfg["guidance_embeds"])
        for i in range(3):
            c.axes_dims_rope[i] = cfg["axes_dims_rope"][i]
        c.dtype = L.dtype_code(self.dtype)
        h = C.c_void_p()
        L.check(L.lib().cs_flux_create(C.byref(c), C.byref(h)))
        self._h = h
        self._finalized = False
        self._ws = None
        self._ws_key = None
        self._rope = {}
        self.residual = "split"
        self._out_f32 = False
        if residual != "split":
            self.set_residual_precision(residual)

    def set_residual_precision(self, mode):
        if mode not in self.RESIDUAL_MODES:
            raise ValueError(f"residual must be one of {sorted(self.RESIDUAL_MODES)}, got {mode!r}")
        L.check(L.lib().cs_flux_set_residual_precision(self._h, self.RESIDUAL_MODES[mode]))
        self.residual = "split" if self.RESIDUAL_MODES[mode] else "plain"
        self._ws, self._ws_key = None, None          # the workspace size depends on the mode
        return self

    def __del__(self):
        L.destroy("flux", self)

    def manifest(self):
        return L.manifest("flux", self._h, cap=2)

    def set_weight(self, name, tensor):
        """tensor: torch tensor (cpu or cuda) of the manifest shape; converted to the model dtype."""
        t = tensor.detach().to(self.dtype).contiguous()
        sh = (C.c_int64 * t.dim())(*t.shape)
        L.check(L.lib().cs_flux_set_weight(self._h, name.encode(), C.c_void_p(t.data_ptr()), int(t.is_cuda), sh, t.dim()))

    def load_state_dict(self, sd, strict=True):
        want = dict(self.manifest())
        missing = [k for k in want if k not in sd]
        if missing and strict:
            raise KeyError(f"missing {len(missing)} tensors, e.g. {missing[:3]}")
        for name, shape in want.items():             # every shape before the first device allocation
            if tuple(sd[name].shape) != shape:
                raise ValueError(f"{name}: shape {tuple(sd[name].shape)} != {shape}")
        torch.cuda.set_device(self.device)
        for name in want:
            self.set_weight(name, sd[name])
        return self.finalize()

    def finalize(self):
        torch.cuda.set_device(self.device)
        L.check(L.lib().cs_flux_finalize(self._h))
        self._finalized = True
        return self

    def flops(self, batch, txt_len, img_len):
        return float(L.lib().cs_flux_flops(self._h, batch, txt_len, img_len))

    def _rope_dev(self, txt_ids, img_ids):
        # same id objects as the previous call (the edit loop passes them unchanged every step): no D2H copy, no sync
        last = getattr(self, "_rope_last", None)
        ver = lambda t: t._version if torch.is_tensor(t) else 0                     # (in-place edits of either id tensor invalidate the cache)
        if last is not None and last[0] is txt_ids and last[1] is img_ids and last[2] == (ver(txt_ids), ver(img_ids)):
            return last[3]
        out = self._rope_from_values(txt_ids, img_ids)
        self._rope_last = (txt_ids, img_ids, (ver(txt_ids), ver(img_ids)), out)
        return out

    def _rope_from_values(self, txt_ids, img_ids):
        ids = np.concatenate([np.asarray(txt_ids.detach().float().cpu() if torch.is_tensor(txt_ids) else txt_ids, np.float32),
                              np.asarray(img_ids.detach().float().cpu() if torch.is_tensor(img_ids) else img_ids, np.float32)], 0)
        key = ids.tobytes()
        if key not in self._rope:
            cos, sin = rope_tables(ids, self.config["axes_dims_rope"])
            self._rope = {key: (torch.from_numpy(cos).to(self.device), torch.from_numpy(sin).to(self.device))}
        return self._rope[key]

    def __call__(self, hidden_states, timestep, guidance=None, pooled_projections=None, encoder_hidden_states=None,
                 txt_ids=None, img_ids=None, joint_attention_kwargs=None, return_dict=False, out=None, image_latents=None,
                 out_dtype=None, **_ignored):
        """the reference's call (edit_ppo/pipeline.py:1087-1097): ``hidden_states`` [B, I, 64] (the caller's
        ``cat([latents, image_latents], 1)``) -> [B, I, 64].

        Extension used by the native edit loop: ``image_latents=`` [B, I2, 64] passes the Kontext reference-image
        tokens as a second buffer -- the joint sequence [hidden_states | image_latents] is read in place (no per-step
        ``torch.cat``) and the result holds the rows of ``hidden_states`` only ([B, I, 64], i.e. the reference's
        ``noise_pred[:, :latents.size(1)]`` without the slice copy); ``img_ids`` cover I + I2 tokens.
        ``out_dtype=torch.float32`` (split stream only; cs_flux_set_output_dtype): the prediction as the unrounded sum of the output head's two planes instead of
        their hi plane in the model dtype.
        Row broadcast (true classifier-free guidance: [prompt | negative prompt] rows of the same latents): ``hidden_states`` / ``image_latents`` may hold R rows
        beside ``encoder_hidden_states`` / ``pooled_projections`` of G * R rows; batch row b reads latent row b % R and the result is [G * R, I, 64], bit-identical
        to the call on ``hidden_states.repeat(G, 1, 1)``.  A row count that is not a multiple of R raises ValueError."""
        if not self._finalized:
            raise RuntimeError("weights not loaded")
        L.require_cuda(hidden_states, "hidden_states")
        hs = hidden_states.to(self.dtype).contiguous()
        enc = L.require_cuda(encoder_hidden_states, "encoder_hidden_states").to(self.dtype).contiguous()
        R, I, _ = hs.shape
        B, T = enc.shape[0], enc.shape[1]
        if R <= 0 or B % R:
            raise ValueError(f"encoder_hidden_states has {B} rows, not a multiple of the {R} rows of hidden_states")
        il, I2 = None, 0
        if image_latents is not None:
            il = L.require_cuda(image_latents, "image_latents").to(self.dtype).contiguous()
            if il.shape[0] != R or il.shape[2] != hs.shape[2]:
                raise ValueError("image_latents must be [B, I2, in_channels] with the rows of hidden_states")
            I2 = il.shape[1]
        pooled = L.require_cuda(pooled_projections, "pooled_projections").to(torch.float32).contiguous()
        if pooled.shape[0] != B:
            raise ValueError(f"pooled_projections has {pooled.shape[0]} rows, encoder_hidden_states {B}")
        t = timestep.to(device=hs.device, dtype=torch.float32).reshape(-1) if torch.is_tensor(timestep) else \
            torch.full((B,), float(timestep), dtype=torch.float32, device=hs.device)
        if t.numel() == 1:
            t = t.expand(B).contiguous()
        g = None
        if self.config["guidance_embeds"]:
            if guidance is None:
                raise ValueError("guidance is required (guidance_embeds=True)")
            g = guidance.to(device=hs.device, dtype=torch.float32).reshape(-1)
            if g.numel() == 1:
                g = g.expand(B).contiguous()
        if t.numel() != B or (g is not None and g.numel() != B):
            raise ValueError(f"timestep and guidance must hold 1 or {B} values (one per row of encoder_hidden_states)")
        # (an `expand`ed scalar has B elements behind ONE address: the kernels read B consecutive floats)
        t, g = t.contiguous(), (g.contiguous() if g is not None else None)
        cos, sin = self._rope_dev(txt_ids, img_ids)
        if cos.shape[0] != T + I + I2:
            raise ValueError(f"ids cover {cos.shape[0]} tokens, expected {T + I + I2}")
        want_f32 = out_dtype == torch.float32 or (out_dtype is None and out is not None and out.dtype == torch.float32)
        if out_dtype not in (None, torch.float32, self.dtype):
            raise ValueError(f"out_dtype must be the model dtype {self.dtype} or torch.float32, got {out_dtype}")
        if want_f32 != self._out_f32:
            L.check(L.lib().cs_flux_set_output_dtype(self._h, L.CS_F32 if want_f32 else L.dtype_code(self.dtype)))
            self._out_f32 = want_f32
        key = (B, T, I + I2, want_f32)
        if self._ws_key != key:
            n = int(L.lib().cs_flux_workspace_bytes(self._h, B, T, I + I2))
            self._ws = torch.empty(n, dtype=torch.uint8, device=hs.device)
            self._ws_key = key
        odt = torch.float32 if want_f32 else self.dtype
        if out is None:
            out = torch.empty(B, I, self.config["in_channels"], dtype=odt, device=hs.device)
        elif out.dtype != odt or tuple(out.shape) != (B, I, self.config["in_channels"]) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {odt} tensor of shape {(B, I, self.config['in_channels'])}")
        if il is None and R == B:
            L.check(L.lib().cs_flux_forward(self._h, L.ptr(hs), B, I, L.ptr(enc), T, L.ptr(pooled), L.ptr(t), L.ptr(g), L.ptr(cos),
                                            L.ptr(sin), L.ptr(out), L.ptr(self._ws), self._ws.numel(), L.stream_ptr(hs.device)))
        else:
            L.check(L.lib().cs_flux_forward_joint_rows(self._h, L.ptr(hs), I, L.ptr(il), I2, R, B, L.ptr(enc), T, L.ptr(pooled), L.ptr(t),
                                                       L.ptr(g), L.ptr(cos), L.ptr(sin), L.ptr(out), L.ptr(self._ws), self._ws.numel(),
                                                       L.stream_ptr(hs.device)))
        if return_dict:
            return {"sample": out}
        return (out,)


def true_cfg_combine(pos, neg, scale, out_dtype=None, out=None):
    """``neg + scale * (pos - neg)`` rounded once to ``out_dtype`` (cs_true_cfg_combine; edit_ppo/pipeline.py:1115): pos / neg fp32 with any of
    fp32 / fp16 / bf16 out, or a 16-bit dtype in and the same out (the default).  ``out`` may be ``pos`` or ``neg`` when the dtypes are equal."""
    L.require_cuda(pos, "pos"); L.require_cuda(neg, "neg")
    if pos.shape != neg.shape or pos.dtype != neg.dtype:
        raise ValueError(f"pos {tuple(pos.shape)} {pos.dtype} and neg {tuple(neg.shape)} {neg.dtype} differ")
    pos, neg = pos.contiguous(), neg.contiguous()
    if out is None:
        out = torch.empty(pos.shape, dtype=out_dtype or pos.dtype, device=pos.device)
    elif out.shape != pos.shape or not out.is_contiguous() or (out_dtype is not None and out.dtype != out_dtype):
        raise ValueError("out must be a contiguous tensor of the inputs' shape and of out_dtype")
    L.check(L.lib().cs_true_cfg_combine(L.ptr(pos), L.ptr(neg), L.dtype_code(pos.dtype), float(scale), L.ptr(out), L.dtype_code(out.dtype),
                                        pos.numel(), L.stream_ptr(pos.device)))
    return out


class FluxKontextSamplingEngine:
    """The FLUX edit loop (edit_ppo/pipeline.py:1009-1140 minus encoders / VAE): sigma schedule with the
    resolution-dependent shift, [latents | image_latents] joint input, and the scheduler's update: ``FMPPOScheduler`` or any scheduler of
    the same protocol whose ``step(..., return_dict=False)`` returns at least ``(prev_sample,)`` (scheduling_fm.py, baselines.py)."""

    def __init__(self, transformer, scheduler, guidance_scale=2.5):
        self.transformer, self.scheduler, self.guidance_scale = transformer, scheduler, float(guidance_scale)

    @torch.no_grad()
    def generate(self, latents, image_latents, prompt_embeds, pooled_prompt_embeds, latent_hw, image_hw=None,
                 num_inference_steps=8, record=False, negative_prompt_embeds=None, negative_pooled_prompt_embeds=None, true_cfg_scale=1.0,
                 true_cfg_dtype=None):
        """latents / image_latents: packed [B, L, 64]; latent_hw = (H/2, W/2) of the packed grid.
        record=True additionally returns the PPO trajectory records of edit_ppo/denoise_diffusion.py:152-172
        (conds{x, epsilon}, probs, actions, masks; steps i > 0 only).

        True classifier-free guidance (edit_ppo/pipeline.py:937-940, 1100-1115) runs when ``true_cfg_scale > 1`` AND both negative tensors are given;
        otherwise the loop is the unguided one, forward rows included.  Per step: the prompt and the negative-prompt prediction -- one forward of 2 B text
        rows over the B latent rows on a transformer that ``broadcasts_latent_rows``, two forwards on any other callable -- then
        ``v = neg + true_cfg_scale * (pos - neg)`` rounded once to the latents' dtype (cs_true_cfg_combine), then the unchanged ``scheduler.step``;
        the recorded ``epsilon`` history holds the combined v.  ``true_cfg_dtype``: dtype of the two predictions entering the combine, ``torch.float32``
        (the DiT head's unrounded value; HIP model on the split stream only, else ValueError) or the latents' dtype; None = fp32 where available."""
        dev = latents.device
        B, Lq, _ = latents.shape
        sch = self.scheduler
        tr = self.transformer
        do_true_cfg = float(true_cfg_scale) > 1.0 and negative_prompt_embeds is not None and negative_pooled_prompt_embeds is not None
        if do_true_cfg:
            f32_ok = bool(getattr(tr, "is_consolver_hip", False)) and getattr(tr, "residual", None) == "split"
            if true_cfg_dtype is None:
                true_cfg_dtype = torch.float32 if f32_ok else latents.dtype
            if true_cfg_dtype not in (torch.float32, latents.dtype):
                raise ValueError(f"true_cfg_dtype must be torch.float32 or the latents' dtype {latents.dtype}, got {true_cfg_dtype}")
            if true_cfg_dtype == torch.float32 and latents.dtype != torch.float32 and not f32_ok:
                raise ValueError("true_cfg_dtype=torch.float32 needs a transformer with an fp32 output: HipFluxTransformer2DModel on the split stream")
            if negative_prompt_embeds.shape[0] != B or negative_pooled_prompt_embeds.shape[0] != B:
                raise ValueError(f"negative_prompt_embeds / negative_pooled_prompt_embeds must have the {B} rows of the latents")
            okw = {"out_dtype": torch.float32} if true_cfg_dtype == torch.float32 and latents.dtype != torch.float32 else {}
            # one forward for both branches: the text rows [prompt | negative] over the SAME latent rows (needs equal text lengths)
            one_forward = bool(getattr(tr, "broadcasts_latent_rows", False)) and negative_prompt_embeds.shape[1:] == prompt_embeds.shape[1:]
            if one_forward:
                enc2 = torch.cat([prompt_embeds, negative_prompt_embeds.to(prompt_embeds.dtype)], 0)
                pooled2 = torch.cat([pooled_prompt_embeds, negative_pooled_prompt_embeds.to(pooled_prompt_embeds.dtype)], 0)
        sigmas = np.linspace(1.0, 1 / num_inference_steps, num_inference_steps)
        mu = calculate_shift(Lq, sch.config.get("base_image_seq_len", 256), sch.config.get("max_image_seq_len", 4096),
                             sch.config.get("base_shift", 0.5), sch.config.get("max_shift", 1.15))
        sch.set_timesteps(sigmas=sigmas, mu=mu, device=dev)
        sch.set_begin_index(0)
        ids = prepare_latent_image_ids(*latent_hw)
        if image_latents is not None:
            ids = np.concatenate([ids, prepare_latent_image_ids(*(image_hw or latent_hw), first=1.0)], 0)
        txt_ids = np.zeros((prompt_embeds.shape[1], 3), np.float32)
        guidance = torch.full([B], self.guidance_scale, device=dev, dtype=torch.float32)
        if do_true_cfg:
            neg_txt_ids = txt_ids if negative_prompt_embeds.shape[1] == prompt_embeds.shape[1] else np.zeros((negative_prompt_embeds.shape[1], 3), np.float32)
            guidance2 = torch.full([2 * B], self.guidance_scale, device=dev, dtype=torch.float32)
        # timestep / 1000 in the model dtype like the reference (`t.expand(B).to(dtype)` then `/ 1000`, pipeline.py:1084-1089)
        sig = (sch.timesteps.to(latents.dtype) / 1000).to(torch.float32)
        x = latents
        rec = dict(x=[], epsilon=[], probs=[], actions=[], masks=[])
        # a policy-free scheduler (scheduling_fm.py, baselines.py) steps to (prev_sample,) and has nothing to record
        has_policy = getattr(sch, "factor_net", None) is not None
        if record and not has_policy:
            raise ValueError(f"record=True needs a scheduler with a policy; {type(sch).__name__} has none")
        keeps_conds = hasattr(sch, "record_conds")
        if keeps_conds:
            prev_record = sch.record_conds
            sch.record_conds = bool(record)
        try:
            for i, t in enumerate(sch.timesteps):
                # [latents | image_latents] is read in place by the embedder; v holds the latent rows only
                if not do_true_cfg:
                    v = self.transformer(x, sig[i:i + 1].expand(B), guidance=guidance, pooled_projections=pooled_prompt_embeds,
                                         encoder_hidden_states=prompt_embeds, txt_ids=txt_ids, img_ids=ids, image_latents=image_latents)[0]
                else:
                    if one_forward:
                        both = tr(x, sig[i:i + 1].expand(2 * B), guidance=guidance2, pooled_projections=pooled2, encoder_hidden_states=enc2,
                                  txt_ids=txt_ids, img_ids=ids, image_latents=image_latents, **okw)[0]
                        pos, neg = both[:B], both[B:]
                    else:
                        pos = tr(x, sig[i:i + 1].expand(B), guidance=guidance, pooled_projections=pooled_prompt_embeds,
                                 encoder_hidden_states=prompt_embeds, txt_ids=txt_ids, img_ids=ids, image_latents=image_latents, **okw)[0]
                        neg = tr(x, sig[i:i + 1].expand(B), guidance=guidance, pooled_projections=negative_pooled_prompt_embeds,
                                 encoder_hidden_states=negative_prompt_embeds, txt_ids=neg_txt_ids, img_ids=ids, image_latents=image_latents, **okw)[0]
                    # (a fresh tensor per step: the scheduler's history keeps a reference to its model output)
                    v = true_cfg_combine(pos, neg, true_cfg_scale, out_dtype=x.dtype)
                stepped = sch.step(v, t, x, return_dict=False)
                x = stepped[0]
                if record and i > 0:
                    if len(stepped) != 5:
                        raise ValueError(f"record=True: {type(sch).__name__}.step returned {len(stepped)} entries, not the five of a learned solver")
                    _, actions, probs, conds, masks = stepped
                    rec["x"].append(conds["x"].unsqueeze(1)); rec["epsilon"].append(conds["epsilon"].unsqueeze(1))
                    rec["probs"].append(probs.unsqueeze(1)); rec["actions"].append(actions.unsqueeze(1)); rec["masks"].append(masks.unsqueeze(1))
        finally:
            if keeps_conds:
                sch.record_conds = prev_record
        if not record:
            return x
        cat = {k: torch.cat(v, dim=1) for k, v in rec.items()}
        return x, {"x": cat["x"], "epsilon": cat["epsilon"]}, cat["probs"], cat["actions"], cat["masks"]
