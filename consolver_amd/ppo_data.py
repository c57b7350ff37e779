"""Teacher-pair data of the PPO trainer: on-disk format and batch collation.

Format written by gen_pretrain/generate_data.py:180-213 and read by data_processing.py:10-63, one sample per id
``{device_id}_{index:08d}``:  ``{id}.txt`` (prompt), ``{id}.png`` (decoded teacher image, not needed by the reward path:
rewards are computed on the decoded teacher LATENT, train_ppo.py:366-373), ``noise_{id}.pth`` and ``latent_{id}.pth``
(``torch.save`` of ``[4, 64, 64]`` tensors: initial noise and the teacher's final latent).
Host-side logic only (file I/O); the tensors go to the GPU in the caller.
"""
import os
import random

import torch


def teacher_pair_id(device_id, index):
    return f"{device_id}_{index:08d}"          # generate_data.py:189-191


def save_teacher_pair(out_dir, sample_id, prompt, noise, latent):
    """generate_data.py:189-213 (without the PNG)."""
    if torch.isnan(latent).any():
        raise ValueError("teacher latent contains NaN")         # generate_data.py:209
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{sample_id}.txt"), "w") as f:
        f.write(prompt)
    torch.save(noise.detach().cpu().clone(), os.path.join(out_dir, f"noise_{sample_id}.pth"))
    torch.save(latent.detach().cpu().clone(), os.path.join(out_dir, f"latent_{sample_id}.pth"))


class TeacherPairDataset(torch.utils.data.Dataset):
    """data_processing.py:10-63: ids are the ``*.txt`` files of the directory; ``__getitem__`` -> (text, noise, latent).
    A sample whose files are missing or whose latent holds NaN is replaced by a random other one, like the reference
    (:40-61); ``strict=True`` raises instead."""

    def __init__(self, img_dir, strict=False):
        self.img_dir = img_dir
        self.strict = strict
        self.ids = sorted(f[:-4] for f in os.listdir(img_dir) if f.endswith(".txt"))

    def __len__(self):
        return len(self.ids)

    def _load(self, idx):
        sid = self.ids[idx].strip()
        with open(os.path.join(self.img_dir, sid + ".txt")) as f:
            text = f.read().strip()
        noise = torch.load(os.path.join(self.img_dir, f"noise_{sid}.pth"), map_location="cpu")
        latent = torch.load(os.path.join(self.img_dir, f"latent_{sid}.pth"), map_location="cpu")
        if torch.isnan(latent).any():
            raise FileNotFoundError(sid)
        return text, noise, latent

    def __getitem__(self, idx):
        for _ in range(1000):
            try:
                return self._load(idx)
            except (OSError, RuntimeError, FileNotFoundError):
                if self.strict:
                    raise
                idx = random.randint(0, len(self.ids) - 1)
        raise RuntimeError("no loadable teacher pair found")


def collate_teacher_pairs(samples):
    text, noise, latent = zip(*samples)
    return list(text), torch.stack(noise), torch.stack(latent)


def repeat_random_sample(batch, index=None, return_index=False):
    """data_processing.py:65-83: one random sample of the batch repeated batch-size times (the trainer rolls out B
    trajectories of the SAME prompt/noise so that the advantage normalisation compares policies, not prompts).
    ``index``: use this item instead of drawing one; ``return_index=True``: also return the item that was used, for callers that
    hold per-item side data (cached prompt embeddings) -- no hidden state is kept between calls."""
    text, noise, tch = batch
    B = noise.shape[0]
    i = random.randint(0, B - 1) if index is None else int(index)
    out = ([text[i]] * B, noise[i:i + 1].repeat(B, *[1] * (noise.dim() - 1)), tch[i:i + 1].repeat(B, *[1] * (tch.dim() - 1)))
    return out + (i,) if return_index else out


# ---------------------------------------------------------------------------------------------------------------- FLUX teacher pairs
# Tree written by edit_ppo/edit_pretrain/generate.py (generate_flux_teacher.py here) and read by edit_ppo/data_processing.py:
# ``ref_images/{i}.png``, ``prompts/{i}.txt``, ``initial_noises/{i}.pt``, ``obtained_noises/{i}.pt`` (``torch.save`` of packed [1, L, 64]
# latents in the model dtype) and ``edited_images/{i}.png``.
FLUX_PAIR_DIRS = dict(edited="edited_images", initial="initial_noises", obtained="obtained_noises", prompts="prompts", ref="ref_images")


def save_flux_teacher_pair(root_dir, index, initial_latents, obtained_latents, edited_image):
    """edit_pretrain/generate.py:81,133,142.  ``edited_image``: a PIL image."""
    if torch.isnan(obtained_latents).any() or torch.isnan(initial_latents).any():
        raise ValueError(f"teacher latents of item {index} contain NaN")
    for key in ("initial", "obtained", "edited"):
        os.makedirs(os.path.join(root_dir, FLUX_PAIR_DIRS[key]), exist_ok=True)
    torch.save(initial_latents.detach().cpu().clone(), os.path.join(root_dir, FLUX_PAIR_DIRS["initial"], f"{index}.pt"))
    torch.save(obtained_latents.detach().cpu().clone(), os.path.join(root_dir, FLUX_PAIR_DIRS["obtained"], f"{index}.pt"))
    edited_image.save(os.path.join(root_dir, FLUX_PAIR_DIRS["edited"], f"{index}.png"))


class FluxTeacherPairDataset(torch.utils.data.Dataset):
    """data_processing.py:10-91 (``CustomImageDataset``): items are the images of ``edited_images/``, sorted by name; ``__getitem__`` ->
    (edited image [3, H, W] in [-1, 1], prompt, initial latents [L, 64], obtained latents [L, 64], reference image [3, H, W] in [0, 1]).
    ``sample_size = (height, width)``: both images are resized to exactly that with PIL's LANCZOS filter (the reference's torchvision
    ``Resize`` with a tuple size does the same through PIL, and its centre crop to the same size is then a no-op).  An item that fails to
    load or holds NaN is replaced by a random other one, like the reference (:86-89); ``strict=True`` raises instead."""

    def __init__(self, root_dir, sample_size, strict=False):
        self.root_dir, self.strict = root_dir, strict
        self.sample_size = (sample_size, sample_size) if isinstance(sample_size, int) else tuple(sample_size)
        self.img_names = sorted(f for f in os.listdir(os.path.join(root_dir, FLUX_PAIR_DIRS["edited"])) if f.lower().endswith((".png", ".jpg", ".jpeg")))

    def __len__(self):
        return len(self.img_names)

    def _image(self, path):
        import numpy as np
        from PIL import Image
        h, w = self.sample_size
        img = Image.open(path).convert("RGB").resize((w, h), Image.LANCZOS)
        return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.0       # ToTensor

    def _load(self, idx):
        img_name = self.img_names[idx].strip()
        base = os.path.splitext(img_name)[0]
        d = {k: os.path.join(self.root_dir, v) for k, v in FLUX_PAIR_DIRS.items()}
        image = (self._image(os.path.join(d["edited"], img_name)) - 0.5) / 0.5                               # Normalize(0.5, 0.5)
        with open(os.path.join(d["prompts"], base + ".txt"), encoding="utf-8") as f:
            text = f.read().strip()
        noise = torch.load(os.path.join(d["initial"], base + ".pt"), map_location="cpu")[0]
        latent = torch.load(os.path.join(d["obtained"], base + ".pt"), map_location="cpu")[0]
        ref = self._image(os.path.join(d["ref"], img_name))
        if torch.isnan(latent).any() or torch.isnan(noise).any():
            raise ValueError("NaN in tensors")
        return image, text, noise, latent, ref

    def __getitem__(self, idx):
        for _ in range(1000):
            try:
                return self._load(idx)
            except Exception:
                if self.strict:
                    raise
                idx = random.randint(0, len(self.img_names) - 1)
        raise RuntimeError("no loadable FLUX teacher pair found")


def repeat_random_sample_flux(batch, index=None, return_index=False):
    """data_processing.py:93-104: ``repeat_random_sample`` for the FLUX 5-tuple (image, text, noise, teacher latents, reference image)."""
    image, text, noise, tch, ref = batch
    B = image.shape[0]
    i = random.randint(0, B - 1) if index is None else int(index)
    rep = lambda t: t[i:i + 1].repeat(B, *[1] * (t.dim() - 1))
    out = (rep(image), [text[i]] * B, rep(noise), rep(tch), rep(ref))
    return out + (i,) if return_index else out
