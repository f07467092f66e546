"""Regenerates g19_blender.npz: what Pillow and the reference's Blender dataset themselves give on the seeded inputs of
tests/_blender_cases.py.  Only recorded outputs are stored, with each input's byte sum; the inputs are regenerated from their seeds.
  (a) Image.fromarray(a).resize((w, h), Image.LANCZOS) of every RGBA table case, and how many colour bytes of Pillow's premultiplied
      result the RGBa -> RGBA conversion clips at 255;
  (b) the reference's add_perturbation on frame 0 (640 x 640) for seeds 1, 2, 7 x ('occ'), ('color'), both -- stored at 40 x 40 through
      Pillow's own resize, to keep the file small;
  (c) the reference's BlenderDataset on three frames written as PNGs with a transforms_*.json into a temporary directory, at
      img_wh = (40, 40) with both perturbations: split 'train' (all_rays, all_rgbs, all_imgs and two __getitem__ samples: the first on the
      numpy state the constructor leaves behind, the second after np.random.seed; torch seeded before each), split 'test_train' idx 0 and
      1, and the whole_img of eval.py:99-111 (those lines, run here on frame 0).
torchvision's ToTensor / Normalize and kornia's create_meshgrid, which the reference imports, are stubbed from their definitions in this
process only.

    python tests/golden/make_golden_blender.py /path/to/the/reference/checkout
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _blender_cases as B  # noqa: E402


def create_meshgrid(height, width, normalized_coordinates=True):
    """kornia.create_meshgrid for normalized_coordinates=False: [1, H, W, 2] of (x, y)."""
    assert not normalized_coordinates
    xs, ys = torch.linspace(0, width - 1, width), torch.linspace(0, height - 1, height)
    return torch.stack(torch.meshgrid([xs, ys], indexing="ij"), dim=-1).permute(1, 0, 2).unsqueeze(0)


class ToTensor:
    """torchvision.transforms.ToTensor on an 8-bit PIL image."""
    def __call__(self, pic):
        img = torch.from_numpy(np.array(pic, copy=True)).view(pic.size[1], pic.size[0], len(pic.getbands()))
        return img.permute((2, 0, 1)).contiguous().to(dtype=torch.float32).div(255)


class Normalize:
    """torchvision.transforms.Normalize."""
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, tensor):
        tensor = tensor.clone()
        mean = torch.as_tensor(self.mean, dtype=tensor.dtype)[:, None, None]
        std = torch.as_tensor(self.std, dtype=tensor.dtype)[:, None, None]
        return tensor.sub_(mean).div_(std)


def stub_imports():
    kornia = types.ModuleType("kornia")
    kornia.create_meshgrid = create_meshgrid
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.ToTensor, tr.Normalize, tr.Resize = ToTensor, Normalize, (lambda *a, **k: None)
    tv.transforms = tr
    for name, mod in (("kornia", kornia), ("torchvision", tv), ("torchvision.transforms", tr)):
        sys.modules.setdefault(name, mod)


def write_scene(root, frames, poses):
    for split in ("train", "test"):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        meta = {"camera_angle_x": B.CAMERA_ANGLE_X, "frames": []}
        for t, (a, p) in enumerate(zip(frames, poses)):
            Image.fromarray(a).save(os.path.join(root, split, "r_%d.png" % t))
            meta["frames"].append({"file_path": "./%s/r_%d" % (split, t),
                                   "transform_matrix": np.concatenate([p.astype(np.float64), [[0, 0, 0, 1]]], 0).tolist()})
        with open(os.path.join(root, "transforms_%s.json" % split), "w") as f:
            json.dump(meta, f)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    stub_imports()
    from datasets.blender_mask_grid_sample import BlenderDataset, add_perturbation

    out, keys, sums, clips = {}, [], [], []
    for case in B.table_cases():
        key, _, _, H, W, w, h = case
        a = B.case_input(case)
        im = Image.fromarray(a)
        out["out_" + key] = np.asarray(im.resize((w, h), Image.LANCZOS))
        n = 0
        if (w, h) != (W, H):
            pm = np.frombuffer(im.convert("RGBa").resize((w, h), Image.LANCZOS).tobytes(), dtype=np.uint8).reshape(h, w, 4).astype(np.int64)
            al = pm[..., 3:]
            n = int((((al != 0) & (al != 255)) & ((255 * pm[..., :3]) // np.maximum(al, 1) > 255)).sum())
        keys.append(key)
        sums.append(int(a.sum(dtype=np.int64)))
        clips.append(n)

    frames = [B.frame(t) for t in range(B.N_FRAMES)]
    for seed in B.PERTURB_SEEDS:
        for pset in B.PERTURB_SETS:
            img = add_perturbation(Image.fromarray(frames[0]), list(pset), seed)
            out["pert_%d_%s" % (seed, "_".join(pset))] = np.asarray(img.resize(B.IMG_WH, Image.LANCZOS))

    poses = B.poses()
    with tempfile.TemporaryDirectory() as root:
        write_scene(root, frames, poses)
        ds = BlenderDataset(root, batch_size=64, split="train", img_wh=B.IMG_WH, perturbation=["occ", "color"])
        out["train_all_rays"], out["train_all_rgbs"], out["train_all_imgs"] = ds.all_rays.numpy(), ds.all_rgbs.numpy(), ds.all_imgs.numpy()
        len(ds)                                                   # sets ds.iterations, as the DataLoader does
        for n, (np_seed, torch_seed, idx, anneal) in enumerate(((-1, 11, 0, -1), (5, 12, 3, 0.1))):
            if np_seed >= 0:
                np.random.seed(np_seed)
            torch.manual_seed(torch_seed)
            ds.scale_anneal = anneal
            s = ds[idx]
            for k in ("rays", "ts", "rgbs", "whole_img", "rgb_idx", "uv_sample"):
                out["sample%d_%s" % (n, k)] = s[k].numpy()
            out["sample%d_min_scale_cur" % n] = np.float64(s["min_scale_cur"])
            out["sample%d_setup" % n] = np.array([np_seed, torch_seed, idx], dtype=np.int64)
            out["sample%d_anneal" % n] = np.float64(anneal)
        ev = BlenderDataset(root, split="test_train", img_wh=B.IMG_WH, perturbation=["occ", "color"])
        for idx in (0, 1):
            s = ev[idx]
            for k in ("rays", "ts", "rgbs", "valid_mask", "rgb_idx", "original_rgbs", "original_valid_mask"):
                out["eval%d_%s" % (idx, k)] = s[k].numpy()
        # eval.py:99-111
        img = Image.open(os.path.join(root, "train", "r_0.png"))
        img = img.resize(B.IMG_WH, Image.LANCZOS)
        img = ToTensor()(img)
        img = img[:3, :, :] * img[-1:, :, :] + (1 - img[-1:, :, :])
        out["whole_img"] = Normalize(mean=[0.5, 0.5, 0.5], std=[0.5, 0.5, 0.5])(img).unsqueeze(0).numpy()

    np.savez_compressed(B.GOLDEN, keys=np.array(keys), input_sums=np.array(sums, dtype=np.int64), clips=np.array(clips, dtype=np.int64),
                        frame_sums=np.array([int(a.sum(dtype=np.int64)) for a in frames], dtype=np.int64),
                        pillow_version=np.array(PIL.__version__), **out)
    print("%s: %d table cases, %d bytes, Pillow %s; clipped bytes: %s" % (B.GOLDEN, len(keys), os.path.getsize(B.GOLDEN), PIL.__version__,
                                                                         {k: c for k, c in zip(keys, clips) if c}))
