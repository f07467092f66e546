"""Regenerates g18_scene.npz: what the reference's PhototourismDataset.read_meta gives on the two synthetic COLMAP models of
tests/_scene_cases.py (MODELS).  Each model is written with struct into a temporary directory -- dense/sparse/cameras.bin (PINHOLE, camera
id = image id, as read_meta indexes camdata[id_]), images.bin (no 2-D points), points3D.bin (empty tracks) and a .tsv that lists the
images in a shuffled order plus one file that has no image -- and read back by the reference itself: split 'val' for the model at
img_downscale 2, split 'test_train' for the one at img_downscale 1 ('val' would raise that to 2); neither split opens a photo.  kornia and
torchvision, which the reference imports but these splits never call, are stubbed in this process only.  Only recorded results and the
inputs that produced them are stored.

    python tests/golden/make_golden_scene.py /path/to/the/reference/checkout
"""
import os
import struct
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _scene_cases as S  # noqa: E402


def write_model(root, m, order):
    sparse = os.path.join(root, "dense", "sparse")
    os.makedirs(sparse)
    names = {int(i): "img_%04d.jpg" % i for i in m["ids"]}
    with open(os.path.join(sparse, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(m["ids"])))
        for i, p in zip(m["ids"], m["params"]):
            f.write(struct.pack("<iiQQ", int(i), 1, int(p[2] * 2), int(p[3] * 2)))      # model 1 = PINHOLE
            f.write(struct.pack("<4d", *p))
    with open(os.path.join(sparse, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(m["ids"])))
        for i, q, t in zip(m["ids"], m["qvecs"], m["tvecs"]):
            f.write(struct.pack("<i4d3di", int(i), *q, *t, int(i)))
            f.write(names[int(i)].encode() + b"\0")
            f.write(struct.pack("<Q", 0))
    with open(os.path.join(sparse, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(m["xyz"])))
        for k, p in enumerate(m["xyz"]):
            f.write(struct.pack("<Q3d3BdQ", k + 1, *p, 128, 128, 128, 0.5, 0))
    with open(os.path.join(root, "synthetic.tsv"), "w") as f:
        f.write("filename\tid\tsplit\tdataset\n")
        for n, k in enumerate(order):
            f.write("%s\t%d\t%s\tsynthetic\n" % (names[int(m["ids"][k])], n, "train" if n % 3 else "test"))
        f.write("not_in_the_model.jpg\t%d\ttrain\tsynthetic\n" % len(order))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    for name in ("kornia", "torchvision"):
        if name not in sys.modules:
            stub = types.ModuleType(name)
            stub.create_meshgrid = None
            stub.transforms = types.SimpleNamespace(ToTensor=lambda: None, Normalize=lambda **kw: None)
            sys.modules[name] = stub
    from datasets.phototourism_mask_grid_sample import PhototourismDataset

    out = {"numpy_version": np.array(np.__version__)}
    for key, spec in S.MODELS.items():
        m = S.colmap_model(**spec)
        order = np.random.default_rng(spec["seed"]).permutation(spec["n_images"])
        with tempfile.TemporaryDirectory() as root:
            write_model(root, m, order)
            ds = PhototourismDataset(None, root, split="val" if spec["img_downscale"] >= 2 else "test_train", img_downscale=spec["img_downscale"])
        assert ds.img_downscale == spec["img_downscale"]
        ids = np.array(ds.img_ids, dtype=np.int64)
        assert np.array_equal(ids, m["ids"][order])
        out.update({
            key + "_img_ids": ids,
            key + "_Ks": np.stack([ds.Ks[i] for i in ds.img_ids]),
            key + "_poses": np.asarray(ds.poses),
            key + "_nears": np.array([ds.nears[i] for i in ds.img_ids], dtype=np.float64),
            key + "_fars": np.array([ds.fars[i] for i in ds.img_ids], dtype=np.float64),
            key + "_xyz_world": np.asarray(ds.xyz_world),
            key + "_qvecs": m["qvecs"][order], key + "_tvecs": m["tvecs"][order], key + "_params": m["params"][order], key + "_xyz": m["xyz"],
        })
        print("model %s: %d images, %d points, fars %s" % (key, len(ids), len(m["xyz"]), out[key + "_fars"]))
    np.savez_compressed(S.GOLDEN, **out)
    print("%s: %d bytes, numpy %s" % (S.GOLDEN, os.path.getsize(S.GOLDEN), np.__version__))
