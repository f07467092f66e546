"""Regenerates g17_lanczos.npz: what Pillow itself -- Image.fromarray(a).resize((w, h), Image.LANCZOS) -- gives on the seeded inputs of
tests/_lanczos_cases.py.  Only Pillow's outputs are stored (a fraction of their inputs), with each input's byte sum and Pillow's version;
the inputs are regenerated from their seeds.

    python tests/golden/make_golden_lanczos.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _lanczos_cases as L  # noqa: E402

if __name__ == "__main__":
    out, keys, sums = {}, [], []
    for case in L.golden_cases():
        key, kind, seed, H, W, w, h, side = case
        a = L.case_input(case)
        out["out_" + key] = np.asarray(Image.fromarray(a).resize((w, h), Image.LANCZOS))
        keys.append(key)
        sums.append(int(a.sum(dtype=np.int64)))
    np.savez_compressed(L.GOLDEN, keys=np.array(keys), input_sums=np.array(sums, dtype=np.int64), pillow_version=np.array(PIL.__version__), **out)
    print("%s: %d cases, %d bytes, Pillow %s" % (L.GOLDEN, len(keys), os.path.getsize(L.GOLDEN), PIL.__version__))
