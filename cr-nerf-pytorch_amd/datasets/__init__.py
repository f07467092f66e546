"""Mirror of the part of the reference's ``datasets`` package that feeds the hot path: ray generation
(datasets/ray_utils.py), the grid-sample batcher (phototourism_mask_grid_sample.py) and the image preparation between a decoded photo and
the renderer (images.py: PIL's LANCZOS resize + ToTensor / Normalize on the device).  Reading image files / COLMAP binaries is out of
scope."""
from . import images  # noqa: F401  (host-only at import: does not load the HIP library)
