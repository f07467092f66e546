"""Mirror of the part of the reference's ``datasets`` package that feeds the hot path: ray generation
(datasets/ray_utils.py), the grid-sample batcher (phototourism_mask_grid_sample.py), the image preparation between a decoded photo and
the renderer (images.py: PIL's LANCZOS resize + ToTensor / Normalize on the device) and the scene preparation between the parsed COLMAP
arrays and both (scene.py: read_meta's intrinsics, poses, per-image near / far percentiles on the device, scene scale), and the Blender
dataset's RGBA preparation, perturbations, buffers and batcher (blender.py).  Reading image files / COLMAP binaries / transforms_*.json is
out of scope."""
from . import images  # noqa: F401  (host-only at import: does not load the HIP library)
from . import scene  # noqa: F401  (likewise)
from . import blender  # noqa: F401  (likewise)
