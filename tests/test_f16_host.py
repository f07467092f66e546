"""Host-side checks of the fp16-operand entry points and of precision="bf16_fc" (no GPU needed)."""
import os
import re

import crnerf_amd
from crnerf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_SYMBOLS = ["crnerf_packed_mlp_f16_bytes", "crnerf_pack_mlp_weights_f16", "crnerf_mlp_forward_f16", "crnerf_render_rays_f16"]


def test_set_precision_knows_bf16_fc_and_f16():
    before = crnerf_amd.get_precision()
    try:
        crnerf_amd.set_precision("bf16_fc")
        assert crnerf_amd.get_precision() == "bf16_fc"
        crnerf_amd.set_precision("f16")
        assert crnerf_amd.get_precision() == "f16"
        crnerf_amd.set_precision("bf16_hc")                 # the neighbours did not move
        assert crnerf_amd.get_precision() == "bf16_hc"
        crnerf_amd.set_precision("bf16")
        assert crnerf_amd.get_precision() == "bf16"
    finally:
        crnerf_amd.set_precision(before)
    assert crnerf_amd.get_precision() == before


def test_f16_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "crnerf.h")) as f:
        header = f.read()
    for s in F16_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), "%s is not declared in include/crnerf.h" % s
        assert s in _lib.EXPORTS, "%s is not in _lib.EXPORTS (build() checks the library against that list)" % s


def test_f16_is_a_precision_of_its_own():
    from crnerf_amd.precision import resolve
    assert resolve("f16") == "f16" and resolve("bf16") != "f16" and resolve("f32h2") != "f16"
    assert resolve("f16") != "bf16"                         # not an unknown string, and not bf16


def test_new_units_are_audited_and_built():
    import importlib.util
    spec = importlib.util.spec_from_file_location("crnerf_isa_audit_for_f16", os.path.join(ROOT, "tools", "isa_audit.py"))
    audit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(audit)
    spec = importlib.util.spec_from_file_location("crnerf_build_for_f16", os.path.join(ROOT, "cr-nerf-pytorch_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    for unit in ("render_fused_bf16p_f16.hip", "mlp_forward_bf16p_f16.hip"):
        assert unit in audit.AUDITED_UNITS and unit in build.SOURCES
        # the fp16 units are the bf16 units' code: they must be compiled with the bf16 units' flags
        assert build.PER_FILE_FLAGS[unit] == build.PER_FILE_FLAGS[unit.replace("_f16", "")]
