"""CPU-only check of the resources of the kernels of AcrE's parallel way (csrc/kge_acre.hip, the stem k_acrp_), read from the AMDGPU
metadata of the built library with the helpers of test_pull_occupancy.py: no scratch, no register spills (vector or scalar), no dynamic
stack, and the VGPR and LDS figures DESIGN.md section 21 records (all LDS is static, so the metadata counts all of it)."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs: architectural plus accumulation registers, as the metadata counts them; static LDS bytes)
KERNELS = {
    "_ZN3kge9k_acrp_y0E": (23, 0),
    "_ZN3kge11k_acrp_gateILi0EE": (124, 34816), "_ZN3kge11k_acrp_gateILi1EE": (120, 34816),
    "_ZN3kge11k_acrp_gateILi2EE": (128, 34816), "_ZN3kge11k_acrp_gateILi3EE": (128, 34816),
    "_ZN3kge12k_acrp_chsumE": (10, 0),
    "_ZN3kge14k_acrp_gate_gwILb0EE": (84, 0), "_ZN3kge14k_acrp_gate_gwILb1EE": (44, 0), "_ZN3kge13k_acrp_gw_finE": (5, 0),
    "_ZN3kge15k_acrp_conv_bwdE": (129, 68912),
}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_acrp_kernel_resources(metadata, prefix):   # noqa: F811
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1, (prefix, found)
    md = metadata[found[0]]
    vgpr, lds = KERNELS[prefix]
    print(prefix, "vgpr", md["vgpr_count"], "lds", md["group_segment_fixed_size"], "scratch", md["private_segment_fixed_size"])
    assert int(md["private_segment_fixed_size"]) == 0, (prefix, md["private_segment_fixed_size"])
    assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, (prefix, md["vgpr_spill_count"], md["sgpr_spill_count"])
    assert md.get("uses_dynamic_stack", "false") == "false", prefix
    assert int(md["vgpr_count"]) <= vgpr, (prefix, md["vgpr_count"])
    assert int(md["group_segment_fixed_size"]) == lds, (prefix, md["group_segment_fixed_size"])


def test_every_acrp_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_acrp_" in k]
    assert len(kernels) == len(KERNELS), kernels
