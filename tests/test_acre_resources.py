"""CPU-only check of the resources of every AcrE kernel (csrc/kge_acre.hip), read from the AMDGPU metadata of the built library with
the helpers of test_pull_occupancy.py: no scratch, no register spills (vector or scalar), and the VGPR and LDS figures DESIGN.md
section 21 records (all LDS of this file is static, so the metadata counts all of it)."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs: architectural plus accumulation registers, as the metadata counts them; static LDS bytes)
KERNELS = {
    "_ZN3kge16k_acre_row_stats": (28, 0), "_ZN3kge16k_acre_bn0_stats": (38, 0), "_ZN3kge13k_acre_bn_fin": (43, 0),
    "_ZN3kge17k_acre_stats_eval": (19, 0), "_ZN3kge12k_acre_conv1": (36, 1600),
    "_ZN3kge9k_acre_ccILb0E": (140, 53312), "_ZN3kge9k_acre_ccILb1E": (132, 53312), "_ZN3kge14k_acre_c_stats": (20, 0),
    "_ZN3kge9k_acre_fcILb1E": (60, 34816), "_ZN3kge9k_acre_fcILb0E": (52, 34816),
    "_ZN3kge16k_acre_fc_finishILb1E": (53, 0), "_ZN3kge16k_acre_fc_finishILb0E": (46, 0),
    "_ZN3kge14k_acre_bn2_bwd": (52, 0), "_ZN3kge12k_acre_fc_gw": (100, 0), "_ZN3kge12k_acre_fc_da": (60, 34816),
    "_ZN3kge15k_acre_bn1_part": (24, 0), "_ZN3kge18k_acre_bn1_bwd_fin": (24, 0), "_ZN3kge13k_acre_bn1_dc": (40, 0),
    "_ZN3kge12k_acre_cc_gw": (39, 103424), "_ZN3kge13k_acre_c1_bwd": (39, 54496), "_ZN3kge13k_acre_rowsum": (19, 1088),
    "_ZN3kge14k_acre_bn0_fin": (18, 0), "_ZN3kge12k_acre_dcomb": (40, 0), "_ZN3kge14k_acre_scatter": (20, 0),
}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_acre_kernel_resources(metadata, prefix):   # noqa: F811
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


def test_every_acre_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_acre_" in k]
    assert len(kernels) == len(KERNELS), kernels
