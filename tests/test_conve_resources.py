"""CPU-only check of the resources of every ConvE kernel (csrc/kge_conve.hip), read from the AMDGPU metadata of the built library with
the helpers of test_pull_occupancy.py: no scratch, no register spills (vector or scalar), and the VGPR and LDS figures DESIGN.md
section 18 records (all LDS of this file is static, so the metadata counts all of it)."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs: architectural plus accumulation registers, as the metadata counts them; static LDS bytes)
KERNELS = {
    "_ZN3kge17k_conve_img_stats": (25, 0), "_ZN3kge14k_conve_bn_fin": (43, 0), "_ZN3kge18k_conve_stats_eval": (16, 0),
    "_ZN3kge12k_conve_convILb1E": (39, 8192), "_ZN3kge12k_conve_convILb0E": (96, 8192),
    "_ZN3kge10k_conve_fcILb1E": (64, 34816), "_ZN3kge10k_conve_fcILb0E": (52, 34816),
    "_ZN3kge17k_conve_fc_finishILb1E": (53, 0), "_ZN3kge17k_conve_fc_finishILb0E": (16, 0),
    "_ZN3kge15k_conve_bn2_bwd": (52, 0), "_ZN3kge13k_conve_fc_gw": (100, 0), "_ZN3kge13k_conve_fc_da": (56, 34816),
    "_ZN3kge16k_conve_bn1_part": (24, 0), "_ZN3kge19k_conve_bn1_bwd_fin": (24, 0), "_ZN3kge16k_conve_conv_bwd": (54, 50336),
    "_ZN3kge17k_conve_small_fin": (18, 0), "_ZN3kge12k_conve_dimg": (31, 0), "_ZN3kge15k_conve_scatter": (20, 0),
}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_conve_kernel_resources(metadata, prefix):   # noqa: F811
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


def test_every_conve_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_conve_" in k]
    assert len(kernels) == len(KERNELS), kernels
