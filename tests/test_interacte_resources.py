"""CPU-only check of the resources of every InteractE kernel (csrc/kge_interacte.hip), read from the AMDGPU metadata of the built library
with the helpers of test_pull_occupancy.py: no scratch, no register spills (vector or scalar), and the VGPR and LDS figures DESIGN.md
section 20 records (all LDS of this file is static, so the metadata counts all of it)."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs: architectural plus accumulation registers, as the metadata counts them; static LDS bytes)
KERNELS = {
    "_ZN3kge21k_interacte_row_stats": (22, 0), "_ZN3kge18k_interacte_bn_fin": (43, 0), "_ZN3kge22k_interacte_stats_eval": (14, 0),
    "_ZN3kge16k_interacte_convILb1E": (78, 15360), "_ZN3kge16k_interacte_convILb0E": (72, 15360),
    "_ZN3kge14k_interacte_fcILb1E": (60, 34816), "_ZN3kge14k_interacte_fcILb0E": (52, 34816),
    "_ZN3kge21k_interacte_fc_finishILb1E": (53, 0), "_ZN3kge21k_interacte_fc_finishILb0E": (46, 0),
    "_ZN3kge19k_interacte_bn2_bwd": (52, 0), "_ZN3kge17k_interacte_fc_gw": (100, 0), "_ZN3kge17k_interacte_fc_da": (60, 34816),
    "_ZN3kge20k_interacte_bn1_part": (24, 0), "_ZN3kge23k_interacte_bn1_bwd_fin": (24, 0),
    "_ZN3kge19k_interacte_conv_gw": (60, 33792), "_ZN3kge19k_interacte_conv_dx": (76, 22560),
    "_ZN3kge21k_interacte_small_fin": (24, 0), "_ZN3kge17k_interacte_dcomb": (17, 0), "_ZN3kge19k_interacte_scatter": (20, 0),
}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_interacte_kernel_resources(metadata, prefix):   # noqa: F811
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


def test_every_interacte_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_interacte_" in k]
    assert len(kernels) == len(KERNELS), kernels
