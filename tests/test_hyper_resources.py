"""CPU-only check of the resources of every HypER kernel (csrc/kge_hyper.hip), read from the AMDGPU metadata of the built library with
the helpers of test_pull_occupancy.py: no scratch, no register spills (vector or scalar), and the VGPR and LDS figures DESIGN.md
section 19 records (all LDS of this file is static, so the metadata counts all of it)."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs: architectural plus accumulation registers, as the metadata counts them; static LDS bytes)
KERNELS = {
    "_ZN3kge17k_hyper_row_stats": (20, 0), "_ZN3kge14k_hyper_bn_fin": (43, 0), "_ZN3kge18k_hyper_stats_eval": (25, 0),
    "_ZN3kge12k_hyper_filt": (35, 32768),
    "_ZN3kge12k_hyper_convILb1E": (36, 5248), "_ZN3kge12k_hyper_convILb0E": (92, 5248),
    "_ZN3kge10k_hyper_fcILb1E": (64, 34816), "_ZN3kge10k_hyper_fcILb0E": (52, 34816),
    "_ZN3kge17k_hyper_fc_finishILb1E": (53, 0), "_ZN3kge17k_hyper_fc_finishILb0E": (44, 0),
    "_ZN3kge15k_hyper_bn2_bwd": (52, 0), "_ZN3kge13k_hyper_fc_gw": (100, 0), "_ZN3kge13k_hyper_fc_da": (52, 34816),
    "_ZN3kge16k_hyper_bn1_part": (24, 0), "_ZN3kge19k_hyper_bn1_bwd_fin": (24, 0), "_ZN3kge16k_hyper_conv_bwd": (52, 25760),
    "_ZN3kge17k_hyper_small_fin": (18, 0), "_ZN3kge14k_hyper_fc1_gw": (40, 0), "_ZN3kge12k_hyper_drel": (42, 2304),
    "_ZN3kge12k_hyper_dent": (42, 0), "_ZN3kge15k_hyper_scatter": (20, 0),
}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_hyper_kernel_resources(metadata, prefix):   # noqa: F811
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


def test_every_hyper_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_hyper_" in k]
    assert len(kernels) == len(KERNELS), kernels
