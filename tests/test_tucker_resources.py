"""CPU-only check of the resources of every TuckER kernel (csrc/kge_tucker.hip), read from the AMDGPU metadata of the built library
with the helpers of test_pull_occupancy.py: no scratch, no vector-register spills, and LDS within the figures DESIGN.md section 15
records (the matrix-core kernels take their rel tile as dynamic LDS, which the metadata does not count).  The rank pass's two glue
kernels are shared with ProjE_pointwise: tests/test_projection_resources.py."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs, most static LDS bytes)
KERNELS = {
    "_ZN3kge13k_tucker_prep": (64, 0), "_ZN3kge15k_tucker_finish": (64, 0), "_ZN3kge17k_tucker_bwd_prep": (64, 0),
    "_ZN3kge13k_tucker_gent": (64, 0), "_ZN3kge16k_tucker_scatter": (64, 0),
    "_ZN3kge13k_tucker_coreILi0ELb0E": (128, 0), "_ZN3kge13k_tucker_coreILi0ELb1E": (128, 0),
    "_ZN3kge13k_tucker_coreILi1ELb0E": (128, 0), "_ZN3kge13k_tucker_coreILi1ELb1E": (128, 0),
    "_ZN3kge11k_tucker_gwILb0E": (512, 33792), "_ZN3kge11k_tucker_gwILb1E": (512, 33792),
    "_ZN3kge13k_tucker_grelILb0E": (64, 0), "_ZN3kge13k_tucker_grelILb1E": (64, 0),
}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_tucker_kernel_resources(metadata, prefix):   # noqa: F811
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1, (prefix, found)
    md = metadata[found[0]]
    vgpr, lds = KERNELS[prefix]
    print(prefix, "vgpr", md["vgpr_count"], "lds", md["group_segment_fixed_size"], "scratch", md["private_segment_fixed_size"])
    assert int(md["private_segment_fixed_size"]) == 0, (prefix, md["private_segment_fixed_size"])
    assert int(md["vgpr_spill_count"]) == 0, (prefix, md["vgpr_spill_count"])
    assert md.get("uses_dynamic_stack", "false") == "false", prefix
    assert int(md["vgpr_count"]) <= vgpr, (prefix, md["vgpr_count"])
    assert int(md["group_segment_fixed_size"]) <= lds, (prefix, md["group_segment_fixed_size"])


def test_every_tucker_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_tucker_" in k]
    assert len(kernels) == len(KERNELS), kernels
