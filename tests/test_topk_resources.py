"""CPU-only check of the resources of every row-select kernel (csrc/kge_topk.hip), read from the AMDGPU metadata of the built library
with the helpers of test_pull_occupancy.py: no scratch, no vector-register spills, no dynamic stack, and VGPRs / static LDS within the
figures DESIGN.md records for the select."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs, most static LDS bytes)
KERNELS = {
    "_ZN3kge11k_topk_mask": (13, 0),
    "_ZN3kge13k_topk_selectIjE": (30, 9292),      # float32 rows: uint32 keys
    "_ZN3kge13k_topk_selectImE": (32, 13392),     # float64 rows: uint64 keys
}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_topk_kernel_resources(metadata, prefix):   # noqa: F811
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1, (prefix, found)
    md = metadata[found[0]]
    vgpr, lds = KERNELS[prefix]
    print(prefix, "vgpr", md["vgpr_count"], "sgpr", md.get("sgpr_count"), "lds", md["group_segment_fixed_size"], "scratch",
          md["private_segment_fixed_size"])
    assert int(md["private_segment_fixed_size"]) == 0, (prefix, md["private_segment_fixed_size"])
    assert int(md["vgpr_spill_count"]) == 0, (prefix, md["vgpr_spill_count"])
    assert int(md.get("sgpr_spill_count", 0)) == 0, (prefix, md.get("sgpr_spill_count"))
    assert md.get("uses_dynamic_stack", "false") == "false", prefix
    assert int(md["vgpr_count"]) <= vgpr, (prefix, md["vgpr_count"])
    assert int(md["group_segment_fixed_size"]) <= lds, (prefix, md["group_segment_fixed_size"])


def test_every_topk_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_topk_" in k]
    assert len(kernels) == len(KERNELS), kernels
