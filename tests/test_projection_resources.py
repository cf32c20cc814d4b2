"""CPU-only check of the resources of the two glue kernels of the shared 1-N rank pass (csrc/kge_projection.hip), read from the AMDGPU
metadata of the built library with the helpers of test_pull_occupancy.py: no scratch, no spills, and the VGPR and LDS figures of the
tables in DESIGN.md sections 15 and 16."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (VGPRs, static LDS bytes)
KERNELS = {"_ZN3kge21k_projection_eval_idsE": (15, 0), "_ZN3kge23k_projection_pack_ranksE": (12, 0)}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_projection_kernel_resources(metadata, prefix):   # noqa: F811
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1, (prefix, found)
    md = metadata[found[0]]
    vgpr, lds = KERNELS[prefix]
    print(prefix, "vgpr", md["vgpr_count"], "lds", md["group_segment_fixed_size"], "scratch", md["private_segment_fixed_size"])
    assert int(md["private_segment_fixed_size"]) == 0, (prefix, md["private_segment_fixed_size"])
    assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, (prefix, md["vgpr_spill_count"], md["sgpr_spill_count"])
    assert md.get("uses_dynamic_stack", "false") == "false", prefix
    assert int(md["vgpr_count"]) == vgpr, (prefix, md["vgpr_count"])
    assert int(md["group_segment_fixed_size"]) == lds, (prefix, md["group_segment_fixed_size"])


def test_every_projection_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_projection_" in k]
    assert len(kernels) == len(KERNELS), kernels
