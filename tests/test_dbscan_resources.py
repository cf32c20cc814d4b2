"""CPU-only check of the resources of every DBSCAN kernel (csrc/kge_dbscan.hip), read from the AMDGPU metadata of the built library as
test_silhouette_resources.py reads them: no scratch, no spills, no dynamic stack, VGPRs / static LDS within DESIGN.md section 37."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs, most static LDS bytes); the sweep's modes are 0 count, 1 round, 2 border, each for L2 and cosine, and hold
# 64 accumulators for the four column tiles of a step
KERNELS = {"_ZN3kge10k_dbs_rows": (8, 0), "_ZN3kge10k_dbs_core": (12, 0), "_ZN3kge13k_dbs_compact": (20, 4096),
           "_ZN3kge14k_dbs_compress": (8, 0), "_ZN3kge12k_dbs_number": (24, 4096), "_ZN3kge11k_dbs_label": (8, 0)}
KERNELS.update({"_ZN3kge11k_dbs_sweepILi%dELb%dEE" % (mode, cos): (296, 38144) for mode in range(3) for cos in range(2)})


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_dbscan_kernel_resources(metadata, prefix):   # noqa: F811
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1 and len([k for k in metadata if "k_dbs_" in k]) == len(KERNELS), (prefix, found)
    md = metadata[found[0]]
    vgpr, lds = KERNELS[prefix]
    print(prefix, "vgpr", md["vgpr_count"], "lds", md["group_segment_fixed_size"], "scratch", md["private_segment_fixed_size"])
    assert int(md["private_segment_fixed_size"]) == 0 and md.get("uses_dynamic_stack", "false") == "false", prefix
    assert int(md["vgpr_spill_count"]) == 0 and int(md.get("sgpr_spill_count", 0)) == 0, prefix
    assert int(md["vgpr_count"]) <= vgpr and int(md["group_segment_fixed_size"]) <= lds, (prefix, md)
