"""CPU-only check of the resources of every k-means kernel (csrc/kge_kmeans.hip), read from the AMDGPU metadata of the built library
with the helpers of test_pull_occupancy.py: no scratch, no register spills, no dynamic stack, and VGPRs / static LDS within the
figures DESIGN.md section 35 records."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs, most static LDS bytes)
KERNELS = {
    "_ZN3kge14k_kmeans_begin": (8, 0),
    "_ZN3kge14k_kmeans_cnorm": (8, 0),
    "_ZN3kge15k_kmeans_assignILi1EE": (112, 24072),   # (accumulators included: 16 per 32 rows of the tile)
    "_ZN3kge15k_kmeans_assignILi2EE": (160, 30216),
    "_ZN3kge13k_kmeans_hist": (56, 17408),
    "_ZN3kge13k_kmeans_scan": (16, 32768),
    "_ZN3kge16k_kmeans_scatter": (8, 0),
    "_ZN3kge15k_kmeans_update": (56, 0),               # (the column-block loop: 52)
    "_ZN3kge15k_kmeans_finish": (24, 2048),
    "_ZN3kge18k_kmeans_seed_fold": (32, 256),
    "_ZN3kge18k_kmeans_seed_pick": (48, 16656),       # (256 bytes of the workgroup vote over centre 0's row)
}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_kmeans_kernel_resources(metadata, prefix):   # noqa: F811
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


def test_every_kmeans_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_kmeans_" in k]
    assert len(kernels) == len(KERNELS), kernels
