"""CPU-only check of the resources of every nearest-neighbour kernel (csrc/kge_knn.hip), read from the AMDGPU metadata of the built
library with the helpers of test_pull_occupancy.py: no scratch, no register spills, no dynamic stack, and VGPRs / static LDS within the
figures DESIGN.md records for the search.  The sweep's buffers and operand slabs are dynamic LDS, sized by k on the host: at most
63 360 bytes (32 queries x 160 places), 63 616 with the static part."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs, most static LDS bytes)
KERNELS = {
    "_ZN3kge11k_knn_norms": (8, 0),
    "_ZN3kge12k_knn_finish": (26, 17416),
}
# k_knn_sweep<NQ, METRIC>: 32 * NQ queries per tile (NQ = 1: k > 32), metric 0 = dot, 1 = cosine, 2 = l2; the 256 static bytes are
# the workgroup vote's
KERNELS.update({"_ZN3kge11k_knn_sweepILi%dELi%dEE" % (nq, metric): (96 if nq == 1 else 156, 256) for nq in (1, 2) for metric in (0, 1, 2)})


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_knn_kernel_resources(metadata, prefix):   # noqa: F811
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


def test_every_knn_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_knn_" in k]
    assert len(kernels) == len(KERNELS), kernels
