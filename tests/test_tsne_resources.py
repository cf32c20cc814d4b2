"""CPU-only check of the resources of every t-SNE kernel (csrc/kge_tsne.hip), read from the AMDGPU metadata of the built library with
the helpers of test_pull_occupancy.py: no scratch, no register spills, no dynamic stack, and VGPRs / static LDS within the figures
DESIGN.md section 32 records.  No kernel takes dynamic LDS: the sweep's two tile buffers are 2 x 2 KiB of static LDS."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs, most static LDS bytes)
KERNELS = {
    "_ZN3kge17k_tsne_affinities": (84, 0),      # the float64 search: exp and log in double
    "_ZN3kge14k_tsne_repulse": (57, 4128),      # eight waves per SIMD; x and y tiles twice + the workgroup sum
    "_ZN3kge13k_tsne_record": (18, 32),
}
# k_tsne_attract<UPDATE, RECORD>: the float64 log of the KL terms costs the registers of the RECORD forms
KERNELS.update({"_ZN3kge14k_tsne_attractILb%dELb%dEE" % (u, r): (81 if r else 45, 40) for u in (0, 1) for r in (0, 1)})


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_tsne_kernel_resources(metadata, prefix):   # noqa: F811
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


def test_every_tsne_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_tsne_" in k]
    assert len(kernels) == len(KERNELS), kernels
