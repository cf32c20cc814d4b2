"""CPU-only check of the resources of every PCA kernel (csrc/kge_pca.hip), read from the AMDGPU metadata of the built library as
test_dbscan_resources.py reads them: no scratch, no spills, no dynamic stack, VGPRs / static LDS within DESIGN.md section 38."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

# prefix -> (most VGPRs, most static LDS bytes).  Gram sweep: 2 x 2 float64 accumulators, one chunk ahead, two slabs of 32 x 80 doubles;
# 168 registers still give three waves per SIMD.  A Jacobi lane (1024 threads) can have 128; matrices and transform slabs are dynamic LDS
KERNELS = {"_ZN3kge12k_pca_colsum": (48, 256), "_ZN3kge10k_pca_mean": (24, 0), "_ZN3kge10k_pca_gram": (168, 40960),
           "_ZN3kge9k_pca_cov": (24, 0), "_ZN3kge12k_pca_jacobiILb0EEE": (128, 256), "_ZN3kge12k_pca_jacobiILb1EEE": (128, 256),
           "_ZN3kge15k_pca_transform": (64, 0)}


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_pca_kernel_resources(metadata, prefix):   # noqa: F811
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1 and len([k for k in metadata if "k_pca_" in k]) == len(KERNELS), (prefix, found)
    md = metadata[found[0]]
    vgpr, lds = KERNELS[prefix]
    print(prefix, "vgpr", md["vgpr_count"], "lds", md["group_segment_fixed_size"], "scratch", md["private_segment_fixed_size"])
    assert int(md["private_segment_fixed_size"]) == 0 and md.get("uses_dynamic_stack", "false") == "false", prefix
    assert int(md["vgpr_spill_count"]) == 0 and int(md.get("sgpr_spill_count", 0)) == 0, prefix
    assert int(md["vgpr_count"]) <= vgpr and int(md["group_segment_fixed_size"]) <= lds, (prefix, md)
