"""CPU-only check of the register budget of every OctonionE kernel (csrc/kge_octonion.hip), read from the AMDGPU metadata of the
built library with the helpers of test_pull_occupancy.py: no scratch and no spills at any hidden size (the kernels walk rows in
chunks of the lane group, so their live state does not grow with d; DESIGN.md section 13 lists VGPRs and occupancy)."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

PREFIXES = ("_ZN3kge11k_oct_scoreILi32ELb0E", "_ZN3kge11k_oct_scoreILi64ELb0E", "_ZN3kge11k_oct_scoreILi32ELb1E",
            "_ZN3kge11k_oct_scoreILi64ELb1E", "_ZN3kge15k_oct_pointwiseILi32E", "_ZN3kge15k_oct_pointwiseILi64E",
            "_ZN3kge10k_oct_cand", "_ZN3kge13k_oct_queries")


@pytest.mark.parametrize("prefix", PREFIXES)
def test_octonione_kernel_has_no_scratch_and_no_spills(metadata, prefix):   # noqa: F811
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1, (prefix, found)
    md = metadata[found[0]]
    assert int(md["private_segment_fixed_size"]) == 0, (prefix, md["private_segment_fixed_size"])
    assert int(md["vgpr_spill_count"]) == 0, (prefix, md["vgpr_spill_count"])
    assert md.get("uses_dynamic_stack", "false") == "false", prefix


def test_every_octonione_kernel_is_checked(metadata):   # noqa: F811
    oct_kernels = [k for k in metadata if "k_oct_" in k]
    assert len(oct_kernels) == len(PREFIXES), oct_kernels
