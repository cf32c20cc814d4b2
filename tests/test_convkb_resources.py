"""CPU-only check of the register budget of every ConvKB kernel (csrc/kge_convkb.hip), read from the AMDGPU metadata of the built
library with the helpers of test_pull_occupancy.py: no scratch and no spills (the kernels walk rows in chunks of the lane group, so
their live state does not grow with the hidden size).  As in test_octonione_resources.py the counts are scratch bytes and vector
register spills; the sampler-fused step keeps a few scalar values in spare vector lanes (sgpr_spill_count 10), which costs no memory
traffic and no scratch."""
import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

PREFIXES = ("_ZN3kge17k_convkb_collapse", "_ZN3kge16k_convkb_forwardILi32E", "_ZN3kge16k_convkb_forwardILi64E",
            "_ZN3kge13k_convkb_stepILi32ELb0E", "_ZN3kge13k_convkb_stepILi64ELb0E", "_ZN3kge13k_convkb_stepILi32ELb1E",
            "_ZN3kge13k_convkb_stepILi64ELb1E", "_ZN3kge15k_convkb_finish", "_ZN3kge16k_convkb_fc_grad",
            "_ZN3kge16k_convkb_projectILi32E", "_ZN3kge16k_convkb_projectILi64E", "_ZN3kge14k_convkb_sweep", "_ZN3kge14k_convkb_ranks")


@pytest.mark.parametrize("prefix", PREFIXES)
def test_convkb_kernel_has_no_scratch_and_no_spills(metadata, prefix):   # noqa: F811
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1, (prefix, found)
    md = metadata[found[0]]
    assert int(md["private_segment_fixed_size"]) == 0, (prefix, md["private_segment_fixed_size"])
    assert int(md["vgpr_spill_count"]) == 0, (prefix, md["vgpr_spill_count"])
    assert md.get("uses_dynamic_stack", "false") == "false", prefix


def test_every_convkb_kernel_is_checked(metadata):   # noqa: F811
    kernels = [k for k in metadata if "k_convkb_" in k]
    assert len(kernels) == len(PREFIXES), kernels
