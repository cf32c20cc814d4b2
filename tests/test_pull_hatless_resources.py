"""CPU-only check of the register budget of the hat-less C1 step's two kernels (csrc/kge_pull.hip, switch KGE_PULL_HATLESS), read from
the AMDGPU metadata of the built library the way tests/test_pull_occupancy.py reads the shipped pair's: k_pull_eval_nohat<L1, 32, 1> --
which carries one extra register for the eight inverse norms of a lane group -- and k_pull_step_nohat<Adam, 32, 1> must each fit
8 waves per SIMD (at most 64 VGPRs) with no scratch and no spills, or the launches lose their single residency round."""
import pytest

from test_pull_occupancy import metadata   # noqa: F401  (module-scoped fixture: the kernels' metadata notes of the built library)

KERNELS = {
    "k_pull_eval_nohat<true, 32, 1>": "_ZN3kge17k_pull_eval_nohatILb1ELi32ELi1EEEv",
    "k_pull_step_nohat<Adam, 32, 1>": "_ZN3kge17k_pull_step_nohatILi1ELi32ELi1EEEv",
}


@pytest.mark.parametrize("label", sorted(KERNELS))
def test_hatless_kernel_fits_eight_waves_without_scratch(metadata, label):   # noqa: F811
    found = [k for k in metadata if k.startswith(KERNELS[label])]
    assert len(found) == 1, (label, found)
    md = metadata[found[0]]
    vgpr = int(md["vgpr_count"])   # (unified total: architectural VGPRs plus AGPRs)
    assert vgpr <= 64, "%s: %d VGPRs (arch + acc): fewer than 8 waves per SIMD" % (label, vgpr)
    assert int(md["private_segment_fixed_size"]) == 0, "%s: %s bytes of scratch per lane" % (label, md["private_segment_fixed_size"])
    assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, (label, md["vgpr_spill_count"], md["sgpr_spill_count"])
    assert md.get("uses_dynamic_stack", "false") == "false", label
