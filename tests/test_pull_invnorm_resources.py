"""CPU-only check of the register budget of the C1 two-phase step's kernels after the stored-inverse-norm change (csrc/kge_pull.hip),
read from the AMDGPU metadata of the built library the way tests/test_pull_hatless_resources.py reads it: both evaluation kernels the
flagship line can run -- k_pull_eval_nohat<L1, 32, 1>, whose eight scales now arrive in SGPRs, and k_pull_eval<L1, 32, 1>, which shares
the new direction codes -- must fit 8 waves per SIMD (at most 64 VGPRs) with no scratch, and the hat-less owners, which now store the
inverse norm they used to drop, must not need more than the 58 VGPRs they had before."""
import pytest

from test_pull_occupancy import metadata   # noqa: F401  (module-scoped fixture: the kernels' metadata notes of the built library)

KERNELS = {
    "k_pull_eval_nohat<true, 32, 1>": ("_ZN3kge17k_pull_eval_nohatILb1ELi32ELi1EEEv", 64),
    "k_pull_eval<true, 32, 1>": ("_ZN3kge11k_pull_evalILb1ELi32ELi1EEEv", 64),
    "k_pull_step_nohat<Adam, 32, 1>": ("_ZN3kge17k_pull_step_nohatILi1ELi32ELi1EEEv", 58),
}


@pytest.mark.parametrize("label", sorted(KERNELS))
def test_kernel_keeps_its_registers_without_scratch(metadata, label):   # noqa: F811
    symbol, ceiling = KERNELS[label]
    found = [k for k in metadata if k.startswith(symbol)]
    assert len(found) == 1, (label, found)
    md = metadata[found[0]]
    vgpr = int(md["vgpr_count"])   # (unified total: architectural VGPRs plus AGPRs)
    assert vgpr <= ceiling, "%s: %d VGPRs (arch + acc), ceiling %d" % (label, vgpr, ceiling)
    assert int(md["private_segment_fixed_size"]) == 0, "%s: %s bytes of scratch per lane" % (label, md["private_segment_fixed_size"])
    assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, (label, md["vgpr_spill_count"], md["sgpr_spill_count"])
    assert md.get("uses_dynamic_stack", "false") == "false", label
