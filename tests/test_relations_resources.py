"""CPU-only check of the resources of the relation-ranking kernels (csrc/kge_relations.hip, the kge_relation_csr_* kernels of
csrc/kge_index.hip), read from the AMDGPU metadata of the built library with the helpers of test_pull_occupancy.py.  Every
k_rank_relations<M, G, NCH> whose k_score_fwd<M, G, NCH> twin of the same build has no scratch and no spills must have none either;
nothing uses a dynamic stack or LDS; VGPRs stay within the figures of DESIGN.md section 28."""
import re

import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

GEOMETRIES = [(32, 1), (32, 2), (32, 4), (32, 8), (64, 8), (64, 16), (64, 32)]
# model id (enum kge_model) -> most VGPRs of k_rank_relations per geometry, in GEOMETRIES order: the figures the build gave
VGPRS = {
    0: [47, 52, 62, 84, 81, 139, 262],       # TransE
    1: [49, 55, 66, 91, 90, 156, 253],       # TransH
    2: [47, 54, 68, 116, 115, 208, 346],     # TransD
    3: [54, 64, 83, 124, 122, 204, 379],     # RotatE
    6: [33, 39, 51, 82, 81, 141, 255],       # DistMult
    7: [37, 48, 68, 114, 113, 202, 367],     # ComplEx
    8: [43, 60, 93, 158, 158, 283, 512],     # ANALOGY
    9: [48, 54, 69, 91, 89, 138, 249],       # TransM
    10: [33, 39, 51, 82, 81, 141, 255],      # CP
    11: [42, 52, 71, 115, 114, 207, 368],    # SimplE
    12: [42, 52, 71, 115, 114, 207, 368],    # SimplE_ignr
    13: [63, 67, 100, 177, 176, 338, 512],   # QuatE
    18: [55, 64, 78, 117, 116, 209, 370],    # KG2E
}
# The exception set: the instantiations whose k_score_fwd twin itself spills in this build -- the many-row models at the widest rows
# (ANALOGY's 9 roles at d > 512, QuatE's 12, KG2E's 6 and RotatE's sincosf chains at d > 1024: NCH = 32 registers per role exceed the
# 512-VGPR file before anything else is live).  Only these may use scratch here; it is the set kge_candidates.hip's kernel is allowed.
MAY_SPILL = {(8, 64, 16), (8, 64, 32), (13, 64, 32), (18, 64, 32), (3, 64, 32)}
SMALL = {"_ZN3kge10k_rel_args": 8, "_ZN3kge13k_relcsr_keys": 12, "_ZN3kge14k_relcsr_queryILb0E": 24, "_ZN3kge14k_relcsr_queryILb1E": 24}


def _key(name):
    return tuple(int(x) for x in re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)E", name).groups())


def _clean(md):
    return (int(md["private_segment_fixed_size"]) == 0 and int(md["vgpr_spill_count"]) == 0 and int(md.get("sgpr_spill_count", 0)) == 0)


def _instances(metadata, stem):   # noqa: F811
    return {_key(k): v for k, v in metadata.items() if ("%d%sI" % (len(stem), stem)) in k}


def test_every_model_and_geometry_is_instantiated(metadata):   # noqa: F811
    rel = _instances(metadata, "k_rank_relations")
    assert sorted(rel) == sorted((m, g, nch) for m in VGPRS for g, nch in GEOMETRIES)
    assert set(rel) <= set(_instances(metadata, "k_score_fwd"))
    assert set(rel) == set(_instances(metadata, "k_rank_candidates"))      # the same thirteen models


@pytest.mark.parametrize("model", sorted(VGPRS))
def test_rank_relations_needs_no_more_than_its_score_forward_twin(metadata, model):   # noqa: F811
    rel, fwd = _instances(metadata, "k_rank_relations"), _instances(metadata, "k_score_fwd")
    for i, (g, nch) in enumerate(GEOMETRIES):
        key = (model, g, nch)
        md = rel[key]
        print(key, "vgpr", md["vgpr_count"], "sgpr", md.get("sgpr_count"), "scratch", md["private_segment_fixed_size"], "spills",
              md["vgpr_spill_count"], md.get("sgpr_spill_count"), "| twin vgpr", fwd[key]["vgpr_count"], "clean" if _clean(fwd[key]) else "spills")
        assert md.get("uses_dynamic_stack", "false") == "false", key
        assert int(md["group_segment_fixed_size"]) == 0, key
        assert int(md["vgpr_count"]) <= VGPRS[model][i], (key, md["vgpr_count"])
        if _clean(fwd[key]):
            assert _clean(md), (key, md["private_segment_fixed_size"], md["vgpr_spill_count"], md.get("sgpr_spill_count"))
        else:
            assert key in MAY_SPILL, key


@pytest.mark.parametrize("prefix", sorted(SMALL))
def test_argument_and_csr_kernels(metadata, prefix):   # noqa: F811
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1, (prefix, found)
    md = metadata[found[0]]
    assert _clean(md) and md.get("uses_dynamic_stack", "false") == "false", prefix
    assert int(md["vgpr_count"]) <= SMALL[prefix] and int(md["group_segment_fixed_size"]) == 0, (prefix, md["vgpr_count"])
