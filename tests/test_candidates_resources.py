"""CPU-only check of the resources of the candidate-ranking kernels (csrc/kge_candidates.hip), read from the AMDGPU metadata of the
built library with the helpers of test_pull_occupancy.py.  Every k_rank_candidates<M, G, NCH> whose k_score_fwd<M, G, NCH> twin of the
same build has no scratch and no spills must have none either; nothing uses a dynamic stack; VGPRs and static LDS stay within the
figures of DESIGN.md section 26."""
import re

import pytest

from test_pull_occupancy import metadata  # noqa: F401  (module fixture: {kernel name: metadata} of the gfx950 code objects)

GEOMETRIES = [(32, 1), (32, 2), (32, 4), (32, 8), (64, 8), (64, 16), (64, 32)]
# model id (enum kge_model) -> most VGPRs of k_rank_candidates per geometry, in GEOMETRIES order: the figures the build gave
VGPRS = {
    0: [41, 47, 58, 85, 84, 130, 250],       # TransE
    1: [46, 54, 71, 111, 107, 179, 333],     # TransH
    2: [47, 57, 81, 126, 124, 212, 358],     # TransD
    3: [48, 60, 82, 134, 131, 227, 417],     # RotatE
    6: [38, 43, 55, 84, 83, 127, 251],       # DistMult
    7: [44, 51, 73, 118, 116, 204, 350],     # ComplEx
    8: [48, 63, 97, 166, 164, 284, 512],     # ANALOGY
    9: [44, 50, 61, 87, 86, 142, 254],       # TransM
    10: [38, 43, 55, 84, 83, 127, 251],      # CP
    11: [42, 52, 72, 117, 116, 204, 356],    # SimplE
    12: [42, 52, 72, 117, 116, 204, 356],    # SimplE_ignr
    13: [60, 67, 108, 186, 184, 324, 512],   # QuatE
    18: [51, 62, 80, 122, 120, 208, 355],    # KG2E
}
# the many-row models at the widest rows: their k_score_fwd twins spill too (the issue's "may keep doing so")
MAY_SPILL = {(8, 64, 16), (8, 64, 32), (13, 64, 32), (18, 64, 32), (3, 64, 32)}
SMALL = {"_ZN3kge12k_cand_items": (24, 8192), "_ZN3kge24k_rank_lists_from_scoresIfE": (24, 0), "_ZN3kge24k_rank_lists_from_scoresIdE": (24, 0)}


def _key(name):
    return tuple(int(x) for x in re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)E", name).groups())


def _clean(md):
    return (int(md["private_segment_fixed_size"]) == 0 and int(md["vgpr_spill_count"]) == 0 and int(md.get("sgpr_spill_count", 0)) == 0)


def _instances(metadata, stem):   # noqa: F811
    return {_key(k): v for k, v in metadata.items() if ("%d%sI" % (len(stem), stem)) in k}


def test_every_model_and_geometry_is_instantiated(metadata):   # noqa: F811
    cand = _instances(metadata, "k_rank_candidates")
    assert sorted(cand) == sorted((m, g, nch) for m in VGPRS for g, nch in GEOMETRIES)
    assert set(cand) <= set(_instances(metadata, "k_score_fwd"))


@pytest.mark.parametrize("model", sorted(VGPRS))
def test_rank_candidates_needs_no_more_than_its_score_forward_twin(metadata, model):   # noqa: F811
    cand, fwd = _instances(metadata, "k_rank_candidates"), _instances(metadata, "k_score_fwd")
    for i, (g, nch) in enumerate(GEOMETRIES):
        key = (model, g, nch)
        md = cand[key]
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
def test_scan_and_count_kernels(metadata, prefix):   # noqa: F811
    found = [k for k in metadata if k.startswith(prefix)]
    assert len(found) == 1, (prefix, found)
    md = metadata[found[0]]
    vgpr, lds = SMALL[prefix]
    assert _clean(md) and md.get("uses_dynamic_stack", "false") == "false", prefix
    assert int(md["vgpr_count"]) <= vgpr and int(md["group_segment_fixed_size"]) <= lds, (prefix, md["vgpr_count"], md["group_segment_fixed_size"])
