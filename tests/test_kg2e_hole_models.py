"""KG2E and HoLE as drop-in model classes (CPU only): importer keys and ids, constructor contract, parameter names and order
against the reference's state dicts frozen in tests/golden/ref_{kg2e,kg2e_clip,hole}.npz, KG2E's sigma initialisation, the
legacy-FFT closed form of HoLE against the reference's scores, the refusal of CPU tensors, and the library's exports."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pykg2vec_amd
from golden_util import Case
from pykg2vec_amd import _lib, integration, kernels
from pykg2vec_amd.common import TrainingStrategy

CASES = {"kg2e": "kg2e", "kg2e_clip": "kg2e", "hole": "hole"}
CLASSES = {"kg2e": "KG2E", "hole": "HoLE"}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(case, **over):
    c = Case(case)
    kw = dict(c.hp)
    kw.update(tot_entity=c.E, tot_relation=c.R)
    kw.update(over)
    return c, pykg2vec_amd.import_model(CASES[case])(**kw)


@pytest.mark.parametrize("name", list(CLASSES))
def test_import_model_returns_the_class(name):
    cls = pykg2vec_amd.import_model(name)
    assert cls.__name__ == CLASSES[name]
    assert pykg2vec_amd.import_model(name.upper()) is cls
    assert pykg2vec_amd.import_model(CLASSES[name]) is cls
    assert kernels.MODEL_IDS[name] == {"kg2e": _lib.KG2E, "hole": _lib.HOLE}[name]
    assert (_lib.KG2E, _lib.HOLE) == (18, 19)


@pytest.mark.parametrize("case", list(CASES))
def test_state_dict_and_parameter_list_match_the_reference(case):
    c, m = build(case)
    init = {k[len("init."):]: c.z[k] for k in c.z.files if k.startswith("init.")}
    sd = m.state_dict()
    assert list(sd) == list(init)
    for k, v in init.items():
        assert tuple(sd[k].shape) == v.shape, k
    named = {id(p): n for n, p in m.named_parameters()}
    want = (["ent_embeddings_mu.weight", "ent_embeddings_sigma.weight", "rel_embeddings_mu.weight", "rel_embeddings_sigma.weight"]
            if CASES[case] == "kg2e" else ["ent_embeddings.weight", "rel_embeddings.weight"])
    assert [named[id(e.weight)] for e in m.parameter_list] == want
    m.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})   # reference weights load as they are


SEEDS = {"kg2e": 3201, "kg2e_clip": 3202, "hole": 3203}   # tools/make_golden_kg2e_hole.py: torch.manual_seed, then the constructor


@pytest.mark.parametrize("case", list(CASES))
def test_initialisation_equals_the_reference_under_its_seed(case):
    """Same draws in the same order (four / two xavier_uniform_ tables), then KG2E's sigma clip: the whole initial state
    equals the fixture's, so the clip is the reference's max(cmin, min(cmax, sigma + 1))."""
    torch.manual_seed(SEEDS[case])
    c, m = build(case)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), c.z["init." + k]), k
    if case == "kg2e":   # the reference's swapped defaults cmax = 0.05, cmin = 5.0: every sigma entry is exactly 5.0
        assert np.all(m.ent_embeddings_sigma.weight.detach().numpy() == 5.0)
        assert np.all(m.rel_embeddings_sigma.weight.detach().numpy() == 5.0)
    if case == "kg2e_clip":   # cmax = 5.0, cmin = 0.05: sigma + 1, rows of varying norm
        w = m.ent_embeddings_sigma.weight.detach().numpy()
        assert 0.05 < w.min() and w.max() < 5.0 and np.linalg.norm(w, axis=1).std() > 0.01


@pytest.mark.parametrize("name", list(CLASSES))
def test_model_name_strategy_and_missing_parameter(name):
    _, m = build(name)
    assert m.model_name == name
    assert m.training_strategy == TrainingStrategy.PAIRWISE_BASED
    assert m.loss.__name__ == "pairwise_hinge"
    for missing in ("tot_entity", "cmax"):
        kw = dict(Case(name).hp, tot_entity=5, tot_relation=3)
        del kw[missing]
        with pytest.raises(Exception, match=missing):
            pykg2vec_amd.import_model(name)(**kw)


def test_names_are_installed_by_integration():
    for n in ("KG2E", "HoLE"):
        assert n in integration.PAIRWISE


@pytest.mark.parametrize("name", list(CLASSES))
def test_cpu_tensors_are_refused(name):
    _, m = build(name)
    h = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(_lib.KgeHipError):
        m(h, h, h)


def test_embed_returns_the_reference_tuples():
    _, m = build("kg2e_clip")
    i = torch.tensor([0, 1])
    out = m.embed(i, i, i)
    assert len(out) == 6
    hm = m.ent_embeddings_mu.weight[:2]
    assert torch.allclose(out[0], hm / hm.norm(dim=1, keepdim=True))
    assert torch.allclose(out[3], m.rel_embeddings_sigma.weight[:2] / m.rel_embeddings_sigma.weight[:2].norm(dim=1, keepdim=True))
    _, m = build("hole")
    eh, er, et = m.embed(i, i, i)
    assert torch.equal(eh, m.ent_embeddings.weight[:2]) and torch.equal(er, m.rel_embeddings.weight[:2])


# ---------------------------------------------------------------- HoLE's legacy-FFT closed form
def hole_energy64(ent, rel, h, r, t):
    d = ent.shape[1]
    jk = np.outer(np.arange(d), np.arange(d)) % d
    C, S = np.cos(2 * np.pi * jk / d), np.sin(2 * np.pi * jk / d)
    rr = rel[r] / np.maximum(np.linalg.norm(rel[r], axis=1, keepdims=True), 1e-12)
    eh, et = ent[h], ent[t]
    x = ((eh @ C) * (et @ C) * (rr @ C) - (eh @ S) * (et @ S) * (rr @ S)).sum(1) / d
    return -1.0 / (1.0 + np.exp(-x))


def test_hole_closed_form_reproduces_the_reference():
    c = Case("hole")
    ent, rel = c.z["init.ent_embeddings.weight"].astype(np.float64), c.z["init.rel_embeddings.weight"].astype(np.float64)
    b = c.batch(0)
    assert np.allclose(hole_energy64(ent, rel, b[0], b[1], b[2]), c.z["scores0_pos"], atol=1e-6, rtol=0)
    assert np.allclose(hole_energy64(ent, rel, b[3], b[4], b[5]), c.z["scores0_neg"], atol=1e-6, rtol=0)
    ent, rel = c.z["adam.final.ent_embeddings.weight"].astype(np.float64), c.z["adam.final.rel_embeddings.weight"].astype(np.float64)
    E = c.E
    rows = []
    for h, r, t in c.test[:4]:
        rows.append(hole_energy64(ent, rel, np.full(E, h), np.full(E, r), np.arange(E)))
        rows.append(hole_energy64(ent, rel, np.arange(E), np.full(E, r), np.full(E, t)))
    assert np.allclose(np.stack(rows), c.z["eval.sweeps"], atol=1e-6, rtol=0)
    # the score is symmetric in h and t
    assert np.allclose(hole_energy64(ent, rel, b[0], b[1], b[2]), hole_energy64(ent, rel, b[2], b[1], b[0]), atol=1e-12)


def test_library_still_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "kge_hip.h")).read()
    declared = set(re.findall(r"\b(kge_[a-z0-9_]+)\s*\(", header))
    lib = os.path.join(ROOT, "pykg2vec_amd", "libkge_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert declared and declared <= exported, sorted(declared - exported)
    assert "KGE_KG2E = 18" in header and "KGE_HOLE = 19" in header
