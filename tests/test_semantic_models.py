"""SLM, SME and SME_BL as drop-in model classes (CPU only): importer keys, constructor contract, parameter names and order
against the reference's state dicts frozen in tests/golden/ref_{slm,sme,sme_bl}.npz, and the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import pykg2vec_amd
from golden_util import Case
from pykg2vec_amd import _lib, integration, kernels
from pykg2vec_amd.common import TrainingStrategy

CLASSES = {"slm": "SLM", "sme": "SME", "sme_bl": "SME_BL"}


def build(name, **over):
    c = Case(name)
    kw = dict(c.hp)
    kw.update(tot_entity=c.E, tot_relation=c.R)
    kw.update(over)
    return c, pykg2vec_amd.import_model(name)(**kw)


@pytest.mark.parametrize("name", list(CLASSES))
def test_import_model_returns_the_class(name):
    cls = pykg2vec_amd.import_model(name)
    assert cls.__name__ == CLASSES[name]
    assert pykg2vec_amd.import_model(name.upper()) is cls
    assert kernels.MODEL_IDS[name] == {"slm": _lib.SLM, "sme": _lib.SME, "sme_bl": _lib.SME_BL}[name]
    assert (_lib.SLM, _lib.SME, _lib.SME_BL) == (15, 16, 17)


@pytest.mark.parametrize("name", list(CLASSES))
def test_state_dict_and_parameter_list_match_the_reference(name):
    c, m = build(name)
    init = {k[len("init."):]: c.z[k] for k in c.z.files if k.startswith("init.")}
    sd = m.state_dict()
    assert list(sd) == list(init)
    for k, v in init.items():
        assert tuple(sd[k].shape) == v.shape, k
    named = {id(p): n for n, p in m.named_parameters()}
    assert [named[id(e.weight)] for e in m.parameter_list] == list(init)
    assert [e.name for e in m.parameter_list][:2] == ["ent_embedding", "rel_embedding"]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})   # reference weights load as they are
    assert torch.equal(m.ent_embeddings.weight, torch.from_numpy(init["ent_embeddings.weight"]))


@pytest.mark.parametrize("name", list(CLASSES))
def test_model_name_strategy_and_missing_parameter(name):
    _, m = build(name)
    assert m.model_name == name
    assert m.training_strategy == TrainingStrategy.PAIRWISE_BASED
    assert m.loss.__name__ == "pairwise_hinge"
    kw = dict(Case(name).hp, tot_relation=3)
    with pytest.raises(Exception, match="tot_entity"):
        pykg2vec_amd.import_model(name)(**kw)


def test_names_are_installed_by_integration():
    for n in ("SLM", "SME", "SME_BL"):
        assert n in integration.PAIRWISE
    from pykg2vec_amd import pairwise
    assert issubclass(pairwise.SME_BL, pairwise.SME)


@pytest.mark.parametrize("name", list(CLASSES))
def test_cpu_tensors_are_refused(name):
    _, m = build(name)
    h = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(_lib.KgeHipError):
        m(h, h, h)


def test_embed_returns_the_reference_tuple():
    _, m = build("sme")
    h = torch.tensor([0, 1])
    eh, er, et = m.embed(h, h, h)
    assert eh.shape == (2, m.hidden_size) and er.shape == (2, m.hidden_size)
    assert np.array_equal(eh.detach().numpy(), m.ent_embeddings.weight[:2].detach().numpy())
