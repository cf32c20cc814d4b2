"""`pykg2vec_amd.integration.install_models` patches the drop-in classes into the reference's model
modules (`pykg2vec.models.pairwise` / `.pointwise`, where the reference's Importer looks them up) and its handle puts the
originals back.  The reference's modules are stood in for by empty modules holding one placeholder class per name, so what is
under test is the patch / undo logic, not the reference."""
import sys
import types

import pytest


@pytest.fixture
def stand_in_reference(monkeypatch):
    """`pykg2vec.models.pairwise` / `.pointwise` as modules of placeholder classes, for one test (sys.modules restored after)."""
    from pykg2vec_amd import integration
    root, models = types.ModuleType("pykg2vec"), types.ModuleType("pykg2vec.models")
    root.__path__, models.__path__ = [], []
    root.models = models
    mods = {"pykg2vec": root, "pykg2vec.models": models}
    for sub, names in (("pairwise", integration.PAIRWISE), ("pointwise", integration.POINTWISE)):
        name = "pykg2vec.models." + sub
        m = types.ModuleType(name)
        for n in names:
            setattr(m, n, type(n, (), {"__module__": name}))
        setattr(models, sub, m)
        mods[name] = m
    for name, m in mods.items():
        monkeypatch.setitem(sys.modules, name, m)
    return mods["pykg2vec.models.pairwise"], mods["pykg2vec.models.pointwise"]


def test_install_models_is_undone_by_its_handle(stand_in_reference):
    from pykg2vec_amd import integration
    ref_pw, ref_pt = stand_in_reference
    before = {(m, n): getattr(m, n) for m, names in ((ref_pw, integration.PAIRWISE), (ref_pt, integration.POINTWISE)) for n in names}
    with integration.install_models():
        assert ref_pw.TransE.__module__ == "pykg2vec_amd.pairwise" and ref_pt.Complex.__module__ == "pykg2vec_amd.pointwise"
        with integration.install_models():          # nested / repeated installs keep the ORIGINAL classes on record
            pass
        assert ref_pw.TransE.__module__ == "pykg2vec_amd.pairwise"
    for (m, n), cls in before.items():
        assert getattr(m, n) is cls, n
