"""The host layer of the conv 1-N models (ConvE, HypER, InteractE, AcrE) without a GPU: the op schemas, the size of `saved` the fake
kernels answer against the library's kge_<stem>_saved_floats, every descriptor-builder refusal that fires before a device pointer is
taken, and the bookkeeping of forward() / fused_projection_step (dropout offset, direction argument, num_batches_tracked).  Needs the
built library, no device."""
import ctypes
import os
import re
import sys
import types

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pykg2vec_amd import _lib as L, kernels as K, projection  # noqa: E402

STEMS = ("conve", "hyper", "interacte", "acre")
E, R = 10, 3


# ---------------------------------------------------------------- 1. schemas
FORWARD = "kge::%s_body(SymInt key, Tensor e, Tensor r, SymInt %s, SymInt seed, SymInt offset, Tensor[] weights) -> (Tensor, Tensor)"
BACKWARD = ("kge::%s_body_backward(SymInt key, Tensor e, Tensor r, SymInt %s, SymInt seed, SymInt offset, Tensor dx, Tensor saved, "
            "Tensor[] weights) -> Tensor[]")
SCHEMAS = {
    "conve_body": FORWARD % ("conve", "side"), "conve_body_backward": BACKWARD % ("conve", "side"),
    "hyper_body": FORWARD % ("hyper", "row0"), "hyper_body_backward": BACKWARD % ("hyper", "row0"),
    "interacte_body": FORWARD % ("interacte", "row0"), "interacte_body_backward": BACKWARD % ("interacte", "row0"),
    "acre_body": FORWARD % ("acre", "row0"), "acre_body_backward": BACKWARD % ("acre", "row0"),
}


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_schema_is_the_recorded_one(name):
    from pykg2vec_amd import ops
    assert str(getattr(torch.ops.kge, name).default._schema) == SCHEMAS[name]
    assert callable(getattr(ops, name))      # the module-level name stays importable


# ---------------------------------------------------------------- 2. the size of `saved`
def _dummy(desc_type, names, **geometry):
    """A descriptor with dummy pointers, as the _desc() helpers of the test_*_model.py files build it: kge_*_saved_floats reads the
    geometry and refuses null tables, it dereferences nothing."""
    d = desc_type()
    d.tot_entity, d.tot_relation, d.train = E, R, 1
    for f, v in geometry.items():
        setattr(d, f, v)
    for i in range(3):
        d.eps[i], d.momentum[i] = 1e-5, 0.1
    for f in tuple(names) + L.CONVE_BUFFERS + tuple("g_" + n for n in names):
        setattr(d, f, 0x1000)
    return d


def _conve(k, h1):
    return (_dummy(L.ConveDesc, L.CONVE_TABLES, hidden_size=k, hidden_size_1=h1), K.conve_shapes(E, R, k, h1)[0], k)


def _hyper(D, Dr):
    return (_dummy(L.HyperDesc, L.HYPER_TABLES, ent_hidden_size=D, rel_hidden_size=Dr), K.hyper_shapes(E, R, D, Dr)[0], D)


def _interacte(rh, rw, P, NF, ks):
    d = _dummy(L.InteracteDesc, L.INTERACTE_TABLES, reshape_height=rh, reshape_width=rw, feature_permutation=P, num_filters=NF,
               kernel_size=ks)
    d.perm = d.inv_perm = 0x1000
    return (d, K.interacte_shapes(E, R, rh, rw, P, NF, ks)[0], rh * rw)


def _acre(C, way, bias):
    names, shapes, _ = K.acre_shapes(E, R, C, way, bias)
    d = _dummy(L.AcreDesc, names, hidden_size=200, in_channels=C, way=way, first_atrous=1, second_atrous=2, third_atrous=3,
               acre_bias=int(bias))
    return (d, shapes, 200)


GEOMETRIES = [("conve", _conve, (6, 3)), ("conve", _conve, (20, 5)),
              ("hyper", _hyper, (9, 1)), ("hyper", _hyper, (20, 12)),
              ("interacte", _interacte, (1, 1, 1, 1, 3)), ("interacte", _interacte, (3, 2, 2, 3, 3))] \
    + [("acre", _acre, (1, way, bias)) for way in (0, 1) for bias in (True, False)] \
    + [("acre", _acre, (3, 0, True)), ("acre", _acre, (3, 1, True))]


@pytest.mark.parametrize("n", [2, 5])
@pytest.mark.parametrize("stem,make,geometry", GEOMETRIES, ids=["%s-%s" % (s, "x".join(str(int(v)) for v in g)) for s, _, g in GEOMETRIES])
def test_fake_kernel_answers_the_library_s_saved_size(stem, make, geometry, n):
    from pykg2vec_amd import ops  # noqa: F401  (registers torch.ops.kge.*)
    d, shapes, k = make(*geometry)
    want = int(getattr(L.load(), "kge_%s_saved_floats" % stem)(ctypes.byref(d), n))
    assert want > 0, L.load().kge_last_error()
    with FakeTensorMode():
        ids = torch.empty(n, dtype=torch.int64)
        x, saved = getattr(torch.ops.kge, stem + "_body")(0, ids, ids, 0, 0, 0, [torch.empty(s) for s in shapes])
    print("%s %s n=%d: fake saved %d, library %d" % (stem, geometry, n, saved.numel(), want))
    assert tuple(x.shape) == (n, k)
    assert saved.numel() == want and saved.dim() == 1 and saved.dtype == torch.float32


# ---------------------------------------------------------------- 3. builder refusals that need no device
def _perm(P, k):
    return torch.stack([torch.arange(2 * k).flip(0) if p % 2 else torch.arange(2 * k) for p in range(P)])


def _case(stem):
    """(builder, its keywords, the tables' names, the tables and the buffers as CPU tensors) on the models' fixture geometries."""
    if stem == "conve":
        kw = dict(tot_entity=E, tot_relation=R, hidden_size=20, hidden_size_1=5)
        names, (st, sb) = L.CONVE_TABLES, K.conve_shapes(E, R, 20, 5)
    elif stem == "hyper":
        kw = dict(tot_entity=E, tot_relation=R, ent_hidden_size=20, rel_hidden_size=12)
        names, (st, sb) = L.HYPER_TABLES, K.hyper_shapes(E, R, 20, 12)
    elif stem == "interacte":
        kw = dict(tot_entity=E, tot_relation=R, reshape_height=3, reshape_width=2, feature_permutation=2, num_filters=3, kernel_size=3,
                  chequer_perm=_perm(2, 6))
        names, (st, sb) = L.INTERACTE_TABLES, K.interacte_shapes(E, R, 3, 2, 2, 3, 3)
    else:
        kw = dict(tot_entity=E, tot_relation=R, in_channels=3)
        names, st, sb = K.acre_shapes(E, R, 3, 0, True)
    return getattr(K, stem + "_desc"), kw, tuple(names), [torch.zeros(s) for s in st], [torch.zeros(s) for s in sb]


COUNT = {"conve": "conve: 13 tensors and 6 running buffers expected, got %d and %d",
         "hyper": "hyper: 13 tensors and 6 running buffers expected, got %d and %d",
         "interacte": "interacte: 12 tensors and 6 running buffers expected, got %d and %d",
         "acre": "acre: 17 tensors and 6 running buffers expected (way 'serial', acre_bias True), got %d and %d"}


def _raises(sentence, exc=L.KgeHipError):
    return pytest.raises(exc, match="^" + re.escape(sentence) + "$")


@pytest.mark.parametrize("stem", STEMS)
def test_builder_refuses_wrong_counts(stem):
    build, kw, names, tables, buffers = _case(stem)
    n = len(tables)
    with _raises(COUNT[stem] % (n - 1, 6)):
        build(tables[:-1], buffers, **kw)
    with _raises(COUNT[stem] % (n, 5)):
        build(tables, buffers[:-1], **kw)
    with _raises(COUNT[stem] % (n, 7)):
        build(tables, buffers + buffers[:1], **kw)


@pytest.mark.parametrize("stem", STEMS)
def test_builder_refuses_the_cumulative_moving_average(stem):
    build, kw, names, tables, buffers = _case(stem)
    with _raises("%s: momentum None (the cumulative moving average) is not built" % stem):
        build(tables, buffers, momentum=(0.1, None, 0.1), **kw)
    # the counts are looked at first
    with _raises(COUNT[stem] % (len(tables) - 1, 6)):
        build(tables[:-1], buffers, momentum=(0.1, None, 0.1), **kw)


@pytest.mark.parametrize("stem", STEMS)
def test_builder_refuses_wrong_shapes(stem):
    build, kw, names, tables, buffers = _case(stem)
    i = names.index("fc_w")
    bad = list(tables)
    bad[i] = torch.zeros(tables[i].shape[0], tables[i].shape[1] + 1)
    with _raises("%s: fc_w must be %s (got %s)" % (stem, tuple(tables[i].shape), tuple(bad[i].shape))):
        build(bad, buffers, **kw)
    bad = list(buffers)
    bad[3] = torch.zeros(buffers[3].shape[0] + 1)
    with _raises("%s: bn1_var must be %s (got %s)" % (stem, tuple(buffers[3].shape), tuple(bad[3].shape))):
        build(tables, bad, **kw)
    i, rel = names.index("ent"), tables[names.index("rel")]
    bad = list(tables)
    bad[i] = torch.zeros(E - 1, tables[i].shape[1])
    with _raises("%s: ent_embeddings must be [>= %d, %d] (got %s): an nn.Embedding lookup would raise IndexError"
                 % (stem, E, tables[i].shape[1], tuple(bad[i].shape))):
        build(bad, buffers, **kw)
    bad = list(tables)
    bad[names.index("rel")] = torch.zeros(rel.shape[0] - 1, rel.shape[1])
    with _raises("%s: rel_embeddings must be [>= %d, %d] (got %s): an nn.Embedding lookup would raise IndexError"
                 % (stem, rel.shape[0], rel.shape[1], (rel.shape[0] - 1, rel.shape[1]))):
        build(bad, buffers, **kw)
    # more rows than ids is fine for the two embedding tables: the next refusal is the device's, and it names the first table bound
    bad = list(tables)
    bad[i] = torch.zeros(E + 1, tables[i].shape[1])
    with _raises("%s must live on the HIP device (got cpu); the HIP path has no CPU fallback" % ("perm" if stem == "interacte" else names[0])):
        build(bad, buffers, **kw)


@pytest.mark.parametrize("stem", STEMS)
def test_builder_refuses_a_wrong_gradient_count(stem, monkeypatch):
    """The gradient count is looked at after the tables are bound, so a CPU tensor never gets there: the device test is stubbed out
    (the pointers are bound into the descriptor and never followed)."""
    build, kw, names, tables, buffers = _case(stem)
    monkeypatch.setattr(K, "_dev", lambda t, dtype, what: ctypes.c_void_p(t.data_ptr()))
    grads = [torch.zeros_like(t) for t in tables]
    with _raises("%s: %d gradient tensors expected, got %d" % (stem, len(tables), len(tables) - 1)):
        build(tables, buffers, grads[:-1], **kw)
    with _raises("grad shape (1, 2) != tensor shape %s" % (tuple(tables[1].shape),), ValueError):
        build(tables, buffers, grads[:1] + [torch.zeros(1, 2)] + grads[2:], **kw)
    d = build(tables, buffers, grads, eps=(1e-3, 2e-3, 3e-3), momentum=(0.25, 0.5, 1.0), dropouts=(0.125, 0.25, 0.5), train=True, seed=7,
              offset=3, **kw)
    assert [d.eps[i] for i in range(3)] == [ctypes.c_float(v).value for v in (1e-3, 2e-3, 3e-3)]
    assert [d.momentum[i] for i in range(3)] == [0.25, 0.5, 1.0]
    assert (d.input_dropout, d.feature_map_dropout, d.hidden_dropout) == (0.125, 0.25, 0.5)
    assert (d.train, d.seed, d.offset, d.tot_entity, d.tot_relation) == (1, 7, 3, E, R)
    for name, t, g in zip(names, tables, grads):
        assert getattr(d, name) == t.data_ptr() and getattr(d, "g_" + name) == g.data_ptr(), name
    for name, t in zip(L.CONVE_BUFFERS, buffers):
        assert getattr(d, name) == t.data_ptr(), name
    assert d._ws is None and d._keepalive[0] is tables and d._keepalive[1] is buffers and d._keepalive[2] is grads
    assert build(tables, buffers, **kw).g_fc_w is None


def test_acre_refuses_a_bad_way():
    build, kw, names, tables, buffers = _case("acre")
    with _raises("acre: way must be 'serial' or 'parallel' (got 'both')"):
        build(tables, buffers, way="both", **kw)
    with _raises("acre: way must be 'serial' or 'parallel' (got 'both')"):     # before the counts
        build(tables[:-1], buffers, way="both", **kw)
    with _raises("acre: 19 tensors and 6 running buffers expected (way 'parallel', acre_bias True), got 17 and 6"):
        build(tables, buffers, way="parallel", **kw)
    with _raises("acre: 14 tensors and 6 running buffers expected (way 0, acre_bias False), got 17 and 6"):
        build(tables, buffers, way=0, acre_bias=False, **kw)


def test_interacte_refuses_a_missing_or_broken_chequer_perm():
    build, kw, names, tables, buffers = _case("interacte")
    cp = kw.pop("chequer_perm")
    with _raises("interacte: chequer_perm (or the pair interacte_perm made of it) is required"):
        build(tables, buffers, **kw)
    with _raises(COUNT["interacte"] % (11, 6)):     # the counts and the momenta are looked at first
        build(tables[:-1], buffers, **kw)
    with _raises("interacte: momentum None (the cumulative moving average) is not built"):
        build(tables, buffers, momentum=(None, 0.1, 0.1), **kw)
    bad = cp.clone()
    bad[1, 0] = bad[1, 1]
    with _raises("interacte: row 1 of chequer_perm is not a permutation of [0, 12)"):
        build(tables, buffers, chequer_perm=bad, **kw)
    with _raises("interacte: perm must be (2, 12) (got (1, 12))"):
        build(tables, buffers, perms=(cp[:1].to(torch.int32), cp.to(torch.int32)), **kw)


# ---------------------------------------------------------------- 4. model bookkeeping
MODELS = {
    "conve": ("ConvE", dict(tot_entity=E, tot_relation=R, hidden_size=20, hidden_size_1=5, lmbda=0.1), "b.weight"),
    "hyper": ("HypER", dict(tot_entity=E, tot_relation=R, ent_hidden_size=20, rel_hidden_size=12), "b"),
    "interacte": ("InteractE", dict(tot_entity=E, tot_relation=R, hidden_size=6, feature_permutation=2, num_filters=3, kernel_size=3,
                                    reshape_height=3, reshape_width=2), "bias"),
    "acre": ("AcrE", dict(tot_entity=E, tot_relation=R, hidden_size=200, in_channels=3, way="serial", first_atrous=1, second_atrous=2,
                          third_atrous=3, acre_bias=True), "bias"),
}


def _model(stem, rates):
    cls, kw, bias = MODELS[stem]
    m = getattr(projection, cls)(input_dropout=rates[0], feature_map_dropout=rates[1], hidden_dropout=rates[2], seed=11, **kw)
    return m, dict(m.named_parameters())[bias]


def _stub_ops(monkeypatch, stem):
    calls = []

    def body(key, e, r, side, seed, offset, weights):
        calls.append(("body", key, e, r, side, seed, offset, list(weights)))
        return torch.zeros(e.numel(), 4), torch.zeros(1)

    def head(x, ent, bias, bf16):
        calls.append(("head", x, ent, bias, bf16))
        return torch.zeros(x.shape[0], ent.shape[0])

    from pykg2vec_amd import ops  # noqa: F401  (registers torch.ops.kge.*)
    getattr(torch.ops.kge, stem + "_body"), torch.ops.kge.one_to_n_scores      # (resolved, so that monkeypatch restores them)
    monkeypatch.setattr(torch.ops.kge, stem + "_body", body)
    monkeypatch.setattr(torch.ops.kge, "one_to_n_scores", head)
    return calls


def _counters(m):
    return [int(bn.num_batches_tracked) for bn in (m.bn0, m.bn1, m.bn2)]


@pytest.mark.parametrize("stem", STEMS)
def test_forward_bookkeeping(stem, monkeypatch):
    calls = _stub_ops(monkeypatch, stem)
    e, r = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 2])
    head_arg = 1 if stem == "conve" else e.numel()

    m, bias = _model(stem, (0.2, 0.0, 0.3))
    assert m.training and m.kernel_name == stem
    for bn in (m.bn0, m.bn1, m.bn2):
        bn.num_batches_tracked += 5
    out = m.forward(e, r, direction="tail")
    assert tuple(out.shape) == (3, E)
    m.forward(e, r, direction="head")
    bodies, heads = [c for c in calls if c[0] == "body"], [c for c in calls if c[0] == "head"]
    assert [c[0] for c in calls] == ["body", "head", "body", "head"]
    assert [c[6] for c in bodies] == [0, 1] and [c[4] for c in bodies] == [0, head_arg]
    assert all(c[1] == m._kge_op_key and c[2] is e and c[3] is r and c[5] == 11 for c in bodies)
    tt = m.trainable_tensors()
    assert all(len(c[7]) == len(tt) and all(a is b for a, b in zip(c[7], tt)) for c in bodies)
    assert all(c[2] is m.ent_embeddings.weight and c[3] is bias and c[4] is False for c in heads)
    assert m.dropout_offset == 2 and _counters(m) == [7, 7, 7]
    with pytest.raises(AssertionError, match="^Unknown forward direction$"):
        m.forward(e, r, direction="sideways")
    assert m.dropout_offset == 2 and _counters(m) == [7, 7, 7] and len(calls) == 4

    del calls[:]
    m.eval()
    m.forward(e, r, direction="tail")
    m.forward(e, r, direction="head")
    assert [c[6] for c in calls if c[0] == "body"] == [-1, -1] and [c[4] for c in calls if c[0] == "body"] == [0, head_arg]
    assert m.dropout_offset == 2 and _counters(m) == [7, 7, 7]
    rank = m.predict_tail_rank(e, r, topk=2)
    assert tuple(rank.shape) == (3, 2) and tuple(m.predict_head_rank(e, r, topk=4).shape) == (3, 4)
    assert [c[4] for c in calls if c[0] == "body"][2:] == [0, head_arg]

    del calls[:]
    m, _ = _model(stem, (0.0, 0.0, 0.0))
    m.forward(e, r, direction="tail")
    m.forward(e, r, direction="head")
    assert [c[6] for c in calls if c[0] == "body"] == [0, 0] and [c[4] for c in calls if c[0] == "body"] == [0, head_arg]
    assert m.dropout_offset == 0 and _counters(m) == [2, 2, 2]


@pytest.mark.parametrize("stem", STEMS)
@pytest.mark.parametrize("smoothing", [0.1, None])
def test_fused_step_bookkeeping(stem, smoothing):
    m, _ = _model(stem, (0.2, 0.2, 0.3))
    seen = []
    stub = types.SimpleNamespace(**{stem + "_train_bce": lambda *a: seen.append(a)})
    config = types.SimpleNamespace(label_smoothing=0.1) if smoothing is not None else types.SimpleNamespace()
    desc, h, r, t, loss = object(), object(), object(), object(), object()
    m.fused_projection_step(stub, desc, h, r, t, ("ho", "hi"), ("to", "ti"), None, config, loss)
    assert seen == [(desc, h, r, t, "ho", "hi", "to", "ti", smoothing, loss)]
    assert _counters(m) == [2, 2, 2] and m.dropout_offset == 0     # the offset of a fused step is its caller's
    assert [tuple(b.shape) for b in m.running_buffers()] == [tuple(t.shape) for bn in (m.bn0, m.bn1, m.bn2)
                                                             for t in (bn.running_mean, bn.running_var)]
    assert all(a is b for a, b in zip(m.running_buffers(), [t for bn in (m.bn0, m.bn1, m.bn2) for t in (bn.running_mean, bn.running_var)]))
