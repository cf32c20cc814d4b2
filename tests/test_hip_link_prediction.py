"""Batched link prediction on the GPU (Evaluator.predict_tails / predict_heads / predict_rels, Trainer.infer_*) for one toy golden case
per model family, loaded the way each family's own GPU test loads it.  The expected value of every list is the numpy restatement of
the select's total order (tests/topk_ref.py) over the rows model.score_rows returns for the same queries: ids exact, scores bit for
bit, nothing has a tolerance."""
import numpy as np
import pytest
import torch

import topk_ref
from golden_util import Case, tie_bracket

pytestmark = pytest.mark.gpu

FLAT = ["transe_l1", "complex", "rescal", "transr_l1", "ntn", "slm", "hole", "kg2e", "octonione", "simple_ties"]   # kge_model_desc models
OWN = ["convkb", "murp"]
PROJECTION = ["tucker", "conve", "proje"]
MAX_QUERIES = 64


@pytest.fixture(autouse=True)
def no_leaked_switches(monkeypatch):
    """Other test modules of this suite leave KGE_* A/B switches set in the process environment: every test here starts without them."""
    from test_tucker_model import SWITCHES
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def load(name):
    """(model on the GPU, E, R, train, valid, test, config hyper-parameters, config keywords) of a toy case."""
    import hip_util
    if name in FLAT:
        c = Case(name)
        prefix = "adam.final." if any(k.startswith("adam.final.") for k in c.z.files) else "init."
        return hip_util.model_from_case(c, prefix), c.E, c.R, c.train, c.valid, c.test, c.hp, {}
    if name == "convkb":
        from test_convkb_model import ConvCase
        c = ConvCase(name)
        return c.build("adam.final.", device="cuda"), c.E, c.R, c.train, c.valid, c.test, c.hp, {}
    if name == "murp":
        from test_murp_model import golden, tables
        from test_hip_murp import model_with
        g = golden("ref_murp")
        hp = dict(hidden_size=int(g["k"]), neg_rate=3, lmbda=0.0)
        q = g["eval.queries"]
        return (model_with(g, tables(g, "live.")), int(g["E"]), int(g["R"]), g["eval.known"], q[:4], q, hp,
                dict(optimizer="riemannian", lr=50.0, batch_size=8))
    if name == "tucker":
        from test_tucker_model import fixture, tables
        from test_hip_tucker import DROP, model_for
        z = fixture(name)
        m = model_for(tables(z), DROP)
    elif name == "conve":
        from test_conve_model import fixture, tables
        from test_hip_conve import model_for
        z = fixture(name)
        m = model_for(tables(z), (0.2, 0.2, 0.3), counters=2)
    else:
        from test_proje_model import fixture, tables
        from test_hip_proje import model_for
        z = fixture(name)
        m = model_for(tables(z), p=0.5)
    return m, int(z["E"]), int(z["R"]), z["train"], z["valid"], z["test"], {"neg_rate": 1 if name == "proje" else 0}, dict(batch_size=9)


class Env:
    def __init__(self, name):
        import hip_util
        from pykg2vec_amd.evaluator import Evaluator
        self.name = name
        self.m, self.E, self.R, train, valid, test, hp, kw = load(name)
        self.m.eval()
        self.cfg = hip_util.make_config(self.E, self.R, hp, train, valid, test, **kw)
        self.cfg.knowledge_graph.cache.update(idx2entity={i: "entity %d" % i for i in range(self.E)},
                                              idx2relation={i: "relation %d" % i for i in range(self.R)})
        self.q = np.ascontiguousarray(test[:MAX_QUERIES], dtype=np.int64)
        self.n = len(self.q)
        self.ev = Evaluator(self.m, self.cfg)
        self.k = min(self.E, 1024)
        self.largest = bool(self.m.higher_is_better)
        self.hr_t, self.tr_h = self.cfg.knowledge_graph.cache["hr_t"], self.cfg.knowledge_graph.cache["tr_h"]
        qd = hip_util.dev(self.q)
        # the reference rows, computed once: side 0 = tails of (h, r), side 1 = heads of (r, t).  RESCAL's evaluation renormalises
        # its tables in place on every call, which may move a row by an ulp: iterate to the fixed point, where every later call sees
        # the same tables
        for _ in range(8):
            before = [p.detach().clone() for p in self.m.parameters()]
            self.rows = [self.m.score_rows(qd, side).cpu().numpy() for side in (0, 1)]
            if all(torch.equal(a, b) for a, b in zip(before, self.m.parameters())):
                break
        else:
            raise AssertionError("%s: the evaluation form keeps changing the tables" % name)

    def predict(self, side, **kw):
        q = self.q
        out = self.ev.predict_heads(q[:, 1], q[:, 2], **kw) if side else self.ev.predict_tails(q[:, 0], q[:, 1], **kw)
        return tuple(x.cpu().numpy() for x in out)

    def known(self, i, side):
        h, r, t = (int(x) for x in self.q[i])
        return self.tr_h[(t, r)] if side else self.hr_t[(h, r)]


_ENVS = {}


@pytest.fixture(params=FLAT + OWN + PROJECTION)
def env(request):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    if request.param not in _ENVS:
        _ENVS[request.param] = Env(request.param)
    return _ENVS[request.param]


def same(got, want):
    ids, vals = got
    assert ids.dtype == np.int64 and np.array_equal(ids, want[0]), np.argwhere(ids != want[0])[:8]
    live = want[0] >= 0
    assert np.array_equal(topk_ref.bits(vals)[live], topk_ref.bits(want[1])[live]) and np.isnan(vals[~live]).all()


def test_unfiltered_predictions_are_the_total_order_of_score_rows(env):
    """(a): mixed relations in one call; the answer does not depend on the chunk size."""
    assert env.n > 8 and len(set(env.q[:, 1].tolist())) > 1
    assert env.largest == (env.name in PROJECTION + ["murp"])
    assert env.rows[0].dtype == (np.float64 if env.name == "murp" else np.float32) and env.rows[0].shape == (env.n, env.E)
    budget = type(env.ev).PREDICT_SCRATCH_BYTES
    for side in (0, 1):
        want = topk_ref.topk_ref(env.rows[side], env.k, env.largest)
        same(env.predict(side, topk=env.k), want)
        try:
            for rows in (1, 7, env.n):
                env.ev.PREDICT_SCRATCH_BYTES = rows * env.E * env.ev.PREDICT_ROW_ITEM_BYTES
                same(env.predict(side, topk=env.k), want)
        finally:
            env.ev.PREDICT_SCRATCH_BYTES = budget
        same(env.predict(side, topk=3), tuple(a[:, :3] for a in want[:2]))


def test_filtered_predictions_leave_known_entities_out_and_bracket_the_true_one(env):
    """(b), and (c) for the flat-descriptor models: the true entity's place equals rank_all's filtered rank wherever no candidate
    ties it."""
    places = np.full((2, env.n), -1)
    for side in (0, 1):
        ids, _ = env.predict(side, topk=env.k, filtered=True)
        true = env.q[:, 0 if side else 2]
        kept, _ = env.predict(side, topk=env.k, filtered=True, keep=true.tolist())
        for i in range(env.n):
            known = env.known(i, side)
            assert not set(ids[i][ids[i] >= 0].tolist()) & known, (side, i)
            row = env.rows[side][i]
            _, _, fless, fties = tie_bracket(-row if env.largest else row, int(true[i]), known)
            where = np.flatnonzero(kept[i] == true[i])
            if fless + fties < env.k:
                assert len(where) == 1 and fless <= where[0] <= fless + fties, (side, i, where, fless, fties)
                places[side, i] = where[0]
    if env.name in FLAT:
        ranks, ties = env.ev.rank_all(env.q, env.n, return_ties=True)
        ranks, ties = ranks.cpu().numpy(), ties.cpu().numpy()      # ranks: head, tail, filtered head, filtered tail; ties: head, tail
        for side, frank, tie in ((0, ranks[3], ties[1]), (1, ranks[2], ties[0])):
            pick = (tie == 0) & (places[side] >= 0)
            assert pick.sum() > 0 or (tie < 0).all()     # (-1: a sweep that does not count ties, NTN / SLM)
            assert np.array_equal(places[side][pick], frank[pick]), (side, places[side][pick], frank[pick])


def test_predict_rels(env):
    """(d): the total order of forward() over all relations; refused for the projection models."""
    import hip_util
    h, t = env.q[:, 0], env.q[:, 2]
    if env.name in PROJECTION:
        with pytest.raises(ValueError, match="projection"):
            env.ev.predict_rels(h, t, topk=3)
        return
    R, n = env.R, env.n
    rel = torch.arange(R, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        rows = env.m.forward(hip_util.dev(h).repeat_interleave(R), rel.repeat(n), hip_util.dev(t).repeat_interleave(R)).view(n, R)
    k = min(R, 1024)
    got = tuple(x.cpu().numpy() for x in env.ev.predict_rels(h, t, topk=k))
    same(got, topk_ref.topk_ref(rows.cpu().numpy(), k, env.largest))


def test_existing_rank_hook_is_unchanged(env):
    """(f): predict_tail_rank still lists ids in torch.topk's order of the row it always swept (MuRP: its stable sort)."""
    import hip_util
    h, r, t = (hip_util.dev(env.q[:1, j]) for j in range(3))
    got = env.m.predict_tail_rank(h, r, topk=5).cpu().numpy().reshape(-1)
    row = torch.from_numpy(env.rows[0][0]).cuda()
    if env.name == "murp":
        want = torch.sort(row, descending=bool(env.m.rank_order), stable=True)[1]
    elif env.name in PROJECTION:
        want = torch.topk(-row, k=5)[1]
    else:
        want = torch.topk(row, k=5)[1]
    assert np.array_equal(got, want.cpu().numpy().reshape(-1))


def test_trainer_infer(env):
    """(e): the reference's {id: name} dict in prediction order; projection models answer in evaluation form whatever their mode and
    draw nothing."""
    from pykg2vec_amd.trainer import Trainer
    tr = Trainer(env.m, env.cfg)
    tr.build_model()
    h, r, t = (int(x) for x in env.q[0])
    names = env.cfg.knowledge_graph.cache["idx2entity"]
    tails = topk_ref.row_order(env.rows[0][0], env.largest)[:5].tolist()
    heads = [e for e in topk_ref.row_order(env.rows[1][0], env.largest).tolist() if e not in env.tr_h[(t, r)]][:5]
    env.m.eval()
    assert list(tr.infer_tails(h, r, topk=5).items()) == [(e, names[e]) for e in tails]
    assert list(tr.infer_heads(r, t, topk=5, filtered=True).items()) == [(e, names[e]) for e in heads]
    rels = tr.infer_rels(h, t, topk=3)
    if env.name in PROJECTION:
        assert rels == {}
        env.m.train()
        try:
            offset = env.m.dropout_offset
            buffers = [b.clone() for b in env.m.buffers()]
            assert list(tr.infer_tails(h, r, topk=5)) == tails and list(tr.infer_heads(r, t, topk=5, filtered=True)) == heads
            assert env.m.dropout_offset == offset and env.m.training
            assert all(torch.equal(a, b) for a, b in zip(buffers, env.m.buffers()))
        finally:
            env.m.eval()
    else:
        ids, _ = env.ev.predict_rels([h], [t], topk=3)
        assert list(rels) == [i for i in ids.cpu().numpy()[0].tolist() if i >= 0] and len(rels) == min(3, env.R)
        assert all(v == "relation %d" % i for i, v in rels.items())
