"""Every rank pass of the library at its chunk, tile, threshold and tie edges against plain numpy counts (tests/rank_edges_ref.py).

Set A: query counts around the 16 / 8-query wave passes, the 64-row body tiles, the 256-triple chunks of the materialise-and-count
passes and the 512-row matrix-core threshold, at entity counts around the 64- / 256-candidate tiles (and E = 1, 2).  The integer
output (raw rank, filtered rank, tie count) must equal the numpy count over the family's OWN evaluation rows with no tolerance and no
allowed mismatch; the rows themselves are tied to their queries by a nearest-row check against forward() (a materialise-and-count
pass reads its ranks from the rows it returns, so a shared offset bug would pass the count) and to rounding by a closeness bound.
Set B: the true entity's rows copied onto other entities.  The copy must tie the original bit for bit, which a one-ulp disagreement
between the kernel of the true candidate's energy and the sweep kernel would break (rank + 1, tie count 0).

Rank entry points of include/kge_hip.h and the families below that reach them (ENTRY):
kge_eval_ranks / kge_eval_ranks_ties, kge_eval_ranks_grouped / kge_eval_ranks_grouped_ties, kge_head_1n_rank, kge_convkb_eval_ranks,
kge_murp_eval_ranks, kge_tucker_eval_ranks, kge_proje_eval_ranks, kge_conve_eval_ranks, kge_hyper_eval_ranks,
kge_interacte_eval_ranks, kge_acre_eval_ranks.

Closeness of a sweep row to forward(): atol = rtol = 2e-5, the sweep-versus-forward tolerance of the KG2E / HoLE, semantic, OctonionE
and ConvKB test files; the 21 flat models use the same figure (each side is held to atol = rtol = 1e-5 of the reference by
test_hip_parity.py).  The 1-N head has no such figure: its energies and forward()'s predictions are both measured against the float64
head sigmoid(x @ ent.T + b) of the same fp32 body rows x, and the energies are allowed 4 x forward()'s deviation, floored at one fp32
ulp of 1 (2^-23).  MuRP uses test_murp_model.near.  profiles/r23_rank_edges.txt lists what was measured."""
import numpy as np
import pytest
import torch

import rank_edges_ref as ref
from golden_util import CASES, Case, rank_band_ok

gpu = pytest.mark.gpu
R = 8
SET_A = [(n, E) for E in (65, 257) for n in (1, 17, 255, 256, 257, 515)] + [(3, 1), (3, 2)]
TOL = 2e-5
ULP = 2.0 ** -23

# family -> the rank entry points of include/kge_hip.h its case runs
FLAT_ENTRY = "kge_eval_ranks kge_eval_ranks_ties"
ENTRY = {name: FLAT_ENTRY for name in CASES}
ENTRY.update({"transh_l1": FLAT_ENTRY + " kge_eval_ranks_grouped kge_eval_ranks_grouped_ties",
              "transh_l2": FLAT_ENTRY + " kge_eval_ranks_grouped kge_eval_ranks_grouped_ties",
              "transd_l1": FLAT_ENTRY + " kge_eval_ranks_grouped kge_eval_ranks_grouped_ties",
              "transd_l2": FLAT_ENTRY + " kge_eval_ranks_grouped kge_eval_ranks_grouped_ties",
              "transr_l1": FLAT_ENTRY + " kge_eval_ranks_grouped kge_eval_ranks_grouped_ties",
              "transr_l2": FLAT_ENTRY + " kge_eval_ranks_grouped kge_eval_ranks_grouped_ties",
              "sme": FLAT_ENTRY, "sme_bl": FLAT_ENTRY, "hole": FLAT_ENTRY, "octonione": FLAT_ENTRY,        # launch_dot_eval
              "kg2e": FLAT_ENTRY, "slm": FLAT_ENTRY,                                                        # materialise and count (+ ntn)
              "conve": "kge_conve_eval_ranks kge_head_1n_rank", "hyper": "kge_hyper_eval_ranks kge_head_1n_rank",
              "interacte": "kge_interacte_eval_ranks kge_head_1n_rank", "acre_serial": "kge_acre_eval_ranks kge_head_1n_rank",
              "acre_parallel": "kge_acre_eval_ranks kge_head_1n_rank", "tucker": "kge_tucker_eval_ranks kge_head_1n_rank",
              "proje": "kge_proje_eval_ranks kge_head_1n_rank",
              "convkb": "kge_convkb_eval_ranks", "murp": "kge_murp_eval_ranks", "murp_order1": "kge_murp_eval_ranks"})
ONE_TO_N = ("conve", "hyper", "interacte", "acre_serial", "acre_parallel", "tucker", "proje")
NO_TIE_REPORT = ("ntn", "slm", "convkb")       # the documented -1 (NTN's and SLM's sweeps; ConvKB's entry point has no tie argument)
TWO_WIDTHS = [f for f in ENTRY if f not in ONE_TO_N]
FAMILIES = [(f, w) for f in ENTRY for w in ((6, 32) if f in TWO_WIDTHS else (0,))]
GROUP_ALL = ("transh_l1", "transh_l2", "transd_l1", "transd_l2")     # run once more with GROUPED_MIN_TRIPLES_PER_RELATION = 0
IDS = ["%s-w%d" % fw for fw in FAMILIES]


@pytest.fixture(autouse=True)
def no_leaked_switches(monkeypatch):
    from test_tucker_model import SWITCHES
    for k in SWITCHES + ("KGE_EVAL_GEMM",):
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------- the numpy helper on a hand-written row (no GPU)
def test_reference_counts_on_a_hand_written_row():
    #                 0    1    2    3    4    5    6
    row = np.asarray([3.0, 1.0, 2.0, 2.0, 0.5, 2.0, 4.0], dtype=np.float32)
    # true id 2 (energy 2.0): lower 1, 4; tied 3, 5.  Known: 1 (lower), 5 (tied), 2 (the true id itself), 6 (higher)
    assert ref.counts(row, 2, ()) == (2, 2, 2, 2)
    assert ref.counts(row, 2, {1, 5, 2, 6}) == (2, 1, 2, 1)
    assert ref.counts(row, 2, {2}) == (2, 2, 2, 2)
    assert ref.counts(-row, 2, {1, 5, 2, 6}) == (2, 1, 2, 1)     # negated ("higher is better") rows: 0 and 6 are now lower
    assert ref.counts(row, 4, set(range(7))) == (0, 0, 0, 0)
    assert ref.counts(row, 6, set(range(7))) == (6, 0, 0, 0)
    got = ref.counts_all(np.stack([row, row]), [2, 6], [{1, 5, 2, 6}, ()])
    assert got.tolist() == [[2, 6], [1, 6], [2, 0], [1, 0]]
    rng = np.random.default_rng(0)
    for n, E in SET_A:
        q = ref.distinct_queries(rng, n, E, R)
        known = ref.known_triples(rng, q, E, R)
        assert q.shape == (n, 3) and not ((known[:, 0] == q[0, 0]) & (known[:, 1] == q[0, 1])).any()
        heads = {int(h) for h, r, t in known if (r, t) == (q[-1, 1], q[-1, 2])}
        assert len(heads) >= E - 1
        off, ids = ref.csr([{3, 1}, set(), {2}])
        assert off.tolist() == [0, 2, 2, 3] and ids.tolist() == [1, 3, 2] and ids.dtype == np.int32


# ---------------------------------------------------------------- random small models
def _hp(name, d):
    c = Case(name)
    hp = {k: v for k, v in c.hp.items() if k != "theta"}
    for k in ("hidden_size", "ent_hidden_size", "rel_hidden_size"):
        if k in hp:
            hp[k] = d
    return c.model, hp


def build(family, width, E, seed=5):
    """The family's random model on the GPU in eval mode: its test file's random-shape builder where it has one, at the smallest
    shape it accepts.  AcrE takes two channels: with one, the ReLU behind bn2 leaves so little of the body at E = 65 that many
    distinct (e, r) pairs have the same prediction row in exact arithmetic, and the nearest-row check needs rows that differ."""
    import hip_util
    import pykg2vec_amd as pa
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    if family in ("kg2e", "hole"):
        from test_hip_kg2e_hole import random_case
        m = random_case(hip_util, family, E, R, width, seed)[0]
    elif family == "octonione":
        from test_hip_octonione import random_model
        m = random_model(hip_util, E, R, width, seed)
    elif family == "convkb":
        from test_hip_convkb import random_model
        m = random_model(E, R, width, 3, [1, 2, 3], seed)
        with torch.no_grad():   # rows of varying length and well above fc1's bias: at the xavier scale the constant dominates every
            for p in m.parameter_list:      # score and two queries' rows differ by less than the rounding of one
                p.weight.mul_(torch.from_numpy(rng.uniform(8.0, 32.0, (p.weight.shape[0], 1)).astype(np.float32)).to(p.weight.device))
    elif family.startswith("murp"):
        k = width
        m = pa.import_model("murp")(tot_entity=E, tot_relation=R, hidden_size=k, lmbda=0.0, device="cuda")
        if E >= 10:
            from test_hip_murp import random_case
            tabs = random_case(seed, E, R, k, 4)[0]
        else:
            tabs = [rng.uniform(-1, 1, (R, k)), 0.3 * rng.standard_normal(E), 0.3 * rng.standard_normal(E),
                    0.4 / np.sqrt(k) * rng.standard_normal((E, k)), 0.4 / np.sqrt(k) * rng.standard_normal((R, k))]
        with torch.no_grad():
            for (_, p), a in zip(m.named_parameters(), tabs):
                p.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))
        m.rank_order = 1 if family == "murp_order1" else 0
    elif family == "conve":
        from test_hip_conve import model_for, problem
        m = model_for(problem(43, E=E, R=R, k=20, h1=5, B=2)[0])
    elif family == "hyper":
        from test_hip_hyper import model_for, problem
        m = model_for(problem(112, E=E, R=R, D=9, Dr=3, B=2)[0])
    elif family == "interacte":
        from test_hip_interacte import model_for, problem
        m = model_for(*problem(107, E=E, R=R, rh=3, rw=1, NP=1, NF=3, ks=3, B=2)[:2])
    elif family == "acre_serial":
        from test_hip_acre import model_for, problem
        m = model_for(*problem(100, E=E, R=R, C=2, dil=(1, 2, 2), B=2)[:2])
    elif family == "acre_parallel":
        from test_hip_acre import model_for
        from test_hip_acre_parallel import problem
        m = model_for(*problem(100, E=E, R=R, C=2, dil=(1, 2, 2), B=2)[:2])
    elif family == "tucker":
        from test_hip_tucker import model_for, problem
        m = model_for(problem(7, E=E, R=R, d1=33, d2=7, B=2)[0])
    elif family == "proje":
        from test_hip_proje import model_for, problem
        m = model_for(problem(7, E=E, R=R, k=33, B=2, n_neg=1)[0])
    else:
        model, hp = _hp(family, width)
        train = np.stack([rng.integers(E, size=64), rng.integers(R, size=64), rng.integers(E, size=64)], 1).astype(np.int64)
        m = hip_util.model_from_params(model, {}, hp, E, R, train=train)
    m.eval()
    if m.kernel_name == "rescal":
        settle_rescal(m)
    return m


def settle_rescal(m):
    """RESCAL's evaluation renormalises both tables in place on every call: iterate to the fixed point first, where every later
    call sees the same tables (a copy of a settled row is settled too).  A row can alternate between two neighbours for ever (its
    norm rounds to 1 - ulp, then to 1 + ulp): after a few rounds such rows are replaced by rows of four entries +-0.5, whose norm
    is 1 exactly, distinct per row."""
    for it in range(64):
        before = [p.detach().clone() for p in m.parameters()]
        m.normalize_tables()
        moved = [(a != b).any(1) for a, b in zip(before, m.parameters())]
        if not any(bool(x.any()) for x in moved):
            return
        if it >= 8:
            with torch.no_grad():
                for p, rows_moved in zip(m.parameters(), moved):
                    for i in torch.nonzero(rows_moved).view(-1).tolist():
                        p[i] = 0.0
                        for j in range(4):
                            p[i, (i + j) % p.shape[1]] = -0.5 if (i >> j) & 1 else 0.5
    raise AssertionError("rescal: the renormalisation keeps changing the tables")


def entity_indexed(m, E):
    """The parameters indexed by entity id: tables with E rows (both roles of SimplE and CP, mu and sigma of KG2E, TransD's transfer
    table, MuRP's bs / bo, the 1-N heads' bias) and ConvE's [1, E] bias; never a relation table (QuatE's carry E rows too)."""
    out = []
    for name, p in m.named_parameters():
        if name.startswith("rel"):
            continue
        if p.dim() >= 1 and p.shape[0] == E:
            out.append((name, p, 0))
        elif p.dim() == 2 and tuple(p.shape) == (1, E):
            out.append((name, p, 1))
    return out


def copy_entity(m, E, src, dst):
    tabs = entity_indexed(m, E)
    assert tabs, "no entity table found"
    with torch.no_grad():
        for _, p, axis in tabs:
            if axis == 0:
                p[dst] = p[src]
            else:
                p[0, dst] = p[0, src]
    return [name for name, _, _ in tabs]


class Env:
    """A model, its queries and known triples, the rows of its own sweep and the numpy counts over them."""

    def __init__(self, family, width, E, q, known, m=None):
        import hip_util
        from pykg2vec_amd import kernels as K
        self.K, self.family, self.E, self.q, self.n = K, family, E, q, len(q)
        self.m = m if m is not None else build(family, width, E)
        m = self.m
        empty = known[:0]
        self.cfg = hip_util.make_config(E, R, {"neg_rate": 1}, known, empty, empty, batch_size=9)
        cache = self.cfg.knowledge_graph.cache
        self.lists = ref.known_lists(q, cache["hr_t"], cache["tr_h"])       # python sets: [tails, heads]
        self.trip = hip_util.dev(q)
        self.one_to_n = family in ONE_TO_N
        self.flip = family == "murp_order1"       # rank = #{s_e > s_true}: count over the negated row
        self.rows = [r.cpu().numpy() for r in self.sweep_rows()]
        if self.flip:
            self.rows = [-r for r in self.rows]
        self.true = [q[:, 2], q[:, 0]]
        self.want = [ref.counts_all(self.rows[s], self.true[s], self.lists[s]) for s in (0, 1)]
        self.want_raw = [ref.counts_all(self.rows[s], self.true[s], None) for s in (0, 1)]

    def desc(self):
        return self.K.model_desc(self.m)

    def body(self, side):
        e, r = self.trip[:, 2 if side else 0].contiguous(), self.trip[:, 1].contiguous()
        with torch.no_grad():
            return self.m._eval_body(e, r, side)

    def sweep_rows(self):
        """[tail rows, head rows] of the family's own evaluation, energies (lower = more plausible) but for MuRP's logits."""
        K, m = self.K, self.m
        if self.one_to_n:      # kge_head_1n_rank's `energies` output: -sigmoid(x . ent[e] + b[e])
            bias = m._head_bias()
            return [K.head_1n_rank(self.body(s), m.ent_embeddings.weight, bias, self.trip[:, 0 if s else 2].contiguous(), energies=True)
                    for s in (0, 1)]
        if m.kernel_name == "transr":
            return [m.score_rows(self.trip, s) for s in (0, 1)]
        both = K.eval_sweep_scores(self.desc(), self.trip)
        return [both[0::2], both[1::2]]

    def forward_rows(self, side):
        """forward() on the explicit (query, candidate) triples, in the rows' sign."""
        m, n, E = self.m, self.n, self.E
        with torch.no_grad():
            if self.family == "proje":       # (its forward is the scalar loss: the head's forward over the same body)
                return -m.score_rows(self.trip, side)
            if self.one_to_n:
                return -m.forward(self.trip[:, 2 if side else 0].contiguous(), self.trip[:, 1].contiguous(), "head" if side else "tail")
            cand = torch.arange(E, dtype=torch.int64, device="cuda").repeat(n)
            fixed = self.trip[:, 2 if side else 0].repeat_interleave(E)
            r = self.trip[:, 1].repeat_interleave(E)
            out = (m.forward(cand, r, fixed) if side else m.forward(fixed, r, cand)).view(n, E)
            return -out if self.flip else out

    def csr(self, tails=True, heads=True):
        import hip_util
        args = []
        for use, lists in ((tails, self.lists[0]), (heads, self.lists[1])):
            if use:
                off, ids = ref.csr(lists)
                args += [hip_util.dev(off), hip_util.dev(ids, torch.int32)]
            else:
                args += [None, None]
        return args

    def eval_ranks(self, tails=True, heads=True):
        """(ranks [4, n], ties [2, n]) of K.eval_ranks with host-built filter lists; TransR: one call per relation."""
        import hip_util
        K = self.K
        ties = torch.zeros((2, self.n), dtype=torch.int32, device="cuda")
        if self.m.kernel_name != "transr":
            ranks = K.eval_ranks(self.desc(), self.trip, *self.csr(tails, heads), ties=ties)
            return ranks.cpu().numpy(), ties.cpu().numpy()
        ranks = torch.empty((4, self.n), dtype=torch.int32, device="cuda")
        for rel in np.unique(self.q[:, 1]).tolist():
            idx = np.flatnonzero(self.q[:, 1] == rel)
            args = []
            for use, lists in ((tails, self.lists[0]), (heads, self.lists[1])):
                off, ids = ref.csr([lists[i] for i in idx])
                args += [hip_util.dev(off), hip_util.dev(ids, torch.int32)] if use else [None, None]
            t = torch.zeros((2, len(idx)), dtype=torch.int32, device="cuda")
            d = hip_util.dev(idx)
            ranks[:, d] = K.eval_ranks(self.desc(), self.trip[d].contiguous(), *args, ties=t)
            ties[:, d] = t
        return ranks.cpu().numpy(), ties.cpu().numpy()

    def check_counts(self, ranks, ties, tails=True, heads=True, tag=""):
        """Raw rank, filtered rank and tie count of every query and side equal the numpy counts over the rows: no tolerance."""
        for side, use, rrow, frow, trow in ((0, tails, 1, 3, 1), (1, heads, 0, 2, 0)):
            want = self.want[side] if use else self.want_raw[side]
            for what, got, exp in (("rank", ranks[rrow], want[0]), ("filtered rank", ranks[frow], want[1])):
                bad = np.flatnonzero(got != exp)
                assert bad.size == 0, (self.family, tag, "side", side, what, "queries", bad[:8], "got", got[bad[:8]], "want", exp[bad[:8]])
            if self.family in NO_TIE_REPORT:
                assert (ties[trow] == -1).all(), (self.family, tag, "tie report must be the documented -1", ties[trow][:8])
            else:
                bad = np.flatnonzero(ties[trow] != want[2])
                assert bad.size == 0, (self.family, tag, "side", side, "ties", bad[:8], ties[trow][bad[:8]], want[2][bad[:8]])

    def rank_all(self, grouped_min=None):
        from pykg2vec_amd.evaluator import Evaluator
        ev = Evaluator(self.m, self.cfg)
        if grouped_min is not None:
            ev.GROUPED_MIN_TRIPLES_PER_RELATION = grouped_min
        ranks, ties = ev.rank_all(self.q, self.n, return_ties=True)
        assert ev.setup_stats["csr_source"] == "triples"       # the device CSR builder made these filter lists
        grouped = ev._fingerprint(self.q, self.n) in ev._groups
        return ranks.cpu().numpy(), ties.cpu().numpy(), grouped


def check_rows_against_forward(env, report):
    """A sweep row is nearer to forward() of its own query than to any other query's (the pairs are distinct), and close to it.
    Nearest: argmin_j max_e |row_i[e] - F_j[e]| = i.  Where several j share that minimum exactly (MuRP: the largest deviation of a
    row sits on a candidate saturated at the last clamp, whose score does not depend on the relation, so two queries with one head
    share it bit for bit) the sum over e decides among them.  E = 1, 2: a row of one or two energies cannot tell queries apart."""
    for side in (0, 1):
        rows = torch.from_numpy(np.ascontiguousarray(env.rows[side])).cuda()
        F = env.forward_rows(side).to(rows.dtype)
        if env.E >= 65:
            for lo in range(0, env.n, 64):
                diff = (rows[lo:lo + 64, None, :] - F[None, :, :]).abs()                 # [<= 64, n, E]
                dist, total = diff.amax(2), diff.double().sum(2)
                tied = dist == dist.amin(1, keepdim=True)
                masked = torch.where(tied, total, torch.full_like(total, float("inf")))
                own = np.arange(lo, min(lo + 64, env.n))
                # (queries the model itself cannot tell apart -- forward() rows equal bit for bit, as MuRP's are for one head outside
                # the ball under any relation -- are no alternatives)
                same = (F[lo:lo + 64, None, :] == F[None, :, :]).all(2)
                same[torch.arange(len(own), device="cuda"), torch.as_tensor(own, device="cuda")] = False
                masked[same] = float("inf")
                near = masked.argmin(1).cpu().numpy()
                assert np.array_equal(near, own), (env.family, "side", side, "rows", lo, np.flatnonzero(near != own) + lo, near[near != own])
                best = masked[torch.arange(len(own), device="cuda"), torch.as_tensor(own, device="cuda")]
                assert int((masked == best[:, None]).sum()) == len(own), (env.family, "side", side, "rows", lo, "two queries fit a row equally well")
        dev = float((rows - F).abs().max())
        if env.one_to_n:
            x = env.body(side).detach().double()
            logit = x @ env.m.ent_embeddings.weight.detach().double().T
            if env.m._head_bias() is not None:
                logit = logit + env.m._head_bias().detach().double().view(1, -1)
            exact = -torch.sigmoid(logit)
            e_rows, e_fwd = float((rows.double() - exact).abs().max()), float((F.double() - exact).abs().max())
            report.append((env.family, env.n, env.E, side, "energies vs float64 head", e_rows, "forward vs float64 head", e_fwd))
            assert e_rows <= max(4 * e_fwd, ULP), (env.family, side, e_rows, e_fwd)
        elif env.family.startswith("murp"):
            from test_murp_model import near, worst
            report.append((env.family, env.n, env.E, side, "sweep vs forward", worst(rows.cpu().numpy(), F.cpu().numpy())))
            assert near(rows.cpu().numpy(), F.cpu().numpy()), (env.family, side, worst(rows.cpu().numpy(), F.cpu().numpy()))
        else:
            report.append((env.family, env.n, env.E, side, "sweep vs forward", dev))
            assert torch.allclose(rows, F, atol=TOL, rtol=TOL), (env.family, side, dev)


def check_rank_all(env, first, grouped_min=None, tag=""):
    """Evaluator.rank_all (device-built filter lists) equals K.eval_ranks (host-built ones).  TransH / TransD: the triples that go
    through the per-relation candidate tables round differently from the in-sweep transform whose rows are fetched here (no entry
    point returns the grouped form's rows), so there a rank may differ by k only where k candidates lie inside the fp32 band of
    the true one (golden_util.rank_band_ok)."""
    ranks, ties, grouped = env.rank_all(grouped_min)
    if grouped and env.m.kernel_name in ("transh", "transd"):
        for side, rrow, frow in ((0, 1, 3), (1, 0, 2)):
            for i in range(env.n):
                for row in (rrow, frow):
                    ok, near = rank_band_ok(env.rows[side][i], int(env.true[side][i]), ranks[row][i], first[0][row][i], atol=TOL, rtol=TOL)
                    assert ok, (env.family, tag, side, i, ranks[row][i], first[0][row][i], near)
        return grouped
    assert np.array_equal(ranks, first[0]), (env.family, tag, np.argwhere(ranks != first[0])[:8])
    assert np.array_equal(ties, first[1]), (env.family, tag, np.argwhere(ties != first[1])[:8])
    return grouped


# ---------------------------------------------------------------- set A: query counts and entity counts
@gpu
@pytest.mark.parametrize("family,width", FAMILIES, ids=IDS)
def test_query_and_entity_count_edges(family, width):
    run_count_edges(family, width, SET_A)


def run_count_edges(family, width, cases):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pykg2vec_amd import _lib as L
    report, refusals = [], []
    models = {}
    for n, E in cases:
        rng = np.random.default_rng(1000 * E + n)
        q = ref.distinct_queries(rng, n, E, R)
        known = ref.known_triples(rng, q, E, R)
        if E not in models:
            if E < 65:     # a constructor or the library may refuse such an entity count: recorded, and it must be a loud refusal
                try:
                    models[E] = build(family, width, E)
                    Env(family, width, E, q, known, models[E]).eval_ranks()
                except (ValueError, L.KgeHipError) as exc:
                    refusals.append((family, width, E, type(exc).__name__, str(exc)[:200]))
                    models[E] = None
            else:
                models[E] = build(family, width, E)
        if models[E] is None:
            continue
        env = Env(family, width, E, q, known, models[E])
        assert len(env.lists[0][0]) == 0 and len(env.lists[1][-1]) >= E - 1
        if n >= 255:
            assert min(len(env.lists[s][i]) for s in (0, 1) for i in (255 if n > 255 else n - 1, n - 1)) >= min(ref.LONG_LIST, E) - 1
        first = env.eval_ranks()
        env.check_counts(*first, tag="n=%d E=%d" % (n, E))
        env.check_counts(*env.eval_ranks(heads=False), heads=False, tag="n=%d E=%d tail filter only" % (n, E))
        env.check_counts(*env.eval_ranks(tails=False), tails=False, tag="n=%d E=%d head filter only" % (n, E))
        check_rank_all(env, first, tag="rank_all n=%d E=%d" % (n, E))
        if family in GROUP_ALL:
            assert check_rank_all(env, first, grouped_min=0, tag="rank_all all grouped n=%d E=%d" % (n, E))
        check_rows_against_forward(env, report)
    for line in refusals:
        print("REFUSED", line)
    # the refusals are recorded here so that a new one is seen: QuatE's rel_{s,x,y,z} tables carry tot_entity rows (the reference's
    # quirk) and are indexed by relation ids, so the library refuses E < R; every other family ranks at E = 1 and E = 2
    small = sorted({E for _, E in cases if E < 65})
    assert [(f, E) for f, _, E, _, _ in refusals] == ([("quate", E) for E in small] if family == "quate" else []), refusals
    assert all("indexed by relation ids" in msg for *_, msg in refusals), refusals
    worst = {}
    for line in report:
        for what, v in zip(line[4::2], line[5::2]):
            worst[what] = max(worst.get(what, 0.0), float(v) if not isinstance(v, tuple) else float(max(v)))
    print("MEASURED", family, width, worst)


# ---------------------------------------------------------------- set B: planted exact ties
SET_B_E = 257
HAND = np.asarray([(10, 0, 40), (70, 1, 100), (130, 2, 160), (200, 3, 230), (20, 4, 50), (90, 5, 120)], dtype=np.int64)
COPIES = [(40, 256),           # (a) the true tail of query 0 onto the entity of the last, one-candidate tile
          (70, 6),             # (b) the true head of query 1 onto an entity of the other 64-tile of the same 128-wide half
          (160, 161), (160, 3),    # (c) the true tail of query 2 onto two entities; 161 is in the query's known list
          (231, 232), (51, 52), (121, 122)]     # (d) pairs of entities that are true in none of queries 0..5


def planted_case(n):
    rng = np.random.default_rng(77 + n)
    E = SET_B_E
    special = {int(e) for pair in COPIES for e in pair}
    pool = ref.distinct_queries(rng, n + 64, E, R)[::-1]
    hr, rt = {(h, r) for h, r, t in HAND.tolist()}, {(r, t) for h, r, t in HAND.tolist()}
    rest = [row for row in pool.tolist() if (row[0], row[1]) not in hr and (row[1], row[2]) not in rt
            and row[0] not in special and row[2] not in special][:n - len(HAND)]
    q = np.concatenate([HAND, np.asarray(rest, dtype=np.int64)])
    assert q.shape == (n, 3)
    known = np.concatenate([ref.known_triples(rng, q, E, R), q[:1], np.asarray([(130, 2, 161)], dtype=np.int64)])
    return q, known


def run_planted(family, width, n, report=None):
    E = SET_B_E
    q, known = planted_case(n)
    m = build(family, width, E)
    for src, dst in COPIES:
        names = copy_entity(m, E, src, dst)
    env = Env(family, width, E, q, known, m)
    assert 161 in env.lists[0][2] and 3 not in env.lists[0][2]
    # the copies are bit-identical candidates in the family's own rows (a materialise-and-count pass is checked through these)
    assert env.rows[0][0][256] == env.rows[0][0][40] and env.rows[1][1][6] == env.rows[1][1][70], (family, names)
    assert env.rows[0][2][161] == env.rows[0][2][160] == env.rows[0][2][3], (family, names)
    ranks, ties = env.eval_ranks()
    env.check_counts(ranks, ties, tag="planted n=%d" % n)
    if family in NO_TIE_REPORT:
        assert (ties == -1).all()
    else:   # independently of the rows: a true-candidate kernel that rounds unlike its sweep loses these ties
        assert ties[1][0] >= 1 and ties[0][1] >= 1 and ties[1][2] >= 2, (family, "planted ties lost", ties[1][0], ties[0][1], ties[1][2])
    want = env.want[0]
    assert want[3][2] == want[2][2] - 1, (family, "the known copy of query 2 leaves the filtered tie count", want[:, 2])
    check_rank_all(env, (ranks, ties), tag="planted rank_all n=%d" % n)
    if family in GROUP_ALL + ("transr_l1", "transr_l2"):
        # the grouped form has no rows to fetch: the copies still tie there, whatever its rounding
        r2, t2, grouped = env.rank_all(0)
        assert grouped and t2[1][0] >= 1 and t2[0][1] >= 1 and t2[1][2] >= 2, (family, "grouped: planted ties lost", t2[:, :3])


@gpu
@pytest.mark.parametrize("n", [40, 300])
@pytest.mark.parametrize("family,width", FAMILIES, ids=IDS)
def test_planted_copies_tie_bit_for_bit(family, width, n):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    run_planted(family, width, n)


@gpu
@pytest.mark.parametrize("gemm", ["0", "1"])
@pytest.mark.parametrize("family,width", [fw for fw in FAMILIES if ENTRY[fw[0]].startswith(FLAT_ENTRY) and fw[0] not in ("ntn", "slm", "kg2e")],
                         ids=["%s-w%d" % fw for fw in FAMILIES if ENTRY[fw[0]].startswith(FLAT_ENTRY) and fw[0] not in ("ntn", "slm", "kg2e")])
def test_planted_copies_tie_on_the_forced_sweeps(family, width, gemm, monkeypatch):
    """KGE_EVAL_GEMM = 1 sends every sweep that can take them to the matrix cores (k_eval_gemm, true energies from
    k_eval_target_filter_chain), 0 to the VALU sweep (k_eval_sweep / k_eval_target_filter)."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    monkeypatch.setenv("KGE_EVAL_GEMM", gemm)
    run_planted(family, width, 40)


# ---------------------------------------------------------------- set C: wide sweeps
# The two widths above keep the sweep width K (csrc/kge_eval.hip:68-77 sweep_K: d, 2d or 4d by model; launch_dot_eval callers: d + 1 for
# SME / SME_BL, 2d for HoLE, 8d for OctonionE) at or below 128, so the K splits of the candidate layout kernels (k_eval_prepare4: every
# segment % 4 == 0, chunks of 128 over grid.y; k_eval_prepare: chunks of 64) and the padded tail beyond K (Kpad: K rounded up to 8, to 16
# in the dot form) never ran with more than one chunk.  Four further widths per family put K on (a) a value % 4 != 0 just above 64 (the
# dword layout kernel with a K split of two), (b) exactly 128, (c) 132 (two 128-chunks of k_eval_prepare4), (d) 260 -- or, where K is an
# even multiple of d, on the nearest values the family can take.  The comparison is set A's at (n, E) = (17, 65) and set B's at n = 40:
# integer ranks and tie counts equal the numpy count over the family's own rows, no mismatch allowed.
K_TIMES_2 = ("complex", "complexn3", "rotate", "analogy", "cp", "simple", "simple_ignr", "hole")
SEMANTIC = ("sme", "sme_bl", "slm")
SET_C_LIMITS = {     # (family, width) -> the limit that rules the width out, as the sources state it
    ("ntn", 260): "NTN sweep: ent_hidden_size and rel_hidden_size <= 256 (csrc/kge_ntn_eval.hip:275)",
    ("analogy", 33): "ANALOGY needs an even hidden size (csrc/kge_api.hip:60), so its K = 2d is always a multiple of 4",
}
for _f in ("transr_l1", "transr_l2"):
    for _w in (132, 260):
        SET_C_LIMITS[(_f, _w)] = "TransR: hidden sizes <= TR_MAXD = 128 (csrc/kge_transr.hip:24, :274)"
for _f in SEMANTIC:
    for _w in (127, 131, 259):
        SET_C_LIMITS[(_f, _w)] = "SLM / SME / SME_BL take hidden sizes 1..kSemMaxDim = 100 (csrc/kge_semantic.hip:43, :89)"


def set_c_widths(family):
    if family in K_TIMES_2:
        return (33, 64, 66, 130)          # K = 66, 128, 132, 260
    if family == "quate":
        return (17, 33, 65)               # K = 68, 132, 260 (K = 128 is width 32 of the sets above)
    if family == "octonione":
        return (9, 16, 17, 33)            # K = 8d = 72, 128, 136, 264
    if family in SEMANTIC:
        return (64, 100, 127, 131, 259)   # K = d + 1 = 65, 101 (the widest row the family takes), 128, 132, 260
    return (65, 128, 132, 260)            # K = d


SET_C = [pytest.param(f, w, id="%s-w%d" % (f, w),
                      marks=[pytest.mark.skip(reason=SET_C_LIMITS[(f, w)])] if (f, w) in SET_C_LIMITS else [])
         for f in TWO_WIDTHS for w in set_c_widths(f)]


@gpu
@pytest.mark.parametrize("family,width", SET_C)
def test_wide_sweeps_count_and_tie_exactly(family, width):
    run_count_edges(family, width, [(17, 65)])
    run_planted(family, width, 40)

