"""Helpers to read tests/golden/ref_*.npz (frozen outputs of the live reference)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = ["transe_l1", "transe_l2", "transh_l1", "transh_l2", "transd_l1", "transd_l2", "rotate",
         "rescal", "ntn", "distmult", "complex", "complexn3", "analogy",
         "transm_l1", "transm_l2", "cp", "simple", "simple_ignr", "quate", "transr_l1", "transr_l2"]
ORACLE_NAME = {"transe_l1": "transe", "transe_l2": "transe", "transh_l1": "transh", "transh_l2": "transh",
               "transd_l1": "transd", "transd_l2": "transd", "transm_l1": "transm", "transm_l2": "transm",
               "transr_l1": "transr", "transr_l2": "transr", "simple_ties": "simple"}
POINTWISE = ("distmult", "complex", "complexn3", "analogy", "cp", "simple", "simple_ignr", "quate")
# state_dict entries that are parameter tables of the scoring path (QuatE also carries unused fc / bn modules)
TABLES = {"cp": ("sub_embeddings", "rel_embeddings", "obj_embeddings"),
          "quate": tuple("%s_%s_embedding" % (a, c) for a in ("ent", "rel") for c in "sxyz") + ("rel_w_embedding",)}

# fp32 tolerance of BASELINE.json north_star ("within 1e-5 fp32"); SURVEY.md section 7 explains why an
# absolute 1e-5 alone is below fp32 rounding for L1 energies ~14, hence atol + rtol.
ATOL = 1e-5
RTOL = 1e-5


class Case:
    def __init__(self, name):
        self.name = name
        self.model = ORACLE_NAME.get(name, name)
        self.z = np.load(os.path.join(GOLDEN, "ref_%s.npz" % name))
        z = self.z
        self.E, self.R, self.B = int(z["E"]), int(z["R"]), int(z["B"])
        self.hp = {k[3:]: z[k].item() for k in z.files if k.startswith("hp_")}
        if "theta" in z.files:  # TransM's fixed per-relation weights (a function of the train split)
            self.hp["theta"] = z["theta"]
        self.pointwise = self.model in POINTWISE
        self.train, self.valid, self.test = z["train"], z["valid"], z["test"]

    def params(self, prefix="init."):
        out = {}
        for k in self.z.files:
            if k.startswith(prefix) and k.endswith(".weight"):
                name = k[len(prefix):-len(".weight")]
                if self.model not in TABLES or name in TABLES[self.model]:
                    out[name] = self.z[k].copy()
        return out

    def batch(self, s):
        n = 4 if self.pointwise else 6
        return tuple(self.z["batch%d.%d" % (s, i)] for i in range(n))

    def filters(self):
        allt = np.concatenate([self.train, self.valid, self.test])
        hr_t, tr_h = {}, {}
        for h, r, t in allt:
            hr_t.setdefault((int(h), int(r)), set()).add(int(t))
            tr_h.setdefault((int(t), int(r)), set()).add(int(h))
        return hr_t, tr_h


def close(a, b, atol=ATOL, rtol=RTOL):
    return np.allclose(a, b, atol=atol, rtol=rtol)


# ---- heavy-tailed ids.  Uniform draws give every C1 entity row ~4 incidences per batch; real graphs put thousands on a few hubs,
# which is where the owner-computes steps split rows over several work items, walk overflow chains and pre-reduce relation lists.
def zipf_ids(rng, n, N, s, perm=None):
    """n ids of range(N) with p(rank k) proportional to (k + 1)^-s (a finite Zipf law).  The ranks are mapped through `perm`, by
    default a permutation drawn from rng, so the hubs are not ids 0, 1, 2..."""
    if perm is None:
        perm = rng.permutation(N)
    p = np.arange(1, N + 1, dtype=np.float64) ** -float(s)
    return np.asarray(perm, dtype=np.int64)[rng.choice(N, size=n, p=p / p.sum())]


def harmonic(N, s):
    """H(N, s) = sum_{k=1..N} k^-s: the heaviest id of zipf_ids(.., N, s) is drawn with probability 1 / H(N, s)."""
    return float(np.sum(np.arange(1, N + 1, dtype=np.float64) ** -float(s)))


def skewed_triples(rng, n, E, R, s_ent=0.9, s_rel=1.0):
    """n int64 triples (h, r, t): heads and tails Zipf(s_ent) over ONE entity permutation (a hub is heavy on both sides),
    relations Zipf(s_rel)."""
    ent_perm = rng.permutation(E)
    h = zipf_ids(rng, n, E, s_ent, ent_perm)
    r = zipf_ids(rng, n, R, s_rel)
    t = zipf_ids(rng, n, E, s_ent, ent_perm)
    return np.stack([h, r, t], 1)


# ---- BASELINE.json configs at FULL table size, frozen from the live reference (oracle/make_golden_fullsize.py).
# Only seeds and outputs are stored: tables and triples are re-created from the seed on either box (numpy Generator
# streams of the same numpy build), so the fixtures stay small.
FULLSIZE = {
    "c1_transe_l1": dict(model="transe", E=14951, R=1345, splits=(483142, 50000, 59071), seed=9101,
                         hp=dict(hidden_size=100, l1_flag=True, margin=1.0), n_scores=256, step_B=4096, n_rank=32),
    "c1_transe_l2": dict(model="transe", E=14951, R=1345, splits=(483142, 50000, 59071), seed=9102,
                         hp=dict(hidden_size=100, l1_flag=False, margin=1.0), n_scores=256, step_B=4096, n_rank=32),
    "c2_complex": dict(model="complex", E=40943, R=11, splits=(86835, 3034, 3134), seed=9103,
                       hp=dict(hidden_size=200, lmbda=1e-4), n_scores=256, step_B=1000, n_rank=32),
    "c3_rotate": dict(model="rotate", E=14541, R=237, splits=(272115, 17535, 20466), seed=9104,
                      hp=dict(hidden_size=1000, margin=24.0, neg_rate=16, alpha=1.0), n_scores=64, step_B=32, n_rank=32),
    "c4_rescal": dict(model="rescal", E=123182, R=37, splits=(1079040, 5000, 5000), seed=9105,
                      hp=dict(hidden_size=200, margin=1.0), n_scores=64, step_B=64, n_rank=0),
    # the C4 relation-matrix width with an entity set small enough for the reference's own sweep (it gathers E*k*k floats
    # per query, pairwise.py:829-865: 320 MB here, 19.7 GB at YAGO3-10 size): the rank fixture C4 itself cannot have
    "c4_rescal_smallE": dict(model="rescal", E=2000, R=37, splits=(40000, 500, 500), seed=9106,
                             hp=dict(hidden_size=200, margin=1.0), n_scores=64, step_B=64, n_rank=16),
}


# the same configs on heavy-tailed ids (`skew` = (s_ent, s_rel): Zipf exponents of entities / relations over one seeded permutation
# each, shared by every split).  Step fixtures only (DEFAULT_STEP): no forward / rank fixtures exist for them.
FULLSIZE_SKEWED = {
    "%s_zipf" % base: dict(FULLSIZE[base], seed=seed, skew=(0.9, 1.0))
    for base, seed in (("c1_transe_l1", 9111), ("c2_complex", 9113), ("c3_rotate", 9114), ("c4_rescal", 9115))}
HEAVY_ENT_ROWS, HEAVY_REL_ROWS = 16, 8      # heaviest rows of a skewed step batch that its fixture lists in full


def heavy_step_rows(pos, nh, nr, nt, E, R):
    """(entity rows, relation rows): the HEAVY_ENT_ROWS / HEAVY_REL_ROWS rows of a step batch with the most incidences (heads and
    tails of positives and negatives; relations of both), ties by id."""
    ent = np.bincount(np.concatenate([pos[:, 0], pos[:, 2], nh, nt]), minlength=E)
    rel = np.bincount(np.concatenate([pos[:, 1], nr]), minlength=R)
    return (np.lexsort((np.arange(E), -ent))[:HEAVY_ENT_ROWS].astype(np.int64),
            np.lexsort((np.arange(R), -rel))[:HEAVY_REL_ROWS].astype(np.int64))


def fullsize_spec(name):
    return FULLSIZE[name] if name in FULLSIZE else FULLSIZE_SKEWED[name]


def fullsize_inputs(name):
    """Deterministic inputs of a FULLSIZE / FULLSIZE_SKEWED case: (spec, params, train, valid, test, score_ids, step_batch)."""
    import kge_oracle as ko
    spec = fullsize_spec(name)
    rng = np.random.default_rng(spec["seed"])
    E, R = spec["E"], spec["R"]
    skew = spec.get("skew")
    if skew is not None:
        ent_perm, rel_perm = rng.permutation(E), rng.permutation(R)

    def draw(n):
        if skew is not None:
            return np.stack([zipf_ids(rng, n, E, skew[0], ent_perm), zipf_ids(rng, n, R, skew[1], rel_perm),
                             zipf_ids(rng, n, E, skew[0], ent_perm)], 1)
        return np.stack([rng.integers(E, size=n), rng.integers(R, size=n), rng.integers(E, size=n)], 1).astype(np.int64)

    train, valid, test = (draw(n) for n in spec["splits"])
    shape_kw = dict(tot_entity=E, tot_relation=R, hidden_size=spec["hp"]["hidden_size"])
    if spec["model"] == "rotate":
        shape_kw["margin"] = spec["hp"]["margin"]
    P = ko.init_params(spec["model"], rng, **shape_kw)
    ids = draw(spec["n_scores"])
    B, neg = spec["step_B"], spec["hp"].get("neg_rate", 1)
    pos = train[rng.permutation(len(train))[:B]]
    flip = rng.random(B * neg) > 0.5
    ent = rng.integers(E, size=B * neg)
    nh = np.where(flip, np.repeat(pos[:, 0], neg), ent)
    nt = np.where(flip, ent, np.repeat(pos[:, 2], neg))
    nr = np.repeat(pos[:, 1], neg)
    if spec["model"] in POINTWISE:
        batch = ko.pointwise_layout(pos, nh, nr, nt, neg)
    else:
        batch = (pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy(), nh, nr, nt)
    return spec, P, train, valid, test, ids, tuple(np.ascontiguousarray(a) for a in batch)


def query_filters(all_triples, queries, R):
    """hr_t / tr_h (train+valid+test, kgcontroller.py:410-428) restricted to the keys the evaluated queries look up."""
    want_hr = {(int(h), int(r)) for h, r, t in queries}
    want_tr = {(int(t), int(r)) for h, r, t in queries}
    hr_t, tr_h = {k: set() for k in want_hr}, {k: set() for k in want_tr}
    key_hr = all_triples[:, 0] * R + all_triples[:, 1]
    key_tr = all_triples[:, 2] * R + all_triples[:, 1]
    q_hr = np.fromiter((h * R + r for h, r in want_hr), dtype=np.int64)
    q_tr = np.fromiter((t * R + r for t, r in want_tr), dtype=np.int64)
    for row in all_triples[np.isin(key_hr, q_hr)]:
        hr_t[(int(row[0]), int(row[1]))].add(int(row[2]))
    for row in all_triples[np.isin(key_tr, q_tr)]:
        tr_h[(int(row[2]), int(row[1]))].add(int(row[0]))
    return hr_t, tr_h


DIGEST_COLS = 256  # columns kept of the full rows of very wide tables (RESCAL's k*k relation matrices)


def grad_digest(g, rows):
    """What the fixture keeps of a dense [rows, d] gradient: per-row sums, per-row absolute sums (float64
    accumulation) and the full rows listed in `rows`."""
    g64 = np.asarray(g, dtype=np.float64)
    return g64.sum(1).astype(np.float32), np.abs(g64).sum(1).astype(np.float32), np.asarray(g)[rows].copy()


def rank_band_ok(scores_row, true_id, got, ref, atol=ATOL, rtol=RTOL):
    """A rank that differs from the reference's by k needs at least k candidates whose order against the true
    candidate can flip inside the fp32 tolerance band: |s(e) - s(true)| <= 2 * (atol + rtol * |s|) (both energies may
    move by one band).  Returns (ok, near_ties)."""
    st = float(scores_row[true_id])
    band = 2.0 * (atol + rtol * abs(st))
    near = int(np.sum(np.abs(scores_row.astype(np.float64) - st) <= band)) - 1   # the true candidate itself excluded
    return abs(int(got) - int(ref)) <= near, near


def tie_bracket(scores_row, true_id, known=()):
    """(less, ties, fless, fties) of one sweep: candidates strictly below the true one's energy / exactly tied with it
    (true one excluded), all candidates and known-filtered.  The reference's scan of the topk ordering
    (utils/evaluator.py:70-123) finds the true candidate after every strictly lower one and after an ATen-dependent subset of
    its tie group, so   less <= rank_ref <= less + ties   and   fless <= frank_ref <= fless + fties."""
    st = scores_row[true_id]
    lower, tied = scores_row < st, scores_row == st
    tied[true_id] = False
    keep = np.ones(len(scores_row), dtype=bool)
    kn = np.fromiter((e for e in known if e != true_id), dtype=np.int64)
    if kn.size:
        keep[kn] = False
    return int(lower.sum()), int(tied.sum()), int((lower & keep).sum()), int((tied & keep).sum())


# ---- ONE training step of every BASELINE config through the path the bench TIMES (Trainer.train_model_epoch with one batch of the
# bench's size: the sampler-fused default kernels), pinned to the live reference: oracle/make_golden_fullsize.py restates the device
# generator's first batch on the host (same permutation rule, Philox draws by oracle/sampler_oracle.py), runs the reference's
# train_step + backward + optimizer.step on it and freezes digests of the updated tables and optimiser state.
DEFAULT_STEP = {
    "c1_transe_l1": dict(B=32768, optimizer="adam", lr=0.01),
    "c1_transe_l2": dict(B=32768, optimizer="adam", lr=0.01),
    "c2_complex": dict(B=5000, optimizer="adagrad", lr=0.01),
    "c3_rotate": dict(B=1024, optimizer="adam", lr=0.01),
    "c4_rescal": dict(B=1024, optimizer="adam", lr=0.01),
    "c1_transe_l1_zipf": dict(B=32768, optimizer="adam", lr=0.01),
    "c2_complex_zipf": dict(B=5000, optimizer="adagrad", lr=0.01),
    "c3_rotate_zipf": dict(B=1024, optimizer="adam", lr=0.01),
    "c4_rescal_zipf": dict(B=1024, optimizer="adam", lr=0.01),
}
GENERATOR_SEED = 0


# ---- TRAINED tables at the BASELINE sizes (round 6).  Every full-size rank fixture of rounds 4-5 sits on freshly initialised tables,
# where near-ties are densest.  Tables that have been trained cannot be committed (65 / 116 MB at C2 / C3) and the reference cannot
# train on the GPU box, so they are DEFINED as what the drop-in Trainer's default step path -- bit-reproducible on every one of these
# configs -- leaves after `epochs` epochs over the whole synthetic train split from the seeded initial tables: produced once on the GPU
# (tools/make_trained_tables.py), ranked by the live reference in the build container (oracle/make_golden_trained.py), re-produced by
# the GPU test and recognised by their SHA-256 (tests/test_trained_ranks.py).
TRAINED = {
    "c1_transe_l1": dict(B=32768, optimizer="adam", lr=0.01, epochs=30, n_rank=512),
    "c2_complex": dict(B=5000, optimizer="adagrad", lr=0.1, epochs=60, n_rank=512),
    "c3_rotate": dict(B=1024, optimizer="adam", lr=0.001, epochs=4, n_rank=512),
}


def trained_queries(name, train, test):
    """Queries of a TRAINED case: half held-out test triples (ranks spread over the entity set), half TRAINING triples (ranks near the
    top, where a trained model's real test triples live)."""
    n = TRAINED[name]["n_rank"]
    pick = np.random.default_rng(4242).permutation(len(train))[:n // 2]
    return np.concatenate([test[:n - n // 2], train[pick]])


def tables_sha256(tables):
    """SHA-256 over the float32 bytes of the tables in key order."""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(tables):
        h.update(k.encode())
        h.update(np.ascontiguousarray(tables[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def generator_first_batch(train, batch_size, seed=GENERATOR_SEED):
    """Rows of the train split that form batch 0 of pykg2vec_amd.generator.Generator(seed): one permutation per run
    (data/generator.py:23), the slice ordered by relation id (a batch is a set)."""
    perm = np.random.default_rng(seed).permutation(len(train))
    sl = perm[:batch_size]
    return sl[np.argsort(train[sl, 1], kind="stable")]


def default_step_batch(name):
    """(spec, step, params, train, positives [B,3], (nh, nr, nt)) of the first default-path step of a FULLSIZE case: uniform corruption
    drawn from the device sampler's Philox stream (seed GENERATOR_SEED, counter = slot), train-set rejection."""
    import sampler_oracle as so
    spec, P, train, valid, test, _ids, _batch = fullsize_inputs(name)
    step = DEFAULT_STEP[name]
    pos = train[generator_first_batch(train, step["B"])]
    neg_rate = spec["hp"].get("neg_rate", 1)
    train_set = set(map(tuple, train.tolist()))
    neg = so.corrupt(pos[:, 0], pos[:, 1], pos[:, 2], neg_rate, spec["E"], None, train_set, GENERATOR_SEED, 0)
    return spec, step, P, train, pos, neg


def table_digest(w, rows):
    """What a fixture keeps of an updated [rows, d] table: float64 row sums and row absolute sums of every row, and the listed
    rows in full (first DIGEST_COLS columns)."""
    w64 = np.asarray(w, dtype=np.float64)
    return w64.sum(1).astype(np.float32), np.abs(w64).sum(1).astype(np.float32), np.asarray(w)[rows][:, :DIGEST_COLS].copy()


# ---- a learnable synthetic graph for trajectory-level parity (oracle/make_golden_trajectory.py, tests/test_hip_trajectory.py):
# triples (h, r, t) with t the entity nearest (L1) to ent[h] + rel[r] in a planted 8-dimensional translation model
TRAJECTORY = {
    "transe_l1_adam": dict(model="transe", ref="pairwise.TransE", hp=dict(hidden_size=32, l1_flag=True, margin=1.0), optimizer="adam", lr=0.01,
                           batch=256, neg=1, epochs=30),
    "complex_adagrad": dict(model="complex", ref="pointwise.Complex", hp=dict(hidden_size=32, lmbda=1e-5), optimizer="adagrad", lr=0.1,
                            batch=256, neg=1, epochs=30),
    "rotate_adam": dict(model="rotate", ref="pairwise.RotatE", hp=dict(hidden_size=32, margin=6.0, alpha=1.0), optimizer="adam", lr=0.01,
                        batch=256, neg=4, epochs=30),
}
TRAJECTORY_SEEDS = 5
TRAJECTORY_TEST = 200


def planted_graph(seed=7, E=400, R=6, dp=8):
    """(E, R, train, valid, test) int64 triples of the planted translation graph."""
    rng = np.random.default_rng(seed)
    ent = rng.normal(size=(E, dp))
    rel = rng.normal(size=(R, dp)) * 1.5
    trip = set()
    for h in range(E):
        for r in range(R):
            t = int(np.argmin(np.abs(ent[h] + rel[r] - ent).sum(1) + 1e9 * (np.arange(E) == h)))
            trip.add((h, r, t))
    trip = np.asarray(sorted(trip), dtype=np.int64)
    trip = trip[rng.permutation(len(trip))]
    n = TRAJECTORY_TEST
    return E, R, trip[2 * n:], trip[:n], trip[n:2 * n]
