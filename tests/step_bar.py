"""The per-element bar that holds one training step's gradient to the float64 oracle (shared by tests/test_hip_skew.py and
tests/test_hip_width_edges.py; no GPU needed to compute it).

One SGD step with lr = 1 through train_model_epoch turns a step into its own gradient (p_before - p_after).  It is held, per element,
to the float64 oracle gradient of the batch kge_sample_batch restates, with a bar per row r of c_r incidences:
    2e-6 + 2e-4 |g64| + c_r 2^-23 a_r [+ 2^-24 |p_after|]   (the uniform tests' atol 2e-6 / rtol 2e-4, plus the fp32 summation bound,
                                                             plus the rounding of the stored update p - g, which before - after
                                                             cannot undo)
where a_r = sum over the row's incidences of |that incidence's contribution| (float64; fp32 sums of c_r terms in any order stay inside
it).  The a_r term is needed on short rows too: TransE's per-incidence contributions pass the normalisation backward and are ~10 for
rows of norm ~0.1, while five of them can cancel to 1e-3 -- the fp32 numpy oracle itself misses atol 2e-6 there.  a_r comes from the
oracle: every incidence is moved onto its own fresh copy of its row, so the dense gradient of the copies is the per-incidence
contributions.

Which side (entity ids or relation ids) indexes a table is read from its name: QuatE's rel_{s,x,y,z} tables carry tot_entity rows (the
reference's quirk) and are still indexed by relation ids.  NTN's mr1 / mr2 / br / mr are indexed by neither (every scored triple
contributes to every element) and its regulariser does not depend on the batch: see hub_bounds."""
import numpy as np

import kge_oracle as ko

NEAR_MARGIN = 1e-5     # hinge pairs this close to the margin may be decided differently in fp32 and float64
NEAR_ZERO = 1e-6       # ... and L1 residual components this close to 0 may take either sign
HINGE = ("transe", "transm", "transh", "transd", "transr", "rescal", "ntn")
GLOBAL_TABLES = {"ntn": ("mr1", "mr2", "br", "mr")}


def table_side(name):
    """"ent" / "rel": the id columns of a batch that index the rows of table `name` (oracle/kge_oracle.py: PARAM_NAMES)."""
    return "rel" if name.startswith("rel") or name == "w" else "ent"


def columns(model, batch):
    """(entity id arrays, relation id arrays) of a batch in its layout: the arrays every row reference comes from."""
    if model in ko.PAIRWISE:
        ph, pr, pt, nh, nr, nt = batch
        return [ph, pt, nh, nt], [pr, nr]
    h, r, t, _y = batch
    return [h, t], [r]


def _global_bounds(model, P, batch, hp, names):
    """NTN's tables that no id indexes: every scored triple is one incidence.  a = sum over the triples of |that triple's contribution|
    (the loss is a sum over pairs, so the gradient is the sum of single-triple gradients with the batch's own dL/dscore)."""
    ph, pr, pt, nh, nr, nt = batch
    pos = ko.score(model, P, ph, pr, pt, dtype=np.float64, **hp)
    neg = ko.score(model, P, nh, nr, nt, dtype=np.float64, **hp)
    _l, dpos, dneg = ko.pairwise_hinge(pos, neg, hp["margin"])
    a = {k: np.zeros(np.shape(P[k]), np.float64) for k in names}
    per = {k: [] for k in names}
    for (h, r, t), ds in (((ph, pr, pt), dpos), ((nh, nr, nt), dneg)):
        for i in range(len(h)):
            g = ko.score_grad(model, P, h[i:i + 1], r[i:i + 1], t[i:i + 1], ds[i:i + 1], dtype=np.float64, **hp)
            for k in names:
                a[k] += np.abs(g[k])
                per[k].append(g[k])
    return a, per, 2 * len(ph)


def hub_bounds(model, P, batch, hp, E, R):
    """Float64 oracle gradient, per-row incidence counts and per-element a_r of every row -> (G64, scores, cnt, side_of, a, ctx).
    cnt[k] is per table (the incidences of its side; for NTN's global tables the number of scored triples, + 1 for the regulariser)."""
    loss, G64, scores, _ = ko.train_step_grads(model, P, batch, dtype=np.float64, **hp)
    hp_inc = hp
    if model in ("ntn", "simple", "simple_ignr"):
        # NTN.get_reg does not depend on the batch: it is one more summand of every element, added below.  SimplE.get_reg is a function
        # of the id VALUES (oracle/kge_oracle.py: pointwise_reg) and has no gradient: the copies' fresh ids would change the loss only
        hp_inc = dict(hp, lmbda=0.0)
        loss, G_inc, _s, _ = ko.train_step_grads(model, P, batch, dtype=np.float64, **hp_inc)
    else:
        G_inc = G64
    ent_cols, rel_cols = columns(model, batch)
    cnt_side = {"ent": np.bincount(np.concatenate(ent_cols), minlength=E), "rel": np.bincount(np.concatenate(rel_cols), minlength=R)}
    glob = GLOBAL_TABLES.get(model, ())
    side_of = {k: table_side(k) for k in P if k not in glob}
    for k, s in side_of.items():
        assert np.shape(P[k])[0] >= (E if s == "ent" else R), (k, np.shape(P[k]))
    # every incidence gets its own fresh copy of its row, appended to the table (tables of one side are padded to one row count)
    touched = {s: np.flatnonzero(cnt_side[s] > 0) for s in cnt_side}
    n_rows = {s: max([np.shape(P[k])[0] for k in side_of if side_of[k] == s] + [E if s == "ent" else R]) for s in cnt_side}
    copies, new_cols = {}, {}
    for s, cols in (("ent", ent_cols), ("rel", rel_cols)):
        nxt = n_rows[s]
        src, out = [], []
        for col in cols:
            col = np.asarray(col, dtype=np.int64).copy()
            at = np.flatnonzero(np.isin(col, touched[s]))
            src.append(col[at])
            col[at] = nxt + np.arange(len(at))
            nxt += len(at)
            out.append(col)
        copies[s] = np.concatenate(src) if src else np.zeros(0, np.int64)
        new_cols[s] = out
    Pext = {}
    for k, v in P.items():
        v = np.asarray(v, np.float64)
        if k in glob:
            Pext[k] = v
            continue
        s = side_of[k]
        pad = np.zeros((n_rows[s] - v.shape[0],) + v.shape[1:], np.float64)
        Pext[k] = np.concatenate([v, pad, v[copies[s]]])
    if model in ko.PAIRWISE:
        ph, pt, nh, nt = new_cols["ent"]
        pr, nr = new_cols["rel"]
        ext_batch = (ph, pr, pt, nh, nr, nt)
    else:
        h, t = new_cols["ent"]
        (r,) = new_cols["rel"]
        ext_batch = (h, r, t, batch[3])
    hp_ext = hp_inc
    if "theta" in hp_inc:     # TransM's fixed per-relation weights follow the relation rows onto their copies
        theta = np.asarray(hp_inc["theta"], np.float64)
        hp_ext = dict(hp_inc, theta=np.concatenate([theta, np.zeros(n_rows["rel"] - len(theta)), theta[copies["rel"]]]))
    _l2, Gext, _s, _ = ko.train_step_grads(model, Pext, ext_batch, dtype=np.float64, **hp_ext)
    assert np.isclose(_l2, loss, rtol=1e-12), (_l2, loss)
    a, cnt = {}, dict(cnt_side)      # cnt["ent"] / cnt["rel"]: the sides' own counts, next to the per-table ones
    for k, v in P.items():
        if k in glob:
            continue
        s = side_of[k]
        cnt[k] = cnt_side[s] if np.shape(v)[0] == len(cnt_side[s]) else np.bincount(copies[s], minlength=np.shape(v)[0])
        acc = np.zeros(np.shape(v), np.float64)
        np.add.at(acc, copies[s], np.abs(Gext[k][n_rows[s]:]))
        a[k] = acc
        # the copies' contributions sum to the rows' gradient: a check of the construction itself
        summed = np.zeros_like(acc)
        np.add.at(summed, copies[s], Gext[k][n_rows[s]:])
        tv = touched[s]
        assert np.allclose(summed[tv], G_inc[k][tv], atol=1e-12, rtol=1e-9), k
    if glob:
        ag, per, n_inc = _global_bounds(model, P, batch, hp_inc, glob)
        for k in glob:
            assert np.allclose(np.sum(per[k], axis=0), G_inc[k], atol=1e-12, rtol=1e-9), k
            a[k] = ag[k]
            cnt[k] = np.full(np.shape(P[k])[0], n_inc, dtype=np.int64)
    if model == "ntn":
        for k in G64:
            a[k] = a[k] + np.abs(G64[k] - G_inc[k])
            cnt[k] = cnt[k] + 1
    return G64, scores, cnt, side_of, a, (G64, side_of, new_cols, Gext, n_rows)


def _l1_residual(P, h, r, t):
    """TransE's / TransM's L1 residual u = a^ + b^ - c^ (float64; its signs are the L1 gradient) and the saved normalisation terms."""
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    a, b, c = P["ent_embeddings"][h], P["rel_embeddings"][r], P["ent_embeddings"][t]
    return (a, b, c), ko._trans_tail(a, b, c, True)[1]


def ambiguity_allowance(model, P, scores, batch, hp, ctx):
    """Per-element widening of the bar for what fp32 and float64 may legitimately decide differently, and how many pairs that is.
    Hinge pairs within NEAR_MARGIN of the margin: the pair's whole contribution may be present or not -- its rows get 2 x |that
    incidence's contribution| (the row copies give it).  TransE / TransM L1 residual components within NEAR_ZERO of 0 may take either
    sign: the rows get |the gradient of flipping those signs|, through the normalisation backward.  No row is left out.  (Tables that
    no id indexes -- NTN's -- get no allowance: a near-margin pair there is counted and left to the cap on ambiguous pairs.)"""
    G64, side_of, cols_ext, Gext, n_rows = ctx
    allow = {k: np.zeros_like(v) for k, v in G64.items()}
    if model not in HINGE:
        return allow, 0
    pos, neg = scores
    v = pos + float(hp["margin"]) - neg
    near = np.abs(v) < NEAR_MARGIN
    ph, pr, pt, nh, nr, nt = batch
    ents = (ph, pt, nh, nt)
    rels = (pr, nr)
    if near.any():
        idx = np.flatnonzero(near)
        for k in side_of:
            s = side_of[k]
            for col, col_ext in zip(ents if s == "ent" else rels, cols_ext[s]):
                np.add.at(allow[k], np.asarray(col)[idx], 2.0 * np.abs(Gext[k][np.asarray(col_ext)[idx]]))
    n_amb = near.copy()
    if model in ("transe", "transm") and hp.get("l1_flag"):
        _loss, dpos, dneg = ko.pairwise_hinge(pos, neg, hp["margin"])
        eps = np.float64(ko.EPS_NORMALIZE)
        for (h, r, t), ds in (((ph, pr, pt), dpos), ((nh, nr, nt), dneg)):
            if model == "transm":      # the energy is theta_r x the distance: so is the coefficient of the residual's signs
                ds = ds * np.asarray(hp["theta"], np.float64)[np.asarray(r)]
            (a, b, c), (ah, na, bh, nb, ch, nc, u) = _l1_residual(P, h, r, t)
            flip = (np.abs(u) < NEAR_ZERO) & (ds != 0)[:, None]
            rows = np.flatnonzero(flip.any(1))
            n_amb[rows] = True
            if not len(rows):
                continue
            dg = 2.0 * flip[rows] * np.abs(ds[rows])[:, None]
            for arr, (xh, nx, x) in ((h, (ah, na, a)), (r, (bh, nb, b)), (t, (ch, nc, c))):
                d = np.abs(ko._normalize_bwd(xh[rows], nx[rows], ko._norm_rows(x[rows]) > eps, dg))
                key = "rel_embeddings" if arr is r else "ent_embeddings"
                np.add.at(allow[key], np.asarray(arr)[rows], d)
    return allow, int(n_amb.sum())


def tolerance(g, c, a, after=None, allow=0.0):
    """The bar of one table: g its float64 gradient, c the incidence count of every row, a the per-element a_r."""
    c = np.asarray(c).reshape((-1,) + (1,) * (g.ndim - 1)).astype(np.float64)
    # (+ the rounding of the stored update p - g itself, which before - after cannot undo)
    return 2e-6 + 2e-4 * np.abs(g) + c * 2.0 ** -23 * a + (0.0 if after is None else 2.0 ** -24 * np.abs(after)) + allow


def sampled(tr, B, neg, E, pointwise):
    """The first batch of the trainer's generator, restated by kge_sample_batch on the same counters (numpy arrays)."""
    from pykg2vec_amd import kernels as K
    gen = tr.generator
    return tuple(x.cpu().numpy() for x in K.sample_batch(gen.triples, gen.perm, 0, B, neg, E, gen.bern, gen.slots, gen.seed, 0,
                                                       pointwise=pointwise))


def one_step(hip, tr, m):
    """Run one epoch of one batch; the updated tables (float32 numpy) and the flat state."""
    import torch
    loss = tr.train_model_epoch(0)
    tr.sync_model()
    torch.cuda.synchronize()
    tables = {k[:-len(".weight")]: p.detach().cpu().numpy().copy() for k, p in hip.table_parameters(m)}
    state = None if tr.flat.state1 is None else tr.flat.state1.clone()
    return tables, tr.flat.param.clone(), state, float(loss)


def normalisation_allowance(model, P, batch, hp):
    """A derived widening of the bar of the same kind as the c_r term, for the in-row reduction the a_r term cannot see: the backward of
    F.normalize, (g - x^ (x^ . g)) / n with x^ = x / n.  Its two terms are each of size |g| / n and cancel -- at hidden size 1 exactly
    (x^ = +-1: the float64 contribution is 0, so a_r = 0, while an fp32 x^ one ulp off 1 leaves |g| 2^-23 / n, ~1e-5 for a row of norm
    0.01).  With u = 2^-24: the fp32 norm (a sum of d squares, a square root) is within (d / 2 + 1) u relative, so x^_k within
    (d / 2 + 2) u; the inner product s = sum_k x^_k g_k adds d u A, A = sum_k |x^_k g_k|, to the (d / 2 + 2) u A of its factors; the
    product x^_i s then carries |x^_i| (1.5 d + 2) u A + (d / 2 + 2) u |x^_i| |s| <= |x^_i| (2 d + 4) u A.  Per incidence and element:
        (2 d + 4) 2^-24 A |x^_i| / n
    on the gradient of the normalised vector x, pushed onto the table rows through the absolute values of the model's own map in
    front of the normalisation (TransE / TransM: x is the row itself; TransD: e + (e . e_m) r_m; TransR: the projection e^ M_r of the
    normalised entity row, whose own normalisation passes the term on the same way).
    The term is granted ONLY where the normalised vector has length 1 (d = 6 u A |x^| / n): there the cancellation is exact, a_r is
    identically zero and no fp32 implementation can meet the bar without it.  At every other length the two terms cancel in part only,
    the a_r and rtol terms cover what is left, and the worst-case factor (2 d + 4) would loosen the bar up to a hundredfold at wide
    rows: the kernels are held to the bar without it.  Models without a row normalisation get none.  TransH needs none (at hidden size 1 its
    projected rows are exactly zero); NTN is held without it as well (its push step met the plain bar at ent_hidden_size 1, at 0.91 of
    it: profiles/r24_width_edges.txt)."""
    out = {k: np.zeros(np.shape(v), np.float64) for k, v in P.items()}
    if model not in ("transe", "transm", "transd", "transr"):
        return out
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    u24 = 2.0 ** -24
    l1 = bool(hp.get("l1_flag"))
    ph, pr, pt, nh, nr, nt = [np.asarray(x) for x in batch]
    pos = ko.score(model, P, ph, pr, pt, dtype=np.float64, **hp)
    neg = ko.score(model, P, nh, nr, nt, dtype=np.float64, **hp)
    _l, dpos, dneg = ko.pairwise_hinge(pos, neg, hp["margin"])

    def term(x, g):
        """-> (the bound on the error of dL/dx, x^, n) of one normalisation with upstream gradient g."""
        xh, n = ko._normalize(x)
        if x.shape[-1] != 1:       # (see above: only the degenerate length, where the float64 contribution vanishes identically)
            return np.zeros_like(xh), xh, n
        A = np.sum(np.abs(xh * g), axis=-1, keepdims=True)
        return (2 * x.shape[-1] + 4) * u24 * A * np.abs(xh) / n, xh, n

    def through_normalize(x, dxh):
        """|J^T| applied to a bound dxh on the gradient of x^ = x / n: (|dxh| + |x^| (|x^| . |dxh|)) / n."""
        xh, n = ko._normalize(x)
        return (dxh + np.abs(xh) * np.sum(np.abs(xh) * dxh, axis=-1, keepdims=True)) / n

    for (h, r, t), ds in (((ph, pr, pt), dpos), ((nh, nr, nt), dneg)):
        if model == "transm":
            ds = ds * np.asarray(hp["theta"], np.float64)[r]
        eh, et, rl = P["ent_embeddings"][h], P["ent_embeddings"][t], P["rel_embeddings"][r]
        if model in ("transe", "transm"):
            a, b, c = eh, rl, et
        elif model == "transd":
            hm, tm, rm = P["ent_mappings"][h], P["ent_mappings"][t], P["rel_mappings"][r]
            a = eh + np.sum(eh * hm, axis=-1, keepdims=True) * rm
            c = et + np.sum(et * tm, axis=-1, keepdims=True) * rm
            b = rl
        else:
            M = P["rel_matrix"][r].reshape(len(r), eh.shape[1], rl.shape[1])
            hh, th, b = ko._normalize(eh)[0], ko._normalize(et)[0], ko._normalize(rl)[0]
            a, c = np.einsum("na,nab->nb", hh, M), np.einsum("na,nab->nb", th, M)
        _s, (ah, na, bh, nb, ch, nc, uu) = ko._trans_tail(a, b, c, l1)
        if l1:
            g = np.sign(uu)
        else:
            nrm = np.sqrt(np.sum(uu * uu, axis=-1, keepdims=True))
            g = np.where(nrm > 0, uu / np.where(nrm > 0, nrm, 1.0), 0.0)
        g = g * ds[:, None]
        da, db, dc = term(a, g)[0], term(b, g)[0], term(c, g)[0]
        if model in ("transe", "transm"):
            np.add.at(out["ent_embeddings"], h, da)
            np.add.at(out["ent_embeddings"], t, dc)
            np.add.at(out["rel_embeddings"], r, db)
        elif model == "transd":
            for e, m_, ids, dx in ((eh, hm, h, da), (et, tm, t, dc)):
                k = np.sum(dx * np.abs(rm), axis=-1, keepdims=True)
                np.add.at(out["ent_embeddings"], ids, dx + k * np.abs(m_))
                np.add.at(out["ent_mappings"], ids, k * np.abs(e))
                np.add.at(out["rel_mappings"], r, np.abs(np.sum(e * m_, axis=-1, keepdims=True)) * dx)
            np.add.at(out["rel_embeddings"], r, db)
        else:
            absM = np.abs(M)
            for e, xh_, ids, dx in ((eh, hh, h, da), (et, th, t, dc)):
                np.add.at(out["ent_embeddings"], ids, through_normalize(e, np.einsum("nab,nb->na", absM, dx)))
                np.add.at(out["rel_matrix"], r, (np.abs(xh_)[:, :, None] * dx[:, None, :]).reshape(len(r), -1))
            np.add.at(out["rel_embeddings"], r, through_normalize(rl, db))
    return out
