"""HypER on the HIP path (csrc/kge_hyper.hip): parity with the live reference's float64 outputs in tests/golden/ref_hyper{,_ls,_masked}.npz
(predictions in both forms, the fused step with its 13 gradients and six running buffers, the padding rows, exact ranks), run-to-run
determinism, the autograd path, other shapes against the float64 restatement of tools/hyper_reference.py with shared Philox masks, the
public Trainer / Evaluator classes against the restatement's Adam and SGD trajectories, and the refusals.

Tolerances (the rule of DESIGN.md sections 15 and 18): on every test shape the plain fp32 numpy run of the same formulas
(hyper_reference.step(dtype=np.float32)) is compared with the float64 one; the HIP path is allowed FACTOR = 4 times that error per
quantity (predictions, loss, each gradient, each running buffer), floored at one fp32 ulp (2^-23) of the quantity's max-abs: a measured
error of zero cannot be a bound.  Where a gradient vanishes analytically (hyper_reference.VANISHING: fc.bias without hidden dropout,
bn1.bias without feature-map and hidden dropout, bn0.weight while bn0.bias = 0) and is below 1e-3 of the sum of the absolute values of
its summands in the float64 run (its cancellation scale), the floor is 2^-23 of that sum.  The figures are printed where they are used;
DESIGN.md section 19 lists them."""
import numpy as np
import pytest
import torch

from test_hyper_model import BUFFERS, COUNTERS, NAMES, TENSORS, fixture, hr, recorded_masks, tables  # noqa: F401

pytestmark = pytest.mark.gpu
FACTOR = 4.0
ULP = 2.0 ** -23
MARGIN = 1e-5


@pytest.fixture(autouse=True)
def no_leaked_switches(monkeypatch):
    """A Trainer reads the KGE_* A/B switches from the process environment, and other test modules of this suite leave some of them
    set: every test here starts without them."""
    from test_tucker_model import SWITCHES
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def hip():
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def csr(y):
    off = np.concatenate([[0], np.cumsum((y != 0).sum(1))]).astype(np.int64)
    ids = np.concatenate([np.flatnonzero(row) for row in y] + [np.zeros(0, np.int64)]).astype(np.int32)
    return torch.from_numpy(off).cuda(), torch.from_numpy(ids).cuda()


def model_for(P, rates=(0.0, 0.0, 0.0), counters=0, seed=0):
    """The drop-in model holding the restatement's state P (parameters and running buffers)."""
    from pykg2vec_amd.projection import HypER
    E, D = P["ent_embeddings.weight"].shape
    R, Dr = P["rel_embeddings.weight"].shape
    m = HypER(tot_entity=E, tot_relation=R, ent_hidden_size=D, rel_hidden_size=Dr, input_dropout=rates[0], feature_map_dropout=rates[1],
              hidden_dropout=rates[2], seed=seed)
    sd = {key: torch.from_numpy(np.asarray(P[key], dtype=np.float32)) for key in TENSORS + BUFFERS}
    sd.update({key: torch.tensor(counters) for key in COUNTERS})
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def buffers_of(m):
    return {key: v.detach().cpu().numpy().astype(np.float64) for key, v in m.state_dict().items() if key in BUFFERS}


def fused(P, h, r, t, y1, y2, rates=(0.0, 0.0, 0.0), seed=0, offset=0, ls=None, raw=False):
    """dict(loss, grads, buffers, counters) of kge_hyper_train_bce through the model's fused step; raw: the device tensors instead."""
    from pykg2vec_amd import kernels as K
    import types
    m = model_for(P, rates, counters=2)
    m.train()
    ws = m.trainable_tensors()
    gs = [torch.zeros_like(w) for w in ws]
    d = m.make_desc(ws, gs, train=True, seed=seed, offset=offset)
    loss = K.new_loss_buffer(ws[0].device)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda()
    m.fused_projection_step(K, d, dev(h), dev(r), dev(t), csr(y1), csr(y2), None, types.SimpleNamespace(label_smoothing=ls), loss)
    if raw:
        return loss.clone(), gs, [b.clone() for b in m.running_buffers()]
    return dict(loss=K.read_loss(loss).item(), grads={key: g.cpu().numpy().astype(np.float64) for key, g in zip(TENSORS, gs)},
                buffers=buffers_of(m), counters=[int(m.state_dict()[key]) for key in COUNTERS])


def bounds(P, h, r, t, y1, y2, **kw):
    """The float64 step and FACTOR x the fp32 restatement's error per quantity (b["ent0"]: of the head-only row 0 of grad(ent))."""
    ref = hr.step(P, h, r, t, y1, y2, **kw)
    f32 = hr.step(P, h, r, t, y1, y2, dtype=np.float32, **kw)
    b = {"loss": FACTOR * max(abs(f32["loss"] - ref["loss"]), ULP * abs(ref["loss"])),
         "preds": FACTOR * max(np.abs(f32["pred_tails"] - ref["pred_tails"]).max(), np.abs(f32["pred_heads"] - ref["pred_heads"]).max(), ULP)}
    vanishing = hr.VANISHING(kw.get("dropouts", (0.0, 0.0, 0.0)), P["bn0.bias"])
    for key in TENSORS:
        size = np.abs(ref["grads"][key]).max()
        if key in vanishing and size < 1e-3 * ref["scale"][key]:
            size = ref["scale"][key]      # cancelled by the batch norm that follows: the floor is an ulp of what was summed
        b[key] = FACTOR * max(np.abs(f32["grads"][key] - ref["grads"][key]).max(), ULP * size)
    for key in BUFFERS:
        b[key] = FACTOR * max(np.abs(f32["buffers"][key] - ref["buffers"][key]).max(), ULP * np.abs(ref["buffers"][key]).max())
    b["ent0"] = FACTOR * max(np.abs(f32["head_ent0"] - ref["head_ent0"]).max(), ULP * np.abs(ref["head_ent0"]).max())
    return ref, b


def check_step(tag, got, want, b):
    """want: dict(loss, grads, buffers) in float64."""
    err = abs(got["loss"] - want["loss"])
    print(tag, "loss err %.3g (bound %.3g)" % (err, b["loss"]))
    bad = [] if err <= b["loss"] else ["loss"]
    for key in TENSORS:
        err = np.abs(got["grads"][key] - want["grads"][key]).max()
        print(tag, "grad", key, "err %.3g (bound %.3g, max-abs %.3g)" % (err, b[key], np.abs(want["grads"][key]).max()))
        if not err <= b[key]:
            bad.append(key)
    for key in BUFFERS:
        err = np.abs(got["buffers"][key] - want["buffers"][key]).max()
        print(tag, key, "err %.3g (bound %.3g, max-abs %.3g)" % (err, b[key], np.abs(want["buffers"][key]).max()))
        if not err <= b[key]:
            bad.append(key)
    assert not bad, (tag, bad)


def check_padding(tag, got, ref, b, h, r, t):
    """padding_idx = 0: grad(rel)[0] is exactly zero, grad(ent)[0] is the head's share alone."""
    assert np.array_equal(got["grads"]["rel_embeddings.weight"][0], np.zeros_like(got["grads"]["rel_embeddings.weight"][0])), tag
    err = np.abs(got["grads"]["ent_embeddings.weight"][0] - ref["head_ent0"]).max()
    print(tag, "grad ent[0] against the head-only value: err %.3g (bound %.3g)" % (err, b["ent0"]))
    assert err <= b["ent0"], tag
    used = [int(x) for x in r if x != 0]
    if used:
        assert np.abs(got["grads"]["rel_embeddings.weight"][used[0]]).max() > 0, tag


def step_kw(z):
    kw = dict(label_smoothing=z["ls"])
    if z["masked"]:
        kw.update(dropouts=z["rates"], seed=int(z["mask_seed"]), offset=int(z["mask_offset"]))
    return kw


def recorded(z):
    return dict(loss=float(z["loss"]), grads={key: z["grad." + key] for key in TENSORS}, buffers={key: z["after." + key] for key in BUFFERS})


# ---------------------------------------------------------------- 1. predictions, both forms, against the live reference
@pytest.mark.parametrize("name", NAMES)
def test_predictions_match_reference(hip, name):
    z = fixture(name)
    P = tables(z)
    _, b = bounds(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], **step_kw(z))
    f32 = [hr.forward(P, z[e], z["r"], d, dtype=np.float32) for e, d in (("h", "tail"), ("t", "head"))]
    b_eval = FACTOR * max(np.abs(f32[0] - z["eval_pred_tails"]).max(), np.abs(f32[1] - z["eval_pred_heads"]).max(), ULP)
    m = model_for(P, z["rates"], counters=2, seed=int(z["mask_seed"]) if z["masked"] else 0)
    before = buffers_of(m)
    m.eval()
    with torch.no_grad():
        pt = m(hip.dev(z["h"]), hip.dev(z["r"]), direction="tail").cpu().numpy()
        ph = m(hip.dev(z["t"]), hip.dev(z["r"]), direction="head").cpu().numpy()
    err = max(np.abs(pt - z["eval_pred_tails"]).max(), np.abs(ph - z["eval_pred_heads"]).max())
    print(name, "eval-form preds err %.3g (bound %.3g)" % (err, b_eval))
    assert err <= b_eval
    after = buffers_of(m)
    assert all(np.array_equal(before[key], after[key]) for key in BUFFERS) and int(m.bn0.num_batches_tracked) == 2   # eval() writes nothing
    m.train()
    with torch.no_grad():     # the buffers and counters move under no_grad too
        if z["masked"]:
            m.dropout_offset = int(z["mask_offset"])
        pt = m(hip.dev(z["h"]), hip.dev(z["r"]), direction="tail").cpu().numpy()
        if z["masked"]:
            assert m.dropout_offset == int(z["mask_offset"]) + 1
            m.dropout_offset = int(z["mask_offset"])     # the step's two directions share one offset
        ph = m(hip.dev(z["t"]), hip.dev(z["r"]), direction="head").cpu().numpy()
    err = max(np.abs(pt - z["pred_tails"]).max(), np.abs(ph - z["pred_heads"]).max())
    print(name, "training-form preds err %.3g (bound %.3g)" % (err, b["preds"]))
    assert err <= b["preds"]
    assert [int(m.state_dict()[key]) for key in COUNTERS] == [4, 4, 4]
    got = buffers_of(m)
    for key in BUFFERS:
        assert np.abs(got[key] - z["after." + key]).max() <= b[key], key


# ---------------------------------------------------------------- 2. the fused step against the live reference
@pytest.mark.parametrize("name", NAMES)
def test_fused_step_matches_reference(hip, name):
    z = fixture(name)
    P = tables(z)
    ref, b = bounds(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], **step_kw(z))
    kw = step_kw(z)
    got = fused(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], kw.get("dropouts", (0.0, 0.0, 0.0)), kw.get("seed", 0), kw.get("offset", 0), z["ls"])
    check_step(name, got, recorded(z), b)      # the masked case: the kernels draw the recorded masks, or nothing here would agree
    check_padding(name, got, ref, b, z["h"], z["r"], z["t"])
    assert np.array_equal(z["grad.rel_embeddings.weight"][0], np.zeros(P["rel_embeddings.weight"].shape[1]))
    assert got["counters"] == [int(z[key]) + 2 for key in COUNTERS] == [int(z["after." + key]) for key in COUNTERS]
    if z["masked"]:
        other = fused(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], z["rates"], int(z["mask_seed"]), int(z["mask_offset"]) + 1, z["ls"])
        assert abs(other["loss"] - float(z["loss"])) > b["loss"]     # another offset: other masks


# ---------------------------------------------------------------- 3. ranks and ties
@pytest.mark.parametrize("name", NAMES)
def test_ranks_are_exact(hip, name):
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.evaluator import Evaluator
    z = fixture(name)
    m = model_for(tables(z), z["rates"], counters=2)
    m.eval()
    before = buffers_of(m)
    known = np.concatenate([z["train"], z["valid"], z["test"]])
    trip = hip.dev(z["test"])
    want = z["ranks"]      # rows: head, tail, filtered head, filtered tail
    t_off, t_ids, h_off, h_ids = K.filter_csr_build(hip.dev(known), trip, int(z["E"]), int(z["R"]))
    ties = torch.zeros((2, len(z["test"])), dtype=torch.int32, device="cuda")
    ranks = K.hyper_eval_ranks(m.make_desc(), trip, t_off, t_ids, h_off, h_ids, ties=ties).cpu().numpy()
    assert np.array_equal(ranks, want), (ranks, want)
    assert int(ties.sum()) == 0
    m.train()     # the rank pass is the eval form whatever the module's mode
    assert np.array_equal(K.eval_ranks(m.make_desc(), trip, t_off, t_ids, h_off, h_ids).cpu().numpy(), want)
    m.eval()
    cfg = hip.make_config(int(z["E"]), int(z["R"]), {"neg_rate": 0}, z["train"], z["valid"], z["test"], batch_size=9)
    got, ev_ties = Evaluator(m, cfg).rank_all(z["test"], len(z["test"]), return_ties=True)
    assert np.array_equal(got.cpu().numpy(), want) and int(ev_ties.sum()) == 0
    desc = m.make_desc(train=False)
    got = K.eval_ranks(desc, trip, None, None, h_off, h_ids).cpu().numpy()
    assert np.array_equal(got[0:2], want[0:2]) and np.array_equal(got[3], got[1]) and np.array_equal(got[2], want[2]), (got, want)
    got = K.eval_ranks(desc, trip, t_off, t_ids, None, None).cpu().numpy()
    assert np.array_equal(got[0:2], want[0:2]) and np.array_equal(got[2], got[0]) and np.array_equal(got[3], want[3]), (got, want)
    one = trip[:1].contiguous()
    got = K.eval_ranks(desc, one, *K.filter_csr_build(hip.dev(known), one, int(z["E"]), int(z["R"]))).cpu().numpy()
    assert got.shape == (4, 1) and np.array_equal(got[:, 0], want[:, 0]), (got, want[:, 0])
    after = buffers_of(m)
    assert all(np.array_equal(before[key], after[key]) for key in BUFFERS) and int(m.bn2.num_batches_tracked) == 2


# ---------------------------------------------------------------- 4. determinism
def test_fused_step_is_bit_identical_run_to_run(hip):
    z = fixture("hyper_masked")
    P = tables(z)
    args = (P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], z["rates"], 3, 1, 0.1)
    a, b = fused(*args, raw=True), fused(*args, raw=True)
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert all(float(g.abs().max()) > 0 for g in a[1])
    c = fused(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], z["rates"], 4, 1, 0.1, raw=True)
    assert not torch.equal(a[1][9], c[1][9])     # another seed: other masks
    p0 = [fused(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], seed=s, raw=True) for s in (3, 4)]
    assert all(torch.equal(x, y) for x, y in zip(p0[0][1], p0[1][1]))   # p = 0 draws nothing: the seed cannot matter


def test_large_batch_is_bit_identical_too(hip):
    """Three 64-row tiles over each direction with a partial last tile, every entity and relation repeated many times: the 13 gradients
    and the six running buffers.  (The loss is the head's: from this size on several of its workgroups share one of the striped loss
    accumulators through float atomics, so it is held to 4 ulp; the fixture-size test above holds it to the bit.)"""
    P, h, r, t, y1, y2 = problem(31, E=70, R=5, D=20, Dr=12, B=150)
    a = fused(P, h, r, t, y1, y2, (0.2, 0.2, 0.3), 3, 1, 0.1, raw=True)
    b = fused(P, h, r, t, y1, y2, (0.2, 0.2, 0.3), 3, 1, 0.1, raw=True)
    diff = [i for i, (x, y) in enumerate(zip(a[1] + a[2], b[1] + b[2])) if not torch.equal(x, y)]
    assert not diff, diff
    assert abs(float(a[0].double().sum()) - float(b[0].double().sum())) <= 4 * ULP * float(a[0].double().sum())


# ---------------------------------------------------------------- 5. the autograd path
def test_autograd_path_agrees_with_fused_step(hip):
    z = fixture("hyper_masked")
    P = tables(z)
    seed, offset = int(z["mask_seed"]), int(z["mask_offset"])
    ref, b = bounds(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], **step_kw(z))
    m = model_for(P, z["rates"], counters=2, seed=seed)
    m.train()
    m.dropout_offset = offset
    pred_tails = m(hip.dev(z["h"]), hip.dev(z["r"]), "tail")
    m.dropout_offset = offset      # the step's two directions share one offset; the head direction's mask rows follow the tail's
    pred_heads = m(hip.dev(z["t"]), hip.dev(z["r"]), "head")
    loss = m.loss(pred_heads, pred_tails, torch.from_numpy(z["tr_h"]).float().cuda(), torch.from_numpy(z["hr_t"]).float().cuda(), z["ls"],
                  int(z["E"]))
    loss.backward()
    got = dict(loss=loss.item(), grads={key: p.grad.cpu().numpy().astype(np.float64) for key, p in zip(TENSORS, m.trainable_tensors())},
               buffers=buffers_of(m))
    check_step("autograd", got, recorded(z), b)
    check_padding("autograd", got, ref, b, z["h"], z["r"], z["t"])
    assert [int(m.state_dict()[key]) for key in COUNTERS] == [4, 4, 4]
    step = fused(P, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], z["rates"], seed, offset, z["ls"])
    check_step("fused", step, recorded(z), b)
    for key in BUFFERS:     # the two paths run the same forward kernels on the same rows
        assert np.array_equal(got["buffers"][key], step["buffers"][key]), key


# ---------------------------------------------------------------- 6. other shapes against the float64 restatement
def problem(seed, E, R, D, Dr, B, repeats=False):
    """Default-init tensors (xavier tables, torch's layer defaults drawn from a seeded generator; the batch norm weights, biases and b
    off their defaults), exact in fp32; running buffers moved off their defaults."""
    rng = np.random.default_rng(seed)
    F = 32 * (D - 8)
    u = lambda shape, bound: rng.uniform(-bound, bound, size=shape)
    P = {"b": 0.1 * rng.normal(size=E), "ent_embeddings.weight": u((E, D), np.sqrt(6.0 / (E + D))),
         "rel_embeddings.weight": u((R, Dr), np.sqrt(6.0 / (R + Dr))),
         "bn0.weight": 1 + 0.2 * rng.normal(size=1), "bn0.bias": 0.1 * rng.normal(size=1),
         "bn1.weight": 1 + 0.2 * rng.normal(size=32), "bn1.bias": 0.1 * rng.normal(size=32),
         "bn2.weight": 1 + 0.2 * rng.normal(size=D), "bn2.bias": 0.1 * rng.normal(size=D),
         "fc.weight": u((D, F), 1 / np.sqrt(F)), "fc.bias": u(D, 1 / np.sqrt(F)),
         "fc1.weight": u((288, Dr), 1 / np.sqrt(Dr)), "fc1.bias": u(288, 1 / np.sqrt(Dr)),
         "bn0.running_mean": 0.1 * rng.normal(size=1), "bn0.running_var": 1 + 0.3 * rng.random(1),
         "bn1.running_mean": 0.1 * rng.normal(size=32), "bn1.running_var": 1 + 0.3 * rng.random(32),
         "bn2.running_mean": 0.1 * rng.normal(size=D), "bn2.running_var": 1 + 0.3 * rng.random(D)}
    P = {key: v.astype(np.float32).astype(np.float64) for key, v in P.items()}
    h, r, t = rng.integers(E, size=B), rng.integers(R, size=B), rng.integers(E, size=B)
    if repeats:     # one entity three times as head, one as both head and tail, a repeated relation, id 0 on both tables: the ordered scatter
        h[0] = h[2] = h[4] = 7
        t[1] = h[3]
        r[0] = r[1] = r[4] = 2
        h[5] = t[6] = 0
        r[5] = r[7] = 0
    y1, y2 = (rng.random((B, E)) < 0.05).astype(np.float64), (rng.random((B, E)) < 0.05).astype(np.float64)
    y1[np.arange(B), t], y2[np.arange(B), h] = 1.0, 1.0
    return P, h, r, t, y1, y2


def representative(P, h, r, t, y1, y2, ref, b, orders=12, slack=0.75, **kw):
    """Is the bound of this input representative?  The bound is FACTOR x the error of ONE fp32 run, the restatement's in numpy's order
    of additions.  With few rows a batch norm subtracts a mean from values that lie close together (a bn2 column that keeps a single
    row under hidden dropout, two rows whose u nearly agree, bn1 over three conv outputs when L = 1); its rstd is then an order of
    magnitude above the others' and the backward amplifies the rounding of those few values by it, so the fp32 error of such an input
    is a matter of luck: whether u1 + u2 happens to be representable moves the two-row gradient of fc.bias by 15 x.  An input is used
    only where the bound also covers the fp32 restatement (a) under `orders` other (seeded, permuted) orders of the fc sum and (b) with
    every conv output, every u and every dx left alone or moved by half an ulp (seeded), `orders` times, with `slack` to spare: numpy's
    fp32 sums, and with them the bounds, differ a little from one CPU to the next, so the tests themselves assert the margin only.
    CPU-only: the seeds below were chosen with this function (choose_seeds, python tests/test_hip_hyper.py) and the margin, never from
    what the kernels give."""
    F = np.asarray(P["fc.weight"]).shape[1]
    for i in range(2 * orders):
        if i < orders:
            perm = np.random.default_rng(1000 + i).permutation(F)
            Q = dict(P)
            Q["fc.weight"] = np.asarray(P["fc.weight"])[:, perm]     # the same model with the feature axis renumbered ...
            got = hr.step(Q, h, r, t, y1, y2, dtype=np.float32, fc_order=perm, **kw)     # ... and A renumbered with it
            back = np.argsort(perm)
        else:
            got, back = hr.step(P, h, r, t, y1, y2, dtype=np.float32, u_flip=i, **kw), slice(None)
        for key in TENSORS:
            g = got["grads"][key]
            if key == "fc.weight":
                g = g[:, back]
            if not np.abs(g - ref["grads"][key]).max() <= slack * b[key]:
                return False
    return True


# seeds chosen on the CPU (choose_seeds) so that no bn2 output of the float64 run is within MARGIN of zero (asserted below) and the
# bounds are representative
SHAPES = {"smallest": dict(seed=112, E=70, R=5, D=9, Dr=3, B=3), "d24_odd_dr": dict(seed=95, E=70, R=5, D=24, Dr=7, B=9),
          "preset": dict(seed=95, E=70, R=5, D=200, Dr=200, B=5), "two_rows": dict(seed=121, E=70, R=5, D=20, Dr=12, B=2),
          "repeats": dict(seed=82, E=70, R=5, D=20, Dr=12, B=9, repeats=True), "row_tile": dict(seed=68, E=70, R=5, D=16, Dr=8, B=70)}
RATES = (0.2, 0.2, 0.3)


@pytest.mark.parametrize("rates", [(0.0, 0.0, 0.0), RATES], ids=["p0", "dropout"])
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_other_shapes_match_float64(hip, case, rates):
    from pykg2vec_amd import kernels as K
    P, h, r, t, y1, y2 = problem(**SHAPES[case])
    kw = dict(dropouts=rates, seed=(7 << 32) | 9, offset=5)
    ref, b = bounds(P, h, r, t, y1, y2, label_smoothing=0.1, **kw)
    print(case, "pre-ReLU margin %.3g" % ref["margin"])
    assert ref["margin"] > MARGIN
    got = fused(P, h, r, t, y1, y2, rates, kw["seed"], kw["offset"], 0.1)
    check_step(case, got, ref, b)
    check_padding(case, got, ref, b, h, r, t)
    # the predictions under the same masks: the body of each direction with the step's seed / offset and mask rows, then the head
    m = model_for(P, rates)
    B = len(h)
    for side, e, want in ((0, h, ref["pred_tails"]), (1, t, ref["pred_heads"])):
        d = m.make_desc(train=True, seed=kw["seed"], offset=kw["offset"])
        x, _ = K.hyper_body_forward(d, hip.dev(e), hip.dev(r), row0=side * B)
        p = K.head_1n_forward(x, m.ent_embeddings.weight.detach(), m.b.detach()).cpu().numpy()
        err = np.abs(p - want).max()
        print(case, "side", side, "preds err %.3g (bound %.3g)" % (err, b["preds"]))
        assert err <= b["preds"]


# ---------------------------------------------------------------- 7. Trainer and Evaluator against the restatement's trajectory
# three Adam steps (and, as a second case, three plain SGD steps) on the fixture's training split with the Philox masks of (config.seed, step)
MASK_SEED = 17     # chosen on the CPU (choose_seeds): the margin, asserted below, and bounds that are representative


@pytest.mark.parametrize("optimizer,lr", [("adam", 0.01), ("sgd", 0.5)])
def test_trainer_matches_float64_trajectory(hip, optimizer, lr):
    from pykg2vec_amd.trainer import Trainer
    z = fixture("hyper_ls")
    P = tables(z)
    E, R, B, seed = int(z["E"]), int(z["R"]), 9, MASK_SEED
    train = z["train"]
    batches = []
    for i in range(3):
        rows = train[i * B:(i + 1) * B]
        y1, y2 = np.zeros((B, E)), np.zeros((B, E))
        for j, (a, rel, c) in enumerate(rows):
            y1[j, train[(train[:, 0] == a) & (train[:, 1] == rel), 2]] = 1.0
            y2[j, train[(train[:, 2] == c) & (train[:, 1] == rel), 0]] = 1.0
        batches.append((rows[:, 0], rows[:, 1], rows[:, 2], y1, y2))
    assert any((b[1] == 0).any() for b in batches) and any((b[0] == 0).any() or (b[2] == 0).any() for b in batches)
    want_losses, want, margin = hr.adam_trajectory(P, batches, lr, RATES, seed, 0.1, optimizer=optimizer)
    f32_losses, f32, _ = hr.adam_trajectory(P, batches, lr, RATES, seed, 0.1, dtype=np.float32, optimizer=optimizer)
    print("pre-ReLU margin over the three steps %.3g" % margin)
    assert margin > MARGIN
    cfg = hip.make_config(E, R, {"neg_rate": 0}, train, z["valid"], z["test"], batch_size=B, optimizer=optimizer, lr=lr, label_smoothing=0.1)
    cfg.seed = seed
    tn = Trainer(model_for(P, RATES, counters=2), cfg)
    tn.build_model()
    tn.model.train()
    for i, (h, r, t, y1, y2) in enumerate(batches):
        loss = tn.train_step_projection(hip.dev(h), hip.dev(r), hip.dev(t), csr(y1), csr(y2)).item()
        tn._reduce_and_step()
        bound = FACTOR * max(abs(f32_losses[i] - want_losses[i]), ULP * abs(want_losses[i]))
        print("step", i, "loss %.9f (float64 %.9f, bound %.3g)" % (loss, want_losses[i], bound))
        assert abs(loss - want_losses[i]) <= bound
    assert [int(tn.model.state_dict()[key]) for key in COUNTERS] == [8, 8, 8]
    sd = tn.model.state_dict()
    bad = []
    for key in TENSORS + BUFFERS:
        got = sd[key].detach().cpu().numpy().astype(np.float64)
        bound = FACTOR * max(np.abs(f32[key] - want[key]).max(), ULP * np.abs(want[key]).max())
        err = np.abs(got - want[key]).max()
        print("final", key, "err %.3g (bound %.3g)" % (err, bound))
        if not err <= bound:
            bad.append(key)
    # (Adam divides by sqrt(v): where a gradient is rounding noise the update is noise of the order of lr, in the fp32 restatement as
    # here, and so is its bound.  The fp32 restatement forms the optimiser's weights 1 - beta in fp32, as csrc/kge_opt_device.h does:
    # in fp32 1 - 0.999 is 1.3e-5 off 0.001, which scales every Adam step by 6e-6 and is most of the fp32 run's error in the
    # well-conditioned tensors.  Plain SGD has neither effect.)
    assert not bad, bad
    # padding_idx = 0: relation row 0 occurs in the batches and never moves, under Adam too (a zero gradient keeps both moments at zero);
    # entity row 0 moves by the head's share alone, which the trajectory above covers
    got_rel0 = sd["rel_embeddings.weight"][0].detach().cpu().numpy()
    assert np.array_equal(got_rel0, z["rel_embeddings.weight"][0]) and np.array_equal(want["rel_embeddings.weight"][0], P["rel_embeddings.weight"][0])
    assert not np.array_equal(sd["ent_embeddings.weight"][0].detach().cpu().numpy(), z["ent_embeddings.weight"][0])
    tn.model.eval()
    ranks = tn.evaluator.rank_all(z["test"], len(z["test"])).cpu().numpy()
    known = np.concatenate([train, z["valid"], z["test"]])
    # "the restatement's ranks" are the restatement's eval form on the parameters the Trainer arrived at (not on the restatement's own
    # final trajectory): the Evaluator is held to exact ranks of the model it was given, the trajectory itself is checked above
    trained = {key: sd[key].detach().cpu().numpy().astype(np.float64) for key in TENSORS + BUFFERS}
    want_ranks, gap = hr.ranks(trained, z["test"], known)
    print("float64 rank gap of the trained model %.3g" % gap)
    assert gap > 1e-6     # fixed seed: no close pair, so every rank must be exact
    assert np.array_equal(ranks, want_ranks), (ranks, want_ranks)


# ---------------------------------------------------------------- 8. refusals
def test_refusals(hip):
    import ctypes
    from pykg2vec_amd import _lib as L, kernels as K
    from pykg2vec_amd.projection import HypER
    from pykg2vec_amd.trainer import Trainer
    from pykg2vec_amd.generator import Generator
    z = fixture("hyper")
    P = tables(z)
    m = model_for(P)
    m.train()
    one = hip.dev(z["h"][:1])
    with pytest.raises(L.KgeHipError, match="kge_hyper_body_forward: batch norm in training form needs more than one row"):
        m(one, hip.dev(z["r"][:1]), "tail")
    m.eval()
    with torch.no_grad():
        assert m(one, hip.dev(z["r"][:1]), "tail").shape == (1, 70)      # one row is fine under eval()
    kw = dict(tot_entity=70, tot_relation=5, rel_hidden_size=12, input_dropout=0.0, feature_map_dropout=0.0, hidden_dropout=0.0)
    two = hip.dev(z["h"][:2])
    for over, msg in ((dict(ent_hidden_size=8), "ent_hidden_size = 8 is shorter than the 9-tap filter"),
                      (dict(ent_hidden_size=20, rel_hidden_size=1025), "exceeds 1024"),
                      (dict(ent_hidden_size=20, hidden_dropout=1.0), r"dropout rate 2 must be in \[0, 1\)")):
        bad = HypER(**dict(kw, **over)).cuda()
        with pytest.raises(L.KgeHipError, match=msg):
            bad(two, hip.dev(z["r"][:2]), "tail")
    m.bn1.momentum = None
    with pytest.raises(L.KgeHipError, match="cumulative moving average"):
        m.make_desc()
    m.bn1.momentum = 0.1
    d = m.make_desc(train=False)
    need = int(L.load().kge_hyper_eval_ranks_workspace_bytes(ctypes.byref(d), 4))
    d._ws = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    trip = hip.dev(z["test"][:4])
    ranks = torch.empty((4, 4), dtype=torch.int32, device="cuda")
    rc = L.load().kge_hyper_eval_ranks(ctypes.byref(d), ctypes.c_void_p(trip.data_ptr()), 4, None, None, None, None,
                                       ctypes.c_void_p(d._ws.data_ptr()), need - 1, ctypes.c_void_p(ranks.data_ptr()), None, None)
    assert rc != 0 and "kge_hyper_eval_ranks: workspace too small" in L.load().kge_last_error().decode()
    cfg = lambda **over: hip.make_config(70, 5, dict({"neg_rate": 0}, **over), z["train"], z["valid"], z["test"], batch_size=9, optimizer="adam")
    with pytest.raises(NotImplementedError, match="HypER: .*neg_rate > 0.* is not supported on the projection path"):
        Trainer(model_for(P), cfg(neg_rate=1)).build_model()
    with pytest.raises(NotImplementedError, match="neg_rate > 0 is not supported"):
        Generator(model_for(P), cfg(neg_rate=2))
    with pytest.raises(NotImplementedError, match="HypER: .*hipGraph capture"):
        Trainer(model_for(P), cfg(), use_graph=True).build_model()
    tn = Trainer(model_for(P), cfg())
    tn.distributed = True
    with pytest.raises(NotImplementedError, match="HypER: data-parallel training"):
        tn.build_model()
    assert K.hyper_shapes(70, 5, 20, 12)[0][9] == (20, 384)


# ---------------------------------------------------------------- seed choice, on the CPU
def trainer_batches(z, B=9):
    train, E = z["train"], int(z["E"])
    batches = []
    for i in range(3):
        rows = train[i * B:(i + 1) * B]
        y1, y2 = np.zeros((B, E)), np.zeros((B, E))
        for j, (a, rel, c) in enumerate(rows):
            y1[j, train[(train[:, 0] == a) & (train[:, 1] == rel), 2]] = 1.0
            y2[j, train[(train[:, 2] == c) & (train[:, 1] == rel), 0]] = 1.0
        batches.append((rows[:, 0], rows[:, 1], rows[:, 2], y1, y2))
    return batches


def choose_seeds(margin=10 * MARGIN, tries=2000):
    """Prints, per shape of SHAPES, the first seed at or after the listed one whose float64 margin exceeds `margin` and whose bounds
    are representative at both rate settings, and the first such mask seed of the Trainer test (there: the fp32 trajectory with the
    half-ulp moves stays within three quarters of every final tensor's bound, under Adam and under SGD).  Needs no GPU."""
    for case, spec in sorted(SHAPES.items()):
        for seed in range(spec["seed"], spec["seed"] + tries):
            P, h, r, t, y1, y2 = problem(**dict(spec, seed=seed))
            for rates in ((0.0, 0.0, 0.0), RATES):
                kw = dict(dropouts=rates, seed=(7 << 32) | 9, offset=5, label_smoothing=0.1)
                ref, b = bounds(P, h, r, t, y1, y2, **kw)
                if not (ref["margin"] > margin and representative(P, h, r, t, y1, y2, ref, b, **kw)):
                    break
            else:
                print(case, "seed", seed)
                break
    z = fixture("hyper_ls")
    P, batches = tables(z), trainer_batches(z)
    for seed in range(MASK_SEED, MASK_SEED + tries):
        for optimizer, lr in (("adam", 0.01), ("sgd", 0.5)):
            _, want, m = hr.adam_trajectory(P, batches, lr, RATES, seed, 0.1, optimizer=optimizer)
            _, f32, _ = hr.adam_trajectory(P, batches, lr, RATES, seed, 0.1, dtype=np.float32, optimizer=optimizer)
            alts = [hr.adam_trajectory(P, batches, lr, RATES, seed, 0.1, dtype=np.float32, optimizer=optimizer, u_flip=i)[1] for i in range(12)]
            if not (m > margin and all(np.abs(alt[key] - want[key]).max() <= 0.75 * FACTOR * max(np.abs(f32[key] - want[key]).max(),
                                                                                              ULP * np.abs(want[key]).max())
                                       for alt in alts for key in TENSORS + BUFFERS)):
                break
        else:
            print("Trainer mask seed", seed)
            break


if __name__ == "__main__":
    choose_seeds()
