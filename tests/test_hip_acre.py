"""AcrE (serial way) on the HIP path (csrc/kge_acre.hip): parity with the live reference's float64 outputs in
tests/golden/ref_acre{,_ls,_masked}.npz (predictions in both forms, the fused step with every gradient and the six running buffers,
exact ranks), run-to-run determinism, the autograd path, other shapes against the float64 restatement of tools/acre_reference.py
with shared Philox masks, the ordered scatter on duplicated ids, the public Trainer / Evaluator classes against the restatement's Adam
and SGD trajectories, and the refusals.  The parallel way is not built on this path; its fixtures are checked on the CPU only
(test_acre_model.py).

Tolerances (the rule of DESIGN.md sections 15, 18 - 20): on every test shape the plain fp32 numpy run of the same formulas
(acre_reference.step(dtype=np.float32)) is compared with the float64 one; the HIP path is allowed FACTOR = 4 times that error per
quantity (predictions, loss, each gradient, each running buffer), floored at one fp32 ulp (2^-23) of the quantity's max-abs: a measured
error of zero cannot be a bound.  Where a gradient vanishes analytically (acre_reference.vanishing: fc.bias without hidden dropout,
conv3.bias always) and is below 1e-3 of the sum of the absolute values of its summands in the float64 run (its cancellation scale),
the floor is 2^-23 of that sum.  The figures are printed where they are used; DESIGN.md section 21 lists them."""
import numpy as np
import pytest
import torch

from test_acre_model import BUFFERS, COUNTERS, SERIAL, ar, fixture, recorded_grad_error, tables  # noqa: F401

pytestmark = pytest.mark.gpu
FACTOR = 4.0
ULP = 2.0 ** -23
MARGIN = 1e-5          # no bn2 output of a test input's float64 run lies this close to zero (a relu follows)
MARGIN1 = 16 * ULP     # ... and no bn1 output this close: the larger shapes have 10^5 - 10^6 of them, all of order 1, so the nearest
                       # lies within 10^-5 of zero by their number alone; 16 ulp keeps the relu's side the same in fp32 and float64
RATES = (0.2, 0.2, 0.3)


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


def model_for(P, G, rates=(0.0, 0.0, 0.0), counters=0, seed=0):
    """The drop-in model holding the restatement's state P (parameters and running buffers)."""
    from pykg2vec_amd.projection import AcrE
    E = P["ent_embeddings.weight"].shape[0]
    R = P["rel_embeddings.weight"].shape[0] // 2
    m = AcrE(tot_entity=E, tot_relation=R, hidden_size=200, input_dropout=rates[0], feature_map_dropout=rates[1], hidden_dropout=rates[2],
             in_channels=int(G["in_channels"]), way=G["way"], first_atrous=int(G["first_atrous"]), second_atrous=int(G["second_atrous"]),
             third_atrous=int(G["third_atrous"]), acre_bias=bool(G["acre_bias"]), seed=seed)
    sd = {key: torch.from_numpy(np.asarray(P[key], dtype=np.float32)) for key in ar.tensors(G) + BUFFERS}
    sd.update({key: torch.tensor(counters) for key in COUNTERS})
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def buffers_of(m):
    return {key: v.detach().cpu().numpy().astype(np.float64) for key, v in m.state_dict().items() if key in BUFFERS}


def fused(P, G, h, r, t, y1, y2, rates=(0.0, 0.0, 0.0), seed=0, offset=0, ls=None, raw=False):
    """dict(loss, grads, buffers, counters) of kge_acre_train_bce through the model's fused step; raw: the device tensors instead."""
    from pykg2vec_amd import kernels as K
    import types
    m = model_for(P, G, rates, counters=2)
    m.train()
    ws = m.trainable_tensors()
    gs = [torch.zeros_like(w) for w in ws]
    d = m.make_desc(ws, gs, train=True, seed=seed, offset=offset)
    loss = K.new_loss_buffer(ws[0].device)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda()
    m.fused_projection_step(K, d, dev(h), dev(r), dev(t), csr(y1), csr(y2), None, types.SimpleNamespace(label_smoothing=ls), loss)
    if raw:
        return loss.clone(), gs, [b.clone() for b in m.running_buffers()]
    return dict(loss=K.read_loss(loss).item(), grads={key: g.cpu().numpy().astype(np.float64) for key, g in zip(ar.tensors(G), gs)},
                buffers=buffers_of(m), counters=[int(m.state_dict()[key]) for key in COUNTERS])


def bounds(P, G, h, r, t, y1, y2, **kw):
    """The float64 step and FACTOR x the fp32 restatement's error per quantity."""
    ref = ar.step(P, G, h, r, t, y1, y2, **kw)
    f32 = ar.step(P, G, h, r, t, y1, y2, dtype=np.float32, **kw)
    b = {"loss": FACTOR * max(abs(f32["loss"] - ref["loss"]), ULP * abs(ref["loss"])),
         "preds": FACTOR * max(np.abs(f32["pred_tails"] - ref["pred_tails"]).max(), np.abs(f32["pred_heads"] - ref["pred_heads"]).max(), ULP)}
    vanishing = ar.vanishing(G, kw.get("dropouts", (0.0, 0.0, 0.0)), P)
    for key in ar.tensors(G):
        size = np.abs(ref["grads"][key]).max()
        if key in vanishing and size < 1e-3 * ref["scale"][key]:
            size = ref["scale"][key]      # cancelled by the batch norm that follows: the floor is an ulp of what was summed
        b[key] = FACTOR * max(np.abs(f32["grads"][key] - ref["grads"][key]).max(), ULP * size)
    for key in BUFFERS:
        b[key] = FACTOR * max(np.abs(f32["buffers"][key] - ref["buffers"][key]).max(), ULP * np.abs(ref["buffers"][key]).max())
    return ref, b


def check_step(tag, G, got, want, b, z=None):
    """want: dict(loss, grads, buffers) in float64.  z: a fixture whose RECORDED gradients are compared as well (the two large ones at
    their recorded sample; the float64 restatement `want`, which test_acre_model.py pins to the fixture at 1e-10, covers every entry)."""
    err = abs(got["loss"] - want["loss"])
    print(tag, "loss err %.3g (bound %.3g)" % (err, b["loss"]))
    bad = [] if err <= b["loss"] else ["loss"]
    for key in ar.tensors(G):
        err = np.abs(got["grads"][key] - want["grads"][key]).max()
        print(tag, "grad", key, "err %.3g (bound %.3g, max-abs %.3g)" % (err, b[key], np.abs(want["grads"][key]).max()))
        if not err <= b[key]:
            bad.append(key)
        if z is not None and not recorded_grad_error(z, key, got["grads"][key])[0] <= b[key]:
            bad.append("recorded " + key)
    for key in BUFFERS:
        err = np.abs(got["buffers"][key] - want["buffers"][key]).max()
        print(tag, key, "err %.3g (bound %.3g, max-abs %.3g)" % (err, b[key], np.abs(want["buffers"][key]).max()))
        if not err <= b[key]:
            bad.append(key)
    assert not bad, (tag, bad)


def step_kw(z):
    kw = dict(label_smoothing=z["ls"])
    if z["masked"]:
        kw.update(dropouts=z["rates"], seed=int(z["mask_seed"]), offset=int(z["mask_offset"]))
    return kw


def recorded(z, ref):
    """The fixture's loss and buffers, and the float64 restatement's gradients (pinned to the fixture's on the CPU)."""
    return dict(loss=float(z["loss"]), grads=ref["grads"], buffers={key: z["after." + key] for key in BUFFERS})


# ---------------------------------------------------------------- 1. the fixtures: predictions in both forms, the fused step, the ranks
@pytest.mark.parametrize("name", SERIAL)
def test_predictions_match_reference(hip, name):
    z = fixture(name)
    P, G = tables(z), z["G"]
    _, b = bounds(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], **step_kw(z))
    f32 = [ar.forward(P, G, z[e], z["r"], d, dtype=np.float32) for e, d in (("h", "tail"), ("t", "head"))]
    b_eval = FACTOR * max(np.abs(f32[0] - z["eval_pred_tails"]).max(), np.abs(f32[1] - z["eval_pred_heads"]).max(), ULP)
    m = model_for(P, G, z["rates"], counters=2, seed=int(z["mask_seed"]) if z["masked"] else 0)
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


@pytest.mark.parametrize("name", SERIAL)
def test_fused_step_matches_reference(hip, name):
    z = fixture(name)
    P, G = tables(z), z["G"]
    kw = step_kw(z)
    ref, b = bounds(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], **kw)
    got = fused(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], kw.get("dropouts", (0.0, 0.0, 0.0)), kw.get("seed", 0), kw.get("offset", 0),
                z["ls"])
    check_step(name, G, got, recorded(z, ref), b, z)      # the masked case: the kernels draw the recorded masks, or nothing here would agree
    assert np.abs(got["grads"]["rel_embeddings.weight"][0]).max() > 0      # no padding_idx: id 0 is scattered like any other
    assert not got["grads"]["rel_embeddings.weight"][5:].any()             # rows R .. 2R-1: reachable only by an id >= R
    assert got["counters"] == [int(z[key]) + 2 for key in COUNTERS] == [int(z["after." + key]) for key in COUNTERS]
    if z["masked"]:
        other = fused(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], z["rates"], int(z["mask_seed"]), int(z["mask_offset"]) + 1, z["ls"])
        assert abs(other["loss"] - float(z["loss"])) > b["loss"]     # another offset: other masks


@pytest.mark.parametrize("name", SERIAL)
def test_ranks_are_exact(hip, name):
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.evaluator import Evaluator
    z = fixture(name)
    m = model_for(tables(z), z["G"], z["rates"], counters=2)
    m.eval()
    before = buffers_of(m)
    known = np.concatenate([z["train"], z["valid"], z["test"]])
    trip = hip.dev(z["test"])
    want = z["ranks"]      # rows: head, tail, filtered head, filtered tail
    t_off, t_ids, h_off, h_ids = K.filter_csr_build(hip.dev(known), trip, int(z["E"]), int(z["R"]))
    ties = torch.zeros((2, len(z["test"])), dtype=torch.int32, device="cuda")
    ranks = K.acre_eval_ranks(m.make_desc(), trip, t_off, t_ids, h_off, h_ids, ties=ties).cpu().numpy()
    assert np.array_equal(ranks, want), (ranks, want)
    assert int(ties.sum()) == 0
    m.train()     # the rank pass is the eval form whatever the module's mode
    assert np.array_equal(K.eval_ranks(m.make_desc(), trip, t_off, t_ids, h_off, h_ids).cpu().numpy(), want)
    m.eval()
    cfg = hip.make_config(int(z["E"]), int(z["R"]), {"neg_rate": 0}, z["train"], z["valid"], z["test"], batch_size=9)
    got, ev_ties = Evaluator(m, cfg).rank_all(z["test"], len(z["test"]), return_ties=True)
    assert np.array_equal(got.cpu().numpy(), want) and int(ev_ties.sum()) == 0
    one = trip[:1].contiguous()
    got = K.eval_ranks(m.make_desc(train=False), one, *K.filter_csr_build(hip.dev(known), one, int(z["E"]), int(z["R"]))).cpu().numpy()
    assert got.shape == (4, 1) and np.array_equal(got[:, 0], want[:, 0]), (got, want[:, 0])
    after = buffers_of(m)
    assert all(np.array_equal(before[key], after[key]) for key in BUFFERS) and int(m.bn2.num_batches_tracked) == 2


# ---------------------------------------------------------------- 2. determinism
def test_fused_step_is_bit_identical_run_to_run(hip):
    """At the fixture shape itself: k = 200 is a multiple of 4, so the head's backward products take their ordered split-K form; B = 9
    is below the head's striped-loss caveat of DESIGN.md section 18, so the loss too."""
    z = fixture("acre_masked")
    P, G = tables(z), z["G"]
    args = (P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], RATES, 3, 1, 0.1)
    a, b = fused(*args, raw=True), fused(*args, raw=True)
    assert torch.equal(a[0], b[0])
    diff = [i for i, (x, y) in enumerate(zip(a[1] + a[2], b[1] + b[2])) if not torch.equal(x, y)]
    assert not diff, diff
    assert all(float(g.abs().max()) > 0 for g in a[1])
    c = fused(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], RATES, 4, 1, 0.1, raw=True)
    assert not torch.equal(a[1][9], c[1][9])     # another seed: other masks (fc.weight)
    p0 = [fused(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], seed=s, raw=True) for s in (3, 4)]
    assert all(torch.equal(x, y) for x, y in zip(p0[0][1], p0[1][1]))   # p = 0 draws nothing: the seed cannot matter


# ---------------------------------------------------------------- 3. the autograd path
def test_autograd_path_agrees_with_fused_step(hip):
    z = fixture("acre_masked")
    P, G = tables(z), z["G"]
    seed, offset = int(z["mask_seed"]), int(z["mask_offset"])
    ref, b = bounds(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], **step_kw(z))
    m = model_for(P, G, z["rates"], counters=2, seed=seed)
    m.train()
    m.dropout_offset = offset
    pred_tails = m(hip.dev(z["h"]), hip.dev(z["r"]), "tail")
    m.dropout_offset = offset      # the step's two directions share one offset; the head direction's mask rows follow the tail's
    pred_heads = m(hip.dev(z["t"]), hip.dev(z["r"]), "head")
    loss = m.loss(pred_heads, pred_tails, torch.from_numpy(z["tr_h"]).float().cuda(), torch.from_numpy(z["hr_t"]).float().cuda(), z["ls"],
                  int(z["E"]))
    loss.backward()
    got = dict(loss=loss.item(), grads={key: p.grad.cpu().numpy().astype(np.float64) for key, p in zip(ar.tensors(G), m.trainable_tensors())},
               buffers=buffers_of(m))
    check_step("autograd", G, got, recorded(z, ref), b, z)
    assert [int(m.state_dict()[key]) for key in COUNTERS] == [4, 4, 4]
    step = fused(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], z["rates"], seed, offset, z["ls"])
    check_step("fused", G, step, recorded(z, ref), b, z)
    for key in BUFFERS:     # the two paths run the same forward kernels on the same rows
        assert np.array_equal(got["buffers"][key], step["buffers"][key]), key


# ---------------------------------------------------------------- 4. other shapes against the float64 restatement
def problem(seed, E, R, C, dil, B, bias=True, repeats=False, high_rel=False):
    """Default-init tensors (xavier tables, torch's layer defaults drawn from a seeded generator; the batch norm weights, biases and
    `bias` off their defaults), exact in fp32; running buffers moved off their defaults."""
    rng = np.random.default_rng(seed)
    G = dict(in_channels=C, way="serial", first_atrous=dil[0], second_atrous=dil[1], third_atrous=dil[2], acre_bias=bias)
    shp = ar.shapes(G, E, R)
    u = lambda shape, bound: rng.uniform(-bound, bound, size=shape)
    P = {}
    for key in ar.tensors(G) + BUFFERS:
        s = shp[key]
        if key == "bias":
            P[key] = 0.1 * rng.normal(size=s)
        elif key.endswith("embeddings.weight"):
            P[key] = u(s, np.sqrt(6.0 / (s[0] + s[1])))
        elif key.startswith("bn") and key.endswith(".weight"):
            P[key] = 1 + 0.2 * rng.normal(size=s)
        elif key.endswith("running_var"):
            P[key] = 1 + 0.3 * rng.random(s)
        elif key.startswith("bn"):
            P[key] = 0.1 * rng.normal(size=s)
        elif key.startswith("fc"):
            P[key] = u(s, 1 / np.sqrt(400 * C))
        else:     # conv weights and biases: torch's default bound 1 / sqrt(fan_in)
            P[key] = u(s, 1 / np.sqrt(9 * (1 if key.startswith("conv1") else C)))
    P = {key: v.astype(np.float32).astype(np.float64) for key, v in P.items()}
    h, r, t = rng.integers(E, size=B), rng.integers(R, size=B), rng.integers(E, size=B)
    if repeats:     # ONE entity as the head of most rows and the tail of some, ONE relation in most rows, id 0 on both tables
        h[:B - 3] = 7
        t[1] = t[4] = 7
        r[:B - 2] = 2
        h[B - 1] = t[B - 2] = 0
        r[B - 1] = 0
    if high_rel:    # an id >= R of the relation table is an ordinary row
        r[B - 3] = R + 1
    y1, y2 = (rng.random((B, E)) < 0.05).astype(np.float64), (rng.random((B, E)) < 0.05).astype(np.float64)
    y1[np.arange(B), t], y2[np.arange(B), h] = 1.0, 1.0
    return P, G, h, r, t, y1, y2


def representative(P, G, h, r, t, y1, y2, ref, b, orders=12, slack=0.75, **kw):
    """Is the bound of this input representative?  The bound is FACTOR x the error of ONE fp32 run, the restatement's in numpy's order
    of additions.  An input is used only where the bound also covers the fp32 restatement under `orders` other (seeded, permuted) orders
    of the fc and conv sums, with a quarter to spare.  CPU-only: the seeds below were chosen with this function (choose_seeds, python
    tests/test_hip_acre.py) and the margins, never from what the kernels give."""
    for i in range(orders):
        got = ar.step(P, G, h, r, t, y1, y2, dtype=np.float32, order=1000 + i, **kw)
        if abs(got["loss"] - ref["loss"]) > slack * b["loss"]:
            return False
        for key in ar.tensors(G):
            if not np.abs(got["grads"][key] - ref["grads"][key]).max() <= slack * b[key]:
                return False
        for key in BUFFERS:
            if not np.abs(got["buffers"][key] - ref["buffers"][key]).max() <= slack * b[key]:
                return False
    return True


# (a) C = 1, n = 2: the least batch norm accepts, one channel in a 16-channel tile
# (b) C = 5, dilations 3 / 1 / 4 (KGE_ACRE_MAX_ATROUS): the largest reach into the padding, a dilation order that is not ascending; n = 17
# (c) C = 32, the presets', both channel tiles full; E = 500 and F = 12 800 are split-K; n = 33; no conv biases
# (d) 70 rows: the second 64-row fc tile is partial; C = 16: exactly one channel tile
# seeds chosen on the CPU (choose_seeds) so that no bn2 / bn1 output of the float64 run is within MARGIN / MARGIN1 of zero (asserted
# below) and the bounds are representative.  (a) is the exception: with n = 2 bn2's normalised values are +-1 whatever u is, every body
# gradient survives through bn2's eps alone, and no seed among 2 000 keeps twelve permuted fp32 orders within the bound of one fp32
# run; it keeps the first seed whose float64 margins hold, fixed before any kernel ran.
SHAPES = {"a_least": dict(seed=100, E=70, R=5, C=1, dil=(1, 2, 2), B=2),
          "b_reach": dict(seed=151, E=70, R=5, C=5, dil=(3, 1, 4), B=17),
          "c_preset": dict(seed=127, E=500, R=5, C=32, dil=(1, 2, 2), B=33, bias=False),
          "d_row_tile": dict(seed=343, E=70, R=5, C=16, dil=(1, 2, 2), B=70)}


@pytest.mark.parametrize("rates", [(0.0, 0.0, 0.0), RATES], ids=["p0", "dropout"])
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_other_shapes_match_float64(hip, case, rates):
    from pykg2vec_amd import kernels as K
    P, G, h, r, t, y1, y2 = problem(**SHAPES[case])
    kw = dict(dropouts=rates, seed=(7 << 32) | 9, offset=5)
    ref, b = bounds(P, G, h, r, t, y1, y2, label_smoothing=0.1, **kw)
    print(case, "pre-ReLU margins: bn1 %.3g, bn2 %.3g" % (ref["margin1"], ref["margin2"]))
    assert ref["margin2"] > MARGIN and ref["margin1"] > MARGIN1
    got = fused(P, G, h, r, t, y1, y2, rates, kw["seed"], kw["offset"], 0.1)
    check_step(case, G, got, ref, b)
    # the predictions under the same masks: the body of each direction with the step's seed / offset and mask rows, then the head
    m = model_for(P, G, rates)
    B = len(h)
    for side, e, want in ((0, h, ref["pred_tails"]), (1, t, ref["pred_heads"])):
        d = m.make_desc(train=True, seed=kw["seed"], offset=kw["offset"])
        x, _ = K.acre_body_forward(d, hip.dev(e), hip.dev(r), row0=side * B)
        p = K.head_1n_forward(x, m.ent_embeddings.weight.detach(), m.bias.detach()).cpu().numpy()
        err = np.abs(p - want).max()
        print(case, "side", side, "preds err %.3g (bound %.3g)" % (err, b["preds"]))
        assert err <= b["preds"]


# ---------------------------------------------------------------- 5. the ordered scatter on duplicated ids
DUP = dict(seed=174, E=70, R=5, C=3, dil=(1, 2, 3), B=40, repeats=True, high_rel=True)


def test_scatter_sums_duplicates(hip):
    """One entity in 37 of 40 head rows (and two tail rows), one relation in 38 rows, id 0 on both tables, one relation id >= R: every
    lookup gradient row is the ordered sum of its rows' shares."""
    P, G, h, r, t, y1, y2 = problem(**DUP)
    assert (h == 7).sum() >= 37 and (r == 2).sum() >= 37 and (h == 0).any() and (r == 0).any() and (r == 6).sum() == 1
    kw = dict(dropouts=RATES, seed=(7 << 32) | 9, offset=5)
    ref, b = bounds(P, G, h, r, t, y1, y2, label_smoothing=0.1, **kw)
    assert ref["margin2"] > MARGIN and ref["margin1"] > MARGIN1
    got = fused(P, G, h, r, t, y1, y2, RATES, kw["seed"], kw["offset"], 0.1)
    check_step("duplicates", G, got, ref, b)
    for key, row in (("ent_embeddings.weight", 7), ("rel_embeddings.weight", 2), ("rel_embeddings.weight", 0), ("rel_embeddings.weight", 6)):
        err = np.abs(got["grads"][key][row] - ref["grads"][key][row]).max()
        print("duplicates", key, row, "err %.3g (bound %.3g, max-abs %.3g)" % (err, b[key], np.abs(ref["grads"][key][row]).max()))
        assert err <= b[key] and np.abs(ref["grads"][key][row]).max() > 0
    # a row that was dropped or doubled would move the repeated relation's gradient by about 1 / 38 of itself
    assert b["rel_embeddings.weight"] < np.abs(ref["grads"]["rel_embeddings.weight"][2]).max() / 38 / 4


# ---------------------------------------------------------------- 6. Trainer and Evaluator against the restatement's trajectory
# three Adam steps (and, as a second case, three plain SGD steps) with the Philox masks of (config.seed, step)
TRAINER = dict(seed=100, E=300, R=5, C=3, dil=(1, 2, 3), B=16, bias=False)
MASK_SEED = 41     # chosen on the CPU (choose_seeds): the margin, asserted below, and bounds that are representative


def trainer_problem():
    P, G, _, _, _, _, _ = problem(**TRAINER)
    rng = np.random.default_rng(TRAINER["seed"] + 1)
    E, R, B = TRAINER["E"], TRAINER["R"], TRAINER["B"]
    trip = np.unique(np.stack([rng.integers(E, size=400), rng.integers(R, size=400), rng.integers(E, size=400)], 1), axis=0)
    trip = trip[rng.permutation(len(trip))]
    train, valid, test = trip[:10 * B], trip[10 * B:10 * B + 12], trip[10 * B + 12:10 * B + 24]
    batches = []
    for i in range(3):
        rows = train[i * B:(i + 1) * B]
        y1, y2 = np.zeros((B, E)), np.zeros((B, E))
        for j, (a, rel, c) in enumerate(rows):
            y1[j, train[(train[:, 0] == a) & (train[:, 1] == rel), 2]] = 1.0
            y2[j, train[(train[:, 2] == c) & (train[:, 1] == rel), 0]] = 1.0
        batches.append((rows[:, 0], rows[:, 1], rows[:, 2], y1, y2))
    return P, G, train, valid, test, batches


@pytest.mark.parametrize("optimizer,lr", [("adam", 0.01), ("sgd", 0.5)])
def test_trainer_matches_float64_trajectory(hip, optimizer, lr):
    from pykg2vec_amd.trainer import Trainer
    P, G, train, valid, test, batches = trainer_problem()
    E, R, B, seed = TRAINER["E"], TRAINER["R"], TRAINER["B"], MASK_SEED
    keys = ar.tensors(G)
    want_losses, want, margin = ar.trajectory(P, G, batches, lr, RATES, seed, 0.1, optimizer=optimizer)
    f32_losses, f32, _ = ar.trajectory(P, G, batches, lr, RATES, seed, 0.1, dtype=np.float32, optimizer=optimizer)
    print("pre-ReLU margins over the three steps: bn1 %.3g, bn2 %.3g" % margin)
    assert margin[1] > MARGIN and margin[0] > MARGIN1
    cfg = hip.make_config(E, R, {"neg_rate": 0}, train, valid, test, batch_size=B, optimizer=optimizer, lr=lr, label_smoothing=0.1)
    cfg.seed = seed
    tn = Trainer(model_for(P, G, RATES, counters=2), cfg)
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
    for key in keys + BUFFERS:
        got = sd[key].detach().cpu().numpy().astype(np.float64)
        bound = FACTOR * max(np.abs(f32[key] - want[key]).max(), ULP * np.abs(want[key]).max())
        err = np.abs(got - want[key]).max()
        print("final", key, "err %.3g (bound %.3g)" % (err, bound))
        if not err <= bound:
            bad.append(key)
    # (Adam divides by sqrt(v): where a gradient is rounding noise the update is noise of the order of lr, in the fp32 restatement as
    # here, and so is its bound.  The fp32 restatement forms the optimiser's weights 1 - beta in fp32, as csrc/kge_opt_device.h does.)
    assert not bad, bad
    tn.model.eval()
    ranks = tn.evaluator.rank_all(test, len(test)).cpu().numpy()
    known = np.concatenate([train, valid, test])
    # "the restatement's ranks" are the restatement's eval form on the parameters the Trainer arrived at (not on the restatement's own
    # final trajectory): the Evaluator is held to exact ranks of the model it was given, the trajectory itself is checked above
    trained = {key: sd[key].detach().cpu().numpy().astype(np.float64) for key in keys + BUFFERS}
    want_ranks, gap = ar.ranks(trained, G, test, known)
    print("float64 rank gap of the trained model %.3g" % gap)
    assert gap > 1e-6     # fixed seed: no close pair, so every rank must be exact
    assert np.array_equal(ranks, want_ranks), (ranks, want_ranks)


# ---------------------------------------------------------------- 7. refusals
def test_refusals(hip):
    import ctypes
    from pykg2vec_amd import _lib as L
    from pykg2vec_amd.projection import AcrE
    from pykg2vec_amd.trainer import Trainer
    from pykg2vec_amd.generator import Generator
    z = fixture("acre")
    P, G = tables(z), z["G"]
    m = model_for(P, G)
    m.train()
    one = hip.dev(z["h"][:1])
    with pytest.raises(L.KgeHipError, match="kge_acre_body_forward: batch norm in training form needs more than one row"):
        m(one, hip.dev(z["r"][:1]), "tail")
    m.eval()
    with torch.no_grad():
        assert m(one, hip.dev(z["r"][:1]), "tail").shape == (1, 70)      # one row is fine under eval()
    kw = dict(tot_entity=70, tot_relation=5, hidden_size=200, input_dropout=0.0, feature_map_dropout=0.0, hidden_dropout=0.0, in_channels=3,
              way="serial", first_atrous=1, second_atrous=2, third_atrous=3, acre_bias=True)
    two = hip.dev(z["h"][:2])
    for over, msg in ((dict(third_atrous=5), r"dilation 3 = 5 must be in \[1, 4\]"),
                      (dict(in_channels=33), "in_channels = 33 exceeds 32"),
                      (dict(hidden_dropout=1.0), r"dropout rate 2 must be in \[0, 1\)")):
        bad = AcrE(**dict(kw, **over)).cuda()
        with pytest.raises(L.KgeHipError, match=msg):
            bad(two, hip.dev(z["r"][:2]), "tail")
    with torch.no_grad():      # the relation table has 2 R rows: id 2 R - 1 is an ordinary row
        assert m(two, torch.full((2,), 9, dtype=torch.long, device="cuda"), "tail").shape == (2, 70)
    d = m.make_desc(train=False)
    need = int(L.load().kge_acre_eval_ranks_workspace_bytes(ctypes.byref(d), 4))
    d._ws = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    trip = hip.dev(z["test"][:4])
    ranks = torch.empty((4, 4), dtype=torch.int32, device="cuda")
    rc = L.load().kge_acre_eval_ranks(ctypes.byref(d), ctypes.c_void_p(trip.data_ptr()), 4, None, None, None, None,
                                      ctypes.c_void_p(d._ws.data_ptr()), need - 1, ctypes.c_void_p(ranks.data_ptr()), None, None)
    assert rc != 0 and "kge_acre_eval_ranks: workspace too small" in L.load().kge_last_error().decode()
    cfg = lambda **over: hip.make_config(70, 5, dict({"neg_rate": 0}, **over), z["train"], z["valid"], z["test"], batch_size=9, optimizer="adam")
    with pytest.raises(NotImplementedError, match="AcrE: .*neg_rate > 0.* is not supported on the projection path"):
        Trainer(model_for(P, G), cfg(neg_rate=1)).build_model()
    with pytest.raises(NotImplementedError, match="neg_rate > 0 is not supported"):
        Generator(model_for(P, G), cfg(neg_rate=2))
    with pytest.raises(NotImplementedError, match="AcrE: .*hipGraph capture"):
        Trainer(model_for(P, G), cfg(), use_graph=True).build_model()
    tn = Trainer(model_for(P, G), cfg())
    tn.distributed = True
    with pytest.raises(NotImplementedError, match="AcrE: data-parallel training"):
        tn.build_model()


# ---------------------------------------------------------------- seed choice, on the CPU
def choose_seeds(margin=MARGIN, tries=2000):
    """Prints, per shape of SHAPES (and for the duplicates case), the first seed at or after the listed one whose float64 margin exceeds
    `margin` and whose bounds are representative at both rate settings, and the first such mask seed of the Trainer test (there: the
    fp32 trajectory under twelve other orders of the fc and conv sums stays within three quarters of every final tensor's bound, under
    Adam and under SGD).  Needs no GPU."""
    for case, spec in sorted(SHAPES.items()) + [("duplicates", DUP)]:
        for seed in range(spec["seed"], spec["seed"] + tries):
            P, G, h, r, t, y1, y2 = problem(**dict(spec, seed=seed))
            for rates in ((0.0, 0.0, 0.0), RATES):
                kw = dict(dropouts=rates, seed=(7 << 32) | 9, offset=5, label_smoothing=0.1)
                ref, b = bounds(P, G, h, r, t, y1, y2, **kw)
                if not (ref["margin2"] > margin and ref["margin1"] > MARGIN1 and representative(P, G, h, r, t, y1, y2, ref, b, **kw)):
                    break
            else:
                print(case, "seed", seed, flush=True)
                break
    P, G, train, valid, test, batches = trainer_problem()
    for seed in range(MASK_SEED, MASK_SEED + tries):
        for optimizer, lr in (("adam", 0.01), ("sgd", 0.5)):
            _, want, m = ar.trajectory(P, G, batches, lr, RATES, seed, 0.1, optimizer=optimizer)
            _, f32, _ = ar.trajectory(P, G, batches, lr, RATES, seed, 0.1, dtype=np.float32, optimizer=optimizer)
            alts = [ar.trajectory(P, G, batches, lr, RATES, seed, 0.1, dtype=np.float32, optimizer=optimizer, order=1000 + i)[1]
                    for i in range(12)]
            if not (m[1] > margin and m[0] > MARGIN1 and all(np.abs(alt[key] - want[key]).max() <= 0.75 * FACTOR * max(np.abs(f32[key] - want[key]).max(),
                                                                                              ULP * np.abs(want[key]).max())
                                       for alt in alts for key in ar.tensors(G) + BUFFERS)):
                break
        else:
            print("Trainer mask seed", seed, flush=True)
            break


if __name__ == "__main__":
    choose_seeds()
