"""InteractE on the HIP path (csrc/kge_interacte.hip): parity with the live reference's float64 outputs in
tests/golden/ref_interacte{,_ls,_masked}.npz (predictions in both forms, the fused step with its 12 gradients and six running buffers,
exact ranks), run-to-run determinism, the autograd path, other shapes against the float64 restatement of tools/interacte_reference.py
with shared Philox masks, the ordered scatter on duplicated ids, the public Trainer / Evaluator classes against the restatement's Adam
and SGD trajectories, and the refusals.

Tolerances (the rule of DESIGN.md sections 15, 18 and 19): on every test shape the plain fp32 numpy run of the same formulas
(interacte_reference.step(dtype=np.float32)) is compared with the float64 one; the HIP path is allowed FACTOR = 4 times that error per
quantity (predictions, loss, each gradient, each running buffer), floored at one fp32 ulp (2^-23) of the quantity's max-abs: a measured
error of zero cannot be a bound.  Where a gradient vanishes analytically (interacte_reference.VANISHING: fc.bias without hidden dropout,
bn0.bias and bn0.weight without input dropout) and is below 1e-3 of the sum of the absolute values of its summands in the float64 run
(its cancellation scale), the floor is 2^-23 of that sum.  The figures are printed where they are used; DESIGN.md section 20 lists them."""
import numpy as np
import pytest
import torch

from test_interacte_model import BUFFERS, COUNTERS, NAMES, TENSORS, fixture, ir, recorded_masks, tables  # noqa: F401

pytestmark = pytest.mark.gpu
FACTOR = 4.0
ULP = 2.0 ** -23
MARGIN = 1e-5          # no bn2 output of a test input's float64 run lies this close to zero (a relu follows)
MARGIN1 = 16 * ULP     # ... and no bn1 output this close: the larger shapes have 10^5 of them, all of order 1, so the nearest lies
                       # within 10^-5 of zero by their number alone; 16 ulp keeps the relu's side the same in fp32 and float64


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
    """The drop-in model holding the restatement's state P (parameters and running buffers) and the geometry's chequer permutation."""
    from pykg2vec_amd.projection import InteractE
    E, k = P["ent_embeddings.weight"].shape
    R = P["rel_embeddings.weight"].shape[0]
    m = InteractE(tot_entity=E, tot_relation=R, hidden_size=k, input_dropout=rates[0], feature_map_dropout=rates[1], hidden_dropout=rates[2],
                  feature_permutation=int(G["feature_permutation"]), num_filters=int(G["num_filters"]), kernel_size=int(G["kernel_size"]),
                  reshape_height=int(G["reshape_height"]), reshape_width=int(G["reshape_width"]), seed=seed)
    m.chequer_perm = torch.from_numpy(np.asarray(G["chequer_perm"]).astype(np.int64))
    sd = {key: torch.from_numpy(np.asarray(P[key], dtype=np.float32)) for key in TENSORS + BUFFERS}
    sd.update({key: torch.tensor(counters) for key in COUNTERS})
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def buffers_of(m):
    return {key: v.detach().cpu().numpy().astype(np.float64) for key, v in m.state_dict().items() if key in BUFFERS}


def fused(P, G, h, r, t, y1, y2, rates=(0.0, 0.0, 0.0), seed=0, offset=0, ls=None, raw=False):
    """dict(loss, grads, buffers, counters) of kge_interacte_train_bce through the model's fused step; raw: the device tensors instead."""
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
    return dict(loss=K.read_loss(loss).item(), grads={key: g.cpu().numpy().astype(np.float64) for key, g in zip(TENSORS, gs)},
                buffers=buffers_of(m), counters=[int(m.state_dict()[key]) for key in COUNTERS])


def bounds(P, G, h, r, t, y1, y2, **kw):
    """The float64 step and FACTOR x the fp32 restatement's error per quantity."""
    ref = ir.step(P, G, h, r, t, y1, y2, **kw)
    f32 = ir.step(P, G, h, r, t, y1, y2, dtype=np.float32, **kw)
    b = {"loss": FACTOR * max(abs(f32["loss"] - ref["loss"]), ULP * abs(ref["loss"])),
         "preds": FACTOR * max(np.abs(f32["pred_tails"] - ref["pred_tails"]).max(), np.abs(f32["pred_heads"] - ref["pred_heads"]).max(), ULP)}
    vanishing = ir.VANISHING(kw.get("dropouts", (0.0, 0.0, 0.0)), P["bn0.bias"])
    for key in TENSORS:
        size = np.abs(ref["grads"][key]).max()
        if key in vanishing and size < 1e-3 * ref["scale"][key]:
            size = ref["scale"][key]      # cancelled by the batch norm that follows: the floor is an ulp of what was summed
        b[key] = FACTOR * max(np.abs(f32["grads"][key] - ref["grads"][key]).max(), ULP * size)
    for key in BUFFERS:
        b[key] = FACTOR * max(np.abs(f32["buffers"][key] - ref["buffers"][key]).max(), ULP * np.abs(ref["buffers"][key]).max())
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


def step_kw(z):
    kw = dict(label_smoothing=z["ls"])
    if z["masked"]:
        kw.update(dropouts=z["rates"], seed=int(z["mask_seed"]), offset=int(z["mask_offset"]))
    return kw


def recorded(z):
    return dict(loss=float(z["loss"]), grads={key: z["grad." + key] for key in TENSORS}, buffers={key: z["after." + key] for key in BUFFERS})


# ---------------------------------------------------------------- 1. the fixtures: predictions in both forms, the fused step, the ranks
@pytest.mark.parametrize("name", NAMES)
def test_predictions_match_reference(hip, name):
    z = fixture(name)
    P, G = tables(z), z["G"]
    _, b = bounds(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], **step_kw(z))
    f32 = [ir.forward(P, G, z[e], z["r"], d, dtype=np.float32) for e, d in (("h", "tail"), ("t", "head"))]
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


@pytest.mark.parametrize("name", NAMES)
def test_fused_step_matches_reference(hip, name):
    z = fixture(name)
    P, G = tables(z), z["G"]
    ref, b = bounds(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], **step_kw(z))
    kw = step_kw(z)
    got = fused(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], kw.get("dropouts", (0.0, 0.0, 0.0)), kw.get("seed", 0), kw.get("offset", 0),
                z["ls"])
    check_step(name, got, recorded(z), b)      # the masked case: the kernels draw the recorded masks, or nothing here would agree
    assert np.abs(got["grads"]["rel_embeddings.weight"][0]).max() > 0      # no padding_idx: id 0 is scattered like any other
    assert got["counters"] == [int(z[key]) + 2 for key in COUNTERS] == [int(z["after." + key]) for key in COUNTERS]
    if z["masked"]:
        other = fused(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], z["rates"], int(z["mask_seed"]), int(z["mask_offset"]) + 1, z["ls"])
        assert abs(other["loss"] - float(z["loss"])) > b["loss"]     # another offset: other masks


@pytest.mark.parametrize("name", NAMES)
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
    ranks = K.interacte_eval_ranks(m.make_desc(), trip, t_off, t_ids, h_off, h_ids, ties=ties).cpu().numpy()
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
    one = trip[:1].contiguous()
    got = K.eval_ranks(desc, one, *K.filter_csr_build(hip.dev(known), one, int(z["E"]), int(z["R"]))).cpu().numpy()
    assert got.shape == (4, 1) and np.array_equal(got[:, 0], want[:, 0]), (got, want[:, 0])
    after = buffers_of(m)
    assert all(np.array_equal(before[key], after[key]) for key in BUFFERS) and int(m.bn2.num_batches_tracked) == 2


# ---------------------------------------------------------------- 2. determinism
DET = dict(seed=100, E=70, R=5, rh=3, rw=4, NP=2, NF=3, ks=3, B=9)     # k = 12, an 8 x 3 image


def test_fused_step_is_bit_identical_run_to_run(hip):
    """B = 9: below the head's striped-loss caveat of DESIGN.md section 18, so the loss too.  k = 12, not the fixtures' 6: the head's
    backward products (kge_head_1n_bce, not this model's code) take their reproducible split-K form only where k is a multiple of 4,
    as it is at every preset (k = 200); elsewhere their partial tiles meet in float atomics.  The body is held to the bit at k = 6 below."""
    P, G, h, r, t, y1, y2 = problem(**DET)
    args = (P, G, h, r, t, y1, y2, RATES, 3, 1, 0.1)
    a, b = fused(*args, raw=True), fused(*args, raw=True)
    assert torch.equal(a[0], b[0])
    diff = [i for i, (x, y) in enumerate(zip(a[1] + a[2], b[1] + b[2])) if not torch.equal(x, y)]
    assert not diff, diff
    assert all(float(g.abs().max()) > 0 for g in a[1])
    c = fused(P, G, h, r, t, y1, y2, RATES, 4, 1, 0.1, raw=True)
    assert not torch.equal(a[1][10], c[1][10])     # another seed: other masks (fc.weight)
    p0 = [fused(P, G, h, r, t, y1, y2, seed=s, raw=True) for s in (3, 4)]
    assert all(torch.equal(x, y) for x, y in zip(p0[0][1], p0[1][1]))   # p = 0 draws nothing: the seed cannot matter


def test_body_is_bit_identical_run_to_run_at_the_fixture_shape(hip):
    """The body's forward and backward alone (no head) on the fixture's rows, k = 6, under dropout, with a fixed gradient at x: x, what
    is saved, the 11 gradients of the body (bias is the head's) and the six running buffers."""
    from pykg2vec_amd import kernels as K
    z = fixture("interacte_masked")
    P, G = tables(z), z["G"]
    dx = torch.from_numpy(np.random.default_rng(5).normal(size=(len(z["h"]), 6)).astype(np.float32)).cuda()
    runs = []
    for _ in range(2):
        m = model_for(P, G, z["rates"], counters=2)
        ws = m.trainable_tensors()
        gs = [torch.zeros_like(w) for w in ws]
        d = m.make_desc(ws, gs, train=True, seed=3, offset=1)
        x, saved = K.interacte_body_forward(d, hip.dev(z["h"]), hip.dev(z["r"]), row0=0)
        K.interacte_body_backward(d, hip.dev(z["h"]), hip.dev(z["r"]), dx, saved, row0=0)
        runs.append([x, saved] + gs + [b.clone() for b in m.running_buffers()])
    diff = [i for i, (x, y) in enumerate(zip(*runs)) if not torch.equal(x, y)]
    assert not diff, diff
    assert float(runs[0][2].abs().max()) == 0 and all(float(g.abs().max()) > 0 for g in runs[0][3:14])


# ---------------------------------------------------------------- 3. the autograd path
def test_autograd_path_agrees_with_fused_step(hip):
    z = fixture("interacte_masked")
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
    got = dict(loss=loss.item(), grads={key: p.grad.cpu().numpy().astype(np.float64) for key, p in zip(TENSORS, m.trainable_tensors())},
               buffers=buffers_of(m))
    check_step("autograd", got, recorded(z), b)
    assert [int(m.state_dict()[key]) for key in COUNTERS] == [4, 4, 4]
    step = fused(P, G, z["h"], z["r"], z["t"], z["hr_t"], z["tr_h"], z["rates"], seed, offset, z["ls"])
    check_step("fused", step, recorded(z), b)
    for key in BUFFERS:     # the two paths run the same forward kernels on the same rows
        assert np.array_equal(got["buffers"][key], step["buffers"][key]), key


# ---------------------------------------------------------------- 4. other shapes against the float64 restatement
def problem(seed, E, R, rh, rw, NP, NF, ks, B, repeats=False):
    """Default-init tensors (xavier tables and filter, torch's layer defaults drawn from a seeded generator; the batch norm weights,
    biases and `bias` off their defaults), exact in fp32; running buffers moved off their defaults; the chequer permutation of `seed`."""
    rng = np.random.default_rng(seed)
    k, C = rh * rw, NP * NF
    F = C * 2 * k
    G = dict(reshape_height=rh, reshape_width=rw, feature_permutation=NP, num_filters=NF, kernel_size=ks)
    G["chequer_perm"] = ir.chequer_perm(G, seed)
    u = lambda shape, bound: rng.uniform(-bound, bound, size=shape)
    P = {"bias": 0.1 * rng.normal(size=E), "conv_filt": u((NF, 1, ks, ks), np.sqrt(6.0 / (ks * ks * (1 + NF)))),
         "ent_embeddings.weight": u((E, k), np.sqrt(6.0 / (E + k))), "rel_embeddings.weight": u((R, k), np.sqrt(6.0 / (R + k))),
         "bn0.weight": 1 + 0.2 * rng.normal(size=NP), "bn0.bias": 0.1 * rng.normal(size=NP),
         "bn1.weight": 1 + 0.2 * rng.normal(size=C), "bn1.bias": 0.1 * rng.normal(size=C),
         "bn2.weight": 1 + 0.2 * rng.normal(size=k), "bn2.bias": 0.1 * rng.normal(size=k),
         "fc.weight": u((k, F), 1 / np.sqrt(F)), "fc.bias": u(k, 1 / np.sqrt(F)),
         "bn0.running_mean": 0.1 * rng.normal(size=NP), "bn0.running_var": 1 + 0.3 * rng.random(NP),
         "bn1.running_mean": 0.1 * rng.normal(size=C), "bn1.running_var": 1 + 0.3 * rng.random(C),
         "bn2.running_mean": 0.1 * rng.normal(size=k), "bn2.running_var": 1 + 0.3 * rng.random(k)}
    P = {key: v.astype(np.float32).astype(np.float64) for key, v in P.items()}
    h, r, t = rng.integers(E, size=B), rng.integers(R, size=B), rng.integers(E, size=B)
    if repeats:     # ONE entity as the head of most rows and the tail of some, ONE relation in most rows, id 0 on both tables
        h[:B - 3] = 7
        t[1] = t[4] = 7
        r[:B - 2] = 2
        h[B - 1] = t[B - 2] = 0
        r[B - 1] = 0
    y1, y2 = (rng.random((B, E)) < 0.05).astype(np.float64), (rng.random((B, E)) < 0.05).astype(np.float64)
    y1[np.arange(B), t], y2[np.arange(B), h] = 1.0, 1.0
    return P, G, h, r, t, y1, y2


def representative(P, G, h, r, t, y1, y2, ref, b, orders=8, slack=0.75, **kw):
    """Is the bound of this input representative?  The bound is FACTOR x the error of ONE fp32 run, the restatement's in numpy's order
    of additions.  With few rows a batch norm subtracts a mean from values that lie close together and the backward amplifies the
    rounding of those few values by its rstd, so the fp32 error of such an input is a matter of luck.  An input
    is used only where the bound also covers the fp32 restatement under `orders` other (seeded, permuted) orders of the fc sum, with
    `slack` to spare.  CPU-only: the seeds below were chosen with this function (choose_seeds, python tests/test_hip_interacte.py) and the
    margin, never from what the kernels give."""
    F = np.asarray(P["fc.weight"]).shape[1]
    for i in range(orders):
        perm = np.random.default_rng(1000 + i).permutation(F)
        Q = dict(P)
        Q["fc.weight"] = np.asarray(P["fc.weight"])[:, perm]     # the same model with the feature axis renumbered ...
        got = ir.step(Q, G, h, r, t, y1, y2, dtype=np.float32, fc_order=perm, **kw)     # ... and A renumbered with it
        back = np.argsort(perm)
        for key in TENSORS:
            g = got["grads"][key]
            if key == "fc.weight":
                g = g[:, back]
            if not np.abs(g - ref["grads"][key]).max() <= slack * b[key]:
                return False
    return True


# (a) H = 2, W = 3, odd k = 3, F = 18 (no multiple of 4), one permutation, n = 2: the least batch norm accepts
# (b) pad = 3 = min(H, W): the largest wrap allowed; three permutations; n = 17
# (c) the presets' 20 x 20 image; n = 33 straddles nothing within a 64-row tile but E = 500 and F = 6 400 are split-K
# (d) 70 rows: the second 64-row fc tile is partial
# seeds chosen on the CPU (choose_seeds) so that no bn2 / bn1 output of the float64 run is within MARGIN / MARGIN1 of zero (asserted
# below) and the bounds are representative
SHAPES = {"a_least": dict(seed=107, E=70, R=5, rh=3, rw=1, NP=1, NF=3, ks=3, B=2),
          "b_full_wrap": dict(seed=104, E=70, R=5, rh=3, rw=2, NP=3, NF=2, ks=7, B=17),
          "c_preset_image": dict(seed=269, E=500, R=5, rh=20, rw=10, NP=2, NF=8, ks=9, B=33),
          "d_row_tile": dict(seed=100, E=70, R=5, rh=3, rw=2, NP=2, NF=3, ks=3, B=70)}
RATES = (0.2, 0.2, 0.3)


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
    check_step(case, got, ref, b)
    # the predictions under the same masks: the body of each direction with the step's seed / offset and mask rows, then the head
    m = model_for(P, G, rates)
    B = len(h)
    for side, e, want in ((0, h, ref["pred_tails"]), (1, t, ref["pred_heads"])):
        d = m.make_desc(train=True, seed=kw["seed"], offset=kw["offset"])
        x, _ = K.interacte_body_forward(d, hip.dev(e), hip.dev(r), row0=side * B)
        p = K.head_1n_forward(x, m.ent_embeddings.weight.detach(), m.bias.detach()).cpu().numpy()
        err = np.abs(p - want).max()
        print(case, "side", side, "preds err %.3g (bound %.3g)" % (err, b["preds"]))
        assert err <= b["preds"]


# ---------------------------------------------------------------- 5. the ordered scatter on duplicated ids
DUP = dict(seed=100, E=70, R=5, rh=3, rw=2, NP=2, NF=3, ks=3, B=40, repeats=True)


def test_scatter_sums_duplicates(hip):
    """One entity in 37 of 40 head rows (and two tail rows), one relation in 38 rows, id 0 on both tables: every lookup gradient row is
    the ordered sum of its rows' shares."""
    P, G, h, r, t, y1, y2 = problem(**DUP)
    assert (h == 7).sum() >= 37 and (r == 2).sum() >= 38 and (h == 0).any() and (r == 0).any()
    kw = dict(dropouts=RATES, seed=(7 << 32) | 9, offset=5)
    ref, b = bounds(P, G, h, r, t, y1, y2, label_smoothing=0.1, **kw)
    assert ref["margin2"] > MARGIN and ref["margin1"] > MARGIN1
    got = fused(P, G, h, r, t, y1, y2, RATES, kw["seed"], kw["offset"], 0.1)
    check_step("duplicates", got, ref, b)
    for key, row in (("ent_embeddings.weight", 7), ("rel_embeddings.weight", 2), ("rel_embeddings.weight", 0)):
        err = np.abs(got["grads"][key][row] - ref["grads"][key][row]).max()
        print("duplicates", key, row, "err %.3g (bound %.3g, max-abs %.3g)" % (err, b[key], np.abs(ref["grads"][key][row]).max()))
        assert err <= b[key] and np.abs(ref["grads"][key][row]).max() > 0
    # a row that was dropped or doubled would move the repeated relation's gradient by about 1 / 38 of itself
    assert b["rel_embeddings.weight"] < np.abs(ref["grads"]["rel_embeddings.weight"][2]).max() / 38 / 4


# ---------------------------------------------------------------- 6. Trainer and Evaluator against the restatement's trajectory
# three Adam steps (and, as a second case, three plain SGD steps) with the Philox masks of (config.seed, step)
TRAINER = dict(seed=100, E=300, R=5, rh=3, rw=2, NP=2, NF=3, ks=3, B=16)
MASK_SEED = 24     # chosen on the CPU (choose_seeds): the margin, asserted below, and bounds that are representative


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
    want_losses, want, margin = ir.adam_trajectory(P, G, batches, lr, RATES, seed, 0.1, optimizer=optimizer)
    f32_losses, f32, _ = ir.adam_trajectory(P, G, batches, lr, RATES, seed, 0.1, dtype=np.float32, optimizer=optimizer)
    print("pre-ReLU margin over the three steps %.3g" % margin)
    assert margin > MARGIN
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
    for key in TENSORS + BUFFERS:
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
    trained = {key: sd[key].detach().cpu().numpy().astype(np.float64) for key in TENSORS + BUFFERS}
    want_ranks, gap = ir.ranks(trained, G, test, known)
    print("float64 rank gap of the trained model %.3g" % gap)
    assert gap > 1e-6     # fixed seed: no close pair, so every rank must be exact
    assert np.array_equal(ranks, want_ranks), (ranks, want_ranks)


# ---------------------------------------------------------------- 7. refusals
def test_refusals(hip):
    import ctypes
    from pykg2vec_amd import _lib as L, kernels as K
    from pykg2vec_amd.projection import InteractE
    from pykg2vec_amd.trainer import Trainer
    from pykg2vec_amd.generator import Generator
    z = fixture("interacte")
    P, G = tables(z), z["G"]
    m = model_for(P, G)
    m.train()
    one = hip.dev(z["h"][:1])
    with pytest.raises(L.KgeHipError, match="kge_interacte_body_forward: batch norm in training form needs more than one row"):
        m(one, hip.dev(z["r"][:1]), "tail")
    m.eval()
    with torch.no_grad():
        assert m(one, hip.dev(z["r"][:1]), "tail").shape == (1, 70)      # one row is fine under eval()
    kw = dict(tot_entity=70, tot_relation=5, hidden_size=6, input_dropout=0.0, feature_map_dropout=0.0, hidden_dropout=0.0,
              feature_permutation=2, num_filters=3, kernel_size=3, reshape_height=3, reshape_width=2)
    two = hip.dev(z["h"][:2])
    for over, msg in ((dict(kernel_size=4), "kernel_size = 4 must be odd and at least 3"),
                      (dict(kernel_size=9), r"kernel_size / 2 = 4 exceeds min\(H, W\) = 3"),
                      (dict(kernel_size=13), "kernel_size = 13 exceeds 11"),
                      (dict(hidden_dropout=1.0), r"dropout rate 2 must be in \[0, 1\)")):
        bad = InteractE(**dict(kw, **over)).cuda()
        with pytest.raises(L.KgeHipError, match=msg):
            bad(two, hip.dev(z["r"][:2]), "tail")
    notperm = model_for(P, G)
    notperm.chequer_perm = torch.zeros(2, 12, dtype=torch.long)
    with pytest.raises(L.KgeHipError, match="row 0 of chequer_perm is not a permutation"):
        notperm(two, hip.dev(z["r"][:2]), "tail")
    m.bn1.momentum = None
    with pytest.raises(L.KgeHipError, match="cumulative moving average"):
        m.make_desc()
    m.bn1.momentum = 0.1
    d = m.make_desc(train=False)
    need = int(L.load().kge_interacte_eval_ranks_workspace_bytes(ctypes.byref(d), 4))
    d._ws = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    trip = hip.dev(z["test"][:4])
    ranks = torch.empty((4, 4), dtype=torch.int32, device="cuda")
    rc = L.load().kge_interacte_eval_ranks(ctypes.byref(d), ctypes.c_void_p(trip.data_ptr()), 4, None, None, None, None,
                                           ctypes.c_void_p(d._ws.data_ptr()), need - 1, ctypes.c_void_p(ranks.data_ptr()), None, None)
    assert rc != 0 and "kge_interacte_eval_ranks: workspace too small" in L.load().kge_last_error().decode()
    cfg = lambda **over: hip.make_config(70, 5, dict({"neg_rate": 0}, **over), z["train"], z["valid"], z["test"], batch_size=9, optimizer="adam")
    with pytest.raises(NotImplementedError, match="InteractE: .*neg_rate > 0.* is not supported on the projection path"):
        Trainer(model_for(P, G), cfg(neg_rate=1)).build_model()
    with pytest.raises(NotImplementedError, match="neg_rate > 0 is not supported"):
        Generator(model_for(P, G), cfg(neg_rate=2))
    with pytest.raises(NotImplementedError, match="InteractE: .*hipGraph capture"):
        Trainer(model_for(P, G), cfg(), use_graph=True).build_model()
    tn = Trainer(model_for(P, G), cfg())
    tn.distributed = True
    with pytest.raises(NotImplementedError, match="InteractE: data-parallel training"):
        tn.build_model()
    assert K.interacte_shapes(70, 5, 3, 2, 2, 3, 3)[0][10] == (6, 72)
    # the device copies of the permutation follow the weights and a reassignment
    moved = model_for(P, G)
    assert moved._perms()[0].is_cuda and moved._perms()[0] is moved._perms()[0]
    first = moved._perms()[0]
    moved.chequer_perm = torch.from_numpy(np.asarray(G["chequer_perm"]).astype(np.int64)).cuda()
    assert moved._perms()[0] is not first and torch.equal(moved._perms()[0], first)


# ---------------------------------------------------------------- seed choice, on the CPU
def choose_seeds(margin=10 * MARGIN, tries=2000):
    """Prints, per shape of SHAPES (and for the duplicates case), the first seed at or after the listed one whose float64 margin exceeds
    `margin` and whose bounds are representative at both rate settings, and the first such mask seed of the Trainer test (there: the
    fp32 trajectory under twelve other orders of the fc sums stays within three quarters of every final tensor's bound, under Adam and
    under SGD: Adam divides by sqrt(v), so where a gradient is mostly rounding its update is too).  Needs no GPU."""
    for case, spec in sorted(SHAPES.items()) + [("duplicates", DUP)]:
        for seed in range(spec["seed"], spec["seed"] + tries):
            P, G, h, r, t, y1, y2 = problem(**dict(spec, seed=seed))
            for rates in ((0.0, 0.0, 0.0), RATES):
                kw = dict(dropouts=rates, seed=(7 << 32) | 9, offset=5, label_smoothing=0.1)
                ref, b = bounds(P, G, h, r, t, y1, y2, **kw)
                if not (ref["margin2"] > margin and ref["margin1"] > 2 * MARGIN1 and representative(P, G, h, r, t, y1, y2, ref, b, **kw)):
                    break
            else:
                print(case, "seed", seed, flush=True)
                break
    P, G, train, valid, test, batches = trainer_problem()
    F = P["fc.weight"].shape[1]
    for seed in range(MASK_SEED, MASK_SEED + tries):
        for optimizer, lr in (("adam", 0.01), ("sgd", 0.5)):
            _, want, m = ir.adam_trajectory(P, G, batches, lr, RATES, seed, 0.1, optimizer=optimizer)
            _, f32, _ = ir.adam_trajectory(P, G, batches, lr, RATES, seed, 0.1, dtype=np.float32, optimizer=optimizer)
            alts = [ir.adam_trajectory(P, G, batches, lr, RATES, seed, 0.1, dtype=np.float32, optimizer=optimizer,
                                       fc_order=np.random.default_rng(1000 + i).permutation(F))[1] for i in range(12)]
            if not (m > margin and all(np.abs(alt[key] - want[key]).max() <= 0.75 * FACTOR * max(np.abs(f32[key] - want[key]).max(),
                                                                                              ULP * np.abs(want[key]).max())
                                       for alt in alts for key in TENSORS + BUFFERS)):
                break
        else:
            print("Trainer mask seed", seed, flush=True)
            break


if __name__ == "__main__":
    choose_seeds()
