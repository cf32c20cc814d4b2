"""The 1-N head's GEMMs (pykg2vec_amd/csrc/kge_head.hip) at their tile, slab, split-K, alignment and dispatch edges, against float64.

tests/head_edges_ref.py holds the float64 reference, the a-priori elementwise bounds (derived there and in DESIGN.md section 33, fixed
before any GPU run), the restatement of the host dispatcher (plan) and the case lists.  Case sets, one dimension walking its edges
while the others stay at the ragged base (65, 131, 36) or its d % 4 != 0 twin (65, 131, 35):

    F   forward, MODE 0: every hidden size around a K-slab edge of every forward kernel (1 .. 5 slabs), B and E around both tile
        edges and the whole / partial vector store; every kernel that can serve a shape runs it, the fp32 ones must agree bit for bit
        (csrc/kge_head.hip:156-157 "bit-identical logits"), and so must the two bf16 ones (:954)
    X   tile numbering: 1 .. 9 entity tiles at both tile sizes, KGE_HEAD_XCD unset and 0: identical results
    L   fused loss: no positives, an empty row next to a full one, corner positives, more positives than k_head_bce_pos has lanes
    Bk  backward products, autograd and fused form, small and wide kernels: E over all residues of E % 4, B and d over the tile edges,
        shapes around the B E >= 4 rule; the atomic-free epilogues twice, bit for bit
    S   split-K edges under KGE_HEAD_MINK=16: 15 / 16 / 17 splits, last splits of 1, 15, 16 elements
    A   accumulate (loss, g_ent, g_bias: prefilled) and overwrite (dx: prefilled with NaN), two directions in a row, each epilogue
    M   operands that are 4-byte but not 16-byte aligned
    D   the default thresholds without switches: 198 / 200 wide tiles, B = 2559 / 2560 without a workspace

The CPU tests hold the fp32 numpy restatement of every case to the same bounds, check that one dropped term would exceed them
(where that is arithmetically possible: see test_one_dropped_term_exceeds_the_bound), and check with plan() that the lists reach
every kernel instantiation, epilogue, parts-sum width, split edge, slab count and tile-count residue.

Switches are set through the environment only (the library reads it on every call, csrc/kge_debug.hip:20-28); K.set_switch is not
used: its overrides are process-wide and outrank the environment for every later test module."""
import ctypes
import os

import numpy as np
import pytest

import head_edges_ref as R

gpu = pytest.mark.gpu
REPORT = "r28_head_edges"


@pytest.fixture(autouse=True)
def no_head_switches(monkeypatch):
    for name in list(os.environ):
        if name.startswith("KGE_HEAD_"):
            monkeypatch.delenv(name)


def set_env(monkeypatch, env):
    for name in R.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        assert name in R.SWITCHES, name
        monkeypatch.setenv(name, value)


# =============================================================================================================== CPU
def test_reference_restates_the_oracle():
    """The float64 loss and its derivative here are kge_oracle's multi_class_bce_dir in float64 (up to the fp32-rounded smoothed labels
    the entry point forms), and the products are its head_1n_backward."""
    import kge_oracle as ko
    B, E, d = R.BASE
    i = R.inputs(B, E, d)
    for ls in R.L_LS:
        r = R.fused_case(i.x, i.ent, i.bias, i.labels, ls)
        _z, p = R.forward64(i.x, i.ent, i.bias)
        loss, dp = ko.multi_class_bce_dir(p, i.labels, ls, E if ls is not None else None, dtype=np.float64)
        assert np.isclose(r.ref["loss"], loss, rtol=1e-7, atol=0)
        dx, ge, gb = ko.head_1n_backward(i.x, i.ent, p, dp, dtype=np.float64)
        for name, want in (("dx", dx), ("g_ent", ge), ("g_bias", gb)):
            assert np.allclose(r.ref[name], want, rtol=1e-6, atol=1e-7 / (B * E)), name


@pytest.mark.parametrize("which", R.SETS)
def test_fp32_restatement_meets_every_bound(which):
    worst, _least, _ins = R.survey(which)
    print(which, "largest error / bound of the fp32 numpy restatement:", {k: round(v, 4) for k, v in worst.items()})
    assert worst and all(v <= 1.0 for v in worst.values()), worst


def _beyond_reach(case, name):
    """Where the bounds cannot separate ONE term: they grow with K^2 u (the chain bound times the sum) and, in the fused form, with
    K (d + 1) u (the logit bound enters every dz element), the smallest term does not grow at all.  With magnitudes in [0.5, 1] the
    8 x margin is arithmetically out of reach from about K (d + 1) = 8192 (fused) and K = 512 (autograd); DESIGN.md section 33."""
    kind, B, E, d = case[:4]
    K = E if name == "dx" else B
    return K * (d + 1) > 8192 if kind in ("fused", "acc") else K > 512


@pytest.mark.parametrize("which", R.SETS)
def test_one_dropped_term_exceeds_the_bound(which):
    """The smallest single term of every output element is at least 8 x that element's bound, for every case and output up to the
    reach of the bounds (_beyond_reach: long sums, where a dropped float4 of one slab still shows in the shorter twin of the same
    set, which is inside the reach)."""
    _worst, least, insensitive = R.survey(which)
    print(which, "smallest term / bound:", {k: round(v, 2) for k, v in least.items()}, "beyond reach:", len(insensitive))
    bad = [(c, n, s) for c, n, s in insensitive if not _beyond_reach(c, n)]
    assert not bad, bad


def test_plan_reaches_every_branch():
    plans = [(c, R.plan(c.B, c.E, c.d, c.aligned, c.have_ws, c.fused, c.env)) for c in R.plan_cases()]
    runs_backward = lambda c: c.fused or c.set in ("Bk", "S", "M") or (c.set == "D" and not c.have_ws)
    fwd = [p["forward"] for c, p in plans if c.fused or c.set in ("F", "X", "M") or (c.set == "D" and c.have_ws)]
    bf = [p["forward_bf16"] for c, p in plans if c.set in ("F", "X", "M") and not c.fused]
    dx = [p["dx"] for c, p in plans if runs_backward(c)]
    dent = [p["dent"] for c, p in plans if runs_backward(c)]
    missing = []

    def need(what, ok):
        if not ok:
            missing.append(what)

    kernels = {f["kernel"] for f in fwd} | {f["kernel"] for f in bf} | {q["kernel"] for q in dx + dent}
    for k in ["k_head_gemm<0>", "k_head_gemm<1>", "k_head_gemm64x<0>", "k_head_gemm64x<1>", "k_head_gemm128x<0>", "k_head_gemm128x<1>",
              "k_head_gemm_bf16", "k_head_gemm128_bf16", "k_head_dx", "k_head_dent", "k_head_dx128<false>", "k_head_dx128<true>",
              "k_head_dent128<false>", "k_head_dent128<true>"]:
        need(k, k in kernels)
    for name, qs in (("dx", dx), ("dent", dent)):
        for emode in (R.DIRECT, R.PARTS):
            for form in ("128<true>", "128<false>"):
                need((name, emode, form), any(q["emode"] == emode and q["kernel"].endswith(form) for q in qs))
        need((name, "atomic, small"), any(q["emode"] == R.ATOMIC and "128" not in q["kernel"] for q in qs))
        need((name, "atomic, wide"), any(q["emode"] == R.ATOMIC and q["kernel"].endswith("128<false>") for q in qs))
        parts = [q for q in qs if q["emode"] == R.PARTS]
        need((name, "L = 1 at 15 splits"), any(q["splits"] == 15 and q["L"] == 1 for q in parts))
        need((name, "L = 8 at 16 splits"), any(q["splits"] == 16 and q["L"] == 8 for q in parts))
        need((name, "L = 8 at 17 splits"), any(q["splits"] == 17 and q["L"] == 8 for q in parts))
        for form in ("128<true>", "128<false>"):
            wide = [q for q in qs if q["kernel"].endswith(form) and q["splits"] > 1]
            need((name, form, "last split of 1"), any(q["last"] == 1 for q in wide))
            need((name, form, "last split of 15"), any(q["last"] == 15 for q in wide))
            need((name, form, "last split of one full slab"), any(q["last"] == 16 == q["per"] for q in wide))
            need((name, form, "last split of per > one slab"), any(q["last"] == q["per"] > 16 for q in wide))
        small = [q for q in qs if "128" not in q["kernel"] and q["splits"] > 1]
        need((name, "small, last split of 1"), any(q["last"] == 1 for q in small))
        need((name, "small, last split of per"), any(q["last"] == q["per"] for q in small))
    for k in ("k_head_gemm<0>", "k_head_gemm64x<0>", "k_head_gemm128x<0>", "k_head_gemm_bf16", "k_head_gemm128_bf16"):
        slabs = {f["nslab"] for f in fwd + bf if f["kernel"] == k}
        need((k, "slab counts", sorted(slabs)), {1, 2, 3, 4, 5} <= slabs)
    for tile in (R.HT, R.HT2):
        res = {f["T"] & 7 for c, p in plans if c.set == "X" for f in (p["forward"], p["forward_bf16"]) if f["tile"] == tile and f["xcd_runs"]}
        need(("T & 7", tile, sorted(res)), res == (set(range(8)) if tile == R.HT2 else {0, 2, 4, 6}))
        plain = {f["T"] for c, p in plans if c.set == "X" for f in (p["forward"],) if f["tile"] == tile and not f["xcd_runs"]}
        need(("plain numbering", tile), len(plain) == 9)
    # the default thresholds, straddled (csrc/kge_head.hip:593 tiles >= 200, :975 B >= 2560 without a workspace)
    d_fwd = [R.plan(B, E, d, True, True, False, {})["forward"] for B, E, d in R.D_FWD]
    need(("198 / 200 tiles", d_fwd), [(f["kernel"], _tiles128(B, E)) for f, (B, E, _d) in zip(d_fwd, R.D_FWD)]
         == [("k_head_gemm64x<0>", 198), ("k_head_gemm128x<0>", 200)])
    d_bwd = [R.plan(B, E, d, True, False, False, {})["dent"] for B, E, d in R.D_BWD]
    need(("B = 2559 / 2560", d_bwd), [(q["kernel"], q["emode"]) for q in d_bwd] == [("k_head_dent", R.ATOMIC), ("k_head_dent128<false>", R.ATOMIC)])
    # the B E >= 4 rule of the autograd form, both sides (:977)
    small = {(B, E): R.plan(B, E, 4, True, True, False, {"KGE_HEAD_TILE": "1"})["dx"]["kernel"] for B, E, _d in R.BK_SMALL}
    need(("B E >= 4", small), small == {(1, 1): "k_head_dx", (1, 3): "k_head_dx", (3, 1): "k_head_dx", (1, 4): "k_head_dx128<false>",
                                       (2, 2): "k_head_dx128<false>"})
    # what set A relies on
    for (B, E, d), env, emodes in R.A_CASES:
        p = R.plan(B, E, d, True, True, True, env)
        need(("A", (B, E, d), env), (p["dx"]["emode"], p["dent"]["emode"]) == emodes)
    # a misaligned operand changes kernels, forward and backward (:588-604, :972)
    p = R.plan(*R.BASE, aligned=False, have_ws=True, fused=False, env={})
    need(("misaligned", p), (p["forward"]["kernel"], p["dx"]["kernel"], p["dent"]["kernel"]) == ("k_head_gemm<0>", "k_head_dx", "k_head_dent"))
    assert not missing, missing


def _tiles128(B, E):
    return -(-B // R.HT2) * -(-E // R.HT2)


# =============================================================================================================== GPU
@pytest.fixture(scope="module")
def hip():
    import torch
    import hip_util
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip_util


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the cached inputs are read-only)


def off_by_one_float(t):
    """A contiguous copy of t that starts one float into a larger buffer: 4-byte but not 16-byte aligned."""
    import torch
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def raw_bce(x, ent, bias, off, ids, ls, loss_buf, dx, g_ent, g_bias):
    """kge_head_1n_bce through the library handle, with the caller's dx (K.head_1n_bce allocates its own)."""
    import torch
    from pykg2vec_amd import _lib as L
    lib = L.load()
    (B, d), E, n_pos = x.shape, ent.shape[0], int(ids.numel())
    ws = torch.empty(lib.kge_head_1n_bce_workspace_bytes(B, E, n_pos), dtype=torch.uint8, device=x.device)
    for t in (x, ent, bias, loss_buf, dx, g_ent, g_bias):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())
    assert off.dtype == torch.int64 and ids.dtype == torch.int32 and tuple(dx.shape) == (B, d) and tuple(g_ent.shape) == (E, d)
    L.check(lib.kge_head_1n_bce(_p(x), B, d, _p(ent), E, _p(bias), _p(off), _p(ids) if n_pos else None, n_pos,
                                -1.0 if ls is None else float(ls), _p(ws), ws.numel(), _p(loss_buf), _p(dx), _p(g_ent), _p(g_bias),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "kge_head_1n_bce")
    return dx


def raw_backward(x, ent, preds, dpreds, dx, g_ent, g_bias, workspace=True):
    """kge_head_1n_backward through the library handle, with the caller's (possibly misaligned) dx and g_ent."""
    import torch
    from pykg2vec_amd import _lib as L
    lib = L.load()
    (B, d), E = x.shape, ent.shape[0]
    for t in (x, ent, preds, dpreds, dx, g_ent, g_bias):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())
    assert tuple(preds.shape) == (B, E) == tuple(dpreds.shape) and tuple(dx.shape) == (B, d) and tuple(g_ent.shape) == (E, d)
    ws = torch.empty(lib.kge_head_1n_backward_workspace_bytes(), dtype=torch.uint8, device=x.device) if workspace else None
    L.check(lib.kge_head_1n_backward(_p(x), B, d, _p(ent), E, _p(preds), _p(dpreds), _p(dx), _p(g_ent), _p(g_bias), _p(ws),
                                     ws.numel() if workspace else 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "kge_head_1n_backward")


def held(hip, which, got, res, names, where):
    """Every named output within its bound; the largest error / bound of the set goes to the report.  Returns the misses."""
    arrays = {k: (v if isinstance(v, float) else v.cpu().numpy()) for k, v in got.items() if v is not None}
    ratios = R.worst_ratio(arrays, res, [n for n in names if n in arrays])
    for name, r in ratios.items():
        hip.record_max(REPORT, "%s.%s" % (which, name), r)
    return ["%s %s: error / bound = %.3g" % (where, n, r) for n, r in ratios.items() if not r <= 1.0]


def run_fused(K, B, E, d, kind, ls):
    import torch
    i = R.inputs(B, E, d, kind)
    off, ids = R.csr_of(i.labels)
    loss_buf = K.new_loss_buffer("cuda")
    g_ent, g_bias = torch.zeros((E, d), device="cuda"), torch.zeros(E, device="cuda")
    dx = K.head_1n_bce(dev(i.x), dev(i.ent), dev(i.bias), dev(off), dev(ids), ls, loss_buf, g_ent, g_bias)
    return dict(loss=float(K.read_loss(loss_buf).item()), dx=dx, g_ent=g_ent, g_bias=g_bias)


def run_autograd(K, B, E, d, workspace, need_bias):
    i = R.inputs(B, E, d)
    dx, g_ent, g_bias = K.head_1n_backward(dev(i.x), dev(i.ent), dev(R.auto_preds(B, E, d)), dev(i.dpreds), need_bias=need_bias,
                                           workspace=workspace)
    return dict(dx=dx, g_ent=g_ent, g_bias=g_bias)


def same(a, b, names):
    import torch
    return [n for n in names if a.get(n) is not None and not torch.equal(a[n], b[n])]


GRADS = ("dx", "g_ent", "g_bias")


def forward_ways(hip, monkeypatch, which, B, E, d, with_bias, ways, extra_env=None):
    """The predictions of every kernel that serves the shape: each within its bound; {way: tensor}, misses."""
    from pykg2vec_amd import kernels as K
    i = R.inputs(B, E, d)
    xd, ed, bd = dev(i.x), dev(i.ent), dev(i.bias) if with_bias else None
    out, misses = {}, []
    for name, env, bf in ways:
        set_env(monkeypatch, dict(env, **(extra_env or {})))
        out[name] = K.head_1n_forward(xd, ed, bd, precision="bf16" if bf else "f32")
        misses += held(hip, which + (".bf16" if bf else ""), dict(preds=out[name]), R.fwd_result(B, E, d, with_bias, bf), ("preds",), name)
    return out, misses


def equal_among(out, ways):
    """The fp32 kernels keep one k-ordered chain per element, the two bf16 kernels one 16-k chain: identical predictions."""
    import torch
    misses = []
    for bf in (False, True):
        names = [n for n, _e, b in ways if b == bf]
        misses += ["%s != %s" % (names[0], n) for n in names[1:] if not torch.equal(out[names[0]], out[n])]
    return misses


@gpu
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B,E,d", R.F_SHAPES)
def test_forward_edges(hip, monkeypatch, B, E, d, with_bias):
    out, misses = forward_ways(hip, monkeypatch, "F", B, E, d, with_bias, R.fwd_ways(d))
    misses += equal_among(out, R.fwd_ways(d))
    assert not misses, misses


@gpu
@pytest.mark.parametrize("B,E,d,tile", R.X_SHAPES)
def test_tile_numbering(hip, monkeypatch, B, E, d, tile):
    from pykg2vec_amd import kernels as K
    ways = R.X_WAYS[tile]
    runs, misses = {}, []
    for xcd in ({}, {"KGE_HEAD_XCD": "0"}):
        out, m = forward_ways(hip, monkeypatch, "X", B, E, d, True, ways, xcd)
        misses += m + equal_among(out, ways)
        for name, env, bf in ways:
            if not bf:          # MODE 1: the same numbering under the fused loss
                set_env(monkeypatch, dict(env, **xcd))
                out[name + "<1>"] = run_fused(K, B, E, d, "random", 0.1)
                misses += held(hip, "X", out[name + "<1>"], R.fused_result(B, E, d), ("loss",) + GRADS, name + "<1>")
        runs[bool(xcd)] = out
    import torch
    for name in runs[False]:
        a, b = runs[False][name], runs[True][name]
        differ = same(a, b, GRADS) if isinstance(a, dict) else ([] if torch.equal(a, b) else ["preds"])
        misses += ["%s: %s differs between the tile numberings" % (name, n) for n in differ]
    assert not misses, misses


@gpu
@pytest.mark.parametrize("shape,env,kind,ls", R.L_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_fused_loss_label_extremes(hip, monkeypatch, shape, env, kind, ls):
    from pykg2vec_amd import kernels as K
    B, E, d = shape
    n_pos = int(R.inputs(B, E, d, kind).labels.sum())
    assert {"none": n_pos == 0, "all": n_pos == B * E > 8 * 4096}.get(kind, True)
    set_env(monkeypatch, env)
    misses = held(hip, "L", run_fused(K, B, E, d, kind, ls), R.fused_result(B, E, d, kind, ls), ("loss",) + GRADS, kind)
    assert not misses, misses


def backward_forms(hip, monkeypatch, which, B, E, d, envs, forms):
    """Every (switches, form) of a shape, twice: within the bounds, and bit for bit where no epilogue is atomic."""
    from pykg2vec_amd import kernels as K
    misses = []
    for env in envs:
        for form, ws, need_bias in forms:
            set_env(monkeypatch, env)
            if form == "bce":
                run = lambda: run_fused(K, B, E, d, "random", 0.1)
                res, names = R.fused_result(B, E, d), ("loss",) + GRADS
            else:
                run = lambda: run_autograd(K, B, E, d, ws, need_bias)
                res, names = R.auto_result(B, E, d), GRADS
            where = "%s %s ws=%s bias=%s" % (env, form, ws, need_bias)
            a, b = run(), run()
            misses += held(hip, "%s.%s" % (which, form), a, res, names, where)
            p = R.plan(B, E, d, True, ws, form == "bce", env)
            fixed = [n for n, q in (("dx", p["dx"]), ("g_ent", p["dent"]), ("g_bias", p["dent"])) if q["emode"] != R.ATOMIC]
            misses += ["%s %s: not reproduced bit for bit" % (where, n) for n in same(a, b, fixed)]
    return misses


@gpu
@pytest.mark.parametrize("B,E,d", R.BK_SHAPES)
def test_backward_products(hip, monkeypatch, B, E, d):
    misses = backward_forms(hip, monkeypatch, "Bk", B, E, d, R.BK_ENVS, R.BK_FORMS)
    assert not misses, misses


@gpu
@pytest.mark.parametrize("B,E,d,env", R.S_CASES, ids=lambda v: "-".join(v.values()) if isinstance(v, dict) else str(v))
def test_split_edges(hip, monkeypatch, B, E, d, env):
    misses = backward_forms(hip, monkeypatch, "S", B, E, d, (env,), R.S_FORMS)
    assert not misses, misses


@gpu
@pytest.mark.parametrize("shape,env,emodes", R.A_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_accumulates_and_overwrites(hip, monkeypatch, shape, env, emodes):
    """loss, g_ent and g_bias are added to (prefilled, two directions in a row), dx is overwritten (prefilled with NaN)."""
    import torch
    from pykg2vec_amd import kernels as K
    B, E, d = shape
    i1, i2, r1, r2 = R.accumulate_result(B, E, d)
    pre = R.prefill(E, d)
    loss_buf, g_ent, g_bias = dev(pre.loss), dev(pre.g_ent), dev(pre.g_bias)
    ed, bd = dev(i1.ent), dev(i1.bias)
    set_env(monkeypatch, env)
    misses = []
    for step, (i, r) in enumerate(((i1, r1), (i2, r2))):
        off, ids = R.csr_of(i.labels)
        dx = torch.full((B, d), float("nan"), device="cuda")
        raw_bce(dev(i.x), ed, bd, dev(off), dev(ids), 0.1, loss_buf, dx, g_ent, g_bias)
        got = dict(loss=float(K.read_loss(loss_buf).item()), dx=dx, g_ent=g_ent.clone(), g_bias=g_bias.clone())
        assert bool(torch.isfinite(dx).all()), "dx keeps part of what it held before the call"
        misses += held(hip, "A", got, r, ("loss",) + GRADS, "direction %d" % (step + 1))
    assert not misses, misses


@gpu
@pytest.mark.parametrize("B,E,d", R.M_SHAPES)
def test_misaligned_operands(hip, monkeypatch, B, E, d):
    """x, ent, preds / dpreds and g_ent one float into a larger buffer: other kernels serve (csrc/kge_head.hip:592, :600, :972), the
    results stay within the bounds, and equal the aligned run's where the source claims one chain (forward; the autograd form's
    wide products, whose preds / dpreds fetches are 4-byte aligned by design, :651-653)."""
    import torch
    from pykg2vec_amd import kernels as K
    i = R.inputs(B, E, d)
    off, ids = R.csr_of(i.labels)
    xd, ed, bd, pd, qd = dev(i.x), dev(i.ent), dev(i.bias), dev(R.auto_preds(B, E, d)), dev(i.dpreds)
    xm, em, pm, qm = (off_by_one_float(t) for t in (xd, ed, pd, qd))
    misses = []
    for bf in (False, True):
        prec = "bf16" if bf else "f32"
        a, m = K.head_1n_forward(xd, ed, bd, precision=prec), K.head_1n_forward(xm, em, bd, precision=prec)
        for where, t in (("aligned", a), ("misaligned", m)):
            misses += held(hip, "M" + (".bf16" if bf else ""), dict(preds=t), R.fwd_result(B, E, d, True, bf), ("preds",), where + " " + prec)
        if not torch.equal(a, m):
            misses.append("forward %s: misaligned x / ent change the predictions" % prec)

    def autograd(x, ent, preds, dpreds, misaligned_g_ent=False):
        dx, g_bias = torch.empty((B, d), device="cuda"), torch.zeros(E, device="cuda")
        g_ent = torch.zeros((E, d), device="cuda")
        g_ent = off_by_one_float(g_ent) if misaligned_g_ent else g_ent
        raw_backward(x, ent, preds, dpreds, dx, g_ent, g_bias)
        return dict(dx=dx, g_ent=g_ent, g_bias=g_bias)

    runs = {"aligned": autograd(xd, ed, pd, qd), "preds, dpreds": autograd(xd, ed, pm, qm), "x, ent": autograd(xm, em, pd, qd),
            "g_ent": autograd(xd, ed, pd, qd, True), "all": autograd(xm, em, pm, qm, True)}
    for where, got in runs.items():
        misses += held(hip, "M.bwd", got, R.auto_result(B, E, d), GRADS, "autograd, misaligned " + where)
    misses += ["autograd, misaligned preds / dpreds: %s differs from the aligned run" % n for n in same(runs["aligned"], runs["preds, dpreds"], GRADS)]

    def fused(x, ent, misaligned_g_ent=False):
        loss_buf, dx, g_bias = K.new_loss_buffer("cuda"), torch.empty((B, d), device="cuda"), torch.zeros(E, device="cuda")
        g_ent = torch.zeros((E, d), device="cuda")
        g_ent = off_by_one_float(g_ent) if misaligned_g_ent else g_ent
        raw_bce(x, ent, bd, dev(off), dev(ids), 0.1, loss_buf, dx, g_ent, g_bias)
        return dict(loss=float(K.read_loss(loss_buf).item()), dx=dx, g_ent=g_ent, g_bias=g_bias)

    for where, got in (("aligned", fused(xd, ed)), ("x, ent", fused(xm, em)), ("g_ent", fused(xd, ed, True))):
        misses += held(hip, "M.bce", got, R.fused_result(B, E, d), ("loss",) + GRADS, "fused, misaligned " + where)
    assert not misses, misses


@gpu
@pytest.mark.parametrize("B,E,d", R.D_FWD)
def test_default_tile_threshold(hip, monkeypatch, B, E, d):
    _out, misses = forward_ways(hip, monkeypatch, "D", B, E, d, True, (("default", {}, False),))
    assert not misses, misses


@gpu
@pytest.mark.parametrize("B,E,d", R.D_BWD)
def test_default_workspace_free_threshold(hip, monkeypatch, B, E, d):
    from pykg2vec_amd import kernels as K
    set_env(monkeypatch, {})
    misses = held(hip, "D.bwd", run_autograd(K, B, E, d, False, True), R.auto_result(B, E, d), GRADS, "workspace-free")
    assert not misses, misses
