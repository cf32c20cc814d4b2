"""OctonionE (pointwise.py:772-1001) on the CPU: importer keys and model id, constructor parity with the frozen reference
(tests/golden/ref_octonione*.npz, tools/make_golden_octonione.py), get_reg, and the float64 restatement of the forward and of the
two rank queries that the GPU tests (test_hip_octonione.py) measure the kernels against."""
import os
import re

import numpy as np
import pytest
import torch

from golden_util import GOLDEN

NAMES = ["octonione", "octonione_neg3"]
SEEDS = {"octonione": 3301, "octonione_neg3": 3302}   # tools/make_golden_octonione.py: torch.manual_seed, then the constructor
ENT = ["ent_embedding_%d" % i for i in range(1, 9)]
REL = ["rel_embedding_%d" % i for i in range(1, 9)]


def load(name):
    return np.load(os.path.join(GOLDEN, "ref_%s.npz" % name))


# ---------------------------------------------------------------- float64 restatement of pointwise.py:905-1001
def qmult(a, b):
    sa, xa, ya, za = a
    sb, xb, yb, zb = b
    return (sa * sb - xa * xb - ya * yb - za * zb, sa * xb + sb * xa + ya * zb - yb * za,
            sa * yb + sb * ya + za * xb - zb * xa, sa * zb + sb * za + xa * yb - xb * ya)


def qstar(q):
    return (q[0], -q[1], -q[2], -q[3])


def omult(h, r):
    a, b, c, d = h[:4], h[4:], r[:4], r[4:]
    lo = [x - y for x, y in zip(qmult(a, c), qmult(qstar(d), b))]
    hi = [x + y for x, y in zip(qmult(d, a), qmult(b, qstar(c)))]
    return lo + hi


def onorm(r):
    den = torch.sqrt(sum(x ** 2 for x in r))
    return [x / den for x in r]


def rows(P, ids, names):
    return [P[n][ids] for n in names]


def energy64(P, h, r, t):
    """P: {table name: float64 tensor}.  -sum_k sum_c o_c t_c with o = omult(h, onorm(r))."""
    o = omult(rows(P, h, ENT), onorm(rows(P, r, REL)))
    return -sum(oc * tc for oc, tc in zip(o, rows(P, t, ENT))).sum(-1)


def reg64(P, h, r, t, p):
    return sum(torch.mean(torch.abs(x) ** p) for x in rows(P, h, ENT) + rows(P, t, ENT) + rows(P, r, REL))


def pointwise_loss64(P, h, r, t, y, lmbda, p=3):
    """Trainer.train_step_pointwise with Criterion.pointwise_logistic and OctonionE.get_reg (utils/trainer.py:176-180)."""
    return torch.nn.functional.softplus(y * energy64(P, h, r, t)).mean() + lmbda * reg64(P, h, r, t, p)


def tail_query(h8, r8):
    """Row that a candidate [e_1 | ... | e_8] is dotted with in the tail sweep: o(h, r^)."""
    return torch.cat(omult(h8, onorm(r8)), -1)


def head_query(r8, t8):
    """The adjoint: with a = h_1..4, b = h_5..8, c = r^_1..4, d = r^_5..8, T1 = t_1..4, T2 = t_5..8,
    [T1 (x) c* + d* (x) T2 | -d (x) T1 + T2 (x) c]."""
    rn = onorm(r8)
    c, d, T1, T2 = rn[:4], rn[4:], t8[:4], t8[4:]
    lo = [x + y for x, y in zip(qmult(T1, qstar(c)), qmult(qstar(d), T2))]
    hi = [y - x for x, y in zip(qmult(d, T1), qmult(T2, c))]
    return torch.cat(lo + hi, -1)


def params64(z, prefix="init."):
    return {k[len(prefix):-len(".weight")]: torch.tensor(z[k], dtype=torch.float64)
            for k in z.files if k.startswith(prefix) and k.endswith(".weight")}


def build(name, seed=None):
    import pykg2vec_amd as pa
    z = load(name)
    hp = {k[3:]: z[k].item() for k in z.files if k.startswith("hp_")}
    if seed is not None:
        torch.manual_seed(seed)
    return z, pa.import_model("octonione")(tot_entity=int(z["E"]), tot_relation=int(z["R"]), **hp)


# ---------------------------------------------------------------- registration
def test_importer_keys_and_model_id():
    import pykg2vec_amd as pa
    from pykg2vec_amd import _lib, integration, kernels, pointwise
    assert pa.import_model("octonione") is pointwise.OctonionE
    assert pa.MODEL_MAP["octonione"] == "pointwise.OctonionE"
    assert kernels.MODEL_IDS["octonione"] == _lib.OCTONIONE == 20
    assert "OctonionE" in integration.POINTWISE
    assert kernels._TABLE_SHAPES["octonione"] == [("E", "d")] * 8 + [("R", "d")] * 8 + [("R", "d")]


def test_header_enum_matches_lib():
    from pykg2vec_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "kge_hip.h")) as f:
        src = f.read()
    body = re.search(r"enum kge_model \{(.*?)\};", src, re.S).group(1)
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"KGE_(\w+)\s*=\s*(\d+)", body)}
    assert enum["OCTONIONE"] == 20 and len(enum) == 21
    for name, value in enum.items():
        assert getattr(_lib, name) == value, name
    assert re.search(r"#define KGE_ABI_VERSION 3\b", src) and re.search(r"#define KGE_MAX_TABLES 12\b", src)
    assert _lib.ABI_VERSION == 3 and _lib.KGE_MAX_TABLES == 12


# ---------------------------------------------------------------- constructor parity
@pytest.mark.parametrize("name", NAMES)
def test_state_dict_names_shapes_and_order(name):
    z, m = build(name)
    init = [k[len("init."):] for k in z.files if k.startswith("init.")]
    sd = m.state_dict()
    assert list(sd) == init
    for k in init:
        assert tuple(sd[k].shape) == z["init." + k].shape, k
    assert [e.name for e in m.parameter_list] == ENT + REL + ["rel_w_embedding"]
    assert m.loss.__name__ == "pointwise_logistic" and m.model_name == "octonione"


@pytest.mark.parametrize("name", NAMES)
def test_initial_state_equals_reference_under_seed(name):
    z, m = build(name, SEEDS[name])
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), z["init." + k]), k


def test_tables_sit_in_component_blocks():
    _, m = build("octonione")
    for group in (m.parameter_list[0:8], m.parameter_list[8:16]):
        w = [e.weight for e in group]
        stride = (w[0].numel() + 3) // 4 * 4
        assert all(x.data_ptr() == w[0].data_ptr() + 4 * c * stride for c, x in enumerate(w))


# ---------------------------------------------------------------- regulariser and forward restatement
@pytest.mark.parametrize("reg_type,p", [("F2", 2), ("N3", 3), ("n3", 3)])
def test_get_reg_matches_float64(reg_type, p):
    z, m = build("octonione", SEEDS["octonione"])   # the reference's initial tables
    rng = np.random.default_rng(5)
    h, r, t = (torch.as_tensor(rng.integers(n, size=40)) for n in (int(z["E"]), int(z["R"]), int(z["E"])))
    P = params64(z)
    got = m.get_reg(h, r, t, reg_type).item()
    assert np.isclose(got, m.lmbda * reg64(P, h, r, t, p).item(), rtol=1e-5)
    assert np.isclose(m.get_reg(h, r, t).item(), m.lmbda * reg64(P, h, r, t, 3).item(), rtol=1e-5)   # default 'N3'
    with pytest.raises(NotImplementedError):
        m.get_reg(h, r, t, "L1")
    from pykg2vec_amd import _lib
    assert m.kernel_reg_type() == _lib.REG_N3_ABS and m.kernel_reg_type("F2") == _lib.REG_F2
    assert m.kernel_lmbda() == m.lmbda / m.hidden_size


@pytest.mark.parametrize("name", NAMES)
def test_float64_forward_matches_reference_scores(name):
    z = load(name)
    P = params64(z)
    h, r, t = (torch.as_tensor(z["batch0.%d" % i]) for i in range(3))
    got = energy64(P, h, r, t).numpy()
    assert np.allclose(got, z["scores0"], atol=2e-6, rtol=1e-5), np.abs(got - z["scores0"]).max()


@pytest.mark.parametrize("name", NAMES)
def test_float64_loss_and_grads_match_reference(name):
    z = load(name)
    P = {k: v.requires_grad_(True) for k, v in params64(z).items()}
    b = [torch.as_tensor(z["batch0.%d" % i]) for i in range(4)]
    loss = pointwise_loss64(P, *b[:3], b[3].double(), float(z["hp_lmbda"]))
    loss.backward()
    assert np.isclose(loss.item(), float(z["loss0"]), rtol=1e-5)
    for k in ENT + REL:
        ref = z["grad0.%s.weight" % k]
        assert np.allclose(P[k].grad.numpy(), ref, atol=1e-6, rtol=1e-4), (k, np.abs(P[k].grad.numpy() - ref).max())
    assert "grad0.rel_w_embedding.weight" not in z.files   # the reference leaves rel_w's .grad None


def test_rank_queries_match_float64_autograd():
    rng = np.random.default_rng(9)
    d = 11
    h8 = [torch.tensor(rng.normal(size=d), requires_grad=True) for _ in range(8)]
    r8 = [torch.tensor(rng.normal(size=d)) for _ in range(8)]
    t8 = [torch.tensor(rng.normal(size=d), requires_grad=True) for _ in range(8)]
    S = sum(oc * tc for oc, tc in zip(omult(h8, onorm(r8)), t8)).sum()
    S.backward()
    dh = torch.cat([x.grad for x in h8])
    dt = torch.cat([x.grad for x in t8])
    assert torch.allclose(head_query(r8, [x.detach() for x in t8]), dh, atol=1e-13)
    assert torch.allclose(tail_query([x.detach() for x in h8], r8), dt, atol=1e-13)
    # the sweeps: energy(e) = -(query . [e_1 | ... | e_8])
    cand = torch.cat([x.detach() for x in t8])
    assert torch.isclose(-(tail_query([x.detach() for x in h8], r8) * cand).sum(), -S.detach())
    cand = torch.cat([x.detach() for x in h8])
    assert torch.isclose(-(head_query(r8, [x.detach() for x in t8]) * cand).sum(), -S.detach())
