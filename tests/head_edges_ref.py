"""Float64 reference, a-priori error bounds, dispatch plan and case list for tests/test_hip_head_edges.py (numpy only, no GPU).

The 1-N head (pykg2vec_amd/csrc/kge_head.hip) computes preds = sigmoid(x @ ent.T + bias), the fused multi_class_bce loss of the
predictions, and the three backward products dX = dZ Ent, g_ent += dZ^T X, g_bias += column sums of dZ.

Inputs (inputs()): every element of x and dpreds has a magnitude uniform in [0.5, 1] and a random sign; ent the same over sqrt(d),
bias the same times 0.1; labels multi-hot.  |logit| stays below about 2.5, so p (1 - p) never vanishes and no term of any sum is
small against the sum: one dropped or doubled term moves an output by many times its bound (min_term / sensitivity).

Bounds, elementwise, u = 2^-24 (the build is -ffp-contract=off without fast-math, csrc/Makefile; sigmoidf_ is expf, one add and a
correctly rounded divide).  Fixed here before any GPU run; nothing below is fitted to a kernel's results:
    logit       dz_b = (d + 1) u (|x| |ent|^T + |bias|)                     one rounding per step of the k chain and the bias add
    prediction  dp_b = p (1 - p) dz_b + c 2^-23 p                          c = 4 (expf, add, divide); c = 8 for sigmoid_fast (bf16 forms)
    autograd    dX    <= (1.25 E + 8) u (|dz| |ent|)                        dz = dpreds p (1 - p) from the given fp32 preds: three roundings,
                g_ent <= (1.25 B + 8) u (|dz|^T |x| + |prefill|)            a k chain of K roundings, at most K / 16 partial sums to combine
                g_bias<= (1.25 B + 8) u (sum_b |dz| + |prefill|)            (KGE_HEAD_MINK=16) and the add into the prefilled output
    fused       the kernel forms dz from its own p with __expf / __logf / rcp:
                ddz = (8 2^-23 (|t1| + |t2|) + (1.07 + dy |1 - 2 p|) dp_b) / (B E)
                with t1 = (sigmoid(p) - y0) p (1 - p), and for a positive label t2 = dy p (1 - p), dy = y1 - y0 (k_head_bce_pos subtracts
                t2 from the stored t1 with a p of its own k chain; a negative has t2 = 0, which leaves 8 2^-23 |dz| + 1.07 dp_b / (B E));
                outputs: the autograd bounds plus ddz |ent|, ddz^T |x|, sum_b ddz
    loss        rtol 2e-5 (tests/test_hip_parity.py, the same entry point)

plan() restates the host dispatcher from the sources (line numbers cited at each rule).  It is used only to assert that the case
list reaches every kernel, epilogue and split edge; it is never an oracle for values."""
import collections
import functools
import zlib

import numpy as np

import kge_oracle as ko

U = 2.0 ** -24
U23 = 2.0 ** -23
LOSS_RTOL = 2e-5          # tests/test_hip_parity.py::test_head_1n_vs_oracle_other_shapes
SENSITIVITY = 8.0         # smallest single term of an output element >= 8 x that element's bound
SWITCHES = ("KGE_HEAD_TILE", "KGE_HEAD_SMALL_X", "KGE_HEAD_XCD", "KGE_HEAD_WIDE_B", "KGE_HEAD_MINK")

# ---- constants of csrc/kge_head.hip, copied from the source (never from a kernel's results)
HT, HK = 64, 32           # :30-31   64 x 64 tile, 32-wide K slab: k_head_gemm, k_head_gemm_bf16, k_head_dx, k_head_dent
HT2, HK2 = 128, 16        # :149     128 x 128 tile, 16-wide K slab: k_head_gemm128x, k_head_dx128, k_head_dent128
HK4 = 32                  # :329     K slab of k_head_gemm64x
HKB = 32                  # :517     K slab of k_head_gemm128_bf16
PART_SLOTS = 768          # :754     kHeadPartSlots
DIRECT, PARTS, ATOMIC = "kOutDirect", "kOutParts", "kOutAtomic"    # :753


def _switch(env, name):
    """switch_value (csrc/kge_debug.hip:20-28): -1 when unset or empty, else atoi."""
    v = (env or {}).get("KGE_" + name, "")
    return int(v) if v != "" else -1


def _cdiv(a, b):
    return -(-a // b)


def _use_128(B, E, d, aligned, env):
    """head_use_128 (csrc/kge_head.hip:588-593)."""
    force = _switch(env, "HEAD_TILE")
    if force >= 0:
        return force == 1 and d % 4 == 0
    return d % 4 == 0 and aligned and _cdiv(E, HT2) * _cdiv(B, HT2) >= 200


def _backward_product(wide, fused, have_ws, tiles, K, env, name):
    """The split lambda and the epilogue choice of head_backward_gemms (csrc/kge_head.hip:983-990, :996, :1011) and
    launch_head_sum_parts (:924-932: L = 8 from 16 splits on)."""
    SK = HK2 if wide else HK
    min_k = _switch(env, "HEAD_MINK") if _switch(env, "HEAD_MINK") > 0 else 128
    splits = PART_SLOTS // tiles if wide else _cdiv(2048, tiles)
    splits = max(1, min(splits, _cdiv(K, min_k) if wide else _cdiv(K, SK)))
    per = _cdiv(_cdiv(K, splits), SK) * SK
    splits = _cdiv(K, per)
    emode = ATOMIC if not wide else (DIRECT if splits == 1 else (PARTS if have_ws else ATOMIC))
    kernel = "%s128<%s>" % (name, "true" if fused else "false") if wide else name
    return dict(kernel=kernel, tile=HT2 if wide else HT, slab=SK, splits=splits, per=per, last=K - (splits - 1) * per, emode=emode,
                L=(8 if splits >= 16 else 1) if emode == PARTS else None, nslab_last=_cdiv(K - (splits - 1) * per, SK))


def plan(B, E, d, aligned=True, have_ws=True, fused=True, env=None):
    """What the host code launches for a head of this shape.  aligned: every operand pointer is 16-byte aligned; have_ws: the
    backward owns a partials workspace (always so in the fused form); fused: kge_head_1n_bce (MODE 1, dz workspace) as opposed to
    kge_head_1n_forward / kge_head_1n_backward (MODE 0, autograd form); env: the KGE_HEAD_* switches."""
    mode = 1 if fused else 0
    have_ws = have_ws or fused                      # launch_head_bce always passes its parts (:1068-1069)
    # launch_head_gemm (:595-604)
    if _use_128(B, E, d, aligned, env):
        fwd = dict(kernel="k_head_gemm128x<%d>" % mode, tile=HT2, slab=HK2)
    elif d % 4 == 0 and aligned and _switch(env, "HEAD_SMALL_X") != 0:
        fwd = dict(kernel="k_head_gemm64x<%d>" % mode, tile=HT, slab=HK4)
    else:
        fwd = dict(kernel="k_head_gemm<%d>" % mode, tile=HT, slab=HK)
    # launch_head_forward, bf16 (:953-959)
    bf = dict(kernel="k_head_gemm128_bf16", tile=HT2, slab=HKB) if _use_128(B, E, d, aligned, env) else \
        dict(kernel="k_head_gemm_bf16", tile=HT, slab=HK)
    for f in (fwd, bf):
        f["nslab"] = _cdiv(d, f["slab"])
        f["T"] = _cdiv(E, f["tile"]) * _cdiv(B, f["tile"])           # head_grid (:584)
        f["xcd_runs"] = _switch(env, "HEAD_XCD") != 0                # :951, :1057
    # head_backward_gemms (:968-1019)
    force = _switch(env, "HEAD_TILE")
    min_b = _switch(env, "HEAD_WIDE_B") if _switch(env, "HEAD_WIDE_B") > 0 else (1 if have_ws else 2560)          # :975
    wide = (d % 4 == 0 and aligned) and (fused or B * E >= 4) and (force == 1 if force >= 0 else B >= min_b)    # :972, :977
    T = HT2 if wide else HT
    dx = _backward_product(wide, fused, have_ws, _cdiv(B, T) * _cdiv(d, T), E, env, "k_head_dx")
    dent = _backward_product(wide, fused, have_ws, _cdiv(E, T) * _cdiv(d, T), B, env, "k_head_dent")
    return dict(forward=fwd, forward_bf16=bf, dx=dx, dent=dent)


# --------------------------------------------------------------------------------------------------------------- inputs
def _signed(rng, shape):
    return rng.uniform(0.5, 1.0, size=shape) * rng.choice((-1.0, 1.0), size=shape)


LABEL_KINDS = ("random", "none", "empty_full", "corners", "all")


def make_labels(rng, B, E, kind):
    lab = np.zeros((B, E), np.float32)
    if kind == "random":
        lab = (rng.random((B, E)) < 0.05).astype(np.float32)
        lab[rng.integers(B), rng.integers(E)] = 1.0
    elif kind == "empty_full":          # a row without positives next to a row of E positives
        lab = (rng.random((B, E)) < 0.05).astype(np.float32)
        lab[0] = 0.0
        lab[min(1, B - 1)] = 1.0
    elif kind == "corners":
        for b in (0, B - 1):
            lab[b, 0] = lab[b, E - 1] = 1.0
    elif kind == "all":
        lab[:] = 1.0
    else:
        assert kind == "none", kind
    return lab


def csr_of(labels):
    """(int64 offsets [B + 1], int32 ids) of the positive columns of a multi-hot [B, E] array."""
    off = np.zeros(labels.shape[0] + 1, np.int64)
    off[1:] = np.cumsum((labels > 0).sum(1))
    ids = np.flatnonzero(labels.reshape(-1) > 0) % labels.shape[1]
    return off, ids.astype(np.int32)


Inputs = collections.namedtuple("Inputs", "x ent bias dpreds labels")


@functools.lru_cache(maxsize=None)
def inputs(B, E, d, labels="random", seed=0):
    rng = np.random.default_rng([seed, B, E, d, zlib.crc32(labels.encode())])
    x = _signed(rng, (B, d)).astype(np.float32)
    ent = (_signed(rng, (E, d)) / np.sqrt(d)).astype(np.float32)
    bias = (_signed(rng, E) * 0.1).astype(np.float32)
    dpreds = _signed(rng, (B, E)).astype(np.float32)
    out = Inputs(x, ent, bias, dpreds, make_labels(rng, B, E, labels))
    for a in out:
        a.setflags(write=False)
    return out


def smoothing(ls, E):
    """(y0, y1) as launch_head_bce forms them in fp32 (csrc/kge_head.hip:1053-1055): ls None -> 0 / 1."""
    if ls is None:
        return 0.0, 1.0
    y0 = np.float32(1.0) / np.float32(E)
    return float(y0), float((np.float32(1.0) - np.float32(ls)) + y0)


# --------------------------------------------------------------------------------------------------------------- float64 reference and bounds
def f64(a):
    return np.asarray(a, np.float64)


def forward64(x, ent, bias):
    z = f64(x) @ f64(ent).T
    if bias is not None:
        z = z + f64(bias)[None, :]
    return z, ko.head_1n_forward(x, ent, bias, dtype=np.float64)


def forward_bounds(x, ent, bias, p, c=4):
    """(logit bound, prediction bound), elementwise."""
    d = x.shape[1]
    mag = np.abs(f64(x)) @ np.abs(f64(ent)).T
    if bias is not None:
        mag = mag + np.abs(f64(bias))[None, :]
    dz_b = (d + 1) * U * mag
    return dz_b, p * (1 - p) * dz_b + c * U23 * p


def min_term(a, b):
    """min over k of |a[m, k] b[k, n]|: the smallest single term of every element of a @ b."""
    a, b = np.abs(f64(a)), np.abs(f64(b))
    out = np.full((a.shape[0], b.shape[1]), np.inf)
    step = max(1, (1 << 22) // max(1, a.shape[0] * b.shape[1]))
    for k in range(0, a.shape[1], step):
        out = np.minimum(out, (a[:, k:k + step, None] * b[None, k:k + step, :]).min(1))
    return out


Result = collections.namedtuple("Result", "ref bound term")     # dicts keyed by output name


def forward_case(x, ent, bias, bf16=False):
    """Reference, bound and smallest-term effect of the predictions.  bf16: the reference on bf16-rounded operands, c = 8."""
    if bf16:
        x, ent = ko.bf16_round(x), ko.bf16_round(ent)
    z, p = forward64(x, ent, bias)
    dz_b, dp_b = forward_bounds(x, ent, bias, p, 8 if bf16 else 4)
    t = min_term(x, f64(ent).T)
    if bias is not None:
        t = np.minimum(t, np.abs(f64(bias))[None, :])
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    moved = np.minimum(np.abs(sig(z + t) - p), np.abs(sig(z - t) - p))     # what dropping the smallest logit term does to p
    return Result(dict(preds=p, logit=z), dict(preds=dp_b, logit=dz_b), dict(preds=moved, logit=t))


def _products(dz, ddz, x, ent, pre_ent=None, pre_bias=None):
    """The three backward products of dz in float64 with their bounds; ddz: elementwise error already in dz (fused form) or None."""
    B, E = dz.shape
    x, ent, adz = f64(x), f64(ent), np.abs(dz)
    ref = dict(dx=dz @ ent, g_ent=dz.T @ x, g_bias=dz.sum(0))
    mag = dict(dx=adz @ np.abs(ent), g_ent=adz.T @ np.abs(x), g_bias=adz.sum(0))
    term = dict(dx=min_term(dz, ent), g_ent=min_term(dz.T, x), g_bias=adz.min(0))
    for name, pre in (("g_ent", pre_ent), ("g_bias", pre_bias)):
        if pre is not None:
            ref[name] = ref[name] + f64(pre)
            mag[name] = mag[name] + np.abs(f64(pre))
            term[name] = np.minimum(term[name], np.abs(f64(pre)))
    bound = dict(dx=(1.25 * E + 8) * U * mag["dx"], g_ent=(1.25 * B + 8) * U * mag["g_ent"], g_bias=(1.25 * B + 8) * U * mag["g_bias"])
    if ddz is not None:
        bound["dx"] = bound["dx"] + ddz @ np.abs(ent)
        bound["g_ent"] = bound["g_ent"] + ddz.T @ np.abs(x)
        bound["g_bias"] = bound["g_bias"] + ddz.sum(0)
    return Result(ref, bound, term)


def given_preds(x, ent, bias):
    """The fp32 predictions handed to the autograd-form backward: the float64 reference's, rounded once."""
    return forward64(x, ent, bias)[1].astype(np.float32)


def autograd_case(x, ent, preds, dpreds, pre_ent=None, pre_bias=None):
    p = f64(preds)
    return _products(f64(dpreds) * p * (1 - p), None, x, ent, pre_ent, pre_bias)


def fused_case(x, ent, bias, labels, ls, pre_ent=None, pre_bias=None, pre_loss=0.0, pre_loss_abs=0.0):
    """kge_head_1n_bce: loss (+ prefill), dX, g_ent, g_bias of one direction."""
    B, E = labels.shape
    _z, p = forward64(x, ent, bias)
    _dz_b, dp_b = forward_bounds(x, ent, bias, p, 4)
    y0, y1 = smoothing(ls, E)
    pos = labels > 0
    y = np.where(pos, y1, y0)
    sg = 1.0 / (1.0 + np.exp(-p))
    loss = float((p + np.log1p(np.exp(-p)) - p * y).sum() / (B * E))
    dz = (sg - y) * p * (1 - p) / (B * E)
    t1 = np.abs((sg - y0) * p * (1 - p))
    t2 = np.where(pos, (y1 - y0) * p * (1 - p), 0.0)
    ddz = (8 * U23 * (t1 + t2) + (1.07 + np.where(pos, (y1 - y0) * np.abs(1 - 2 * p), 0.0)) * dp_b) / (B * E)
    r = _products(dz, ddz, x, ent, pre_ent, pre_bias)
    r.ref["loss"] = loss + pre_loss
    r.bound["loss"] = LOSS_RTOL * (abs(loss) + pre_loss_abs)
    return r


# --------------------------------------------------------------------------------------------------------------- fp32 numpy restatement
def f32_forward(x, ent, bias):
    z = x @ ent.T
    if bias is not None:
        z = z + bias[None, :]
    return (np.float32(1) / (np.float32(1) + np.exp(-z))).astype(np.float32)


def f32_products(dz, x, ent, pre_ent=None, pre_bias=None):
    ge, gb = dz.T @ x, dz.sum(0, dtype=np.float32)
    return dict(dx=dz @ ent, g_ent=ge if pre_ent is None else pre_ent + ge, g_bias=gb if pre_bias is None else pre_bias + gb)


def f32_autograd(x, ent, preds, dpreds, pre_ent=None, pre_bias=None):
    return f32_products(dpreds * preds * (np.float32(1) - preds), x, ent, pre_ent, pre_bias)


def f32_fused(x, ent, bias, labels, ls, pre_ent=None, pre_bias=None):
    """bce_neg_terms / k_head_bce_pos in fp32 numpy: every element as a negative, positives corrected afterwards."""
    B, E = labels.shape
    one = np.float32(1)
    p = f32_forward(x, ent, bias)
    y0, y1 = (np.float32(v) for v in smoothing(ls, E))
    inv = one / (np.float32(B) * np.float32(E))
    u = one + np.exp(-p)
    dz = ((one / u - y0) * p * (one - p)) * inv
    pos = labels > 0
    dz = np.where(pos, dz - (y1 - y0) * p * (one - p) * inv, dz).astype(np.float32)
    lt = p + np.log(u) - p * y0
    loss = np.float32((lt * inv).sum(dtype=np.float32) - (np.where(pos, p, 0) * (y1 - y0) * inv).sum(dtype=np.float32))
    out = f32_products(dz, x, ent, pre_ent, pre_bias)
    out["loss"] = float(loss)
    return out


def worst_ratio(got, res, names=None):
    """{output: max |got - ref| / bound}."""
    out = {}
    for name in (names or got.keys()):
        if got.get(name) is None or name not in res.ref:
            continue
        err = np.abs(f64(got[name]) - res.ref[name])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / res.bound[name])
        out[name] = float(np.max(r)) if np.all(np.isfinite(f64(got[name]))) else float("inf")
    return out


# --------------------------------------------------------------------------------------------------------------- the cases
BASE = (65, 131, 36)          # ragged against both tiles, d % 4 == 0
BASE_ODD = (65, 131, 35)      # its d % 4 != 0 twin

# what serves a forward of a given d: (name, env, bf16)
FWD_WAYS = (("gemm64x", {}, False), ("gemm", {"KGE_HEAD_SMALL_X": "0"}, False), ("gemm128x", {"KGE_HEAD_TILE": "1"}, False),
            ("bf16_64", {}, True), ("bf16_128", {"KGE_HEAD_TILE": "1"}, True))
FWD_WAYS_ODD = (("gemm", {}, False), ("bf16_64", {}, True))


def fwd_ways(d):
    return FWD_WAYS if d % 4 == 0 else FWD_WAYS_ODD


F_D = sorted({1, 2, 3, 5, 31, 33, 63, 65, 95, 97, 129} | {32, 64, 96, 128, 132}                       # k_head_gemm (HK = 32)
             | {4, 12, 16, 20, 28, 32, 36, 60, 64, 68, 92, 96, 100, 128, 132}                        # k_head_gemm64x (HK4 = 32)
             | {4, 12, 16, 20, 28, 32, 36, 44, 48, 52, 64, 68}                                       # k_head_gemm128x (HK2 = 16)
             | {1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65}                                      # k_head_gemm_bf16 (HK = 32)
             | {4, 8, 12, 16, 20, 28, 32, 36, 60, 64, 68})                                           # k_head_gemm128_bf16 (HKB = 32)
F_EDGE = sorted({1, 31, 32, 33, 63, 64, 65} | {1, 63, 64, 65, 127, 128, 129, 130, 131, 132})           # B and E, both tiles
F_SHAPES = ([(BASE[0], BASE[1], d) for d in F_D]
            + [(b, BASE[1], d) for b in F_EDGE for d in (36, 35) if b != BASE[0]]
            + [(BASE[0], e, d) for e in F_EDGE for d in (36, 35) if e != BASE[1]])

X_SHAPES = [(65, (n - 1) * tile + 3, 36, tile) for tile in (HT, HT2) for n in range(1, 10)]            # T = 2 n (64) and n (128)
X_WAYS = {HT: (("gemm64x", {}, False), ("gemm", {"KGE_HEAD_SMALL_X": "0"}, False), ("bf16_64", {}, True)),
          HT2: (("gemm128x", {"KGE_HEAD_TILE": "1"}, False), ("bf16_128", {"KGE_HEAD_TILE": "1"}, True))}

L_LS = (None, 0.0, 0.1)
L_WAYS = ((BASE, {}), (BASE, {"KGE_HEAD_SMALL_X": "0"}), (BASE, {"KGE_HEAD_TILE": "1"}), (BASE_ODD, {}))
L_CASES = [(shape, env, kind, ls) for shape, env in L_WAYS for kind in ("none", "empty_full", "corners") for ls in L_LS] \
    + [((129, 257, d), env, "all", ls) for d, env in ((36, {}), (132, {"KGE_HEAD_TILE": "1"}), (35, {})) for ls in L_LS]

BK_ENVS = ({"KGE_HEAD_TILE": "0"}, {"KGE_HEAD_TILE": "1"}, {"KGE_HEAD_WIDE_B": "1"})
BK_SMALL = [(1, 1, 4), (1, 3, 4), (3, 1, 4), (1, 4, 4), (2, 2, 4)]           # around the B E >= 4 rule of the autograd form
BK_SHAPES = ([(BASE[0], e, BASE[2]) for e in (125, 126, 127, 128, 129, 130, 131, 132, 255, 256, 257, 258)]
             + [(b, BASE[1], BASE[2]) for b in (1, 63, 64, 127, 128, 129, 256)]      # 256: two full splits of g_ent
             + [(BASE[0], BASE[1], d) for d in (4, 124, 128, 132, 3, 33)] + BK_SMALL)
# (form, workspace, need_bias): the autograd entry point four ways, and the fused one
BK_FORMS = (("bwd", True, True), ("bwd", True, False), ("bwd", False, True), ("bwd", False, False), ("bce", True, True))

S_ENV = {"KGE_HEAD_TILE": "1", "KGE_HEAD_MINK": "16"}
S_K = (15, 16, 17, 31, 32, 33, 239, 240, 241, 255, 256, 257, 271, 272, 273)
S_K_SMALL = (31, 32, 33, 63, 64, 65)
S_OTHER = ((65, 4), (129, 132))
# (B, E, d, env): K = E splits dX, K = B splits g_ent
S_CASES = ([(o, k, d, S_ENV) for k in S_K for o, d in S_OTHER] + [(k, o, d, S_ENV) for k in S_K for o, d in S_OTHER]
           + [(65, k, 36, {"KGE_HEAD_TILE": "0"}) for k in S_K_SMALL] + [(k, 65, 36, {"KGE_HEAD_TILE": "0"}) for k in S_K_SMALL])
S_FORMS = (("bce", True, True), ("bwd", True, True), ("bwd", False, True))

# accumulate / overwrite: (B, E, d, env) -> the epilogue of (dX, g_ent), as plan() must confirm
A_CASES = [((65, 125, 36), {}, (DIRECT, DIRECT)), ((129, 131, 36), {}, (PARTS, PARTS)), ((65, 131, 36), {"KGE_HEAD_TILE": "0"}, (ATOMIC, ATOMIC)),
           ((65, 131, 35), {}, (ATOMIC, ATOMIC))]

M_SHAPES = [BASE, (129, 257, 132), (64, 128, 4)]

D_FWD = [(129, 12672, 4), (129, 12673, 4)]         # 198 and 200 wide tiles (head_use_128: tiles >= 200)
D_BWD = [(2559, 5, 4), (2560, 5, 4)]               # workspace-free: wide from B >= 2560


PlanCase = collections.namedtuple("PlanCase", "set B E d aligned have_ws fused env")


def plan_cases():
    """Every (shape, alignment, workspace, form, switches) the GPU tests run, for the reach test."""
    out = []
    for B, E, d in F_SHAPES:
        for _n, env, _bf in fwd_ways(d):
            out.append(PlanCase("F", B, E, d, True, True, False, env))
    for B, E, d, tile in X_SHAPES:
        for _n, env, _bf in X_WAYS[tile]:
            for xcd in ({}, {"KGE_HEAD_XCD": "0"}):
                for fused in (False, True):
                    out.append(PlanCase("X", B, E, d, True, True, fused, dict(env, **xcd)))
    for (B, E, d), env, _kind, _ls in L_CASES:
        out.append(PlanCase("L", B, E, d, True, True, True, env))
    for B, E, d in BK_SHAPES:
        for env in BK_ENVS:
            for form, ws, _nb in BK_FORMS:
                out.append(PlanCase("Bk", B, E, d, True, ws, form == "bce", env))
    for B, E, d, env in S_CASES:
        for form, ws, _nb in S_FORMS:
            out.append(PlanCase("S", B, E, d, True, ws, form == "bce", env))
    for (B, E, d), env, _emodes in A_CASES:
        out.append(PlanCase("A", B, E, d, True, True, True, env))
    for B, E, d in M_SHAPES:
        for fused in (False, True):
            out.append(PlanCase("M", B, E, d, False, True, fused, {}))
            out.append(PlanCase("M", B, E, d, True, True, fused, {}))
    for B, E, d in D_FWD:
        out.append(PlanCase("D", B, E, d, True, True, False, {}))
    for B, E, d in D_BWD:
        out.append(PlanCase("D", B, E, d, True, False, False, {}))
    return out


# --------------------------------------------------------------------------------------------------------------- shared, cached references
@functools.lru_cache(maxsize=None)
def fwd_result(B, E, d, with_bias, bf16):
    i = inputs(B, E, d)
    return forward_case(i.x, i.ent, i.bias if with_bias else None, bf16)


@functools.lru_cache(maxsize=None)
def auto_preds(B, E, d):
    i = inputs(B, E, d)
    return given_preds(i.x, i.ent, i.bias)


@functools.lru_cache(maxsize=None)
def auto_result(B, E, d):
    i = inputs(B, E, d)
    return autograd_case(i.x, i.ent, auto_preds(B, E, d), i.dpreds)


@functools.lru_cache(maxsize=None)
def fused_result(B, E, d, kind="random", ls=0.1):
    i = inputs(B, E, d, kind)
    return fused_case(i.x, i.ent, i.bias, i.labels, ls)


Prefill = collections.namedtuple("Prefill", "g_ent g_bias loss")
LOSS_FLOATS, LOSS_STRIDE = 32 * 32, 32        # pykg2vec_amd/_lib.py: LOSS_SLOTS x LOSS_STRIDE floats, the total is the sum of [k * 32]


@functools.lru_cache(maxsize=None)
def prefill(E, d):
    """Accumulator contents before the call, drawn like the inputs (g_ent like ent, g_bias like bias, the loss stripes like x)."""
    rng = np.random.default_rng([7, E, d])
    return Prefill((_signed(rng, (E, d)) / np.sqrt(d)).astype(np.float32), (_signed(rng, E) * 0.1).astype(np.float32),
                   _signed(rng, LOSS_FLOATS).astype(np.float32))


@functools.lru_cache(maxsize=None)
def accumulate_result(B, E, d, ls=0.1):
    """Two directions in a row into prefilled loss / g_ent / g_bias, as the models call the entry point: (inputs of direction 1,
    inputs of direction 2 -- its ent and bias are direction 1's --, result after 1, result after 2); bounds add up."""
    i1, i2 = inputs(B, E, d), inputs(B, E, d, seed=1)
    pre = prefill(E, d)
    stripes = f64(pre.loss)[::LOSS_STRIDE]
    r1 = fused_case(i1.x, i1.ent, i1.bias, i1.labels, ls, pre.g_ent, pre.g_bias, float(stripes.sum()), float(np.abs(stripes).sum()))
    r2 = fused_case(i2.x, i1.ent, i1.bias, i2.labels, ls, r1.ref["g_ent"], r1.ref["g_bias"], r1.ref["loss"], abs(r1.ref["loss"]))
    for name in ("g_ent", "g_bias", "loss"):
        r2.bound[name] = r2.bound[name] + r1.bound[name]
        # the term whose loss these cases are about is the prefill itself (a store in place of an add); the gradient's own terms are
        # held to their unprefilled bounds by the same shapes in sets L and Bk
        if name != "loss":
            r1.term[name] = np.abs(f64(getattr(pre, name)))
            r2.term[name] = np.abs(f64(getattr(pre, name)))
    return i1, i2, r1, r2


def f32_accumulate(B, E, d, ls=0.1):
    i1, i2 = inputs(B, E, d), inputs(B, E, d, seed=1)
    pre = prefill(E, d)
    o1 = f32_fused(i1.x, i1.ent, i1.bias, i1.labels, ls, pre.g_ent, pre.g_bias)
    o1["loss"] = float(np.float32(pre.loss[::LOSS_STRIDE].sum(dtype=np.float32) + np.float32(o1["loss"])))
    o2 = f32_fused(i2.x, i1.ent, i1.bias, i2.labels, ls, o1["g_ent"], o1["g_bias"])
    o2["loss"] = float(np.float32(np.float32(o1["loss"]) + np.float32(o2["loss"])))
    return o1, o2


def numeric_cases(which):
    """The distinct computations of a case set: ("fwd", B, E, d, with_bias, bf16) / ("auto", B, E, d) / ("fused", B, E, d, labels, ls) /
    ("acc", B, E, d)."""
    out = []
    if which == "F":
        out = [("fwd", B, E, d, wb, bf) for B, E, d in F_SHAPES for wb in (True, False) for bf in sorted({w[2] for w in fwd_ways(d)})]
    elif which == "X":
        out = [("fwd", B, E, d, True, bf) for B, E, d, _t in X_SHAPES for bf in (False, True)] + [("fused", B, E, d, "random", 0.1) for B, E, d, _t in X_SHAPES]
    elif which == "L":
        out = [("fused",) + tuple(shape) + (kind, ls) for shape, _env, kind, ls in L_CASES]
    elif which == "Bk":
        out = [(f, B, E, d) + extra for B, E, d in BK_SHAPES for f, extra in (("auto", ()), ("fused", ("random", 0.1)))]
    elif which == "S":
        out = [(f, B, E, d) + extra for B, E, d, _env in S_CASES for f, extra in (("auto", ()), ("fused", ("random", 0.1)))]
    elif which == "A":
        out = [("acc",) + tuple(shape) for shape, _env, _em in A_CASES]
    elif which == "M":
        out = [c for B, E, d in M_SHAPES for c in (("fwd", B, E, d, True, False), ("fwd", B, E, d, True, True), ("auto", B, E, d),
                                                  ("fused", B, E, d, "random", 0.1))]
    elif which == "D":
        out = [("fwd", B, E, d, True, False) for B, E, d in D_FWD] + [("auto", B, E, d) for B, E, d in D_BWD]
    return list(dict.fromkeys(out))


SETS = ("F", "X", "L", "Bk", "S", "A", "M", "D")


def survey(which):
    """On the CPU: the fp32 numpy restatement of every computation of a set against the float64 reference.  Returns (largest
    error / bound per output, smallest term / bound per output, [(case, output, term / bound)] below SENSITIVITY)."""
    worst, least, insensitive = {}, {}, []
    for c in numeric_cases(which):
        kind, (B, E, d) = c[0], c[1:4]
        pairs = []
        if kind == "fwd":
            i = inputs(B, E, d)
            x, ent = (ko.bf16_round(i.x), ko.bf16_round(i.ent)) if c[5] else (i.x, i.ent)
            pairs.append((dict(preds=f32_forward(x, ent, i.bias if c[4] else None)), fwd_result(*c[1:]), ("preds",)))
        elif kind == "auto":
            i = inputs(B, E, d)
            pairs.append((f32_autograd(i.x, i.ent, auto_preds(B, E, d), i.dpreds), auto_result(B, E, d), ("dx", "g_ent", "g_bias")))
        elif kind == "fused":
            i = inputs(B, E, d, c[4])
            pairs.append((f32_fused(i.x, i.ent, i.bias, i.labels, c[5]), fused_result(*c[1:]), ("loss", "dx", "g_ent", "g_bias")))
        else:
            _i1, _i2, r1, r2 = accumulate_result(B, E, d)
            o1, o2 = f32_accumulate(B, E, d)
            pairs += [(o1, r1, ("loss", "dx", "g_ent", "g_bias")), (o2, r2, ("loss", "dx", "g_ent", "g_bias"))]
        for got, res, names in pairs:
            for name, r in worst_ratio(got, res, names).items():
                worst[name] = max(worst.get(name, 0.0), r)
            for name in names:
                if name == "loss":
                    continue
                s = float(np.min(res.term[name] / res.bound[name]))
                least[name] = min(least.get(name, np.inf), s)
                if s < SENSITIVITY:
                    insensitive.append((c, name, s))
    return worst, least, insensitive
