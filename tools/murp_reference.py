"""MuRP restated in numpy from the formulas: forward, hand-derived backward, BCE-with-logits, the Riemannian
SGD step and both contracted rank sweeps, with the float type as an argument (np.float64, or np.longdouble as the tests' yardstick).

This is the blueprint of csrc/kge_murp.hip -- the same steps under the same names -- and it is checked against the live reference's
recorded outputs (tests/golden/ref_murp*.npz, tests/test_murp_model.py).  The maps are the reference's, quirks included:
arsech(x) = log((1 + sqrt(1 - x^2)) / x) where a Poincare model would use artanh, and 1 / cosh where it would use tanh.

Gradient conventions are autograd's: `where` passes the gradient of the chosen branch only, `clamp` passes it on the closed interval,
the 2-norm has gradient 0 at 0, lookups through the two embeddings give row 0 nothing (padding_idx = 0).
"""
import numpy as np

BALL = 1e-5      # the ball's margin: clamps at 1 - BALL, clips divide by |x| - BALL
TINY = 1e-10


def arsech(x):
    return np.log((1 + np.sqrt(1 - x * x)) / x)


def d_arsech(x):
    return -1 / (x * np.sqrt(1 - x * x))


def _dot(a, b):
    return np.sum(a * b, -1, keepdims=True)


def clip_fwd(x):
    """x / (|x| - 1e-5) where |x| >= 1.  Returns (clipped, norm, mask)."""
    dt = x.dtype.type
    n = np.sqrt(_dot(x, x))
    m = n >= 1
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(m, x / (n - dt(BALL)), x)
    return out, n, m


def clip_bwd(x, n, m, g):
    dt = x.dtype.type
    d = n - dt(BALL)
    with np.errstate(divide="ignore", invalid="ignore"):
        gc = g / d - (_dot(g, x) / (d * d * n)) * x
    return np.where(m, gc, g)


def psum_fwd(x, y):
    dt = x.dtype.type
    hi = dt(1) - dt(BALL)
    sxr, syr, dxy = _dot(x, x), _dot(y, y), _dot(x, y)
    sx, sy = np.clip(sxr, dt(0), hi), np.clip(syr, dt(0), hi)
    A = 1 + 2 * dxy + sy
    B = 1 - sx
    den = 1 + 2 * dxy + sx * sy
    out = (A * x + B * y) / den
    return out, (sxr, syr, sx, sy, A, B, den)


def psum_bwd(x, y, out, saved, g):
    dt = x.dtype.type
    hi = dt(1) - dt(BALL)
    sxr, syr, sx, sy, A, B, den = saved
    g_den = -_dot(g, out) / den
    gA = _dot(g, x) / den
    gB = _dot(g, y) / den
    g_dxy = 2 * gA + 2 * g_den
    g_sy = np.where((syr >= 0) & (syr <= hi), gA + g_den * sx, dt(0))
    g_sx = np.where((sxr >= 0) & (sxr <= hi), -gB + g_den * sy, dt(0))
    gx = (A / den) * g + g_dxy * y + 2 * g_sx * x
    gy = (B / den) * g + g_dxy * x + 2 * g_sy * y
    return gx, gy


def forward(tabs, h, r, t, dtype=np.float64, keep=False):
    """tabs: wu, bs, bo, ent, rel (state-dict order).  preds [n]; keep: also what the backward reads."""
    dt = dtype
    wu, bs, bo, ent, rel = (np.asarray(a, dtype=dt) for a in tabs)
    lo, hi = dt(TINY), dt(1) - dt(BALL)
    eh, et, er, w = ent[h], ent[t], rel[r], wu[r]
    hc, nh, mh = clip_fwd(eh)
    tc, nt, mt = clip_fwd(et)
    rc, nr, mr = clip_fwd(er)
    nh1 = np.sqrt(_dot(hc, hc))
    c = np.clip(nh1, lo, hi)
    ac = arsech(c)
    ue = ac * hc / c
    uw = ue * w
    nwr = np.sqrt(_dot(uw, uw))
    nw = np.maximum(nwr, lo)
    ich = 1 / np.cosh(nw)
    um = ich * uw / nw
    vm, ps1 = psum_fwd(tc, rc)
    umc, num, mu = clip_fwd(um)
    vmc, nvm, mv = clip_fwd(vm)
    z, ps2 = psum_fwd(-umc, vmc)
    nz = np.sqrt(np.sum(z * z, -1))
    cz = np.clip(nz, lo, hi)
    az = arsech(cz)
    sq = (2 * az) ** 2
    preds = -(sq - bs[h] - bo[t])
    if not keep:
        return preds
    return preds, dict(eh=eh, et=et, er=er, w=w, hc=hc, nh=nh, mh=mh, tc=tc, nt=nt, mt=mt, rc=rc, nr=nr, mr=mr, nh1=nh1, c=c, ac=ac,
                       ue=ue, uw=uw, nwr=nwr, nw=nw, ich=ich, um=um, vm=vm, ps1=ps1, umc=umc, num=num, mu=mu, vmc=vmc, nvm=nvm, mv=mv,
                       z=z, ps2=ps2, nz=nz, cz=cz, az=az)


def backward(tabs, h, r, t, dscore, dtype=np.float64):
    """The five dense gradients of sum_i dscore[i] * preds_i, in state-dict order."""
    dt = dtype
    wu, bs, bo, ent, rel = (np.asarray(a, dtype=dt) for a in tabs)
    lo, hi = dt(TINY), dt(1) - dt(BALL)
    _, s = forward(tabs, h, r, t, dt, keep=True)
    gs = np.asarray(dscore, dtype=dt)
    g_wu, g_bs, g_bo, g_ent, g_rel = (np.zeros_like(a) for a in (wu, bs, bo, ent, rel))
    np.add.at(g_bs, h, gs)
    np.add.at(g_bo, t, gs)
    # score = -(sq - bs - bo), sq = (2 arsech(cz))^2
    g_cz = -gs * 8 * s["az"] * d_arsech(s["cz"])
    g_nz = np.where((s["nz"] >= lo) & (s["nz"] <= hi), g_cz, dt(0))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        g_z = np.where(s["nz"][:, None] > 0, g_nz * s["z"] / s["nz"][:, None], dt(0))
    g_x, g_vmc = psum_bwd(-s["umc"], s["vmc"], s["z"], s["ps2"], g_z)
    g_umc = -g_x
    g_um = clip_bwd(s["um"], s["num"], s["mu"], g_umc)
    g_vm = clip_bwd(s["vm"], s["nvm"], s["mv"], g_vmc)
    g_tc, g_rc = psum_bwd(s["tc"], s["rc"], s["vm"], s["ps1"], g_vm)
    g_t = clip_bwd(s["et"], s["nt"], s["mt"], g_tc)
    g_r = clip_bwd(s["er"], s["nr"], s["mr"], g_rc)
    # um = (1 / cosh(nw)) * uw / nw, nw = max(|uw|, 1e-10)
    nw, ich = s["nw"], s["ich"]
    gf = ich / nw
    d_gf = -(np.tanh(nw) * nw + 1) * ich / (nw * nw)      # d/dnw of 1 / (cosh(nw) nw), without cosh^2
    g_nw = np.where(s["nwr"] >= lo, _dot(g_um, s["uw"]) * d_gf, dt(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        g_uw = gf * g_um + np.where(s["nwr"] > 0, g_nw * s["uw"] / s["nwr"], dt(0))
    g_ue = g_uw * s["w"]
    g_w = g_uw * s["ue"]
    # ue = arsech(c) * hc / c, c = clamp(|hc|)
    c, ac = s["c"], s["ac"]
    d_f = (d_arsech(c) * c - ac) / (c * c)
    g_c = np.where((s["nh1"] >= lo) & (s["nh1"] <= hi), _dot(g_ue, s["hc"]) * d_f, dt(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        g_hc = (ac / c) * g_ue + np.where(s["nh1"] > 0, g_c * s["hc"] / s["nh1"], dt(0))
    g_h = clip_bwd(s["eh"], s["nh"], s["mh"], g_hc)
    np.add.at(g_wu, r, g_w)
    np.add.at(g_ent, h, np.where((h != 0)[:, None], g_h, dt(0)))
    np.add.at(g_ent, t, np.where((t != 0)[:, None], g_t, dt(0)))
    np.add.at(g_rel, r, np.where((r != 0)[:, None], g_r, dt(0)))
    return [g_wu, g_bs, g_bo, g_ent, g_rel]


def bce(preds, y, dtype=np.float64):
    """BCEWithLogitsLoss()(preds, clamp(y, 0, 1)) -> (mean loss, d loss / d preds)."""
    dt = dtype
    x = np.asarray(preds, dtype=dt)
    lab = np.clip(np.asarray(y, dtype=dt), dt(0), dt(1))
    loss = np.maximum(x, dt(0)) - x * lab + np.log1p(np.exp(-np.abs(x)))
    sig = np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))
    return np.sum(loss) / dt(len(x)), (sig - lab) / dt(len(x))


def train_bce(tabs, h, r, t, y, dtype=np.float64):
    """(preds, loss, the five gradients) of one batch."""
    preds = forward(tabs, h, r, t, dtype)
    loss, dscore = bce(preds, y, dtype)
    return preds, loss, backward(tabs, h, r, t, dscore, dtype)


def rsgd_step(tabs, grads, lr, riemannian=True, dtype=np.float64):
    """One optimiser step: the Poincare update on the two embeddings (or p - lr g when not riemannian), p - lr g on wu, bs, bo."""
    dt = dtype
    lr = dt(lr)
    tabs = [np.asarray(a, dtype=dt) for a in tabs]
    grads = [np.asarray(a, dtype=dt) for a in grads]
    out = [p - lr * g for p, g in zip(tabs[:3], grads[:3])]
    hi, lo = dt(1) - dt(BALL), dt(TINY)
    for p, g in zip(tabs[3:], grads[3:]):
        if not riemannian:
            out.append(p - lr * g)
            continue
        sq = np.clip(_dot(p, p), dt(0), hi)
        d = g * ((1 - sq) ** 2 / 4)
        v = -lr * d
        nv = np.maximum(np.sqrt(_dot(v, v)), lo)
        y = np.tanh(nv / (1 - sq)) * v / nv
        new, _ = psum_fwd(p, y)
        out.append(np.where(np.any(g != 0, -1, keepdims=True), new, p))
    return out


def _tail(nz2, dtype):
    dt = dtype
    nz = np.sqrt(np.maximum(nz2, dt(0)))
    cz = np.clip(nz, dt(TINY), dt(1) - dt(BALL))
    return (2 * arsech(cz)) ** 2


def _clip_factor(n2, dtype):
    """(factor, clipped squared norm) of a vector with squared norm n2."""
    dt = dtype
    n = np.sqrt(n2)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(n >= 1, 1 / (n - dt(BALL)), dt(1))
    return f, f * f * n2


def _dist2(su, sv, duv, dtype):
    """|p_sum(-u, v)|^2 from |u|^2, |v|^2 and u.v."""
    dt = dtype
    hi = dt(1) - dt(BALL)
    sx, sy = np.clip(su, dt(0), hi), np.clip(sv, dt(0), hi)
    dxy = -duv
    A = 1 + 2 * dxy + sy
    B = 1 - sx
    den = 1 + 2 * dxy + sx * sy
    return (A * A * su - 2 * A * B * duv + B * B * sv) / (den * den)


def query_um(tabs, h, r, dtype=np.float64):
    """The finished (clipped) u_m of (h, r): [k]."""
    dt = dtype
    wu, _, _, ent, _ = (np.asarray(a, dtype=dt) for a in tabs)
    lo, hi = dt(TINY), dt(1) - dt(BALL)
    hc, _, _ = clip_fwd(ent[h][None])
    c = np.clip(np.sqrt(_dot(hc, hc)), lo, hi)
    uw = (arsech(c) * hc / c) * wu[r]
    nw = np.maximum(np.sqrt(_dot(uw, uw)), lo)
    um = (1 / np.cosh(nw)) * uw / nw
    return clip_fwd(um)[0][0]


def sweep_tail(tabs, h, r, dtype=np.float64):
    """preds of (h, r, e) for every e through two dot products per candidate."""
    dt = dtype
    wu, bs, bo, ent, rel = (np.asarray(a, dtype=dt) for a in tabs)
    hi = dt(1) - dt(BALL)
    um = query_um(tabs, h, r, dt)
    rc = clip_fwd(rel[r][None])[0][0]
    su, sr, dru = np.sum(um * um), np.sum(rc * rc), np.sum(rc * um)
    ne2 = np.sum(ent * ent, -1)
    d1, d2 = ent @ rc, ent @ um
    ce, st = _clip_factor(ne2, dt)
    dtr, dtu = ce * d1, ce * d2
    sx, sy = np.clip(st, dt(0), hi), np.clip(sr, dt(0), hi)
    A = 1 + 2 * dtr + sy
    B = 1 - sx
    den = 1 + 2 * dtr + sx * sy
    sv = (A * A * st + 2 * A * B * dtr + B * B * sr) / (den * den)
    duv = (A * dtu + B * dru) / den
    cv, svc = _clip_factor(sv, dt)
    sq = _tail(_dist2(su, svc, cv * duv, dt), dt)
    return -(sq - bs[h] - bo)


def sweep_head(tabs, r, t, dtype=np.float64):
    """preds of (e, r, t) for every e."""
    dt = dtype
    wu, bs, bo, ent, rel = (np.asarray(a, dtype=dt) for a in tabs)
    lo, hi = dt(TINY), dt(1) - dt(BALL)
    tc = clip_fwd(ent[t][None])[0]
    rc = clip_fwd(rel[r][None])[0]
    vm = clip_fwd(psum_fwd(tc, rc)[0])[0][0]
    w = wu[r]
    sv = np.sum(vm * vm)
    ne2 = np.sum(ent * ent, -1)
    d1, d2 = (ent * ent) @ (w * w), ent @ (w * vm)
    ce, sh = _clip_factor(ne2, dt)
    c = np.clip(np.sqrt(sh), lo, hi)
    f = arsech(c) / c * ce                         # u_w = f * (e o w)
    nw = np.maximum(np.sqrt(f * f * d1), lo)
    gf = (1 / np.cosh(nw)) / nw
    su = gf * gf * (f * f * d1)
    duv = gf * f * d2
    cu, suc = _clip_factor(su, dt)
    sq = _tail(_dist2(suc, sv, cu * duv, dt), dt)
    return -(sq - bs - bo[t])


def ranks(scores, true, known=(), rank_order=0):
    """(rank, filtered rank, ties) of candidate `true` by the count convention: candidates that precede it in the order."""
    s = np.asarray(scores)
    before = (s < s[true]) if rank_order == 0 else (s > s[true])
    known = [e for e in known if e != true]
    return int(before.sum()), int(before.sum() - before[known].sum()), int((s == s[true]).sum() - 1)
