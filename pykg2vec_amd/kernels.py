"""Torch-tensor front end of the C ABI: argument checks, descriptor building, stream plumbing.

PyTorch is used here only for device memory and the current HIP stream; all arithmetic happens in
libkge_hip.so.  Every function raises if a tensor is not a contiguous tensor on a HIP device.
"""
import collections
import ctypes
import os
import math

import torch

from . import _lib as L

MODEL_IDS = {"transe": L.TRANSE, "transh": L.TRANSH, "transd": L.TRANSD, "rotate": L.ROTATE, "rescal": L.RESCAL,
             "ntn": L.NTN, "distmult": L.DISTMULT, "complex": L.COMPLEX, "complexn3": L.COMPLEX, "analogy": L.ANALOGY,
             "transm": L.TRANSM, "cp": L.CP, "simple": L.SIMPLE, "simple_ignr": L.SIMPLE_IGNR, "quate": L.QUATE,
             "transr": L.TRANSR, "slm": L.SLM, "sme": L.SME, "sme_bl": L.SME_BL, "kg2e": L.KG2E, "hole": L.HOLE,
             "octonione": L.OCTONIONE}
OPTIMIZER_IDS = {"sgd": L.OPT_SGD, "adam": L.OPT_ADAM, "adagrad": L.OPT_ADAGRAD, "rms": L.OPT_RMSPROP,
                 "gradient": 4}   # KGE_OPT_GRADIENT: kge_pull_step writes the dense gradient instead of updating


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a tensor" % what)
    if not t.is_cuda:
        raise L.KgeHipError("%s must live on the HIP device (got %s); the HIP path has no CPU fallback" % (what, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s (got %s)" % (what, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    return ctypes.c_void_p(t.data_ptr())


def _ids(t, what):
    return _dev(t, torch.int64, what)


# Shape every table of a model must have for the ids the kernels index it with: (rows indexed by, columns).  "E" / "R": the
# kernels read row `entity id` / `relation id`, so the table needs at least tot_entity / tot_relation rows; an int: exactly that
# many rows.  d = dim, k = rel_dim.  (models/pairwise.py, models/pointwise.py constructors; include/kge_hip.h enum kge_model.)
_TABLE_SHAPES = {
    "transe": [("E", "d"), ("R", "d")],
    "transm": [("E", "d"), ("R", "d"), ("R", None)],                      # theta [R]
    "transh": [("E", "d"), ("R", "d"), ("R", "d")],
    "transd": [("E", "d"), ("R", "k"), ("E", "d"), ("R", "k")],
    "rotate": [("E", "d"), ("E", "d"), ("R", "d")],
    "rescal": [("E", "d"), ("R", "d*d")],
    "ntn": [("E", "d"), ("R", "k"), ("d", "k"), ("d", "k"), (1, "k"), ("k", "d*d")],
    "transr": [("E", "d"), ("R", "k"), ("R", "d*k")],
    "slm": [("E", "d"), ("R", "k"), ("d", "k"), ("d", "k")],
    "sme": [("E", "d"), ("R", "d"), ("d", "d"), ("d", "d"), ("d", 1), ("d", "d"), ("d", "d"), ("d", 1)],
    "sme_bl": [("E", "d"), ("R", "d"), ("d", "d"), ("d", "d"), ("d", 1), ("d", "d"), ("d", "d"), ("d", 1)],
    "kg2e": [("E", "d"), ("E", "d"), ("R", "d"), ("R", "d")],
    "hole": [("E", "d"), ("R", "d")],
    "distmult": [("E", "d"), ("R", "d")],
    "complex": [("E", "d"), ("E", "d"), ("R", "d"), ("R", "d")],
    "complexn3": [("E", "d"), ("E", "d"), ("R", "d"), ("R", "d")],
    "analogy": [("E", "d"), ("R", "d"), ("E", "d/2"), ("E", "d/2"), ("R", "d/2"), ("R", "d/2")],
    "cp": [("E", "d"), ("R", "d"), ("E", "d")],
    "simple": [("E", "d"), ("E", "d"), ("R", "d"), ("R", "d")],
    "simple_ignr": [("E", "d"), ("E", "d"), ("R", "d"), ("R", "d")],
    # QuatE's four relation tables are allocated with tot_entity rows (models/pointwise.py:622-631) but looked up by RELATION
    # id: tot_relation > tot_entity is an IndexError in the reference and a refused descriptor here
    "quate": [("E", "d")] * 4 + [("R", "d")] * 4,
    # ent_embedding_1..8, rel_embedding_1..8, rel_w_embedding (never read: the descriptor carries two component blocks)
    "octonione": [("E", "d")] * 8 + [("R", "d")] * 8 + [("R", "d")],
}


def _check_table_shapes(model_name, tables, tot_entity, tot_relation, dim, rel_dim):
    spec = _TABLE_SHAPES.get(model_name)
    if spec is None:
        return
    if len(tables) < len(spec):
        raise L.KgeHipError("%s: %d tables given, the model has %d" % (model_name, len(tables), len(spec)))
    size = {"E": int(tot_entity), "R": int(tot_relation), "d": int(dim), "k": int(rel_dim)}
    cols_of = {"d": size["d"], "k": size["k"], "d*d": size["d"] ** 2, "d*k": size["d"] * size["k"], "d/2": size["d"] // 2}
    for i, ((by, cols), t) in enumerate(zip(spec, tables)):
        rows = t.shape[0]
        want_cols = cols_of.get(cols)
        got_cols = t.numel() // rows if rows else 0
        if by in ("E", "R"):
            need = size[by]
            if rows < need:
                raise L.KgeHipError(
                    "%s: table %d has %d rows but is indexed by %s ids up to %d (tot_%s = %d): an nn.Embedding lookup would raise "
                    "IndexError (models/Domain.py:8-13)" % (model_name, i, rows, "entity" if by == "E" else "relation", need - 1,
                                                             "entity" if by == "E" else "relation", need))
        else:
            need = by if isinstance(by, int) else size[by]
            if rows != need:
                raise L.KgeHipError("%s: table %d must have %d rows (got %d)" % (model_name, i, need, rows))
        if want_cols is not None and (t.dim() != 2 or got_cols != want_cols):
            raise L.KgeHipError("%s: table %d must be [rows, %d] (got %s)" % (model_name, i, want_cols, tuple(t.shape)))


def set_debug(check_ids=True):
    """Debug mode of the library (include/kge_hip.h: kge_set_debug; KGE_DEBUG_IDS=1 in the environment does the same): every id
    handed to an entry point is range-checked against its table first and a bad one raises KgeHipError, as nn.Embedding raises
    IndexError for the reference.  Synchronises the stream on every call: not for the hot loop."""
    L.load().kge_set_debug(1 if check_ids else 0)


def set_switch(name, value):
    """Force (0 / 1 / an integer) or release (None) one of the library's A/B switches (kge_set_switch; e.g. "EVAL_GEMM")."""
    L.check(L.load().kge_set_switch(name.encode(), -1 if value is None else int(value)), "kge_set_switch")


def debug_enabled():
    return bool(L.load().kge_get_debug())


def check_ids(ids, bound, what="ids"):
    """Raise KgeHipError if some id is outside [0, bound) (one scan kernel + a stream synchronisation)."""
    L.check(L.load().kge_check_ids(_ids(ids, what), ids.numel(), int(bound), _stream()), "kge_check_ids(%s)" % what)


def debug_marker(tag):
    """An empty launch of `tag` workgroups ("kge::k_marker"): a cut point in a profiler's dispatch sequence (bench.py)."""
    L.check(L.load().kge_debug_marker(int(tag), _stream()), "kge_debug_marker")


def make_desc(model_name, tables, grads=None, *, tot_entity, tot_relation, dim, rel_dim=None, l1_flag=False,
              margin=0.0):
    """Build a kge_model_desc.  `tables` / `grads`: lists of fp32 device tensors in parameter_list order.  Table shapes are
    checked against (tot_entity, tot_relation, dim, rel_dim): the kernels index rows by id without a bounds test."""
    _check_table_shapes(model_name, tables, tot_entity, tot_relation, dim, rel_dim if rel_dim is not None else dim)
    d = L.ModelDesc()
    d.model = MODEL_IDS[model_name]
    d.flags = L.FLAG_L1 if l1_flag else 0
    d.tot_entity, d.tot_relation = int(tot_entity), int(tot_relation)
    d.dim = int(dim)
    d.rel_dim = int(rel_dim if rel_dim is not None else dim)
    d.margin = float(margin)
    d.phase_scale = 0.0
    if model_name == "rotate":
        # embedding_range = (margin + 2) / hidden_size ; phase = r / (embedding_range / pi)   (pairwise.py:747,781)
        d.phase_scale = 1.0 / (((float(margin) + 2.0) / dim) / 3.14159265358979323846)
    for i, t in enumerate(tables):
        d.tables[i] = _dev(t, torch.float32, "table %d" % i).value
    if grads is not None:
        for i, g in enumerate(grads):
            if g.shape != tables[i].shape:
                raise ValueError("grad %d shape %s != table shape %s" % (i, tuple(g.shape), tuple(tables[i].shape)))
            d.grads[i] = _dev(g, torch.float32, "grad %d" % i).value
    d._keepalive = (tables, grads)  # python-side references
    return d


def _block_of(tensors, rows, dim):
    """The first tensor if tensors[c] is the fp32 contiguous [rows, dim] table at data_ptr(tensors[0]) + c * roundup4(rows * dim)
    floats for every c (a component block of include/kge_hip.h's KGE_OCTONIONE convention, e.g. FlatState's views), else None."""
    stride = (rows * dim + 3) // 4 * 4 * 4
    t0 = tensors[0]
    for c, t in enumerate(tensors):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, dim)
                and t.device == t0.device and t.data_ptr() == t0.data_ptr() + c * stride):
            return None
    return t0


def _pack_block(tensors, rows, dim):
    """A fresh component block holding rows [0, rows) of every table."""
    stride = (rows * dim + 3) // 4 * 4
    for i, t in enumerate(tensors):
        _dev(t, torch.float32, "table %d" % i)
    blk = torch.zeros(len(tensors) * stride, dtype=torch.float32, device=tensors[0].device)
    for c, t in enumerate(tensors):
        blk[c * stride:c * stride + rows * dim].view(rows, dim).copy_(t[:rows])
    return blk


def octonion_desc(tables, grads=None, *, tot_entity, tot_relation, dim):
    """kge_model_desc of OctonionE: `tables` / `grads` in parameter_list order (ent_embedding_1..8, rel_embedding_1..8 and
    optionally rel_w_embedding, which is never read).  Tables that already sit as component blocks (FlatState, or a model kept in
    block layout) are passed by address; otherwise they are packed into temporary blocks, and packed gradients are copied back
    into `grads` by the call that accumulates into them (score_backward / train_pointwise_logistic / _sampled)."""
    _check_table_shapes("octonione", tables, tot_entity, tot_relation, dim, dim)
    E, R, d = int(tot_entity), int(tot_relation), int(dim)
    desc = L.ModelDesc()
    desc.model = L.OCTONIONE
    desc.flags = 0
    desc.tot_entity, desc.tot_relation = E, R
    desc.dim = desc.rel_dim = d
    desc.margin = desc.phase_scale = 0.0
    keep, after = [], []
    for slot, (lo, rows) in enumerate(((0, E), (8, R))):
        parts = list(tables[lo:lo + 8])
        blk = _block_of(parts, rows, d)
        if blk is None:
            blk = _pack_block(parts, rows, d)
        desc.tables[slot] = blk.data_ptr()
        keep.append(blk)
        if grads is not None:
            gparts = list(grads[lo:lo + 8])
            for g, t in zip(gparts, parts):
                if g.shape != t.shape:
                    raise ValueError("grad shape %s != table shape %s" % (tuple(g.shape), tuple(t.shape)))
            gblk = _block_of(gparts, rows, d)
            if gblk is None:
                gblk = _pack_block(gparts, rows, d)
                stride = (rows * d + 3) // 4 * 4

                def unpack(gblk=gblk, gparts=gparts, rows=rows, stride=stride):
                    for c, g in enumerate(gparts):
                        g[:rows].copy_(gblk[c * stride:c * stride + rows * d].view(rows, d))
                after.append(unpack)
            desc.grads[slot] = gblk.data_ptr()
            keep.append(gblk)
    desc._keepalive = (tables, grads, keep)
    desc._after = after
    return desc


def _finish(desc):
    """Work a descriptor asks for after a call that wrote its gradient buffers (octonion_desc's packed gradients)."""
    for fn in getattr(desc, "_after", ()):
        fn()


def model_desc(model, weights=None, grads=None):
    """Descriptor of a drop-in model object (kgmeta.Model.make_desc)."""
    return model.make_desc(weights, grads)


def _workspace(desc, n, device):
    """(ptr, nbytes, keepalive) scratch for a score/train call on n rows; (None, 0, None) for gather-type models."""
    nbytes = L.load().kge_workspace_bytes(ctypes.byref(desc), int(n))
    if nbytes == 0:
        return None, 0, None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ctypes.c_void_p(ws.data_ptr()), nbytes, ws


def score_forward(desc, h, r, t):
    if isinstance(desc, L.MurpDesc):
        return murp_score_forward(desc, h, r, t)
    if isinstance(desc, L.ConvKBDesc):
        return convkb_score_forward(desc, h, r, t)
    n = h.numel()
    if r.numel() != n or t.numel() != n:
        raise ValueError("h, r, t must have equal lengths")
    out = torch.empty(n, dtype=torch.float32, device=h.device)
    wp, wb, _keep = _workspace(desc, n, h.device)
    L.check(L.load().kge_score_forward(ctypes.byref(desc), _ids(h, "h"), _ids(r, "r"), _ids(t, "t"), n,
                                       _dev(out, torch.float32, "scores"), wp, wb, _stream()), "kge_score_forward")
    return out


def score_backward(desc, h, r, t, dscore):
    if isinstance(desc, L.MurpDesc):
        return murp_score_backward(desc, h, r, t, dscore)
    if isinstance(desc, L.ConvKBDesc):
        return convkb_score_backward(desc, h, r, t, dscore)
    n = h.numel()
    wp, wb, _keep = _workspace(desc, n, h.device)
    L.check(L.load().kge_score_backward(ctypes.byref(desc), _ids(h, "h"), _ids(r, "r"), _ids(t, "t"), n,
                                        _dev(dscore, torch.float32, "dscore"), wp, wb, _stream()), "kge_score_backward")
    _finish(desc)


_rescal_scratch = {}


def rescal_normalize(ent, rel, k):
    lib = L.load()
    need = lib.kge_rescal_normalize_scratch_bytes(rel.shape[0], int(k))
    key = (ent.device, need)
    if key not in _rescal_scratch:   # a few hundred floats, kept per (device, size): the call stays allocation-free and capturable
        _rescal_scratch[key] = torch.empty(max(1, need // 4), dtype=torch.float32, device=ent.device)
    sc = _rescal_scratch[key]
    L.check(lib.kge_rescal_normalize_ws(_dev(ent, torch.float32, "ent"), ent.shape[0], _dev(rel, torch.float32, "rel"),
                                        rel.shape[0], k, sc.data_ptr(), sc.numel() * 4, _stream()), "kge_rescal_normalize_ws")


def new_loss_buffer(device):
    return torch.zeros(L.LOSS_SLOTS * L.LOSS_STRIDE, dtype=torch.float32, device=device)


def read_loss(buf):
    """Total of the striped loss accumulators (a device tensor; no sync)."""
    return buf.view(L.LOSS_SLOTS, L.LOSS_STRIDE)[:, 0].sum()


def train_pairwise_hinge(desc, ph, pr, pt, nh, nr, nt, margin, loss_buf):
    n = ph.numel()
    if nh.numel() != n:
        raise ValueError("pairwise_hinge needs neg_rate == 1 (criterion.py:27 adds [B] to [B*neg_rate])")
    wp, wb, _keep = _workspace(desc, n, ph.device)
    L.check(L.load().kge_train_pairwise_hinge(ctypes.byref(desc), _ids(ph, "ph"), _ids(pr, "pr"), _ids(pt, "pt"),
                                              _ids(nh, "nh"), _ids(nr, "nr"), _ids(nt, "nt"), n, float(margin),
                                              wp, wb, _dev(loss_buf, torch.float32, "loss"), _stream()),
            "kge_train_pairwise_hinge")


def train_pairwise_hinge_sampled(desc, triples, perm, start, n, bern_prob, slots, seed, offset, margin, loss_buf,
                                 cursor=None):
    """Sampler + both scores + hinge + backward in ONE launch; the batch equals sample_batch(start, n, neg_rate=1)."""
    bp = _dev(bern_prob, torch.float32, "bern_prob") if bern_prob is not None else None
    sp = ctypes.c_void_p(slots.data_ptr()) if slots is not None else None
    pc = _dev(cursor, torch.int64, "cursor") if cursor is not None else None
    L.check(L.load().kge_train_pairwise_hinge_sampled(ctypes.byref(desc), _ids(triples, "triples"), _ids(perm, "perm"),
                                                      int(start), int(n), bp, sp,
                                                      slots.numel() if slots is not None else 0,
                                                      int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), pc,
                                                      float(margin), _dev(loss_buf, torch.float32, "loss"), _stream()),
            "kge_train_pairwise_hinge_sampled")


def train_pointwise_logistic_sampled(desc, triples, perm, start, n_pos, neg_rate, bern_prob, slots, seed, offset, lmbda,
                                     reg_type, loss_buf, cursor=None):
    """Sampler + scoring + pointwise logistic loss + regulariser + backward in ONE launch; the rows equal
    sample_batch(start, n_pos, neg_rate, pointwise=True)."""
    if isinstance(desc, L.ConvKBDesc):
        _convkb_no_reg(lmbda, reg_type)
        return convkb_train_logistic_sampled(desc, triples, perm, start, n_pos, neg_rate, bern_prob, slots, seed, offset, loss_buf,
                                             cursor=cursor)
    bp = _dev(bern_prob, torch.float32, "bern_prob") if bern_prob is not None else None
    sp = ctypes.c_void_p(slots.data_ptr()) if slots is not None else None
    pc = _dev(cursor, torch.int64, "cursor") if cursor is not None else None
    L.check(L.load().kge_train_pointwise_logistic_sampled(ctypes.byref(desc), _ids(triples, "triples"), _ids(perm, "perm"),
                                                          int(start), int(n_pos), int(neg_rate), bp, sp,
                                                          slots.numel() if slots is not None else 0,
                                                          int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), pc,
                                                          float(lmbda), int(reg_type), _dev(loss_buf, torch.float32, "loss"),
                                                          _stream()), "kge_train_pointwise_logistic_sampled")
    _finish(desc)


def train_pairwise_selfadv_sampled(desc, triples, perm, start, n_pos, neg_rate, alpha, bern_prob, slots, seed, offset,
                                   loss_buf, cursor=None):
    """RotatE: sampler + scores + self-adversarial loss + backward in ONE launch (batch == sample_batch(...))."""
    bp = _dev(bern_prob, torch.float32, "bern_prob") if bern_prob is not None else None
    sp = ctypes.c_void_p(slots.data_ptr()) if slots is not None else None
    pc = _dev(cursor, torch.int64, "cursor") if cursor is not None else None
    L.check(L.load().kge_train_pairwise_selfadv_sampled(ctypes.byref(desc), _ids(triples, "triples"), _ids(perm, "perm"),
                                                        int(start), int(n_pos), int(neg_rate), float(alpha), bp, sp,
                                                        slots.numel() if slots is not None else 0,
                                                        int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), pc,
                                                        _dev(loss_buf, torch.float32, "loss"), _stream()),
            "kge_train_pairwise_selfadv_sampled")


STAGED_CAP = 16   # bucket entries per corrupting entity before the overflow chain


class StagedPlan:
    """struct kge_staged_step for one model: flat parameter / state buffers, the table list with its slot sites, the
    staging buffer and the per-entity registration lists.  `bind(batch_index_views, n_pos)` points it at one batch."""

    LAYOUTS = {   # model -> (static slots per positive, dynamic slots per negative, [(cls, site_a, site_b, dsite)] per table)
        "rotate": (5, 2, [(0, 0, 3, 0), (0, 1, 4, 1), (1, 2, 0, -1)]),                      # h_re h_im r t_re t_im | c_re c_im
        "distmult": (3, 1, [(0, 0, 2, 0), (1, 1, 0, -1)]),                                   # h r t | c
        "complex": (6, 2, [(0, 0, 4, 0), (0, 1, 5, 1), (1, 2, 0, -1), (1, 3, 0, -1)]),      # h_re h_im r_re r_im t_re t_im | c_re c_im
    }

    def __init__(self, kernel_name, flat_param, state1, state2, table_offsets, table_rows, dim, tot_entity, tot_relation,
                 max_pos, neg_rate, sparse=False):
        ns, nd, sites = self.LAYOUTS[kernel_name]
        if len(sites) != len(table_offsets):
            raise L.KgeHipError("staged plan: table list does not match the model")
        dev = flat_param.device
        self.ns, self.nd, self.neg_rate, self.max_pos = ns, nd, int(neg_rate), int(max_pos)
        self.stride = (int(dim) + 3) // 4 * 4
        n_slots = self.max_pos * (ns + nd * self.neg_rate)
        # RotatE rows of more than 512 floats (a bundle's rows over 2 or 4 waves, csrc/kge_score.hip: k_rotate_bundle_staged_split): rows
        # padded to the width the waves cover + one spare slot set behind the used ones -> the kernel's stores carry no predicates
        # (kge_staged_step.stage_spare, round 6)
        self.spare = kernel_name == "rotate" and int(dim) > 512 and os.environ.get("KGE_STAGE_SPARE") != "0"   # (=0: tight rows, A/B)
        if self.spare:
            self.stride = 1024 if int(dim) <= 1024 else 2048
            n_slots += ns + nd
        self.stage = torch.empty(n_slots * self.stride, dtype=torch.float32, device=dev)
        # sparse (SGD / Adagrad with touched-row lists): ONE registration set, count | head back to back so that
        # the train entry point clears it with one memset; the sweep then visits only rows that have a slot.
        # dense: two sets (count, head) alternate between steps and the sweep of a step clears the other one (no memset).
        self.sparse = bool(sparse)
        E = int(tot_entity)
        self.sets = [torch.zeros(2 * E, dtype=torch.int32, device=dev) for _ in range(1 if self.sparse else 2)]
        self.counts = [x[:E] for x in self.sets]
        self.heads = [x[E:2 * E] for x in self.sets]          # overflow chain heads hold pair + 1: zero = empty
        self.dyn_list = torch.zeros(self.max_pos * self.neg_rate, dtype=torch.int32, device=dev) if self.sparse else None
        self.parity = 0
        self.bucket = torch.zeros(tot_entity * STAGED_CAP, dtype=torch.int32, device=dev)
        self.next = torch.zeros(self.max_pos * self.neg_rate, dtype=torch.int32, device=dev)
        self._keep = (flat_param, state1, state2)
        self._cache = {}
        self.n_rel_tables = sum(1 for x in sites if x[0] == 1)
        self.rel_partials = None
        c = self.c = self.cur = L.StagedStep()
        c.param = _dev(flat_param, torch.float32, "param")
        c.state1 = _dev(state1, torch.float32, "state1") if state1 is not None else None
        c.state2 = _dev(state2, torch.float32, "state2") if state2 is not None else None
        for k, ((cls, sa, sb, ds), off, rows) in enumerate(zip(sites, table_offsets, table_rows)):
            c.tables[k].cls, c.tables[k].site_a, c.tables[k].site_b, c.tables[k].dsite = cls, sa, sb, ds
            c.tables[k].flat_off, c.tables[k].rows = int(off), int(rows)
        c.n_tables, c.dim = len(sites), int(dim)
        c.dyn_bucket, c.dyn_next, c.dyn_cap = self.bucket.data_ptr(), self.next.data_ptr(), STAGED_CAP
        c.stage, c.stage_stride = self.stage.data_ptr(), self.stride
        c.stage_spare = 1 if self.spare else 0
        self.dyn_scale = torch.ones(self.max_pos * self.neg_rate, dtype=torch.float32, device=dev) if kernel_name == "rotate" else None
        c.dyn_scale = self.dyn_scale.data_ptr() if self.dyn_scale is not None else None
        c.static_slots, c.dynamic_slots = ns, nd
        c.tot_entity, c.tot_relation = int(tot_entity), int(tot_relation)

    def bind_batch(self, b, index):
        """Point the plan at batch b of a generator.StagedIndex.  The filled descriptor is cached per (batch, parity): the
        eager step is two native calls plus a dictionary lookup, not a dozen pointer validations."""
        key = (b, 0 if self.sparse else self.parity)
        hit = self._cache.get(key)
        if hit is None:
            if self.rel_partials is None and index.max_rel_list > index.LONG_LIST:
                # sized ONCE for the batch with the most chunks: the cached per-batch snapshots below hold this pointer,
                # so the buffer must never be reallocated while the plan lives
                self.rel_partials = torch.empty(max(1, max(index.n_chunks)) * self.n_rel_tables * self.stride,
                                                dtype=torch.float32, device=self.stage.device)
            ent_off, ent_inc, rel_off, rel_inc, n = index.batch(b)
            self.bind(ent_off, ent_inc, rel_off, rel_inc, n, index.chunks(b), index.touched(b) if self.sparse else None)
            snap = L.StagedStep()
            ctypes.memmove(ctypes.byref(snap), ctypes.byref(self.c), ctypes.sizeof(L.StagedStep))
            hit = self._cache[key] = (snap, self._batch, n)
        elif not self.sparse:
            self.parity ^= 1
        self.cur = hit[0]
        return hit[2]

    def bind(self, ent_off, ent_inc, rel_off, rel_inc, n_pos, chunks=None, touched=None):
        if n_pos > self.max_pos:
            raise L.KgeHipError("staged plan: batch larger than the plan")
        self._batch = (ent_off, ent_inc, rel_off, rel_inc, chunks)
        c = self.c
        if chunks is not None:
            chunk_off, chunk_rel, n_chunks = chunks
            need = max(1, n_chunks) * self.n_rel_tables * self.stride
            if self.rel_partials is None or self.rel_partials.numel() < need:
                if self._cache:   # a cached snapshot holds the old pointer: growing now would leave it dangling
                    raise L.KgeHipError("staged plan: relation partial buffer too small for this batch (%d floats needed); "
                                        "bind batches through bind_batch(), which sizes it for the whole index" % need)
                self.rel_partials = torch.empty(need, dtype=torch.float32, device=self.stage.device)
            c.rel_chunk_off, c.chunk_rel = _dev(chunk_off, torch.int32, "rel_chunk_off"), _dev(chunk_rel, torch.int32, "chunk_rel")
            c.rel_partials, c.n_chunks = self.rel_partials.data_ptr(), int(n_chunks)
        else:
            c.rel_chunk_off, c.chunk_rel, c.rel_partials, c.n_chunks = None, None, None, 0
        c.ent_off, c.ent_inc = _dev(ent_off, torch.int32, "ent_off"), _dev(ent_inc, torch.int32, "ent_inc")
        c.rel_off, c.rel_inc = _dev(rel_off, torch.int32, "rel_off"), _dev(rel_inc, torch.int32, "rel_inc")
        c.n_pos, c.n_neg = int(n_pos), int(n_pos) * self.neg_rate
        if self.sparse:
            if touched is None:
                raise L.KgeHipError("staged plan: the sparse sweep needs the batch's touched-row lists")
            t_ent, n_ent, t_rel, n_rel = touched
            self._batch += (t_ent, t_rel)
            c.touched_ent, c.n_touched_ent = _dev(t_ent, torch.int32, "touched_ent"), int(n_ent)
            c.touched_rel, c.n_touched_rel = _dev(t_rel, torch.int32, "touched_rel"), int(n_rel)
            c.dyn_list = self.dyn_list.data_ptr()
            c.dyn_count, c.dyn_head = self.counts[0].data_ptr(), self.heads[0].data_ptr()
            c.dyn_count_next, c.dyn_head_next = None, None
            self.cur = c
            return self
        # this step registers into set `parity`; its optimiser sweep clears the other set for the next step
        q = self.parity
        c.dyn_count, c.dyn_head = self.counts[q].data_ptr(), self.heads[q].data_ptr()
        c.dyn_count_next, c.dyn_head_next = self.counts[q ^ 1].data_ptr(), self.heads[q ^ 1].data_ptr()
        self.parity ^= 1
        self.cur = c
        return self


def train_pairwise_selfadv_sampled_staged(desc, triples, perm, start, n_pos, neg_rate, alpha, bern_prob, slots, seed, offset,
                                          plan, loss_buf):
    """RotatE bundle step with staged (atomic-free) gradient output; follow with optimizer_step_staged(plan)."""
    bp = _dev(bern_prob, torch.float32, "bern_prob") if bern_prob is not None else None
    sp = ctypes.c_void_p(slots.data_ptr()) if slots is not None else None
    L.check(L.load().kge_train_pairwise_selfadv_sampled_staged(
        ctypes.byref(desc), _ids(triples, "triples"), _ids(perm, "perm"), int(start), int(n_pos), int(neg_rate), float(alpha),
        bp, sp, slots.numel() if slots is not None else 0, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
        ctypes.byref(plan.cur), _dev(loss_buf, torch.float32, "loss"), _stream()), "kge_train_pairwise_selfadv_sampled_staged")


def train_pointwise_logistic_sampled_staged(desc, triples, perm, start, n_pos, neg_rate, bern_prob, slots, seed, offset, lmbda,
                                            reg_type, plan, loss_buf):
    """DistMult / ComplEx bundle step with staged (atomic-free) gradient output; follow with optimizer_step_staged(plan)."""
    bp = _dev(bern_prob, torch.float32, "bern_prob") if bern_prob is not None else None
    sp = ctypes.c_void_p(slots.data_ptr()) if slots is not None else None
    L.check(L.load().kge_train_pointwise_logistic_sampled_staged(
        ctypes.byref(desc), _ids(triples, "triples"), _ids(perm, "perm"), int(start), int(n_pos), int(neg_rate), bp, sp,
        slots.numel() if slots is not None else 0, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), float(lmbda),
        int(reg_type), ctypes.byref(plan.cur), _dev(loss_buf, torch.float32, "loss"), _stream()),
        "kge_train_pointwise_logistic_sampled_staged")


def optimizer_step_staged(kind, plan, lr, step):
    L.check(L.load().kge_optimizer_step_staged(OPTIMIZER_IDS[kind], ctypes.byref(plan.cur), float(lr), int(step), _stream()),
            "kge_optimizer_step_staged")


def train_pairwise_selfadv(desc, ph, pr, pt, nh, nr, nt, neg_rate, alpha, loss_buf, workspace=None):
    n = ph.numel()
    if nh.numel() != n * neg_rate:
        raise ValueError("negatives must be [B*neg_rate]")
    if workspace is None or workspace.numel() < n * (1 + neg_rate):
        workspace = torch.empty(n * (1 + neg_rate), dtype=torch.float32, device=ph.device)
    L.check(L.load().kge_train_pairwise_selfadv(ctypes.byref(desc), _ids(ph, "ph"), _ids(pr, "pr"), _ids(pt, "pt"),
                                                _ids(nh, "nh"), _ids(nr, "nr"), _ids(nt, "nt"), n, int(neg_rate),
                                                float(alpha), _dev(workspace, torch.float32, "workspace"),
                                                _dev(loss_buf, torch.float32, "loss"), _stream()),
            "kge_train_pairwise_selfadv")
    return workspace


def train_pointwise_logistic(desc, h, r, t, y, lmbda, reg_type, loss_buf, bundle=1):
    if isinstance(desc, L.ConvKBDesc):
        _convkb_no_reg(lmbda, reg_type)
        return convkb_train_logistic(desc, h, r, t, y, loss_buf, bundle=bundle)
    n = h.numel()
    L.check(L.load().kge_train_pointwise_logistic(ctypes.byref(desc), _ids(h, "h"), _ids(r, "r"), _ids(t, "t"),
                                                  _ids(y, "y"), n, int(bundle), float(lmbda), int(reg_type),
                                                  _dev(loss_buf, torch.float32, "loss"), _stream()),
            "kge_train_pointwise_logistic")
    _finish(desc)


def l2norm_reg(param, grad, lmbda, loss_buf):
    """NTN.get_reg over one flat parameter buffer: loss += lmbda*||param||_2, grad += lmbda*param/||param||_2."""
    scratch = torch.empty(1, dtype=torch.float32, device=param.device)
    L.check(L.load().kge_l2norm_reg(_dev(param, torch.float32, "param"), _dev(grad, torch.float32, "grad"), param.numel(),
                                    float(lmbda), _dev(scratch, torch.float32, "scratch"),
                                    _dev(loss_buf, torch.float32, "loss"), _stream()), "kge_l2norm_reg")


def optimizer_step(kind, param, grad, state1, state2, lr, step, zero_grad=True, dev_hyper=None):
    p1 = _dev(state1, torch.float32, "state1") if state1 is not None else None
    p2 = _dev(state2, torch.float32, "state2") if state2 is not None else None
    ph = _dev(dev_hyper, torch.float32, "dev_hyper") if dev_hyper is not None else None
    L.check(L.load().kge_optimizer_step(OPTIMIZER_IDS[kind], _dev(param, torch.float32, "param"),
                                        _dev(grad, torch.float32, "grad"), p1, p2, param.numel(), float(lr), int(step),
                                        1 if zero_grad else 0, ph, _stream()), "kge_optimizer_step")


def optimizer_step_rows(kind, param, grad, state1, state2, rows, dim, lr, step, zero_grad=True, normalize=False, dev_hyper=None,
                        touched=None, touched_clear=None):
    """kge_optimizer_step_rows: the dense optimiser with one wave per row of a [rows, dim] table (flat views), optionally storing
    the row renormalised (RESCAL: what the next forward's in-place normalisation would make of it).  touched / touched_clear:
    int32 bitmaps of rows with a gradient (this step's, read; the other parity's, reset)."""
    p1 = _dev(state1, torch.float32, "state1") if state1 is not None else None
    p2 = _dev(state2, torch.float32, "state2") if state2 is not None else None
    ph = _dev(dev_hyper, torch.float32, "dev_hyper") if dev_hyper is not None else None
    L.check(L.load().kge_optimizer_step_rows(OPTIMIZER_IDS[kind], _dev(param, torch.float32, "param"), _dev(grad, torch.float32, "grad"),
                                             p1, p2, int(rows), int(dim), float(lr), int(step), 1 if zero_grad else 0,
                                             1 if normalize else 0, ph,
                                             _dev(touched, torch.int32, "touched") if touched is not None else None,
                                             _dev(touched_clear, torch.int32, "touched_clear") if touched_clear is not None else None,
                                             _stream()), "kge_optimizer_step_rows")


class RescalStage:
    """Buffers of the atomic-free entity gradients of the pairwise RESCAL step (struct kge_rescal_stage): gradient rows staged per
    (pair, side), the pairs' hinge coefficients, and per entity the list of staged rows registered with it (all zero between steps)."""
    CAP = 8

    def __init__(self, tot_entity, n_pairs, dim, device):
        self.n_pairs = int(n_pairs)
        self.gstage = torch.zeros(4 * self.n_pairs * int(dim), dtype=torch.float32, device=device)
        self.dsv = torch.zeros(self.n_pairs, dtype=torch.float32, device=device)
        self.count = torch.zeros(int(tot_entity), dtype=torch.int32, device=device)
        self.bucket = torch.zeros(int(tot_entity) * self.CAP, dtype=torch.int32, device=device)
        self.head = torch.zeros(int(tot_entity), dtype=torch.int32, device=device)
        self.next = torch.zeros(4 * self.n_pairs, dtype=torch.int32, device=device)
        self.c = L.RescalStage(self.gstage.data_ptr(), self.dsv.data_ptr(), self.count.data_ptr(), self.bucket.data_ptr(),
                               self.head.data_ptr(), self.next.data_ptr(), self.CAP)


def rescal_stage_ok(desc, n):
    """kge_rescal_stage_ok: the pairwise RESCAL step of n pairs can stage its entity gradients (slab form, d % 4 == 0, n <= 4096)."""
    return bool(L.load().kge_rescal_stage_ok(ctypes.byref(desc), int(n)))


def rescal_pair_step_staged(desc, ph, pr, pt, nh, nt, margin, loss_buf, touched, stage):
    """kge_rescal_pair_step_staged: the pairwise RESCAL step with every entity gradient row staged instead of added atomically."""
    n = ph.numel()
    if nh.numel() != n or n > stage.n_pairs:
        raise ValueError("rescal_pair_step_staged: %d pairs (stage sized for %d; neg_rate must be 1)" % (n, stage.n_pairs))
    wp, wb, _keep = _workspace(desc, n, ph.device)
    L.check(L.load().kge_rescal_pair_step_staged(ctypes.byref(desc), _ids(ph, "ph"), _ids(pr, "pr"), _ids(pt, "pt"), _ids(nh, "nh"),
                                                 _ids(nt, "nt"), n, float(margin), wp, wb, _dev(loss_buf, torch.float32, "loss"),
                                                 _dev(touched, torch.int32, "touched"), ctypes.byref(stage.c), _stream()),
            "kge_rescal_pair_step_staged")


def optimizer_step_rows_staged(kind, param, grad, state1, state2, rows, dim, lr, step, stage, touched, touched_clear=None, normalize=False,
                               dev_hyper=None):
    """kge_optimizer_step_rows_staged: kge_optimizer_step_rows with the gradient of a touched row summed from the stage."""
    p1 = _dev(state1, torch.float32, "state1") if state1 is not None else None
    p2 = _dev(state2, torch.float32, "state2") if state2 is not None else None
    ph = _dev(dev_hyper, torch.float32, "dev_hyper") if dev_hyper is not None else None
    L.check(L.load().kge_optimizer_step_rows_staged(OPTIMIZER_IDS[kind], _dev(param, torch.float32, "param"), _dev(grad, torch.float32, "grad"),
                                                    p1, p2, int(rows), int(dim), float(lr), int(step), 1 if normalize else 0, ph,
                                                    _dev(touched, torch.int32, "touched"),
                                                    _dev(touched_clear, torch.int32, "touched_clear") if touched_clear is not None else None,
                                                    ctypes.byref(stage.c), _stream()), "kge_optimizer_step_rows_staged")


def rescal_pair_step_ok(desc, n):
    return bool(L.load().kge_rescal_pair_step_ok(ctypes.byref(desc), int(n)))


def rescal_pair_step(desc, ph, pr, pt, nh, nt, margin, loss_buf, touched=None):
    """kge_rescal_pair_step: the pairwise RESCAL step for negatives that keep their positives' relations, one launch per
    (relation, 16 pairs) tile; touched: int32 bitmap [ceil(E / 32)] that receives the entity rows with a gradient."""
    n = ph.numel()
    if nh.numel() != n:
        raise ValueError("pairwise_hinge needs neg_rate == 1 (criterion.py:27 adds [B] to [B*neg_rate])")
    wp, wb, _keep = _workspace(desc, n, ph.device)
    L.check(L.load().kge_rescal_pair_step(ctypes.byref(desc), _ids(ph, "ph"), _ids(pr, "pr"), _ids(pt, "pt"), _ids(nh, "nh"),
                                          _ids(nt, "nt"), n, float(margin), wp, wb, _dev(loss_buf, torch.float32, "loss"),
                                          _dev(touched, torch.int32, "touched") if touched is not None else None, _stream()),
            "kge_rescal_pair_step")


def rescal_normalize_relations(rel, k):
    """The relation-matrix half of Rescal's in-place renormalisation (the entity half rides in kge_optimizer_step_rows)."""
    lib = L.load()
    need = lib.kge_rescal_normalize_scratch_bytes(rel.shape[0], int(k))
    key = (rel.device, need)
    if key not in _rescal_scratch:
        _rescal_scratch[key] = torch.empty(max(1, need // 4), dtype=torch.float32, device=rel.device)
    sc = _rescal_scratch[key]
    L.check(lib.kge_rescal_normalize_ws(None, 0, _dev(rel, torch.float32, "rel"), rel.shape[0], k, sc.data_ptr(), sc.numel() * 4,
                                        _stream()), "kge_rescal_normalize_ws")


def optimizer_step_rownorm_ok(rows, dim):
    return bool(L.load().kge_optimizer_step_rownorm_ok(int(rows), int(dim)))


def optimizer_step_rownorm(kind, param, grad, state1, state2, rows, dim, lr, step, zero_grad=True, advance=None):
    """kge_optimizer_step_rownorm: dense optimiser over a [rows, dim] table of wide rows + the in-place row renormalisation, with the
    rows' sums of squares left by the optimiser launch itself.  advance: None, or (hyper, cursor, next_cursor, next_hyper, batch_stride,
    n_batches, draws_per_batch) -- the step-state transition of optimizer_step_advance folded in."""
    lib = L.load()
    need = lib.kge_rescal_normalize_scratch_bytes(int(rows), int(round(dim ** 0.5))) if int(round(dim ** 0.5)) ** 2 == dim else 4 * int(rows) * ((int(dim) + 4095) // 4096)
    need = max(need, 4 * int(rows) * ((int(dim) + 4095) // 4096))
    key = (param.device, need)
    if key not in _rescal_scratch:
        _rescal_scratch[key] = torch.empty(max(1, need // 4), dtype=torch.float32, device=param.device)
    sc = _rescal_scratch[key]
    p1 = _dev(state1, torch.float32, "state1") if state1 is not None else None
    p2 = _dev(state2, torch.float32, "state2") if state2 is not None else None
    if advance is not None:
        hyper, cursor, next_cursor, next_hyper, batch_stride, n_batches, draws = advance
        adv = (_dev(hyper, torch.float32, "hyper"), _dev(cursor, torch.int64, "cursor"), _dev(next_cursor, torch.int64, "next_cursor"),
               _dev(next_hyper, torch.float32, "next_hyper"), int(batch_stride), int(n_batches), int(draws))
    else:
        adv = (None, None, None, None, 0, 1, 0)
    L.check(lib.kge_optimizer_step_rownorm(OPTIMIZER_IDS[kind], _dev(param, torch.float32, "param"), _dev(grad, torch.float32, "grad"), p1, p2,
                                           int(rows), int(dim), float(lr), int(step), 1 if zero_grad else 0, adv[0], sc.data_ptr(), sc.numel() * 4,
                                           adv[1], adv[2], adv[3], adv[4], adv[5], adv[6], _stream()), "kge_optimizer_step_rownorm")


def optimizer_step_rows_rownorm(kind, param, grad, state1, state2, rows, dim, wparam, wgrad, wstate1, wstate2, wrows, wdim, lr, step,
                                normalize=True, dev_hyper=None, touched=None, touched_clear=None, stage=None, advance=None, zero_grad=True):
    """kge_optimizer_step_rows_rownorm: RESCAL's optimiser step in two launches -- the row-owner sweep of the short-row table with the
    wide-row table's optimiser riding in its first workgroups, then the wide rows' rescale.  Arguments as optimizer_step_rows(_staged) and
    optimizer_step_rownorm; bit-identical to calling those two."""
    lib = L.load()
    need = 4 * int(wrows) * ((int(wdim) + 4095) // 4096)
    key = (param.device, "rider", need)
    if key not in _rescal_scratch:
        _rescal_scratch[key] = torch.empty(max(1, need // 4), dtype=torch.float32, device=param.device)
    sc = _rescal_scratch[key]
    f = lambda t, what: _dev(t, torch.float32, what) if t is not None else None
    if advance is not None:
        hyper, cursor, next_cursor, next_hyper, batch_stride, n_batches, draws = advance
        adv = (_dev(cursor, torch.int64, "cursor"), _dev(next_cursor, torch.int64, "next_cursor"), _dev(next_hyper, torch.float32, "next_hyper"),
               int(batch_stride), int(n_batches), int(draws))
        dev_hyper = hyper
    else:
        adv = (None, None, None, 0, 1, 0)
    L.check(lib.kge_optimizer_step_rows_rownorm(
        OPTIMIZER_IDS[kind], _dev(param, torch.float32, "param"), _dev(grad, torch.float32, "grad"), f(state1, "state1"), f(state2, "state2"),
        int(rows), int(dim), _dev(wparam, torch.float32, "wparam"), _dev(wgrad, torch.float32, "wgrad"), f(wstate1, "wstate1"),
        f(wstate2, "wstate2"), int(wrows), int(wdim), float(lr), int(step), 1 if zero_grad else 0, 1 if normalize else 0, f(dev_hyper, "dev_hyper"),
        _dev(touched, torch.int32, "touched") if touched is not None else None,
        _dev(touched_clear, torch.int32, "touched_clear") if touched_clear is not None else None,
        ctypes.byref(stage.c) if stage is not None else None, sc.data_ptr(), sc.numel() * 4, adv[0], adv[1], adv[2], adv[3], adv[4], adv[5],
        _stream()), "kge_optimizer_step_rows_rownorm")


def optimizer_step_advance(kind, param, grad, state1, state2, lr, hyper, cursor, next_cursor, next_hyper, batch_stride,
                           n_batches, draws_per_batch, zero_grad=True):
    """Dense optimiser sweep of a graph-replayed step + the next step's device-resident state (kge_optimizer_step_advance)."""
    p1 = _dev(state1, torch.float32, "state1") if state1 is not None else None
    p2 = _dev(state2, torch.float32, "state2") if state2 is not None else None
    L.check(L.load().kge_optimizer_step_advance(
        OPTIMIZER_IDS[kind], _dev(param, torch.float32, "param"), _dev(grad, torch.float32, "grad"), p1, p2, param.numel(),
        float(lr), 1 if zero_grad else 0, _dev(hyper, torch.float32, "hyper"), _dev(cursor, torch.int64, "cursor"),
        _dev(next_cursor, torch.int64, "next_cursor"), _dev(next_hyper, torch.float32, "next_hyper"), int(batch_stride),
        int(n_batches), int(draws_per_batch), _stream()), "kge_optimizer_step_advance")


def step_advance(cursor, hyper, batch_stride, n_batches, draws_per_batch, lr):
    """Advance the device-resident step state (int64[8] cursor, float32[4] hyper); first kernel of a captured step."""
    L.check(L.load().kge_step_advance(_dev(cursor, torch.int64, "cursor"), _dev(hyper, torch.float32, "hyper"),
                                      int(batch_stride), int(n_batches), int(draws_per_batch), float(lr), _stream()),
            "kge_step_advance")


def eval_workspace(desc, n, device):
    nbytes = L.load().kge_eval_workspace_bytes(ctypes.byref(desc), int(n))
    if nbytes == 0:
        L.check(-1, "kge_eval_workspace_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, workspace=None, ties=None):
    """triples int64 [n,3]; CSR filter lists (int64 offsets [n+1], int32 ids) or None.  Returns int32 [4,n]:
    rank_head, rank_tail, filtered_rank_head, filtered_rank_tail (0-based).  ties: optional int32 [2, n] that receives, per head /
    tail sweep, the number of other candidates whose energy equals the true one's (kge_eval_ranks_ties)."""
    if isinstance(desc, L.MurpDesc):
        return murp_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=ties)
    if isinstance(desc, L.ConvKBDesc):
        if ties is not None:
            ties.fill_(-1)   # not counted
        return convkb_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids)
    if isinstance(desc, L.TuckerDesc):
        return tucker_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=ties)
    if isinstance(desc, L.ProjeDesc):
        return proje_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=ties)
    if isinstance(desc, L.ConveDesc):
        return conve_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=ties)
    if isinstance(desc, L.HyperDesc):
        return hyper_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=ties)
    if isinstance(desc, L.InteracteDesc):
        return interacte_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=ties)
    if isinstance(desc, L.AcreDesc):
        return acre_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=ties)
    n = triples.shape[0]
    if workspace is None:
        workspace = eval_workspace(desc, n, triples.device)
    ranks = torch.empty((4, n), dtype=torch.int32, device=triples.device)
    args = _filter_csr_args(tail_off, tail_ids, head_off, head_ids)
    L.check(L.load().kge_eval_ranks_ties(ctypes.byref(desc), _ids(triples, "triples"), n, *args,
                                         _dev(workspace, torch.uint8, "workspace"), workspace.numel(),
                                         _dev(ranks, torch.int32, "ranks"),
                                         _dev(ties, torch.int32, "ties") if ties is not None else None, _stream()), "kge_eval_ranks")
    return ranks


def eval_ranks_grouped(desc, triples, group_of_triple, group_rel, qblocks, tail_off, tail_ids, head_off, head_ids, ties=None):
    """TransR: triples sorted by relation, several relation groups per call (kge_eval_ranks_grouped).  int32 [4,n]."""
    n, G = triples.shape[0], group_rel.shape[0]
    lib = L.load()
    nbytes = lib.kge_eval_grouped_workspace_bytes(ctypes.byref(desc), int(n), int(G))
    if nbytes == 0:
        L.check(-1, "kge_eval_grouped_workspace_bytes")
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=triples.device)
    ranks = torch.empty((4, n), dtype=torch.int32, device=triples.device)
    args = _filter_csr_args(tail_off, tail_ids, head_off, head_ids)
    L.check(lib.kge_eval_ranks_grouped_ties(ctypes.byref(desc), _ids(triples, "triples"), n,
                                            _dev(group_of_triple, torch.int32, "group_of_triple"), _ids(group_rel, "group_rel"), G,
                                            _dev(qblocks, torch.int32, "qblocks"), qblocks.shape[0], *args,
                                            _dev(workspace, torch.uint8, "workspace"), workspace.numel(),
                                            _dev(ranks, torch.int32, "ranks"),
                                            _dev(ties, torch.int32, "ties") if ties is not None else None, _stream()), "kge_eval_ranks_grouped")
    return ranks


def eval_sweep_scores(desc, triples, workspace=None):
    """float32 [2n, E]: row 2i = energies of (h_i, r_i, e) for all e, row 2i+1 = energies of (e, r_i, t_i)."""
    if isinstance(desc, L.MurpDesc):     # (float64 preds; one-sided entry point only: the two sides interleaved)
        both = torch.stack([murp_sweep_scores_side(desc, triples, 0), murp_sweep_scores_side(desc, triples, 1)], 1)
        return both.view(2 * triples.shape[0], desc.tot_entity)
    if isinstance(desc, L.ConvKBDesc):   # one-sided entry point only: the two sides interleaved
        both = torch.stack([convkb_sweep_scores_side(desc, triples, 0), convkb_sweep_scores_side(desc, triples, 1)], 1)
        return both.view(2 * triples.shape[0], desc.tot_entity)
    n = triples.shape[0]
    if workspace is None:
        workspace = eval_workspace(desc, n, triples.device)
    out = torch.empty((2 * n, desc.tot_entity), dtype=torch.float32, device=triples.device)
    L.check(L.load().kge_eval_sweep_scores(ctypes.byref(desc), _ids(triples, "triples"), n,
                                           _dev(workspace, torch.uint8, "workspace"), workspace.numel(),
                                           _dev(out, torch.float32, "scores"), _stream()), "kge_eval_sweep_scores")
    return out


def eval_sweep_scores_side(desc, triples, side, workspace=None):
    """float32 [n, E]: side 0 = energies of (h_i, r_i, e) for all e, side 1 = energies of (e, r_i, t_i); the other side's query
    is never swept (kge_eval_sweep_scores_side).  TransR / NTN / SLM compute both sides per call: the full sweep, sliced."""
    if isinstance(desc, L.MurpDesc):
        return murp_sweep_scores_side(desc, triples, side)
    if isinstance(desc, L.ConvKBDesc):
        return convkb_sweep_scores_side(desc, triples, side)
    if desc.model in (MODEL_IDS["transr"], MODEL_IDS["ntn"], MODEL_IDS["slm"]):
        return eval_sweep_scores(desc, triples, workspace)[int(side)::2]
    n = triples.shape[0]
    if workspace is None:
        workspace = eval_workspace(desc, n, triples.device)
    out = torch.empty((n, desc.tot_entity), dtype=torch.float32, device=triples.device)
    L.check(L.load().kge_eval_sweep_scores_side(ctypes.byref(desc), _ids(triples, "triples"), n, int(side),
                                                _dev(workspace, torch.uint8, "workspace"), workspace.numel(),
                                                _dev(out, torch.float32, "scores"), _stream()), "kge_eval_sweep_scores_side")
    return out


def rank_from_scores(scores, truth, off, ids):
    """scores float32 [nq, E] -> (rank, filtered rank) int32 [nq] given the true entity per row and a CSR of knowns."""
    nq, E = scores.shape
    rank = torch.empty(nq, dtype=torch.int32, device=scores.device)
    frank = torch.empty_like(rank)
    po = _dev(off, torch.int64, "csr offsets") if off is not None else None
    pi = _dev(ids, torch.int32, "csr ids") if ids is not None else None
    L.check(L.load().kge_rank_from_scores(_dev(scores, torch.float32, "scores"), nq, E, _ids(truth, "truth"), po, pi,
                                          _dev(rank, torch.int32, "rank"), _dev(frank, torch.int32, "frank"), _stream()),
            "kge_rank_from_scores")
    return rank, frank


def eval_ranks_via_forward(desc, triples, tail_off, tail_ids, head_off, head_ids, chunk=64):
    """The reference's own evaluation algorithm (utils/evaluator.py:254-272) on the device: every candidate triple
    goes through the batch scorer, `chunk` test triples x E candidates per kge_score_forward call, then
    kge_rank_from_scores.  Works for every model; kept as an independent cross-check of the sweep kernels (it is what
    tests compare the NTN MFMA sweep with).  int32 [4, n]."""
    n = triples.shape[0]
    E = desc.tot_entity
    dev = triples.device
    ents = torch.arange(E, dtype=torch.int64, device=dev)
    out = torch.empty((4, n), dtype=torch.int32, device=dev)
    for lo in range(0, n, chunk):
        tr = triples[lo:lo + chunk]
        m = tr.shape[0]
        h, r, t = tr[:, 0:1], tr[:, 1:2], tr[:, 2:3]
        cand = ents.view(1, E).expand(m, E)
        tail_scores = score_forward(desc, h.expand(m, E).reshape(-1).contiguous(), r.expand(m, E).reshape(-1).contiguous(),
                                    cand.reshape(-1).contiguous()).view(m, E)
        head_scores = score_forward(desc, cand.reshape(-1).contiguous(), r.expand(m, E).reshape(-1).contiguous(),
                                    t.expand(m, E).reshape(-1).contiguous()).view(m, E)
        to = (tail_off[lo:lo + m + 1]).contiguous() if tail_off is not None else None
        ho = (head_off[lo:lo + m + 1]).contiguous() if head_off is not None else None
        rt, frt = rank_from_scores(tail_scores, tr[:, 2].contiguous(), to, tail_ids)
        rh, frh = rank_from_scores(head_scores, tr[:, 0].contiguous(), ho, head_ids)
        out[0, lo:lo + m], out[1, lo:lo + m], out[2, lo:lo + m], out[3, lo:lo + m] = rh, rt, frh, frt
    return out


def _csr_two_pass(stem, sides, known, queries, tot_entity, tot_relation, names):
    """The two-pass device build behind filter_csr_build / relation_csr_build: kge_<stem>_count writes the `sides` offset arrays
    (int64 [n + 1], argument names `names`) and their totals, ONE host read sizes the id arrays, kge_<stem>_fill writes them.
    Returns (offsets, ids), a list per side; ids is None when there is nothing to count (no query or no known triple)."""
    n, M = int(queries.shape[0]), int(known.shape[0])
    dev = queries.device
    offs = [torch.zeros(n + 1, dtype=torch.int64, device=dev) for _ in range(sides)]
    if n == 0 or M == 0:
        return offs, None
    lib = L.load()
    count, fill = "kge_%s_count" % stem, "kge_%s_fill" % stem
    ws = torch.empty(getattr(lib, "kge_%s_workspace_bytes" % stem)(M, n), dtype=torch.uint8, device=dev)
    totals = torch.empty(sides, dtype=torch.int64, device=dev)
    p_offs = [_dev(o, torch.int64, name) for o, name in zip(offs, names)]
    L.check(getattr(lib, count)(_ids(known, "known triples"), M, _ids(queries, "queries"), n, int(tot_entity), int(tot_relation),
                                _dev(ws, torch.uint8, "workspace"), ws.numel(), *p_offs, _dev(totals, torch.int64, "totals"), _stream()), count)
    ids = [torch.empty(max(int(x), 1), dtype=torch.int32, device=dev)[:int(x)] for x in totals.tolist()]       # the one host read
    L.check(getattr(lib, fill)(_ids(queries, "queries"), n, M, _dev(ws, torch.uint8, "workspace"), *p_offs,
                               *[ctypes.c_void_p(i.data_ptr()) for i in ids], _stream()), fill)
    return offs, ids


def filter_csr_build(known, queries, tot_entity, tot_relation):
    """Per-query filter lists (tail_off int64 [n+1], tail_ids int32, head_off, head_ids) of `queries` [n, 3] against the set of
    `known` triples [M, 3] (train + valid + test), built on the device: kge_filter_csr_count / _fill.  One host read (the two list
    totals) between the calls."""
    (t_off, h_off), ids = _csr_two_pass("filter_csr", 2, known, queries, tot_entity, tot_relation, ("tail_off", "head_off"))
    if ids is None:
        empty = torch.empty(0, dtype=torch.int32, device=queries.device)
        return t_off, empty, h_off, empty.clone()
    return t_off, ids[0], h_off, ids[1]


TOPK_MAX = L.TOPK_MAX


def _skip_csr_args(n, skip_off, skip_ids, dev, sort=False, what="n"):
    """The per-query skip CSR as the library takes it: (skip_off pointer, skip_ids pointer, the id tensor the second pointer is
    of -- the caller holds it until its launch is queued), or (None, None, None) without lists.  n + 1 offsets; sort: make every
    segment ascending first (sort_skip_segments); an empty id array becomes a pointer the library accepts and never reads."""
    if (skip_off is None) != (skip_ids is None):
        raise ValueError("skip_off and skip_ids come together")
    if skip_off is None or n == 0:
        return None, None, None
    if skip_off.numel() != n + 1:
        raise ValueError("skip_off must hold %s + 1 = %d offsets (got %d)" % (what, n + 1, skip_off.numel()))
    if sort:
        skip_ids = sort_skip_segments(skip_off, skip_ids)
    if skip_ids.numel() == 0:
        skip_ids = torch.zeros(1, dtype=torch.int32, device=dev)
    return _dev(skip_off, torch.int64, "skip_off"), _dev(skip_ids, torch.int32, "skip_ids"), skip_ids


def _row_desc_triples(desc, triples, who, hint):
    """The shared opening of rank_candidates / rank_relations: a row-kernel descriptor, triples [n, 3]; (n, empty counts [4, n])."""
    if not isinstance(desc, L.ModelDesc):
        raise L.KgeHipError("%s: %s has no row kernels; rank it via-forward (the model's own forward over %s + rank_lists_from_scores, "
                            "as Evaluator.%s does)" % (who, type(desc).__name__, hint, who))
    if triples.dim() != 2 or triples.shape[1] != 3:
        raise ValueError("triples must be [n, 3]")
    n = int(triples.shape[0])
    return n, torch.empty((4, n), dtype=torch.int32, device=triples.device)


def topk_rows(scores, k, largest=False, skip_off=None, skip_ids=None, keep=None):
    """The k most plausible live candidates of every row of `scores` (float32 or float64 [nq, n_cand], unit inner stride, any row
    stride >= n_cand): (ids int32 [nq, k], values [nq, k], count int32 [nq]) in kge_topk_rows's total order -- better score first
    (lower unless `largest`), lower id first among equal scores, NaN last.  Candidate c of row q is masked when it is in
    skip_ids[skip_off[q] : skip_off[q + 1]] (int32 ids, int64 offsets [nq + 1]) and differs from keep[q] (int64 [nq], optional);
    rows with fewer than k live candidates are padded with id -1 and NaN."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
        raise TypeError("scores must be a 2-D tensor")
    if scores.dtype not in (torch.float32, torch.float64):
        raise TypeError("scores must be float32 or float64 (got %s)" % scores.dtype)
    if not scores.is_cuda:
        raise L.KgeHipError("scores must live on the HIP device (got %s); the HIP path has no CPU fallback" % scores.device)
    k = int(k)
    if not 1 <= k <= TOPK_MAX:
        raise ValueError("k = %d outside 1..%d (KGE_TOPK_MAX)" % (k, TOPK_MAX))
    nq, n_cand = (int(x) for x in scores.shape)
    if n_cand > 1 and scores.stride(1) != 1:
        raise ValueError("scores must have unit inner stride (got %d)" % scores.stride(1))
    row_stride = int(scores.stride(0)) if nq > 1 else n_cand
    dev = scores.device
    ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    vals = torch.empty((nq, k), dtype=scores.dtype, device=dev)
    count = torch.empty(nq, dtype=torch.int32, device=dev)
    if nq == 0:
        return ids, vals, count
    lib = L.load()
    pk = pw = None
    nbytes = 0
    po, pi, skip_ids = _skip_csr_args(nq, skip_off, skip_ids, dev, what="nq")
    if po is not None:
        if keep is not None:
            if keep.numel() != nq:
                raise ValueError("keep must hold one id per row (%d, got %d)" % (nq, keep.numel()))
            pk = _dev(keep, torch.int64, "keep")
        nbytes = lib.kge_topk_workspace_bytes(nq, n_cand, 1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        pw = ctypes.c_void_p(ws.data_ptr())
    L.check(lib.kge_topk_rows(ctypes.c_void_p(scores.data_ptr()), 1 if scores.dtype == torch.float64 else 0, nq, n_cand, row_stride, k,
                              1 if largest else 0, po, pi, pk, pw, nbytes, _dev(ids, torch.int32, "out_ids"),
                              ctypes.c_void_p(vals.data_ptr()), _dev(count, torch.int32, "out_count"), _stream()), "kge_topk_rows")
    return ids, vals, count


KNN_MAX = L.KNN_MAX
KNN_METRICS = L.KNN_METRICS


def _knn_rows_arg(t, what):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise TypeError("%s must be a 2-D tensor" % what)
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s)" % (what, t.dtype))
    if not t.is_cuda:
        raise L.KgeHipError("%s must live on the HIP device (got %s); the HIP path has no CPU fallback" % (what, t.device))
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError("%s must have unit inner stride (got %d)" % (what, t.stride(1)))
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def knn_metric(metric):
    if metric not in KNN_METRICS:
        raise ValueError("metric = %r (one of %s)" % (metric, ", ".join(sorted(KNN_METRICS))))
    return KNN_METRICS[metric]


def knn_rows(table, queries, k, metric="cosine", self_ids=None):
    """The k nearest live rows of `table` (float32 [n_rows, dim], unit inner stride, any row stride >= dim) for every row of `queries`
    (float32 [nq, dim], likewise): (ids int32 [nq, k], scores float32 [nq, k], count int32 [nq]) in kge_knn_rows's total order --
    nearer first ("dot" and "cosine": the higher score, "l2": the lower Euclidean distance), lower id first among equal scores, NaN
    last.  Candidate self_ids[q] (int64 [nq], -1 = none) is not live for row q; rows with fewer than k live candidates are padded
    with id -1 and NaN.  The select runs inside the matrix-core sweep (csrc/kge_knn.hip): no [nq, n_rows] block is written."""
    tstride = _knn_rows_arg(table, "table")
    qstride = _knn_rows_arg(queries, "queries")
    if queries.device != table.device:
        raise ValueError("table and queries live on different devices")
    k = int(k)
    if not 1 <= k <= KNN_MAX:
        raise ValueError("k = %d outside 1..%d (KGE_KNN_MAX)" % (k, KNN_MAX))
    code = knn_metric(metric)
    n_rows, dim = (int(x) for x in table.shape)
    nq = int(queries.shape[0])
    if int(queries.shape[1]) != dim:
        raise ValueError("queries have %d columns, the table %d" % (queries.shape[1], dim))
    dev = table.device
    ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    vals = torch.empty((nq, k), dtype=torch.float32, device=dev)
    count = torch.empty(nq, dtype=torch.int32, device=dev)
    if nq == 0:
        return ids, vals, count
    ps = None
    if self_ids is not None:
        if self_ids.numel() != nq:
            raise ValueError("self_ids must hold one id per query (%d, got %d)" % (nq, self_ids.numel()))
        ps = _dev(self_ids, torch.int64, "self_ids")
    lib = L.load()
    nbytes = lib.kge_knn_workspace_bytes(nq, n_rows, dim, k, code)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.kge_knn_rows(ctypes.c_void_p(table.data_ptr()), n_rows, dim, tstride, ctypes.c_void_p(queries.data_ptr()), nq, qstride, ps,
                             k, code, ctypes.c_void_p(ws.data_ptr()), nbytes, _dev(ids, torch.int32, "out_ids"),
                             _dev(vals, torch.float32, "out_scores"), _dev(count, torch.int32, "out_count"), _stream()), "kge_knn_rows")
    return ids, vals, count


def knn_workspace_bytes(nq, n_rows, dim, k, metric="cosine"):
    """Bytes of workspace a knn_rows call of this shape allocates (kge_knn_workspace_bytes): what the Evaluator chunks its queries by."""
    return int(L.load().kge_knn_workspace_bytes(int(nq), int(n_rows), int(dim), int(k), knn_metric(metric)))


# --- t-SNE projection (csrc/kge_tsne.hip): affinities from the search's neighbour lists, the joint CSR, the gradient, the descent loop
TSNE_TILE = L.TSNE_TILE


class TsneCSR(collections.namedtuple("TsneCSR", "row_off col val n")):
    """The joint probabilities P of a t-SNE run: row_off int64 [n + 1], col int32 [nnz] (ascending within a row, no diagonal, no
    duplicate), val float32 [nnz]."""
    __slots__ = ()

    @property
    def nnz(self):
        return int(self.col.numel())


def _tsne_dev(t, dtype, shape, what):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError("%s must be a %s tensor" % (what, dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be %s (got %s)" % (what, list(shape), list(t.shape)))
    if not t.is_cuda:
        raise L.KgeHipError("%s must live on the HIP device (got %s); the HIP path has no CPU fallback" % (what, t.device))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    return ctypes.c_void_p(t.data_ptr())


def tsne_affinities(ids, dist, count, perplexity):
    """(cond_p float32 [n, k], beta float32 [n]): the conditional probabilities p_{j|i} of every row's neighbours at the given
    perplexity (kge_tsne_affinities).  ids [n, k], dist float32 [n, k] (Euclidean) and count int32 [n] are knn_rows's output under
    metric="l2"; places from count[i] on get 0."""
    if not isinstance(dist, torch.Tensor) or dist.dim() != 2:
        raise TypeError("dist must be a 2-D tensor")
    n, k = (int(x) for x in dist.shape)
    if tuple(ids.shape) != (n, k):
        raise ValueError("ids %s and dist %s differ in shape" % (list(ids.shape), [n, k]))
    if not 1 <= k <= KNN_MAX:
        raise ValueError("k = %d outside 1..%d (KGE_KNN_MAX)" % (k, KNN_MAX))
    pd = _tsne_dev(dist, torch.float32, (n, k), "dist")
    pc = _tsne_dev(count, torch.int32, (n,), "count")
    cond_p = torch.empty((n, k), dtype=torch.float32, device=dist.device)
    beta = torch.empty(n, dtype=torch.float32, device=dist.device)
    L.check(L.load().kge_tsne_affinities(pd, pc, n, k, float(perplexity), ctypes.c_void_p(cond_p.data_ptr()),
                                         ctypes.c_void_p(beta.data_ptr()), _stream()), "kge_tsne_affinities")
    return cond_p, beta


def tsne_joint(ids, cond_p, count):
    """TsneCSR of P_ij = (p_{j|i} + p_{i|j}) / (2 n) over the union of the two neighbour graphs: ONE sort of the 64-bit (i, j) keys of
    both directions on the tensors' device.  A key occurs at most twice (a row's ids are distinct) and a sum of two floats does not
    depend on their order, so P is symmetric bit for bit and the same on every run.  One-time set-up in torch ops; nnz is read."""
    n, k = (int(x) for x in ids.shape)
    dev = ids.device
    ids64 = ids.to(torch.int64)
    rows = torch.arange(n, dtype=torch.int64, device=dev).view(-1, 1).expand(n, k)
    live = (torch.arange(k, dtype=torch.int64, device=dev).view(1, -1) < count.view(-1, 1).to(torch.int64)) & (ids64 >= 0) & (ids64 != rows)
    i, j, p = rows[live], ids64[live], cond_p[live]
    keys, order = torch.sort(torch.cat([i * n + j, j * n + i]))
    vals = torch.cat([p, p])[order]
    first = torch.ones_like(keys, dtype=torch.bool)
    first[1:] = keys[1:] != keys[:-1]
    pair = torch.zeros_like(vals)
    pair[:-1] = torch.where(first[1:], torch.zeros_like(vals[1:]), vals[1:])     # the key's second entry, if it has one
    keys, vals = keys[first], (vals + pair)[first] / float(2 * n)
    row_off = torch.searchsorted(keys, torch.arange(n + 1, dtype=torch.int64, device=dev) * n)
    return TsneCSR(row_off.contiguous(), (keys % n).to(torch.int32).contiguous(), vals.contiguous(), n)


def _tsne_csr_args(csr, Y, what):
    n = int(csr.n)
    pY = _tsne_dev(Y, torch.float32, (n, 2), what)
    nnz = csr.nnz
    if int(csr.val.numel()) != nnz:
        raise ValueError("csr: col holds %d entries, val %d" % (nnz, csr.val.numel()))
    return (n, pY, _tsne_dev(csr.row_off, torch.int64, (n + 1,), "csr.row_off"), _tsne_dev(csr.col, torch.int32, (nnz,), "csr.col"),
            _tsne_dev(csr.val, torch.float32, (nnz,), "csr.val"), nnz)


def tsne_workspace_bytes(n):
    return int(L.load().kge_tsne_workspace_bytes(int(n)))


def tsne_gradient(csr, Y, exaggeration=1.0, want_kl=False):
    """(grad float32 [n, 2], Z float64 [], KL float64 [] or None) of the t-SNE objective at the map Y float32 [n, 2] under the joint
    probabilities `csr` (kge_tsne_gradient): the exact all-pairs gradient, every sum in a fixed order."""
    n, pY, pr, pc, pv, nnz = _tsne_csr_args(csr, Y, "Y")
    dev = Y.device
    lib = L.load()
    nbytes = lib.kge_tsne_workspace_bytes(n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    grad = torch.empty((n, 2), dtype=torch.float32, device=dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    L.check(lib.kge_tsne_gradient(pY, n, pr, pc, pv, nnz, float(exaggeration), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                  ctypes.c_void_p(grad.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                  ctypes.c_void_p(out.data_ptr() + 8) if want_kl else None, _stream()), "kge_tsne_gradient")
    return grad, out[0], (out[1] if want_kl else None)


def tsne_state(Y):
    """(update, gains) a descent starts from: zeros and ones, float32 [n, 2]."""
    return torch.zeros_like(Y), torch.ones_like(Y)


def tsne_run(csr, Y, n_iter, it0=0, exaggeration=1.0, momentum=0.8, learning_rate=200.0, record_every=0, update=None, gains=None,
             trace=None):
    """Iterations [it0, it0 + n_iter) of the t-SNE descent in one C loop (kge_tsne_run): no Python per iteration, no host read.  Y
    float32 [n, 2] is updated IN PLACE, and so are update and gains (tsne_state(Y) when not given): all of a run's state is in
    these three tensors, so a run cut into several calls leaves the bits of one.  Iteration `it` is recorded when
    (it + 1) % record_every == 0: trace[(it + 1) // record_every - 1] = (KL, |grad|_2) of the Y it started from (float64
    [records, 2], NaN where nothing was written; created for it0 + n_iter iterations when not given).  -> (Y, trace)."""
    n, pY, pr, pc, pv, nnz = _tsne_csr_args(csr, Y, "Y")
    dev = Y.device
    update = torch.zeros_like(Y) if update is None else update
    gains = torch.ones_like(Y) if gains is None else gains
    n_iter, it0, record_every = int(n_iter), int(it0), int(record_every)
    records = (it0 + n_iter) // record_every if record_every > 0 else 0
    if trace is None:
        trace = torch.full((records, 2), float("nan"), dtype=torch.float64, device=dev)
    pt = _tsne_dev(trace, torch.float64, (int(trace.shape[0]), 2), "trace") if trace.numel() else None
    lib = L.load()
    nbytes = lib.kge_tsne_workspace_bytes(n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    tmp = torch.empty_like(Y)
    L.check(lib.kge_tsne_run(pY, ctypes.c_void_p(tmp.data_ptr()), _tsne_dev(update, torch.float32, (n, 2), "update"),
                             _tsne_dev(gains, torch.float32, (n, 2), "gains"), n, pr, pc, pv, nnz, it0, it0 + n_iter, float(exaggeration),
                             float(momentum), float(learning_rate), record_every, pt, int(trace.shape[0]),
                             ctypes.c_void_p(ws.data_ptr()), nbytes, _stream()), "kge_tsne_run")
    return Y, trace


CAND_CHUNK = L.CAND_CHUNK


def sort_skip_segments(skip_off, skip_ids):
    """skip_ids with every segment skip_ids[skip_off[i] : skip_off[i + 1]] ascending, the CSR layout kept: ONE torch.sort of
    (segment index, id) keys on the device, no host read."""
    total = int(skip_ids.numel())
    if total == 0:
        return skip_ids
    pos = torch.arange(total, dtype=torch.int64, device=skip_ids.device)
    seg = torch.searchsorted(skip_off.contiguous(), pos, right=True)      # entries of segment i get i + 1: monotone in the position
    keys = (seg << 32) + (skip_ids.to(torch.int64) + (1 << 31))
    keys = torch.sort(keys).values
    return ((keys & 0xffffffff) - (1 << 31)).to(torch.int32)


def rank_candidates(desc, triples, side, cand_off, cand_ids, list_of_query=None, skip_off=None, skip_ids=None, skip_sorted=False):
    """Where the true entity of every triple stands among the ids of its candidate list (kge_rank_candidates): int32 [4, n] =
    #better, #better under the filter, #tied, #tied under the filter (0-based, optimistic end, ties bit for bit).  triples int64
    [n, 3]; side 0 ranks tails, 1 ranks heads; lists as a CSR (cand_off int64 [n_lists + 1], cand_ids int32), query i uses list
    list_of_query[i] (int64 [n]) or list i.  Entries equal to the true entity or outside [0, tot_entity) are ignored (-1 pads).
    skip_off / skip_ids: per-query CSR of known entities to leave out; the segments are sorted here (sort_skip_segments) unless
    skip_sorted says they already are ascending."""
    n, counts = _row_desc_triples(desc, triples, "rank_candidates", "the expanded triples")
    dev = triples.device
    n_lists = int(cand_off.numel()) - 1
    if list_of_query is not None and list_of_query.numel() != n:
        raise ValueError("list_of_query must hold one list index per query (%d, got %d)" % (n, list_of_query.numel()))
    po, pi, skip_ids = _skip_csr_args(n, skip_off, skip_ids, dev, sort=not skip_sorted)
    if n == 0:
        return counts
    lib = L.load()
    if cand_ids.numel() == 0:   # every list is empty: a pointer the library accepts, never read
        cand_ids = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = lib.kge_rank_candidates_workspace_bytes(n, n_lists, int(cand_ids.numel()))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.kge_rank_candidates(ctypes.byref(desc), _ids(triples, "triples"), n, int(side),
                                    _ids(list_of_query, "list_of_query") if list_of_query is not None else None,
                                    _dev(cand_off, torch.int64, "cand_off"), _dev(cand_ids, torch.int32, "cand_ids"), n_lists, po, pi,
                                    ctypes.c_void_p(ws.data_ptr()), nbytes, _dev(counts, torch.int32, "counts"), _stream()),
            "kge_rank_candidates")
    return counts


def rank_lists_from_scores(scores, truth_scores, seg_off, flags=None, largest=False):
    """The counts of rank_candidates from scores computed elsewhere (kge_rank_lists_from_scores): segment i of `scores` (float32 or
    float64, 1-D) = scores[seg_off[i] : seg_off[i + 1]] against truth_scores[i]; flags uint8 per score (bit 0 live, bit 1 live under
    the filter; None: all set); better = lower unless `largest`.  int32 [4, n]."""
    if scores.dtype not in (torch.float32, torch.float64) or truth_scores.dtype != scores.dtype:
        raise TypeError("scores and truth_scores must both be float32 or both float64 (got %s, %s)" % (scores.dtype, truth_scores.dtype))
    n = int(truth_scores.numel())
    if seg_off.numel() != n + 1:
        raise ValueError("seg_off must hold n + 1 = %d offsets (got %d)" % (n + 1, seg_off.numel()))
    dev = truth_scores.device
    counts = torch.empty((4, n), dtype=torch.int32, device=dev)
    if n == 0:
        return counts
    if scores.numel() == 0:
        scores = torch.zeros(1, dtype=scores.dtype, device=dev)
    if flags is not None and flags.numel() == 0:
        flags = None
    L.check(L.load().kge_rank_lists_from_scores(_dev(scores, scores.dtype, "scores"), 1 if scores.dtype == torch.float64 else 0,
                                                _dev(truth_scores, scores.dtype, "truth_scores"), _dev(seg_off, torch.int64, "seg_off"), n,
                                                _dev(flags, torch.uint8, "flags") if flags is not None else None, 1 if largest else 0,
                                                _dev(counts, torch.int32, "counts"), _stream()), "kge_rank_lists_from_scores")
    return counts


REL_CHUNK = L.REL_CHUNK


def relation_csr_build(known, queries, tot_entity, tot_relation):
    """Per query (h, ., t) of `queries` [n, 3] the distinct relations r with (h, r, t) in `known` [M, 3] (train + valid + test),
    ascending: (rel_off int64 [n + 1], rel_ids int32), built on the device with kge_relation_csr_count / _fill.  One host read (the
    list total) between the calls."""
    (off,), ids = _csr_two_pass("relation_csr", 1, known, queries, tot_entity, tot_relation, ("rel_off",))
    return off, torch.empty(0, dtype=torch.int32, device=queries.device) if ids is None else ids[0]


def rank_relations(desc, triples, skip_off=None, skip_ids=None, skip_sorted=False):
    """Where the true relation of every triple stands among all relations (kge_rank_relations): int32 [4, n] = #better, #better under
    the filter, #tied, #tied under the filter (0-based, optimistic end, ties bit for bit).  triples int64 [n, 3]; the number of
    relations is the descriptor's.  skip_off / skip_ids: per-query CSR of the relations known for the pair (h, t), left out of rows
    1 and 3; the segments are sorted here (sort_skip_segments) unless skip_sorted says they already are ascending."""
    n, counts = _row_desc_triples(desc, triples, "rank_relations", "the triples of every other relation")
    dev = triples.device
    po, pi, skip_ids = _skip_csr_args(n, skip_off, skip_ids, dev, sort=not skip_sorted)
    if n == 0:
        return counts
    lib = L.load()
    nbytes = lib.kge_rank_relations_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.kge_rank_relations(ctypes.byref(desc), _ids(triples, "triples"), n, po, pi, ctypes.c_void_p(ws.data_ptr()), nbytes,
                                   _dev(counts, torch.int32, "counts"), _stream()), "kge_rank_relations")
    return counts


TYPED_ATTEMPTS, TYPED_UNIFORM_ATTEMPTS = L.TYPED_ATTEMPTS, L.TYPED_UNIFORM_ATTEMPTS


def classification_fit(scores, rel, label, n_relations, higher_is_better=False):
    """Per-relation classification thresholds of labelled scores (kge_classification_fit): (thr int64 [R], fit int64 [R, 6]).
    scores float32 [n], rel int64 [n], label uint8 [n] (non-zero = true triple).  thr[r] is a KEY (include/kge_hip.h), -1 = nothing is
    positive; fit[r] = {positives, negatives, correct at the chosen cut, AUC wins, AUC ties, 0}.  Exact and bit-identical run to run."""
    n, R = int(scores.numel()), int(n_relations)
    if rel.numel() != n or label.numel() != n:
        raise ValueError("scores, rel and label hold %d, %d and %d elements: one of each per triple" % (n, rel.numel(), label.numel()))
    dev = scores.device
    lib = L.load()
    thr = torch.empty(max(R, 0), dtype=torch.int64, device=dev)
    fit = torch.empty((max(R, 0), 6), dtype=torch.int64, device=dev)
    nbytes = lib.kge_classification_fit_workspace_bytes(n, R)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    L.check(lib.kge_classification_fit(_dev(scores, torch.float32, "scores"), _ids(rel, "rel"), _dev(label, torch.uint8, "label"), n, R,
                                       1 if higher_is_better else 0, _dev(ws, torch.uint8, "workspace"), nbytes,
                                       _ids(thr, "thr"), _ids(fit, "fit"), _stream()), "kge_classification_fit")
    return thr, fit


def classification_apply(scores, rel, thr, seen, thr_global, label=None, higher_is_better=False):
    """Classify scores against fitted thresholds (kge_classification_apply): (pred uint8 [n], conf int64 [R, 4] = {tp, fp, tn, fn} per
    relation, or None without labels).  thr int64 [R]; seen uint8 [R]: 0 = the relation had no validation triple and uses thr_global."""
    n, R = int(scores.numel()), int(thr.numel())
    if rel.numel() != n or (label is not None and label.numel() != n):
        raise ValueError("scores, rel and label must hold one element per triple")
    if seen.numel() != R:
        raise ValueError("seen holds %d flags for %d thresholds" % (seen.numel(), R))
    dev = scores.device
    pred = torch.empty(n, dtype=torch.uint8, device=dev)
    conf = None if label is None else torch.empty((R, 4), dtype=torch.int64, device=dev)
    L.check(L.load().kge_classification_apply(_dev(scores, torch.float32, "scores"), _ids(rel, "rel"),
                                              None if label is None else _dev(label, torch.uint8, "label"), n, R,
                                              1 if higher_is_better else 0, _ids(thr, "thr"), _dev(seen, torch.uint8, "seen"),
                                              int(thr_global), _dev(pred, torch.uint8, "pred"),
                                              None if conf is None else _ids(conf, "conf"), _stream()), "kge_classification_apply")
    return pred, conf


def corrupt_typed(ph, pr, pt, tot_entity, tot_relation, bern_prob, type_off, type_ids, slots, seed, offset):
    """One classification negative per positive (kge_corrupt_typed): (neg int64 [n, 3], n_failed int64 [1], both on the device).
    type_off int64 [2, R + 1] (row 0 = heads, row 1 = tails) + type_ids int32: the per-relation lists the replacement is drawn from;
    slots: the packed set of every known triple (triple_set_build), or None.  A row whose draws were all rejected carries -1 in the
    corrupted column and counts into n_failed: the redraw loop is bounded."""
    n = int(ph.numel())
    dev = ph.device
    if tuple(type_off.shape) != (2, int(tot_relation) + 1):
        raise ValueError("type_off must be [2, tot_relation + 1] (got %s)" % (tuple(type_off.shape),))
    if type_ids.numel() == 0:   # every list is empty: a pointer the library accepts, never read
        type_ids = torch.zeros(1, dtype=torch.int32, device=dev)
    neg = torch.empty((n, 3), dtype=torch.int64, device=dev)
    failed = torch.empty(1, dtype=torch.int64, device=dev)
    bp = _dev(bern_prob, torch.float32, "bern_prob") if bern_prob is not None else None
    sp = ctypes.c_void_p(slots.data_ptr()) if slots is not None else None
    L.check(L.load().kge_corrupt_typed(_ids(ph, "ph"), _ids(pr, "pr"), _ids(pt, "pt"), n, int(tot_entity), int(tot_relation), bp,
                                       _ids(type_off, "type_off"), _dev(type_ids, torch.int32, "type_ids"), sp,
                                       slots.numel() if slots is not None else 0, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                                       _ids(neg, "neg"), _ids(failed, "n_failed"), _stream()), "kge_corrupt_typed")
    return neg, failed


def triple_set_build(triples):
    """Open-addressing hash set of the train triples (uint64 slots, power of two >= 2n)."""
    n = triples.shape[0]
    if n:  # packed key h:24 | r:16 | t:24 (csrc/kge_sampler_device.h): out-of-range ids would alias silently
        _ids(triples, "triples")
        hi = triples.max(dim=0).values.tolist()
        if triples.min().item() < 0 or max(hi[0], hi[2]) >= 1 << 24 or hi[1] >= 1 << 16:
            raise L.KgeHipError("kge_triple_set_build: ids exceed the packed key (entities < 2^24, relations < 2^16): "
                                "max h/r/t = %s" % hi)
    n_slots = 1 << max(4, math.ceil(math.log2(max(2 * n, 2))))
    slots = torch.empty(n_slots, dtype=torch.int64, device=triples.device)  # uint64 payload
    L.check(L.load().kge_triple_set_build(_ids(triples, "triples"), n, ctypes.c_void_p(slots.data_ptr()), n_slots,
                                          _stream()), "kge_triple_set_build")
    return slots


def corrupt(ph, pr, pt, neg_rate, tot_entity, bern_prob, slots, seed, offset):
    n = ph.numel()
    nh = torch.empty(n * neg_rate, dtype=torch.int64, device=ph.device)
    nr = torch.empty_like(nh)
    nt = torch.empty_like(nh)
    bp = _dev(bern_prob, torch.float32, "bern_prob") if bern_prob is not None else None
    sp = ctypes.c_void_p(slots.data_ptr()) if slots is not None else None
    L.check(L.load().kge_corrupt(_ids(ph, "ph"), _ids(pr, "pr"), _ids(pt, "pt"), n, int(neg_rate), int(tot_entity), bp,
                                 sp, slots.numel() if slots is not None else 0, int(seed) & (2 ** 64 - 1),
                                 int(offset) & (2 ** 64 - 1), _ids(nh, "nh"), _ids(nr, "nr"), _ids(nt, "nt"),
                                 _stream()), "kge_corrupt")
    return nh, nr, nt


def sample_buffer(n_pos, neg_rate, pointwise, device):
    rows = 4 * n_pos * (1 + neg_rate) if pointwise else 3 * n_pos * (1 + neg_rate)
    return torch.empty(rows, dtype=torch.int64, device=device)


def sample_batch(triples, perm, start, n_pos, neg_rate, tot_entity, bern_prob, slots, seed, offset, pointwise=False,
                 out=None, cursor=None):
    """One launch: positives triples[perm[start:start+n_pos]] + their corrupted negatives, in the reference's batch
    layout (pairwise: [ph, pr, pt, nh, nr, nt]; pointwise: [h, r, t, y]).  `out`: optional preallocated
    sample_buffer (static addresses for hipGraph capture); `cursor`: optional device {start, offset} added to the
    host arguments."""
    dev = triples.device
    bp = _dev(bern_prob, torch.float32, "bern_prob") if bern_prob is not None else None
    sp = ctypes.c_void_p(slots.data_ptr()) if slots is not None else None
    pc = _dev(cursor, torch.int64, "cursor") if cursor is not None else None
    if pointwise:
        rows = n_pos * (1 + neg_rate)
        buf = (out if out is not None else torch.empty(4 * rows, dtype=torch.int64, device=dev)).view(4, rows)
        outs = [buf[0], buf[1], buf[2], buf[3]]
        ptrs = [ctypes.c_void_p(o.data_ptr()) for o in outs] + [None, None]
    else:
        nneg = n_pos * neg_rate
        buf = out if out is not None else torch.empty(3 * n_pos + 3 * nneg, dtype=torch.int64, device=dev)
        outs = [buf[0:n_pos], buf[n_pos:2 * n_pos], buf[2 * n_pos:3 * n_pos], buf[3 * n_pos:3 * n_pos + nneg],
                buf[3 * n_pos + nneg:3 * n_pos + 2 * nneg], buf[3 * n_pos + 2 * nneg:]]
        ptrs = [ctypes.c_void_p(o.data_ptr()) for o in outs]
    L.check(L.load().kge_sample_batch(_ids(triples, "triples"), _ids(perm, "perm"), int(start), int(n_pos), int(neg_rate),
                                      int(tot_entity), bp, sp, slots.numel() if slots is not None else 0,
                                      int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), 1 if pointwise else 0,
                                      *ptrs, pc, _stream()), "kge_sample_batch")
    return outs


# ---------------------------------------------------------------------------- owner-computes ("pull") training step
def _i32(t, what):
    return _dev(t, torch.int32, what)


def _ptr_pair(tensors):
    """float* const x[2] argument: a 2-slot pointer array (kept alive by the caller for the duration of the call)."""
    arr = (ctypes.c_void_p * 2)()
    for i in range(2):
        arr[i] = tensors[i].data_ptr() if tensors is not None and tensors[i] is not None else None
    return arr


def row_norms(table, out, hat=None):
    """out[r] = ||table[r]||_2 and hat[r] = table[r] / max(norm, 1e-12), in the lane layout / operation order the pull
    step uses for the rows it writes."""
    L.check(L.load().kge_row_norms(_dev(table, torch.float32, "table"), table.shape[0], table.shape[1],
                                   _dev(out, torch.float32, "norms"),
                                   _dev(hat, torch.float32, "normalised") if hat is not None else None, _stream()),
            "kge_row_norms")


def pull_partial_stride(dim):
    return int(L.load().kge_pull_partial_stride(int(dim)))


def pull_hat_stride(dim):
    """Floats between consecutive rows of the owner-computes step's normalised ("hat") tables."""
    return int(L.load().kge_pull_hat_stride(int(dim)))


def pull_groups_per_block(dim):
    return int(L.load().kge_pull_groups_per_block(int(dim)))


class PullListSet:
    """One kge_pull_lists set: per-step sampler output of the owner-computes steps (count all 0 / head all -1 between steps),
    incl. the ready-made visit descriptors (sdesc: one per static incidence, dbucket: one per bucket entry)."""

    def __init__(self, batch_size, tot_entity, device):
        self.pc = torch.empty(batch_size, dtype=torch.int32, device=device)
        self.next = torch.empty(batch_size, dtype=torch.int32, device=device)
        self.count = torch.zeros(tot_entity, dtype=torch.int32, device=device)
        self.bucket = torch.empty(tot_entity * L.PULL_BUCKET, dtype=torch.int32, device=device)
        self.head = torch.full((tot_entity,), -1, dtype=torch.int32, device=device)
        self.sdesc = torch.empty(3 * batch_size, 4, dtype=torch.int32, device=device)
        self.dbucket = torch.empty(tot_entity * L.PULL_BUCKET, 4, dtype=torch.int32, device=device)
        self.c = L.PullLists(self.pc.data_ptr(), self.count.data_ptr(), self.bucket.data_ptr(), self.head.data_ptr(),
                             self.next.data_ptr(), self.sdesc.data_ptr(), self.dbucket.data_ptr())

    def clear(self):
        self.count.zero_()
        self.head.fill_(-1)


def pull_sample(pairs, inv, tot_entity, bern_prob, slots, seed, offset, lists, cursor=None):
    """Draw the corruption of every pair of a batch (the draws kge_sample_batch makes for the same seed / offset) and
    register each pair with the entity it drew (`lists`: a cleared PullListSet)."""
    bp = _dev(bern_prob, torch.float32, "bern_prob") if bern_prob is not None else None
    sp = ctypes.c_void_p(slots.data_ptr()) if slots is not None else None
    pcur = _dev(cursor, torch.int64, "cursor") if cursor is not None else None
    L.check(L.load().kge_pull_sample(_i32(pairs, "pairs"), _i32(inv, "inv"), pairs.shape[0], int(tot_entity), bp, sp,
                                     slots.numel() if slots is not None else 0, int(seed) & (2 ** 64 - 1),
                                     int(offset) & (2 ** 64 - 1), pcur, ctypes.byref(lists.c), _stream()), "kge_pull_sample")


def pull_lists_explicit(pairs, inv, nh, nt, lists):
    if debug_enabled():   # (the entry point is not told the entity count; the list set is sized by it)
        check_ids(nh, lists.count.numel(), "negative heads")
        check_ids(nt, lists.count.numel(), "negative tails")
    L.check(L.load().kge_pull_lists_explicit(_i32(pairs, "pairs"), _i32(inv, "inv"), _ids(nh, "nh"), _ids(nt, "nt"), pairs.shape[0],
                                             ctypes.byref(lists.c), _stream()), "kge_pull_lists_explicit")


class PullDirection:
    """Scratch of the two-phase ("staged direction") form of the owner-computes step (struct kge_pull_direction): one record and
    two direction codes per pair of the batch."""

    def __init__(self, n_pairs, dim, l1, device):
        cb, rb = ctypes.c_size_t(), ctypes.c_size_t()
        L.check(L.load().kge_pull_direction_bytes(int(dim), 1 if l1 else 0, int(n_pairs), ctypes.byref(cb), ctypes.byref(rb)),
                "kge_pull_direction_bytes")
        self.codes = torch.zeros(max(1, cb.value), dtype=torch.uint8, device=device)
        self.recs = torch.zeros(max(4, rb.value // 4), dtype=torch.float32, device=device)
        self.c = L.PullDirection(self.codes.data_ptr(), self.recs.data_ptr(), int(n_pairs), 0)


def _next_sampler_args(sample_next):
    """The nine ride-along sampler arguments of kge_pull_step / kge_transx_grad_step / kge_own_step, from
    sample_next = (next_pairs, next_inv, bern_prob, slots, seed, next_offset, next_lists) or None (no sampler rides along)."""
    if sample_next is None:
        return (None, None, 0, None, None, 0, 0, 0, None)
    npairs, ninv, bern, slots, seed, noff, nlists = sample_next
    return (_i32(npairs, "next_pairs"), _i32(ninv, "next_inv"), npairs.shape[0], _dev(bern, torch.float32, "bern_prob") if bern is not None else None,
            ctypes.c_void_p(slots.data_ptr()) if slots is not None else None, slots.numel() if slots is not None else 0,
            int(seed) & (2 ** 64 - 1), int(noff) & (2 ** 64 - 1), ctypes.byref(nlists.c))


def _prepared(fn, name, args, off_idx, keep):
    """Marshal once, call many times: call(next_offset) repeats fn(*args) with only args[off_idx] -- the ride-along sampler's
    Philox offset, the one argument that differs from epoch to epoch -- replaced.  `keep` holds the arguments' storage alive."""
    args = list(args)

    def call(next_offset=None):
        if next_offset is not None:
            args[off_idx] = int(next_offset) & (2 ** 64 - 1)
        L.check(fn(*args, _stream()), name)
    call.keep = keep
    return call


def pull_step(desc_in, tables_out, hat_in, hat_out, norm_in, norm_out, state1, state2, pairs, lists, items, inc, partials, multi,
              margin, optimizer, lr, step, loss_buf, reset_lists=True, dev_hyper=None, run_finish=True, sample_next=None,
              dense_skip=None, prepare_only=False, direction=None):
    """One whole training step (scoring, hinge, backward, dense optimiser) without atomics: see csrc/kge_pull.hip.
    desc_in: descriptor over the tables READ; tables_out: [ent, rel] of the other half of the double buffer; hat_in /
    hat_out: the row-normalised copies of both halves.
    sample_next = (next_pairs, next_inv, bern_prob, slots, seed, next_offset, next_lists): the sampler of the next batch rides
    in this launch and fills `next_lists` (a cleared second PullListSet)."""
    to, s1, s2, hi, ho = _ptr_pair(tables_out), _ptr_pair(state1), _ptr_pair(state2), _ptr_pair(hat_in), _ptr_pair(hat_out)
    # run_finish=False (timing only): the owners still write their partial sums, the finishing launch is skipped
    n_multi = multi.shape[0] if (multi is not None and run_finish) else 0
    nx = _next_sampler_args(sample_next)
    args = (
        ctypes.byref(desc_in), ctypes.addressof(to), ctypes.addressof(hi), ctypes.addressof(ho) if hat_out is not None else None,
        _dev(norm_in, torch.float32, "norm_in"),
        _dev(norm_out, torch.float32, "norm_out") if norm_out is not None else None,
        ctypes.addressof(s1) if state1 is not None else None,
        ctypes.addressof(s2) if state2 is not None else None, _i32(pairs, "pairs"), ctypes.byref(lists.c),
        _i32(items, "items"), items.shape[0], _i32(dense_skip, "dense_skip") if dense_skip is not None else None,
        _i32(inc, "inc"), _dev(partials, torch.float32, "partials"),
        _i32(multi, "multi") if n_multi else None, n_multi, float(margin), OPTIMIZER_IDS[optimizer], float(lr), int(step),
        _dev(dev_hyper, torch.float32, "dev_hyper") if dev_hyper is not None else None, 1 if reset_lists else 0,
        *nx, _dev(loss_buf, torch.float32, "loss"), ctypes.byref(direction.c) if direction is not None else None)
    keep = (desc_in, to, hi, ho, s1, s2, tables_out, hat_in, hat_out, norm_in, norm_out, state1, state2, pairs, lists, items, inc,
            partials, multi, loss_buf, dense_skip, sample_next, direction)
    if prepare_only:   # (a data-parallel step runs this launch between two collectives: host time per step matters there)
        return _prepared(L.load().kge_pull_step, "kge_pull_step", args, len(args) - 4, keep)
    L.check(L.load().kge_pull_step(*args, _stream()), "kge_pull_step")


def pull_index_build(triples, perm, batch_stride, slice_lo, n_pairs, n_batches, tot_entity, tot_relation, segment,
                     groups_per_block, compact):
    """kge_pull_index_build: the incidence index of `n_batches` batches of the permutation, built on the device.  Returns
    (pairs [nb, n, 4], inc [nb, 3n], inv [nb, 3n], items [nb, item_cap, 4], multi [nb, multi_cap, 4], skip [nb, words] or None,
    counts [nb, 4] = {item slots, multi rows, partial slots, listed rows}) -- int32 device tensors at fixed strides."""
    lib = L.load()
    dev = triples.device
    nb, n = int(n_batches), int(n_pairs)
    item_cap, multi_cap, words = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    ws_bytes = ctypes.c_size_t()
    L.check(lib.kge_pull_index_geometry(nb, n, int(tot_entity), int(tot_relation), int(segment), int(groups_per_block),
                                        1 if compact else 0, ctypes.byref(item_cap), ctypes.byref(multi_cap), ctypes.byref(words),
                                        ctypes.byref(ws_bytes)), "kge_pull_index_geometry")
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    pairs, inc, inv = i32(nb, n, 4), i32(nb, 3 * n), i32(nb, 3 * n)
    items, multi = i32(nb, item_cap.value, 4), i32(nb, multi_cap.value, 4)
    skip = i32(nb, words.value) if compact else None
    counts = i32(nb, 4)
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device=dev)
    L.check(lib.kge_pull_index_build(_ids(triples, "triples"), _ids(perm, "perm"), int(batch_stride), int(slice_lo), n, nb,
                                     int(tot_entity), int(tot_relation), int(segment), int(groups_per_block), 1 if compact else 0,
                                     pairs.data_ptr(), inc.data_ptr(), inv.data_ptr(), items.data_ptr(), multi.data_ptr(),
                                     skip.data_ptr() if skip is not None else None, counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _stream()), "kge_pull_index_build")
    return pairs, inc, inv, items, multi, skip, counts


def pull_index_bytes(n_batches, n_pairs, tot_entity, tot_relation, segment, groups_per_block, compact):
    """(resident bytes, transient workspace bytes) of kge_pull_index_build's output for these sizes -- the exact strides of
    kge_pull_index_geometry, no device needed."""
    item_cap, multi_cap, words = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    ws_bytes = ctypes.c_size_t()
    L.check(L.load().kge_pull_index_geometry(int(n_batches), int(n_pairs), int(tot_entity), int(tot_relation), int(segment),
                                             int(groups_per_block), 1 if compact else 0, ctypes.byref(item_cap), ctypes.byref(multi_cap),
                                             ctypes.byref(words), ctypes.byref(ws_bytes)), "kge_pull_index_geometry")
    nb, n = int(n_batches), int(n_pairs)
    resident = nb * (n * 16 + 2 * 3 * n * 4 + item_cap.value * 16 + multi_cap.value * 16 + (words.value * 4 if compact else 0) + 16)
    return resident, int(ws_bytes.value)


def pull_list_set_bytes(batch_size, tot_entity):
    """Bytes of ONE PullListSet (two are kept per owner-computes path)."""
    return int(batch_size) * (4 + 4 + 3 * 16) + int(tot_entity) * (4 + 4 + L.PULL_BUCKET * 4 + L.PULL_BUCKET * 16)


def _plan_batches(index):
    """The host array of struct kge_pull_batch over every batch of an incidence index."""
    batches = (L.PullBatch * index.n_batches)()
    for b in range(index.n_batches):
        pairs, inc, items, multi = index.batch(b)
        skip = index.skip(b)
        batches[b] = L.PullBatch(pairs.data_ptr(), items.data_ptr() if items.shape[0] else None, items.shape[0],
                                 skip.data_ptr() if skip is not None else None, inc.data_ptr(), index.inv(b).data_ptr(),
                                 multi.data_ptr() if multi.shape[0] else None, multi.shape[0], pairs.shape[0])
    return batches


def _plan_common(c, lists, batches, index, bern, slots, seed, draws_per_batch, loss_buf):
    """The fields kge_pull_plan, kge_transx_plan and kge_own_plan share by name: list sets, batches, sampler, loss."""
    for half in (0, 1):
        c.lists[half] = lists[half].c
    c.batches = ctypes.cast(batches, ctypes.POINTER(L.PullBatch))
    c.n_batches = index.n_batches
    c.bern_prob = bern.data_ptr() if bern is not None else None
    c.slots = slots.data_ptr() if slots is not None else None
    c.n_slots = slots.numel() if slots is not None else 0
    c.seed = int(seed) & (2 ** 64 - 1)
    c.draws_per_batch = int(draws_per_batch)
    c.loss = loss_buf.data_ptr()


def _run(fn, name, c, *args):
    """kge_pull_run / kge_transx_run / kge_own_run on plan struct `c`:
    args = (first_batch, n_steps, [src_half,] cur_list, lists_ready, first_opt_step, first_offset, sample_after_last)."""
    *head, lists_ready, first_opt_step, first_offset, sample_after_last = args
    rc = fn(ctypes.byref(c), *map(int, head), 1 if lists_ready else 0, int(first_opt_step), int(first_offset) & (2 ** 64 - 1),
            int(sample_after_last), _stream())
    if rc:
        L.check(rc, name)


class PullPlan:
    """struct kge_pull_plan for a (model, index, state) triple: everything that does not change from step to step,
    marshalled once.  `run` enqueues a whole sequence of steps with ONE foreign call (the per-step work is ~35 us of GPU
    time: a Python-level loop could not keep the queue full)."""

    def __init__(self, model_name, desc_kwargs, tot_entity, tot_relation, tables, hats, norms, state1, state2, lists, index,
                 partials, margin, optimizer, lr, loss_buf, bern, slots, seed, draws_per_batch, direction=None):
        self.keep = (tables, hats, norms, state1, state2, lists, index, partials, loss_buf, bern, slots, direction)   # keep storage alive
        c = L.PullPlanC()
        for half in (0, 1):
            c.model[half] = make_desc(model_name, tables[half], None, tot_entity=tot_entity, tot_relation=tot_relation, **desc_kwargs)
            c.norm[half] = norms[half].data_ptr()
            for t in (0, 1):
                c.hat[half][t] = hats[half][t].data_ptr()
        for t in (0, 1):
            c.state1[t] = state1[t].data_ptr() if state1 is not None else None
            c.state2[t] = state2[t].data_ptr() if state2 is not None else None
        self.batches = _plan_batches(index)
        _plan_common(c, lists, self.batches, index, bern, slots, seed, draws_per_batch, loss_buf)
        c.partials = partials.data_ptr()
        c.margin, c.optimizer, c.lr = float(margin), OPTIMIZER_IDS[optimizer], float(lr)
        if direction is not None:      # two-phase steps (kge_pull_run fills n_pairs per batch)
            c.direction = direction.c
        self.c = c
        self.fn = L.load().kge_pull_run

    def run(self, first_batch, n_steps, src_half, cur_list, lists_ready, first_opt_step, first_offset, sample_after_last):
        _run(self.fn, "kge_pull_run", self.c, first_batch, n_steps, src_half, cur_list, lists_ready, first_opt_step, first_offset,
             sample_after_last)


# ---------------------------------------------------------------------------- TransH / TransD gradients, two-launch owner-computes form
def transx_groups_per_block(dim):
    return int(L.load().kge_transx_groups_per_block(int(dim)))


def transx_partial_stride(dim):
    return int(L.load().kge_transx_partial_stride(int(dim)))


class TransXScratch:
    """Staging rows (5 / 8 gradient rows per pair) and hinge coefficients of kge_transx_grad_step."""

    def __init__(self, model_name, dim, n_pairs, device):
        sb, rb = ctypes.c_size_t(), ctypes.c_size_t()
        L.check(L.load().kge_transx_scratch_bytes(MODEL_IDS[model_name], int(dim), int(n_pairs), ctypes.byref(sb), ctypes.byref(rb)),
                "kge_transx_scratch_bytes")
        self.stage = torch.empty(max(4, sb.value // 4), dtype=torch.float32, device=device)
        self.recs = torch.zeros(max(1, rb.value // 4), dtype=torch.float32, device=device)


def transx_grad_step(desc, pairs, lists, items, listed, inc, partials, multi, margin, scratch, loss_buf, reset_lists=True,
                     sample_next=None, prepare_only=False):
    """kge_transx_grad_step: the TransH / TransD gradients of one batch into desc's dense gradient tables, no float atomics
    (csrc/kge_pullx.hip).  sample_next as pull_step."""
    n_multi = multi.shape[0] if multi is not None else 0
    nx = _next_sampler_args(sample_next)
    args = [ctypes.byref(desc), _i32(pairs, "pairs"), pairs.shape[0], ctypes.byref(lists.c),
            _i32(items, "items") if items.shape[0] else None, items.shape[0], _i32(listed, "listed") if listed is not None else None,
            _i32(inc, "inc"), _dev(partials, torch.float32, "partials"), _i32(multi, "multi") if n_multi else None, n_multi,
            float(margin), _dev(scratch.stage, torch.float32, "stage"), _dev(scratch.recs, torch.float32, "recs"),
            1 if reset_lists else 0, *nx, _dev(loss_buf, torch.float32, "loss")]
    fn = L.load().kge_transx_grad_step
    if prepare_only:
        return _prepared(fn, "kge_transx_grad_step", args, len(args) - 3,
                         (desc, pairs, lists, items, listed, inc, partials, multi, scratch, loss_buf, sample_next))
    L.check(fn(*args, _stream()), "kge_transx_grad_step")


class TransXPlan:
    """struct kge_transx_plan: everything of the TransH / TransD step that does not change between steps; `run` enqueues a whole
    sequence of steps (gradients without atomics + flat optimiser) with ONE foreign call."""

    def __init__(self, desc, flat, lists, index, partials, scratch, margin, optimizer, lr, loss_buf, bern, slots, seed, draws_per_batch):
        self.keep = (desc, flat, lists, index, partials, scratch, loss_buf, bern, slots)
        c = L.TransXPlanC()
        ctypes.memmove(ctypes.byref(c.model), ctypes.byref(desc), ctypes.sizeof(L.ModelDesc))
        self.batches = _plan_batches(index)
        _plan_common(c, lists, self.batches, index, bern, slots, seed, draws_per_batch, loss_buf)
        c.partials, c.stage, c.recs = partials.data_ptr(), scratch.stage.data_ptr(), scratch.recs.data_ptr()
        c.margin = float(margin)
        c.flat_param, c.flat_grad = flat.param.data_ptr(), flat.grad.data_ptr()
        c.flat_state1 = flat.state1.data_ptr() if flat.state1 is not None else None
        c.flat_state2 = flat.state2.data_ptr() if flat.state2 is not None else None
        c.flat_numel = flat.param.numel()
        c.optimizer, c.lr = OPTIMIZER_IDS[optimizer], float(lr)
        self.c = c
        self.fn = L.load().kge_transx_run

    def run(self, *args):   # (first_batch, n_steps, cur_list, lists_ready, first_opt_step, first_offset, sample_after_last)
        _run(self.fn, "kge_transx_run", self.c, *args)


# ---------------------------------------------------------------------------- two-phase owner-computes step (pointwise models)
def own_groups_per_block(model_name, dim):
    return int(L.load().kge_own_groups_per_block(MODEL_IDS[model_name], int(dim)))


def own_partial_stride(model_name, dim):
    return int(L.load().kge_own_partial_stride(MODEL_IDS[model_name], int(dim)))


def own_stage_floats(model_name, dim, n_pairs):
    """Floats of the staged form's buffer for a batch of n_pairs bundles (kge_own_stage_bytes)."""
    return int(L.load().kge_own_stage_bytes(MODEL_IDS[model_name], int(dim), int(n_pairs))) // 4


def _ptr_array(tensors, n=L.KGE_MAX_TABLES):
    arr = (ctypes.c_void_p * n)()
    for i, t in enumerate(tensors or ()):
        arr[i] = t.data_ptr() if t is not None else None
    return arr


def own_step(desc, pairs, lists, items, listed, inc, partials, dense, lmbda, reg_type, loss_buf, reset_lists=True, sample_next=None,
             stage=None):
    """Phase 1 (kge_own_step): gradient rows of every touched parameter row into desc.grads, no atomics."""
    nx = _next_sampler_args(sample_next)
    L.check(L.load().kge_own_step(ctypes.byref(desc), _i32(pairs, "pairs"), pairs.shape[0], ctypes.byref(lists.c), _i32(items, "items"),
                                  items.shape[0], _i32(listed, "listed") if listed is not None else None, _i32(inc, "inc"),
                                  _dev(partials, torch.float32, "partials"), 1 if dense else 0, float(lmbda), int(reg_type),
                                  1 if reset_lists else 0, *nx, _dev(loss_buf, torch.float32, "loss"),
                                  _dev(stage, torch.float32, "stage") if stage is not None else None, _stream()), "kge_own_step")


def own_apply(desc, state1, state2, pairs, lists, items, listed, multi, partials, dense, optimizer, lr, step):
    """Phase 2 (kge_own_apply): the optimiser, in place, on the rows phase 1 produced gradients for."""
    s1, s2 = _ptr_array(state1), _ptr_array(state2)
    n_multi = multi.shape[0] if multi is not None else 0
    L.check(L.load().kge_own_apply(ctypes.byref(desc), ctypes.addressof(s1) if state1 is not None else None,
                                   ctypes.addressof(s2) if state2 is not None else None, _i32(pairs, "pairs"), pairs.shape[0],
                                   ctypes.byref(lists.c), _i32(items, "items"), items.shape[0],
                                   _i32(listed, "listed") if listed is not None else None, _i32(multi, "multi") if n_multi else None,
                                   n_multi, _dev(partials, torch.float32, "partials"), 1 if dense else 0, OPTIMIZER_IDS[optimizer],
                                   float(lr), int(step), _stream()), "kge_own_apply")


class OwnPlan:
    """struct kge_own_plan: everything of the two-phase step that does not change between steps, marshalled once; `run` enqueues
    a whole sequence of steps (two launches each) with ONE foreign call."""

    def __init__(self, desc, state1, state2, lists, index, partials, optimizer, lr, lmbda, reg_type, loss_buf, bern, slots, seed,
                 draws_per_batch, stage=None):
        self.keep = (desc, state1, state2, lists, index, partials, loss_buf, bern, slots, stage)
        c = L.OwnPlanC()
        ctypes.memmove(ctypes.byref(c.model), ctypes.byref(desc), ctypes.sizeof(L.ModelDesc))
        for i, t in enumerate(state1 or ()):
            c.state1[i] = t.data_ptr() if t is not None else None
        for i, t in enumerate(state2 or ()):
            c.state2[i] = t.data_ptr() if t is not None else None
        self.batches = _plan_batches(index)
        _plan_common(c, lists, self.batches, index, bern, slots, seed, draws_per_batch, loss_buf)
        c.partials = partials.data_ptr()
        c.optimizer, c.lr, c.lmbda, c.reg_type = OPTIMIZER_IDS[optimizer], float(lr), float(lmbda), int(reg_type)
        c.stage = stage.data_ptr() if stage is not None else None
        self.c = c
        self.fn = L.load().kge_own_run

    def run(self, *args):   # (first_batch, n_steps, cur_list, lists_ready, first_opt_step, first_offset, sample_after_last)
        _run(self.fn, "kge_own_run", self.c, *args)


# ---------------------------------------------------------------------------- 1-N scoring head (projection models)
def _f32(t, what):
    return _dev(t, torch.float32, what)


def head_1n_forward(x, ent, bias=None, precision="f32"):
    """sigmoid(x @ ent.T + bias): float32 [B, E]  (kge_head_1n_forward; precision="bf16": operands rounded to bfloat16 on their way
    to the matrix cores, fp32 accumulation -- kge_head_1n_forward_bf16)."""
    if precision not in ("f32", "bf16"):
        raise ValueError("head_1n_forward: precision must be 'f32' or 'bf16'")
    B, d = x.shape
    E = ent.shape[0]
    preds = torch.empty((B, E), dtype=torch.float32, device=x.device)
    lib = L.load()
    fn, name = (lib.kge_head_1n_forward, "kge_head_1n_forward") if precision == "f32" else (lib.kge_head_1n_forward_bf16, "kge_head_1n_forward_bf16")
    L.check(fn(_f32(x, "x"), B, d, _f32(ent, "ent"), E, _f32(bias, "bias") if bias is not None else None, _f32(preds, "preds"), _stream()), name)
    return preds


def head_1n_rank(x, ent, bias, truth, off=None, ids=None, return_ties=False, energies=False):
    """(rank, filtered rank) int32 [2, B] of the true entity of every row under sigmoid(x @ ent.T + bias), without the [B, E] tensor
    (kge_head_1n_rank).  truth int64 [B]; off int64 [B+1] / ids int32: CSR of the entities known for each row (None = unfiltered).
    energies=True (tests): the sweep's float32 [B, E] energies -p instead."""
    B, d = x.shape
    E = ent.shape[0]
    dev = x.device
    trip = torch.zeros((B, 3), dtype=torch.int64, device=dev)
    trip[:, 2] = truth
    lib = L.load()
    ws = torch.empty(max(1, lib.kge_head_1n_rank_workspace_bytes(B, d, E, int(bias is not None))), dtype=torch.uint8, device=dev)
    ranks = torch.empty((2, B), dtype=torch.int32, device=dev)
    ties = torch.empty(B, dtype=torch.int32, device=dev) if return_ties else None
    out = torch.empty((B, E), dtype=torch.float32, device=dev) if energies else None
    L.check(lib.kge_head_1n_rank(_f32(x, "x"), B, d, _f32(ent, "ent"), E, _f32(bias.view(-1), "bias") if bias is not None else None,
                                 _ids(trip, "triples"), _dev(off, torch.int64, "csr offsets") if off is not None else None,
                                 _dev(ids, torch.int32, "csr ids") if ids is not None else None,
                                 _dev(ws, torch.uint8, "workspace"), ws.numel(), _dev(ranks, torch.int32, "ranks"),
                                 _dev(ties, torch.int32, "ties") if ties is not None else None,
                                 _f32(out, "energies") if out is not None else None, _stream()), "kge_head_1n_rank")
    if energies:
        return out
    return (ranks, ties) if return_ties else ranks


def head_1n_backward(x, ent, preds, dpreds, need_bias=True, workspace=True):
    """(dx, g_ent, g_bias) of the head given d loss / d preds (kge_head_1n_backward).  workspace=False: the entry point's
    workspace-free form (split-K partial tiles meet in float atomics instead of being added in a fixed order)."""
    B, d = x.shape
    E = ent.shape[0]
    dx = torch.empty_like(x)
    g_ent = torch.zeros_like(ent)
    g_bias = torch.zeros(E, dtype=torch.float32, device=x.device) if need_bias else None
    lib = L.load()
    # (room for the split-K partial tiles: summed in split order instead of with float atomics -- reproducible gradients)
    ws = torch.empty(lib.kge_head_1n_backward_workspace_bytes(), dtype=torch.uint8, device=x.device) if workspace else None
    L.check(lib.kge_head_1n_backward(_f32(x, "x"), B, d, _f32(ent, "ent"), E, _f32(preds, "preds"),
                                     _f32(dpreds, "dpreds"), _f32(dx, "dx"), _f32(g_ent, "g_ent"),
                                     _f32(g_bias, "g_bias") if need_bias else None,
                                     _dev(ws, torch.uint8, "workspace") if workspace else None, ws.numel() if workspace else 0,
                                     _stream()), "kge_head_1n_backward")
    return dx, g_ent, g_bias


def head_1n_bce(x, ent, bias, label_off, label_ids, label_smoothing, loss_buf, g_ent, g_bias=None):
    """One direction of Criterion.multi_class_bce fused with the head and its backward (kge_head_1n_bce).
    label_off int64 [B+1], label_ids int32 [n_pos]; label_smoothing None = off.  Adds to loss_buf / g_ent / g_bias,
    returns dx [B, d]."""
    B, d = x.shape
    E = ent.shape[0]
    n_pos = int(label_ids.numel())
    lib = L.load()
    ws = torch.empty(lib.kge_head_1n_bce_workspace_bytes(B, E, n_pos), dtype=torch.uint8, device=x.device)
    dx = torch.empty_like(x)
    L.check(lib.kge_head_1n_bce(_f32(x, "x"), B, d, _f32(ent, "ent"), E, _f32(bias, "bias") if bias is not None else None,
                                _dev(label_off, torch.int64, "label_off"),
                                _dev(label_ids, torch.int32, "label_ids") if n_pos else None, n_pos,
                                -1.0 if label_smoothing is None else float(label_smoothing),
                                _dev(ws, torch.uint8, "workspace"), ws.numel(), _f32(loss_buf, "loss"), _f32(dx, "dx"),
                                _f32(g_ent, "g_ent"), _f32(g_bias, "g_bias") if g_bias is not None else None, _stream()),
            "kge_head_1n_bce")
    return dx


# ---------------------------------------------------------------- shared by the models with their own descriptor (ConvKB, TuckER, ProjE, ConvE, HypER)
def _check_embeddings(model, *specs):
    """specs: (name, tensor, rows indexed by id, columns)."""
    for name, t, rows, cols in specs:
        if t.dim() != 2 or t.shape[1] != cols or t.shape[0] < rows:
            raise L.KgeHipError("%s: %s must be [>= %d, %d] (got %s): an nn.Embedding lookup would raise IndexError"
                                % (model, name, rows, cols, tuple(t.shape)))


def _bind_grads(d, fields, names, grads, tables):
    """d.<field> = the gradient tensor's pointer, each gradient shaped like its table."""
    for field, name, g, t in zip(fields, names, grads, tables):
        if g.shape != t.shape:
            raise ValueError("grad shape %s != tensor shape %s" % (tuple(g.shape), tuple(t.shape)))
        setattr(d, field, _dev(g, torch.float32, name).value)


def _set_rng(d, train, seed, offset):
    d.train, d.seed, d.offset = int(bool(train)), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)


def _desc_ws(desc, query, *args):
    """(pointer, bytes) of the descriptor's workspace, grown to what `query` asks for; kept with the descriptor, so the steps of a
    Trainer (captured ones included) allocate nothing once the largest request has been seen."""
    need = int(getattr(L.load(), query)(ctypes.byref(desc), *args))
    if need == 0:
        msg = L.load().kge_last_error()
        raise L.KgeHipError("%s refused the descriptor: %s" % (query, msg.decode() if msg else "?"))
    if desc._ws is None or desc._ws.numel() < need:
        desc._ws = torch.empty(need + need // 8, dtype=torch.uint8, device=desc._keepalive[0][0].device)
    return ctypes.c_void_p(desc._ws.data_ptr()), desc._ws.numel()


def _filter_csr_args(tail_off, tail_ids, head_off, head_ids):
    """The four filter-list pointers of a rank entry point; None = that side unfiltered.  An empty id list has no storage: the
    offsets pointer stands in for it (never read: every list is empty)."""
    args = []
    for off, ids in ((tail_off, tail_ids), (head_off, head_ids)):
        if off is None:
            args += [None, None]
        else:
            po, pi = _dev(off, torch.int64, "csr offsets"), _dev(ids, torch.int32, "csr ids")
            args += [po, pi if ids.numel() else po]
    return args


def _label_csr_args(who, h, r, t, hr_off, hr_ids, tr_off, tr_ids):
    """(B, n_hr, n_tr, the arguments h .. n_tr of a fused 1-N step).  hr_* / tr_*: the label CSRs of the batch (off int64 [B + 1],
    ids int32)."""
    B = h.numel()
    if r.numel() != B or t.numel() != B or hr_off.numel() != B + 1 or tr_off.numel() != B + 1:
        raise ValueError("%s: h, r, t must have equal lengths B and the label offsets B + 1 entries" % who)
    n_hr, n_tr = int(hr_ids.numel()), int(tr_ids.numel())
    return B, n_hr, n_tr, [_ids(h, "h"), _ids(r, "r"), _ids(t, "t"), B,
                           _dev(hr_off, torch.int64, "hr_t offsets"), _dev(hr_ids, torch.int32, "hr_t ids") if n_hr else None, n_hr,
                           _dev(tr_off, torch.int64, "tr_h offsets"), _dev(tr_ids, torch.int32, "tr_h ids") if n_tr else None, n_tr]


def _projection_eval_ranks(symbol, desc, triples, tail_off, tail_ids, head_off, head_ids, ties):
    n = triples.shape[0]
    ranks = torch.empty((4, n), dtype=torch.int32, device=triples.device)
    wp, wb = _desc_ws(desc, symbol + "_workspace_bytes", n)
    L.check(getattr(L.load(), symbol)(ctypes.byref(desc), _ids(triples, "triples"), n,
                                      *_filter_csr_args(tail_off, tail_ids, head_off, head_ids), wp, wb,
                                      _dev(ranks, torch.int32, "ranks"),
                                      _dev(ties, torch.int32, "ties") if ties is not None else None, _stream()), symbol)
    return ranks


def _train_bce(stem, desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf):
    """kge_<stem>_train_bce: the fused BCE step of a 1-N model with its own descriptor (TuckER and the conv 1-N models)."""
    symbol = "kge_%s_train_bce" % stem
    B, n_hr, n_tr, args = _label_csr_args(stem + "_train_bce", h, r, t, hr_off, hr_ids, tr_off, tr_ids)
    wp, wb = _desc_ws(desc, symbol + "_workspace_bytes", B, n_hr, n_tr)
    L.check(getattr(L.load(), symbol)(ctypes.byref(desc), *args, -1.0 if label_smoothing is None else float(label_smoothing), wp, wb,
                                      _dev(loss_buf, torch.float32, "loss"), _stream()), symbol)


# ---------------------------------------------------------------- shared by the conv 1-N models (ConvE, HypER, InteractE, AcrE)
def _conv_1n_desc(d, stem, names, tables, buffers, grads, want, skip, dropouts, eps, momentum, train, seed, offset, count_note="",
                  index_tables=None):
    """Fills `d`, a fresh descriptor of a conv 1-N model, with everything but its geometry, and returns it.  names: the descriptor
    fields of `tables`, in order; want: (the shapes of the tables, those of the six buffers) wherever the geometry is one the library
    accepts, else None (no shape is looked at); skip: the slots of the entity and the relation table, which may have more rows than ids;
    index_tables: a callable answering the model's int32 index tables as (field, tensor, shape) triples, called once the counts are
    known to be good.  Refusals in the order the builders always had: the counts, momentum None, the index tables' own, the embedding
    tables, the other shapes, the device and dtype of each tensor bound, the gradient count, the gradient shapes."""
    if len(tables) != len(names) or len(buffers) != 6:
        raise L.KgeHipError("%s: %d tensors and 6 running buffers expected%s, got %d and %d"
                            % (stem, len(names), count_note, len(tables), len(buffers)))
    if any(m is None for m in momentum):
        raise L.KgeHipError("%s: momentum None (the cumulative moving average) is not built" % stem)
    index = index_tables() if index_tables is not None else ()
    fields, tensors = tuple(names) + L.CONVE_BUFFERS, list(tables) + list(buffers)
    if want is not None:
        i_ent, i_rel = skip
        _check_embeddings(stem, ("ent_embeddings", tables[i_ent]) + want[0][i_ent], ("rel_embeddings", tables[i_rel]) + want[0][i_rel])
        for i, (name, t, shape) in enumerate(zip(fields, tensors, want[0] + want[1])):
            if i not in skip and tuple(t.shape) != shape:
                raise L.KgeHipError("%s: %s must be %s (got %s)" % (stem, name, shape, tuple(t.shape)))
        for name, t, shape in index:
            if tuple(t.shape) != shape:
                raise L.KgeHipError("%s: %s must be %s (got %s)" % (stem, name, shape, tuple(t.shape)))
    d.input_dropout, d.feature_map_dropout, d.hidden_dropout = (float(p) for p in dropouts)
    _set_rng(d, train, seed, offset)
    for i in range(3):
        d.eps[i], d.momentum[i] = float(eps[i]), float(momentum[i])
    for name, t, _ in index:
        setattr(d, name, _dev(t, torch.int32, name).value)
    for name, t in zip(fields, tensors):
        setattr(d, name, _dev(t, torch.float32, name).value)
    if grads is not None:
        if len(grads) != len(names):
            raise L.KgeHipError("%s: %d gradient tensors expected, got %d" % (stem, len(names), len(grads)))
        _bind_grads(d, ["g_" + n for n in names], ["grad of " + n for n in names], grads, tables)
    d._keepalive = (tables, buffers, grads) + ((index,) if index else ())
    d._ws = None
    return d


def _body_forward(stem, desc, e, r, width, side, row0):
    """kge_<stem>_body_forward -> (x float32 [n, width], saved); side: ConvE's, None for the models with one relation table."""
    n = e.numel()
    if r.numel() != n:
        raise ValueError("e, r must have equal lengths")
    lib, symbol = L.load(), "kge_%s_body_forward" % stem
    x = torch.empty((n, width), dtype=torch.float32, device=e.device)
    wp, wb = _desc_ws(desc, symbol + "_workspace_bytes", n)
    saved = torch.empty(max(1, int(getattr(lib, "kge_%s_saved_floats" % stem)(ctypes.byref(desc), n))), dtype=torch.float32, device=e.device)
    L.check(getattr(lib, symbol)(ctypes.byref(desc), _ids(e, "e"), _ids(r, "r"), n, *(() if side is None else (int(side),)), int(row0),
                                 _dev(x, torch.float32, "x"), _dev(saved, torch.float32, "saved"), wp, wb, _stream()), symbol)
    return x, saved


def _body_backward(stem, desc, e, r, dx, saved, side, row0):
    """kge_<stem>_body_backward; side as in _body_forward."""
    n = e.numel()
    symbol = "kge_%s_body_backward" % stem
    wp, wb = _desc_ws(desc, symbol + "_workspace_bytes", n)
    L.check(getattr(L.load(), symbol)(ctypes.byref(desc), _ids(e, "e"), _ids(r, "r"), n, *(() if side is None else (int(side),)), int(row0),
                                      _dev(dx, torch.float32, "dx"), _dev(saved, torch.float32, "saved"), wp, wb, _stream()), symbol)


# ---------------------------------------------------------------- ConvKB (csrc/kge_convkb.hip): its own descriptor and entry points
def _convkb_no_reg(lmbda, reg_type):
    if float(lmbda) != 0.0 and int(reg_type) != L.REG_NONE:
        raise L.KgeHipError("convkb: the model has no regulariser (get_reg is 0.0); got lmbda %r, reg_type %r" % (lmbda, reg_type))


def convkb_desc(tables, grads=None, *, tot_entity, tot_relation, dim, num_filters, filter_sizes, conv_w, conv_b):
    """kge_convkb_desc.  `tables` / `grads`: ent_embeddings.weight, rel_embeddings.weight, fc1.weight, fc1.bias (the model's trainable
    tensors, in this order); conv_w / conv_b: the packed filters (flattened conv_list[j].weight / .bias concatenated in list order), fixed
    inputs.  Shapes are checked here (the kernels index rows by id without a bounds test); the filter geometry is checked by the
    library, which refuses a bad one loudly."""
    sizes = [int(s) for s in filter_sizes]
    E, R, k, F = int(tot_entity), int(tot_relation), int(dim), int(num_filters)
    if len(tables) != 4:
        raise L.KgeHipError("convkb: 4 tensors expected (ent, rel, fc1.weight, fc1.bias), got %d" % len(tables))
    ent, rel, fc_w, fc_b = tables
    _check_embeddings("convkb", ("ent_embeddings", ent, E, k), ("rel_embeddings", rel, R, k))
    W = sum(k - s + 1 for s in sizes)
    for name, t, numel in (("fc1.weight", fc_w, F * W), ("fc1.bias", fc_b, 1), ("conv_w", conv_w, F * 3 * sum(sizes)),
                           ("conv_b", conv_b, F * len(sizes))):
        if 1 <= len(sizes) <= L.CONVKB_MAX_WIDTHS and all(1 <= s <= k for s in sizes) and F >= 1 and t.numel() != numel:
            raise L.KgeHipError("convkb: %s must hold %d floats (got %d)" % (name, numel, t.numel()))
    d = L.ConvKBDesc()
    d.tot_entity, d.tot_relation, d.dim, d.num_filters, d.n_widths = E, R, k, F, len(sizes)
    for j, s in enumerate(sizes[:L.CONVKB_MAX_WIDTHS]):
        d.widths[j] = s
    d.ent, d.rel = _dev(ent, torch.float32, "ent_embeddings").value, _dev(rel, torch.float32, "rel_embeddings").value
    d.fc_w, d.fc_b = _dev(fc_w, torch.float32, "fc1.weight").value, _dev(fc_b, torch.float32, "fc1.bias").value
    d.conv_w, d.conv_b = _dev(conv_w, torch.float32, "conv_w").value, _dev(conv_b, torch.float32, "conv_b").value
    if grads is not None:
        _bind_grads(d, ("g_ent", "g_rel", "g_fc_w", "g_fc_b"), ["grad %d" % i for i in range(4)], grads, tables)
    d._keepalive = (tables, grads, conv_w, conv_b)
    d._ws = None
    return d


def convkb_collapse(desc):
    """float32 [3 dim + 1]: A_h | A_r | A_t | c0."""
    out = torch.empty(3 * desc.dim + 1, dtype=torch.float32, device=desc._keepalive[0][0].device)
    L.check(L.load().kge_convkb_collapse(ctypes.byref(desc), _dev(out, torch.float32, "out"), None, 0, _stream()), "kge_convkb_collapse")
    return out


def convkb_score_forward(desc, h, r, t):
    n = h.numel()
    if r.numel() != n or t.numel() != n:
        raise ValueError("h, r, t must have equal lengths")
    out = torch.empty(n, dtype=torch.float32, device=h.device)
    wp, wb = _desc_ws(desc, "kge_convkb_score_forward_workspace_bytes", n)
    L.check(L.load().kge_convkb_score_forward(ctypes.byref(desc), _ids(h, "h"), _ids(r, "r"), _ids(t, "t"), n,
                                              _dev(out, torch.float32, "scores"), wp, wb, _stream()), "kge_convkb_score_forward")
    return out


def convkb_score_backward(desc, h, r, t, dscore):
    n = h.numel()
    wp, wb = _desc_ws(desc, "kge_convkb_score_backward_workspace_bytes", n)
    L.check(L.load().kge_convkb_score_backward(ctypes.byref(desc), _ids(h, "h"), _ids(r, "r"), _ids(t, "t"), n,
                                               _dev(dscore, torch.float32, "dscore"), wp, wb, _stream()), "kge_convkb_score_backward")


def convkb_train_logistic(desc, h, r, t, y, loss_buf, bundle=1):
    n = h.numel()
    wp, wb = _desc_ws(desc, "kge_convkb_train_logistic_workspace_bytes", n)
    L.check(L.load().kge_convkb_train_logistic(ctypes.byref(desc), _ids(h, "h"), _ids(r, "r"), _ids(t, "t"), _ids(y, "y"), n,
                                               int(bundle), wp, wb, _dev(loss_buf, torch.float32, "loss"), _stream()),
            "kge_convkb_train_logistic")


def convkb_train_logistic_sampled(desc, triples, perm, start, n_pos, neg_rate, bern_prob, slots, seed, offset, loss_buf, cursor=None):
    """Sampler + scoring + pointwise logistic loss + all four gradients; the rows equal sample_batch(start, n_pos, neg_rate,
    pointwise=True)."""
    bp = _dev(bern_prob, torch.float32, "bern_prob") if bern_prob is not None else None
    sp = ctypes.c_void_p(slots.data_ptr()) if slots is not None else None
    pc = _dev(cursor, torch.int64, "cursor") if cursor is not None else None
    wp, wb = _desc_ws(desc, "kge_convkb_train_logistic_sampled_workspace_bytes", int(n_pos), int(neg_rate))
    L.check(L.load().kge_convkb_train_logistic_sampled(ctypes.byref(desc), _ids(triples, "triples"), _ids(perm, "perm"), int(start),
                                                       int(n_pos), int(neg_rate), bp, sp, slots.numel() if slots is not None else 0,
                                                       int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), pc, wp, wb,
                                                       _dev(loss_buf, torch.float32, "loss"), _stream()),
            "kge_convkb_train_logistic_sampled")


def convkb_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids):
    """int32 [4, n] as eval_ranks, in one kge_convkb_eval_ranks call."""
    n = triples.shape[0]
    ranks = torch.empty((4, n), dtype=torch.int32, device=triples.device)
    wp, wb = _desc_ws(desc, "kge_convkb_eval_ranks_workspace_bytes", n)
    L.check(L.load().kge_convkb_eval_ranks(ctypes.byref(desc), _ids(triples, "triples"), n,
                                           *_filter_csr_args(tail_off, tail_ids, head_off, head_ids), wp, wb,
                                           _dev(ranks, torch.int32, "ranks"), _stream()), "kge_convkb_eval_ranks")
    return ranks


def convkb_sweep_scores_side(desc, triples, side):
    """float32 [n, E]: side 0 = preds of (h_i, r_i, e) for all e, side 1 = preds of (e, r_i, t_i)."""
    n = triples.shape[0]
    out = torch.empty((n, desc.tot_entity), dtype=torch.float32, device=triples.device)
    wp, wb = _desc_ws(desc, "kge_convkb_sweep_scores_side_workspace_bytes", n)
    L.check(L.load().kge_convkb_sweep_scores_side(ctypes.byref(desc), _ids(triples, "triples"), n, int(side), wp, wb,
                                                  _dev(out, torch.float32, "scores"), _stream()), "kge_convkb_sweep_scores_side")
    return out


# ---------------------------------------------------------------- MuRP (csrc/kge_murp.hip): its own descriptor and entry points, float64
def murp_desc(tables, grads=None, *, tot_entity, tot_relation, dim, rank_order=0):
    """kge_murp_desc.  `tables` / `grads`: wu, bs, bo, ent_embeddings.weight, rel_embeddings.weight (the model's state-dict order), all
    float64.  Shapes are checked here (the kernels index rows by id without a bounds test); dim and rank_order are checked by the
    library, which refuses bad ones loudly.  rank_order: 0 = ascending score (the reference's lists), 1 = most plausible first."""
    E, R, k = int(tot_entity), int(tot_relation), int(dim)
    if len(tables) != 5:
        raise L.KgeHipError("murp: 5 tensors expected (wu, bs, bo, ent, rel), got %d" % len(tables))
    wu, bs, bo, ent, rel = tables
    _check_embeddings("murp", ("ent_embeddings", ent, E, k), ("rel_embeddings", rel, R, k))
    for name, t, shape in (("wu", wu, (R, k)), ("bs", bs, (E,)), ("bo", bo, (E,))):
        if tuple(t.shape) != shape:
            raise L.KgeHipError("murp: %s must be %s (got %s)" % (name, shape, tuple(t.shape)))
    d = L.MurpDesc()
    d.tot_entity, d.tot_relation, d.dim, d.rank_order = E, R, k, int(rank_order)
    names = ("wu", "bs", "bo", "ent_embeddings", "rel_embeddings")
    for i, (name, t) in enumerate(zip(names, tables)):
        d.tables[i] = _dev(t, torch.float64, name).value
    if grads is not None:
        if len(grads) != 5:
            raise L.KgeHipError("murp: 5 gradient tensors expected, got %d" % len(grads))
        for i, (name, g, t) in enumerate(zip(names, grads, tables)):
            if g.shape != t.shape:
                raise ValueError("grad shape %s != tensor shape %s" % (tuple(g.shape), tuple(t.shape)))
            d.grads[i] = _dev(g, torch.float64, "grad of " + name).value
    d._keepalive = (tables, grads)
    d._ws = None
    return d


def murp_new_loss(device):
    """MuRP's loss accumulator: one float64 (new_loss_buffer / read_loss are the fp32 models')."""
    return torch.zeros(1, dtype=torch.float64, device=device)


def murp_score_forward(desc, h, r, t):
    n = h.numel()
    if r.numel() != n or t.numel() != n:
        raise ValueError("h, r, t must have equal lengths")
    out = torch.empty(n, dtype=torch.float64, device=h.device)
    L.check(L.load().kge_murp_score_forward(ctypes.byref(desc), _ids(h, "h"), _ids(r, "r"), _ids(t, "t"), n,
                                            _dev(out, torch.float64, "preds"), _stream()), "kge_murp_score_forward")
    return out


def murp_score_backward(desc, h, r, t, dscore):
    n = h.numel()
    if r.numel() != n or t.numel() != n or dscore.numel() != n:
        raise ValueError("h, r, t, dscore must have equal lengths")
    L.check(L.load().kge_murp_score_backward(ctypes.byref(desc), _ids(h, "h"), _ids(r, "r"), _ids(t, "t"), n,
                                             _dev(dscore, torch.float64, "dscore"), _stream()), "kge_murp_score_backward")


def murp_train_bce(desc, h, r, t, y, loss):
    """Forward + mean BCE-with-logits on clamp(y, 0, 1) + the five gradients; loss: murp_new_loss's accumulator."""
    n = h.numel()
    if r.numel() != n or t.numel() != n or y.numel() != n:
        raise ValueError("h, r, t, y must have equal lengths")
    L.check(L.load().kge_murp_train_bce(ctypes.byref(desc), _ids(h, "h"), _ids(r, "r"), _ids(t, "t"), _ids(y, "y"), n,
                                        _dev(loss, torch.float64, "loss"), _stream()), "kge_murp_train_bce")


def murp_rsgd_step(desc, lr, riemannian=True):
    """One optimiser launch over all five tensors; clears the gradients it consumed."""
    L.check(L.load().kge_murp_rsgd_step(ctypes.byref(desc), float(lr), 1 if riemannian else 0, _stream()), "kge_murp_rsgd_step")


def murp_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=None):
    """int32 [4, n] as eval_ranks (+ ties int32 [2, n]), by the descriptor's rank_order."""
    return _projection_eval_ranks("kge_murp_eval_ranks", desc, triples, tail_off, tail_ids, head_off, head_ids, ties)


def murp_sweep_scores_side(desc, triples, side):
    """float64 [n, E]: side 0 = preds of (h_i, r_i, e) for all e, side 1 = preds of (e, r_i, t_i)."""
    n = triples.shape[0]
    out = torch.empty((n, desc.tot_entity), dtype=torch.float64, device=triples.device)
    wp, wb = _desc_ws(desc, "kge_murp_sweep_scores_side_workspace_bytes", n)
    L.check(L.load().kge_murp_sweep_scores_side(ctypes.byref(desc), _ids(triples, "triples"), n, int(side), wp, wb,
                                                _dev(out, torch.float64, "scores"), _stream()), "kge_murp_sweep_scores_side")
    return out


# ---------------------------------------------------------------- TuckER (csrc/kge_tucker.hip): its own descriptor and entry points
def tucker_desc(tables, grads=None, *, tot_entity, tot_relation, d1, d2, dropouts=(0.0, 0.0, 0.0), train=False, seed=0, offset=0):
    """kge_tucker_desc.  `tables` / `grads`: ent_embeddings.weight [E, d1], rel_embeddings.weight [R, d2], W.weight [d2, d1 * d1] (the
    model's trainable tensors, in this order).  Shapes are checked here (the kernels index rows by id without a bounds test); the
    dropout rates and the offset are checked by the library, which refuses bad ones loudly."""
    E, R, d1, d2 = int(tot_entity), int(tot_relation), int(d1), int(d2)
    if len(tables) != 3:
        raise L.KgeHipError("tucker: 3 tensors expected (ent, rel, W), got %d" % len(tables))
    ent, rel, W = tables
    _check_embeddings("tucker", ("ent_embeddings", ent, E, d1), ("rel_embeddings", rel, R, d2))
    if W.numel() != d2 * d1 * d1:
        raise L.KgeHipError("tucker: W must hold d2 * d1 * d1 = %d floats (got %d)" % (d2 * d1 * d1, W.numel()))
    d = L.TuckerDesc()
    d.tot_entity, d.tot_relation, d.d1, d.d2 = E, R, d1, d2
    d.input_dropout, d.hidden_dropout1, d.hidden_dropout2 = (float(p) for p in dropouts)
    _set_rng(d, train, seed, offset)
    d.ent, d.rel, d.W = (_dev(t, torch.float32, n).value for t, n in zip(tables, ("ent_embeddings", "rel_embeddings", "W")))
    if grads is not None:
        _bind_grads(d, ("g_ent", "g_rel", "g_W"), ["grad %d" % i for i in range(3)], grads, tables)
    d._keepalive = (tables, grads)
    d._ws = None
    return d


def tucker_saved_floats(desc, n):
    return int(L.load().kge_tucker_saved_floats(ctypes.byref(desc), int(n)))


def tucker_body_forward(desc, e, r):
    """(x float32 [n, d1], saved): the body of TuckER.forward on the rows (e_i, r_i); `saved` is what tucker_body_backward reads."""
    n = e.numel()
    if r.numel() != n:
        raise ValueError("e, r must have equal lengths")
    x = torch.empty((n, desc.d1), dtype=torch.float32, device=e.device)
    saved = torch.empty(max(1, n * (2 * desc.d1 + 2)), dtype=torch.float32, device=e.device)
    wp, wb = _desc_ws(desc, "kge_tucker_body_forward_workspace_bytes", n)
    L.check(L.load().kge_tucker_body_forward(ctypes.byref(desc), _ids(e, "e"), _ids(r, "r"), n, _dev(x, torch.float32, "x"),
                                             _dev(saved, torch.float32, "saved"), wp, wb, _stream()), "kge_tucker_body_forward")
    return x, saved


def tucker_body_backward(desc, e, r, dx, saved):
    """g_* of the descriptor += the body's gradients given d loss / d x (same rows, seed, offset and `saved` as the forward)."""
    n = e.numel()
    wp, wb = _desc_ws(desc, "kge_tucker_body_backward_workspace_bytes", n)
    L.check(L.load().kge_tucker_body_backward(ctypes.byref(desc), _ids(e, "e"), _ids(r, "r"), n, _dev(dx, torch.float32, "dx"),
                                              _dev(saved, torch.float32, "saved"), wp, wb, _stream()), "kge_tucker_body_backward")


def tucker_train_bce(desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf):
    """One train_step_projection: adds to loss_buf and to the descriptor's gradients.  hr_* / tr_*: the label CSRs of the batch
    (off int64 [B + 1], ids int32); label_smoothing None = off."""
    _train_bce("tucker", desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf)


def tucker_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=None):
    """int32 [4, n] as eval_ranks, in one kge_tucker_eval_ranks call; ties: optional int32 [2, n] that receives the head's tie counts."""
    return _projection_eval_ranks("kge_tucker_eval_ranks", desc, triples, tail_off, tail_ids, head_off, head_ids, ties)


# ---------------------------------------------------------------- ProjE_pointwise (csrc/kge_proje.hip): its own descriptor and entry points
def proje_desc(tables, grads=None, *, tot_entity, tot_relation, dim, hidden_dropout=0.0, train=False, seed=0, offset=0):
    """kge_proje_desc.  `tables` / `grads`: ent_embeddings.weight [E, k], rel_embeddings.weight [R, k] and the six rows bc1, De1, Dr1, bc2,
    De2, Dr2 [1, k] (the model's parameter_list order).  Shapes are checked here (the kernels index rows by id without a bounds
    test); the dropout rate and the offset are checked by the library, which refuses bad ones loudly."""
    E, R, k = int(tot_entity), int(tot_relation), int(dim)
    if len(tables) != 8:
        raise L.KgeHipError("proje: 8 tensors expected (ent, rel, bc1, De1, Dr1, bc2, De2, Dr2), got %d" % len(tables))
    _check_embeddings("proje", ("ent_embeddings", tables[0], E, k), ("rel_embeddings", tables[1], R, k))
    for name, t in zip(L.PROJE_TABLES[2:], tables[2:]):
        if t.numel() != k:
            raise L.KgeHipError("proje: %s must hold %d floats (got %s)" % (name, k, tuple(t.shape)))
    d = L.ProjeDesc()
    d.tot_entity, d.tot_relation, d.dim, d.hidden_dropout = E, R, k, float(hidden_dropout)
    _set_rng(d, train, seed, offset)
    for name, t in zip(L.PROJE_TABLES, tables):
        setattr(d, name, _dev(t, torch.float32, name).value)
    if grads is not None:
        if len(grads) != 8:
            raise L.KgeHipError("proje: 8 gradient tensors expected, got %d" % len(grads))
        _bind_grads(d, ["g_" + name for name in L.PROJE_TABLES], ["grad of " + name for name in L.PROJE_TABLES], grads, tables)
    d._keepalive = (tables, grads)
    d._ws = None
    return d


def proje_body_forward(desc, e, r, side):
    """x float32 [n, k] = tanh(ent[e] o De_s + rel[r] o Dr_s + bc_s) * mask on side s (0: the tail direction's f1, 1: the head
    direction's f2)."""
    n = e.numel()
    if r.numel() != n:
        raise ValueError("e, r must have equal lengths")
    x = torch.empty((n, desc.dim), dtype=torch.float32, device=e.device)
    wp, wb = _desc_ws(desc, "kge_proje_body_forward_workspace_bytes", n)
    L.check(L.load().kge_proje_body_forward(ctypes.byref(desc), _ids(e, "e"), _ids(r, "r"), n, int(side), _dev(x, torch.float32, "x"),
                                            wp, wb, _stream()), "kge_proje_body_forward")
    return x


def proje_body_backward(desc, e, r, side, dx):
    """g_* of the descriptor += the body's gradients given d loss / d x (same rows, side, seed and offset as the forward)."""
    n = e.numel()
    wp, wb = _desc_ws(desc, "kge_proje_body_backward_workspace_bytes", n)
    L.check(L.load().kge_proje_body_backward(ctypes.byref(desc), _ids(e, "e"), _ids(r, "r"), n, int(side),
                                             _dev(dx, torch.float32, "dx"), wp, wb, _stream()), "kge_proje_body_backward")


def proje_label_loss(x, ent, pos_off, pos_ids, neg, loss_buf, g_ent):
    """One direction of ProjE's loss over the labelled columns (kge_proje_label_loss): adds to loss_buf and g_ent, returns dx.
    pos_off int64 [B + 1] / pos_ids int32: the rows' positives; neg: int32 ids shared by all rows, or None."""
    B, k = x.shape
    E = ent.shape[0]
    if pos_off.numel() != B + 1 or ent.shape[1] != k or g_ent.shape != ent.shape:
        raise ValueError("proje_label_loss: x [B, k], ent / g_ent [E, k] and B + 1 offsets expected")
    n_pos, n_neg = int(pos_ids.numel()), 0 if neg is None else int(neg.numel())
    lib = L.load()
    need = int(lib.kge_proje_label_loss_workspace_bytes(B, k, n_pos, n_neg))
    if need == 0:
        L.check(-1, "kge_proje_label_loss_workspace_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    dx = torch.empty_like(x)
    L.check(lib.kge_proje_label_loss(_dev(x, torch.float32, "x"), B, k, _dev(ent, torch.float32, "ent"), E,
                                     _dev(pos_off, torch.int64, "positive offsets"),
                                     _dev(pos_ids, torch.int32, "positive ids") if n_pos else None, n_pos,
                                     _dev(neg, torch.int32, "negative ids") if n_neg else None, n_neg,
                                     ctypes.c_void_p(ws.data_ptr()), ws.numel(), _dev(loss_buf, torch.float32, "loss"),
                                     _dev(dx, torch.float32, "dx"), _dev(g_ent, torch.float32, "g_ent"), _stream()),
            "kge_proje_label_loss")
    return dx


def proje_train(desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, neg, lmbda, loss_buf):
    """One train_step_projection of ProjE_pointwise: adds to loss_buf and to the descriptor's gradients.  hr_* / tr_*: the label
    CSRs of the batch (off int64 [B + 1], ids int32); neg: the batch's shared negative ids (int32) or None."""
    B, n_hr, n_tr, args = _label_csr_args("proje_train", h, r, t, hr_off, hr_ids, tr_off, tr_ids)
    n_neg = 0 if neg is None else int(neg.numel())
    wp, wb = _desc_ws(desc, "kge_proje_train_workspace_bytes", B, n_hr, n_tr, n_neg)
    L.check(L.load().kge_proje_train(ctypes.byref(desc), *args, _dev(neg, torch.int32, "negative ids") if n_neg else None, n_neg,
                                     float(lmbda), wp, wb, _dev(loss_buf, torch.float32, "loss"), _stream()), "kge_proje_train")


def proje_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=None):
    """int32 [4, n] as eval_ranks, in one kge_proje_eval_ranks call; ties: optional int32 [2, n] that receives the head's tie counts."""
    return _projection_eval_ranks("kge_proje_eval_ranks", desc, triples, tail_off, tail_ids, head_off, head_ids, ties)


# ---------------------------------------------------------------- ConvE (csrc/kge_conve.hip): its own descriptor and entry points
def conve_shapes(tot_entity, tot_relation, hidden_size, hidden_size_1):
    """The shapes of the 13 parameters (state-dict order) and of the six running buffers."""
    E, R, k, h1 = int(tot_entity), int(tot_relation), int(hidden_size), int(hidden_size_1)
    F = 32 * (2 * (k // h1) - 2) * (h1 - 2)
    return ([(E, k), (2 * R, k), (1, E), (1,), (1,), (32, 1, 3, 3), (32,), (32,), (32,), (k, F), (k,), (k,), (k,)],
            [(1,), (1,), (32,), (32,), (k,), (k,)])


def conve_desc(tables, buffers, grads=None, *, tot_entity, tot_relation, hidden_size, hidden_size_1, dropouts=(0.0, 0.0, 0.0),
               eps=(1e-5, 1e-5, 1e-5), momentum=(0.1, 0.1, 0.1), train=False, seed=0, offset=0):
    """kge_conve_desc.  `tables` / `grads`: the 13 parameters in state-dict order (ent_embeddings.weight, rel_embeddings.weight, b.weight,
    bn0.weight, bn0.bias, conv2d_1.weight, conv2d_1.bias, bn1.weight, bn1.bias, fc.weight, fc.bias, bn2.weight, bn2.bias); `buffers`:
    the running mean / variance of bn0, bn1, bn2, which the training form updates in place.  Shapes are checked here (the kernels index
    by id and by shape without a bounds test) whenever the geometry is one the library accepts; the geometry, the rates, the momenta and
    the offset are checked by the library, which refuses bad ones loudly."""
    E, R, k, h1 = int(tot_entity), int(tot_relation), int(hidden_size), int(hidden_size_1)
    want = conve_shapes(E, R, k, h1) if h1 >= 3 and k % h1 == 0 and 2 * (k // h1) >= 3 else None
    d = _conv_1n_desc(L.ConveDesc(), "conve", L.CONVE_TABLES, tables, buffers, grads, want, (0, 1), dropouts, eps, momentum, train, seed,
                      offset)
    d.tot_entity, d.tot_relation, d.hidden_size, d.hidden_size_1 = E, R, k, h1
    return d


def conve_body_forward(desc, e, r, side, row0=0):
    """(x float32 [n, k], saved): the body of ConvE.forward on the rows (e_i, r_i) of one direction (side 0 = tail, 1 = head); the
    training form updates the descriptor's running buffers once.  `saved` is what conve_body_backward reads."""
    return _body_forward("conve", desc, e, r, desc.hidden_size, side, row0)


def conve_body_backward(desc, e, r, side, dx, saved, row0=0):
    """g_* of the descriptor += the body's gradients given d loss / d x (same rows, side, row0, seed, offset and `saved` as the forward)."""
    _body_backward("conve", desc, e, r, dx, saved, side, row0)


def conve_train_bce(desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf):
    """One train_step_projection of ConvE: adds to loss_buf and to the descriptor's gradients, updates the running buffers twice (tail
    direction, then head).  hr_* / tr_*: the label CSRs of the batch (off int64 [B + 1], ids int32); label_smoothing None = off."""
    _train_bce("conve", desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf)


def conve_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=None):
    """int32 [4, n] as eval_ranks, in one kge_conve_eval_ranks call; ties: optional int32 [2, n] that receives the head's tie counts."""
    return _projection_eval_ranks("kge_conve_eval_ranks", desc, triples, tail_off, tail_ids, head_off, head_ids, ties)


# ---------------------------------------------------------------- HypER (csrc/kge_hyper.hip): its own descriptor and entry points
def hyper_shapes(tot_entity, tot_relation, ent_hidden_size, rel_hidden_size):
    """The shapes of the 13 parameters (state-dict order, b first) and of the six running buffers."""
    E, R, D, Dr = int(tot_entity), int(tot_relation), int(ent_hidden_size), int(rel_hidden_size)
    return ([(E,), (E, D), (R, Dr), (1,), (1,), (32,), (32,), (D,), (D,), (D, 32 * (D - 8)), (D,), (288, Dr), (288,)],
            [(1,), (1,), (32,), (32,), (D,), (D,)])


def hyper_desc(tables, buffers, grads=None, *, tot_entity, tot_relation, ent_hidden_size, rel_hidden_size, dropouts=(0.0, 0.0, 0.0),
               eps=(1e-5, 1e-5, 1e-5), momentum=(0.1, 0.1, 0.1), train=False, seed=0, offset=0):
    """kge_hyper_desc.  `tables` / `grads`: the 13 parameters in state-dict order (b, ent_embeddings.weight, rel_embeddings.weight,
    bn0.weight, bn0.bias, bn1.weight, bn1.bias, bn2.weight, bn2.bias, fc.weight, fc.bias, fc1.weight, fc1.bias); `buffers`: the running
    mean / variance of bn0, bn1, bn2, which the training form updates in place.  Shapes are checked here (the kernels index by id and
    by shape without a bounds test) whenever the geometry is one the library accepts; the geometry, the rates, the momenta and the
    offset are checked by the library, which refuses bad ones loudly."""
    E, R, D, Dr = int(tot_entity), int(tot_relation), int(ent_hidden_size), int(rel_hidden_size)
    want = hyper_shapes(E, R, D, Dr) if D >= 9 and Dr >= 1 else None
    d = _conv_1n_desc(L.HyperDesc(), "hyper", L.HYPER_TABLES, tables, buffers, grads, want, (1, 2), dropouts, eps, momentum, train, seed,
                      offset)
    d.tot_entity, d.tot_relation, d.ent_hidden_size, d.rel_hidden_size = E, R, D, Dr
    return d


def hyper_body_forward(desc, e, r, row0=0):
    """(x float32 [n, D], saved): the body of HypER.forward on the rows (e_i, r_i) of one direction; the training form updates the
    descriptor's running buffers once.  `saved` is what hyper_body_backward reads."""
    return _body_forward("hyper", desc, e, r, desc.ent_hidden_size, None, row0)


def hyper_body_backward(desc, e, r, dx, saved, row0=0):
    """g_* of the descriptor += the body's gradients given d loss / d x (same rows, row0, seed, offset and `saved` as the forward)."""
    _body_backward("hyper", desc, e, r, dx, saved, None, row0)


def hyper_train_bce(desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf):
    """One train_step_projection of HypER: adds to loss_buf and to the descriptor's gradients, updates the running buffers twice (tail
    direction, then head).  hr_* / tr_*: the label CSRs of the batch (off int64 [B + 1], ids int32); label_smoothing None = off."""
    _train_bce("hyper", desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf)


def hyper_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=None):
    """int32 [4, n] as eval_ranks, in one kge_hyper_eval_ranks call; ties: optional int32 [2, n] that receives the head's tie counts."""
    return _projection_eval_ranks("kge_hyper_eval_ranks", desc, triples, tail_off, tail_ids, head_off, head_ids, ties)


# ---------------------------------------------------------------- InteractE (csrc/kge_interacte.hip): its own descriptor and entry points
def interacte_shapes(tot_entity, tot_relation, reshape_height, reshape_width, feature_permutation, num_filters, kernel_size):
    """The shapes of the 12 parameters (state-dict order, bias and conv_filt first) and of the six running buffers."""
    E, R, P, NF, ks = int(tot_entity), int(tot_relation), int(feature_permutation), int(num_filters), int(kernel_size)
    k = int(reshape_height) * int(reshape_width)
    C = P * NF
    return ([(E,), (NF, 1, ks, ks), (E, k), (R, k), (P,), (P,), (C,), (C,), (k,), (k,), (k, C * 2 * k), (k,)],
            [(P,), (P,), (C,), (C,), (k,), (k,)])


def interacte_perm(chequer_perm, feature_permutation, hidden_size, device):
    """(perm, inv_perm): the int32 [P, 2K] device copies kge_interacte_desc points to.  Every row of chequer_perm must be a
    permutation of [0, 2K): the kernels gather by these indices without a bounds test, so this is checked here, on the host;
    inv_perm[p, perm[p, i]] = i."""
    P, n2 = int(feature_permutation), 2 * int(hidden_size)
    cp = torch.as_tensor(chequer_perm).detach().cpu()
    if cp.dtype not in (torch.int64, torch.int32) or tuple(cp.shape) != (P, n2):
        raise L.KgeHipError("interacte: chequer_perm must be an integer tensor of shape %s (got %s %s)" % ((P, n2), cp.dtype, tuple(cp.shape)))
    cp = cp.to(torch.int64)
    want = torch.arange(n2, dtype=torch.int64)
    for p in range(P):
        if not torch.equal(torch.sort(cp[p]).values, want):
            raise L.KgeHipError("interacte: row %d of chequer_perm is not a permutation of [0, %d)" % (p, n2))
    inv = torch.empty_like(cp)
    inv.scatter_(1, cp, want.expand(P, n2).contiguous())
    return cp.to(torch.int32).contiguous().to(device), inv.to(torch.int32).contiguous().to(device)


def interacte_desc(tables, buffers, grads=None, *, tot_entity, tot_relation, reshape_height, reshape_width, feature_permutation, num_filters,
                   kernel_size, chequer_perm=None, perms=None, dropouts=(0.0, 0.0, 0.0), eps=(1e-5, 1e-5, 1e-5), momentum=(0.1, 0.1, 0.1),
                   train=False, seed=0, offset=0):
    """kge_interacte_desc.  `tables` / `grads`: the 12 parameters in state-dict order (bias, conv_filt, ent_embeddings.weight,
    rel_embeddings.weight, bn0.weight, bn0.bias, bn1.weight, bn1.bias, bn2.weight, bn2.bias, fc.weight, fc.bias); `buffers`: the running
    mean / variance of bn0, bn1, bn2, which the training form updates in place.  chequer_perm: the model's [P, 2K] index tensor, checked
    and inverted by interacte_perm; perms: the pair interacte_perm returned for it (a model caches it), instead.  Shapes are checked here
    (the kernels index by id and by shape without a bounds test) whenever the geometry is one the library accepts; the geometry, the
    rates, the momenta and the offset are checked by the library, which refuses bad ones loudly."""
    E, R, rh, rw = int(tot_entity), int(tot_relation), int(reshape_height), int(reshape_width)
    P, NF, ks = int(feature_permutation), int(num_filters), int(kernel_size)
    k = rh * rw

    def index_tables():     # (once the counts are good: tables[2] says where the weights live)
        if perms is None and chequer_perm is None:
            raise L.KgeHipError("interacte: chequer_perm (or the pair interacte_perm made of it) is required")
        pair = perms if perms is not None else interacte_perm(chequer_perm, P, k, tables[2].device)
        return [(name, t, (P, 2 * k)) for name, t in zip(("perm", "inv_perm"), pair)]

    want = interacte_shapes(E, R, rh, rw, P, NF, ks) if min(rh, rw, P, NF) >= 1 and ks >= 3 and ks % 2 == 1 else None
    d = _conv_1n_desc(L.InteracteDesc(), "interacte", L.INTERACTE_TABLES, tables, buffers, grads, want, (2, 3), dropouts, eps, momentum, train,
                      seed, offset, index_tables=index_tables)
    d.tot_entity, d.tot_relation, d.reshape_height, d.reshape_width = E, R, rh, rw
    d.feature_permutation, d.num_filters, d.kernel_size = P, NF, ks
    return d


def interacte_body_forward(desc, e, r, row0=0):
    """(x float32 [n, K], saved): the body of InteractE.forward on the rows (e_i, r_i) of one direction; the training form updates the
    descriptor's running buffers once.  `saved` is what interacte_body_backward reads."""
    return _body_forward("interacte", desc, e, r, desc.reshape_height * desc.reshape_width, None, row0)


def interacte_body_backward(desc, e, r, dx, saved, row0=0):
    """g_* of the descriptor += the body's gradients given d loss / d x (same rows, row0, seed, offset and `saved` as the forward)."""
    _body_backward("interacte", desc, e, r, dx, saved, None, row0)


def interacte_train_bce(desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf):
    """One train_step_projection of InteractE: adds to loss_buf and to the descriptor's gradients, updates the running buffers twice
    (tail direction, then head).  hr_* / tr_*: the label CSRs of the batch (off int64 [B + 1], ids int32); label_smoothing None = off."""
    _train_bce("interacte", desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf)


def interacte_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=None):
    """int32 [4, n] as eval_ranks, in one kge_interacte_eval_ranks call; ties: optional int32 [2, n] that receives the head's tie counts."""
    return _projection_eval_ranks("kge_interacte_eval_ranks", desc, triples, tail_off, tail_ids, head_off, head_ids, ties)


# ---------------------------------------------------------------- AcrE (csrc/kge_acre.hip): its own descriptor and entry points
ACRE_WAYS = {"serial": 0, "parallel": 1}


def acre_shapes(tot_entity, tot_relation, in_channels, way, acre_bias):
    """(names, shapes) of the parameters in state-dict order (bias first) for the way and acre_bias, and the shapes of the six running
    buffers.  The serial way has 17 parameters with acre_bias and 11 + 3 without, the parallel way two more (the gate)."""
    E, R, C, k = int(tot_entity), int(tot_relation), int(in_channels), 200
    Cin = C if way == 0 else 1
    names = ["bias", "ent", "rel", "bn0_w", "bn0_b", "bn1_w", "bn1_b", "bn2_w", "bn2_b", "fc_w", "fc_b"]
    shapes = [(E,), (E, k), (2 * R, k), (1,), (1,), (C,), (C,), (k,), (k,), (k, 400 * C), (k,)]
    for i, cin in enumerate((1, Cin, Cin)):
        names.append("conv%d_w" % (i + 1))
        shapes.append((C, cin, 3, 3))
        if acre_bias:
            names.append("conv%d_b" % (i + 1))
            shapes.append((C,))
    if way == 1:
        names += ["gate_w", "gate_b"]
        shapes += [(400, 1600), (400,)]
    return names, shapes, [(1,), (1,), (C,), (C,), (k,), (k,)]


def acre_desc(tables, buffers, grads=None, *, tot_entity, tot_relation, hidden_size=200, in_channels, way="serial", first_atrous=1,
              second_atrous=2, third_atrous=2, acre_bias=True, dropouts=(0.0, 0.0, 0.0), eps=(1e-5, 1e-5, 1e-5), momentum=(0.1, 0.1, 0.1),
              train=False, seed=0, offset=0):
    """kge_acre_desc.  `tables` / `grads`: the model's parameters in state-dict order (bias, ent_embeddings.weight,
    rel_embeddings.weight, bn0.weight, bn0.bias, bn1.weight, bn1.bias, bn2.weight, bn2.bias, fc.weight, fc.bias, conv1.weight,
    [conv1.bias,] conv2.weight, [conv2.bias,] conv3.weight, [conv3.bias,] [W_gate_e.weight, W_gate_e.bias]): the conv biases are there iff
    acre_bias, the gate iff way is "parallel"; `buffers`: the running mean / variance of bn0, bn1, bn2, which the training form updates
    in place.  way: "serial" / "parallel" (or 0 / 1).  dropouts: (input, feature_map, hidden).  Shapes are checked here (the kernels
    index by id and by shape without a bounds test) whenever the geometry is one the library accepts; the geometry, the rates, the
    momenta and the offset are checked by the library, which refuses bad ones loudly."""
    E, R, k, C = int(tot_entity), int(tot_relation), int(hidden_size), int(in_channels)
    w = ACRE_WAYS.get(way, way)
    if not isinstance(w, int):
        raise L.KgeHipError("acre: way must be 'serial' or 'parallel' (got %r)" % (way,))
    names, shapes, want_b = acre_shapes(E, R, max(C, 1), w, bool(acre_bias))
    want = (shapes, want_b) if k == 200 and 1 <= C <= L.ACRE_MAX_CHANNELS and w in (0, 1) else None
    d = _conv_1n_desc(L.AcreDesc(), "acre", names, tables, buffers, grads, want, (1, 2), dropouts, eps, momentum, train, seed, offset,
                      count_note=" (way %r, acre_bias %r)" % (way, bool(acre_bias)))
    d.tot_entity, d.tot_relation, d.hidden_size, d.in_channels, d.way = E, R, k, C, w
    d.first_atrous, d.second_atrous, d.third_atrous, d.acre_bias = int(first_atrous), int(second_atrous), int(third_atrous), int(bool(acre_bias))
    return d


def acre_body_forward(desc, e, r, row0=0):
    """(x float32 [n, 200], saved): the body of AcrE.forward on the rows (e_i, r_i) of one direction; the training form updates the
    descriptor's running buffers once.  `saved` is what acre_body_backward reads."""
    return _body_forward("acre", desc, e, r, 200, None, row0)


def acre_body_backward(desc, e, r, dx, saved, row0=0):
    """g_* of the descriptor += the body's gradients given d loss / d x (same rows, row0, seed, offset and `saved` as the forward)."""
    _body_backward("acre", desc, e, r, dx, saved, None, row0)


def acre_train_bce(desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf):
    """One train_step_projection of AcrE: adds to loss_buf and to the descriptor's gradients, updates the running buffers twice
    (tail direction, then head).  hr_* / tr_*: the label CSRs of the batch (off int64 [B + 1], ids int32); label_smoothing None = off."""
    _train_bce("acre", desc, h, r, t, hr_off, hr_ids, tr_off, tr_ids, label_smoothing, loss_buf)


def acre_eval_ranks(desc, triples, tail_off, tail_ids, head_off, head_ids, ties=None):
    """int32 [4, n] as eval_ranks, in one kge_acre_eval_ranks call; ties: optional int32 [2, n] that receives the head's tie counts."""
    return _projection_eval_ranks("kge_acre_eval_ranks", desc, triples, tail_off, tail_ids, head_off, head_ids, ties)
