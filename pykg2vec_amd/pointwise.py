"""Drop-in pointwise (semantic-matching) models mirroring pykg2vec/models/pointwise.py (DistMult, Complex,
ComplexN3, ANALOGY, CP, SimplE, SimplE_ignr, QuatE, OctonionE, ConvKB, MuRP), scored by HIP kernels.  `get_reg` keeps the reference's
tensor-level form for use under the unmodified reference Trainer; the fused training kernel applies the same
regulariser from registers."""
import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import kernels as K
from .criterion import Criterion
from .kgmeta import NamedEmbedding, PointwiseModel


def _xavier(*embs):
    for e in embs:
        nn.init.xavier_uniform_(e.weight)


def _power_reg(rows, reg_type, use_abs):
    reg_type = reg_type.lower()
    if reg_type not in ("f2", "n3"):
        raise NotImplementedError("Unknown regularizer type: %s" % reg_type)
    p = 2 if reg_type == "f2" else 3
    total = 0
    for x in rows:
        total = total + torch.sum((x.abs() if use_abs else x) ** p, -1)
    return torch.mean(total)


class DistMult(PointwiseModel):
    """pointwise.py:391-458.  energy = -sum(h * r * t)."""
    kernel_name = "distmult"
    default_reg, reg_abs = "F2", False

    def __init__(self, **kwargs):
        super().__init__(self.__class__.__name__.lower())
        self.__dict__.update(self.load_params(["tot_entity", "tot_relation", "hidden_size", "lmbda"], kwargs))
        self.ent_embeddings = NamedEmbedding("ent_embedding", self.tot_entity, self.hidden_size)
        self.rel_embeddings = NamedEmbedding("rel_embedding", self.tot_relation, self.hidden_size)
        _xavier(self.ent_embeddings, self.rel_embeddings)
        self.parameter_list = [self.ent_embeddings, self.rel_embeddings]
        self.loss = Criterion.pointwise_logistic

    def desc_kwargs(self):
        return dict(dim=self.hidden_size)

    def embed(self, h, r, t):
        return self.ent_embeddings(h), self.rel_embeddings(r), self.ent_embeddings(t)

    def reg_rows(self, h, r, t):
        return self.embed(h, r, t)

    def get_reg(self, h, r, t, reg_type=None):
        return self.lmbda * _power_reg(self.reg_rows(h, r, t), reg_type or self.default_reg, self.reg_abs)

    def kernel_lmbda(self):
        """lmbda as the fused kernel applies it: lmbda/n_rows * sum over the gathered rows."""
        return self.lmbda

    def kernel_reg_type(self, reg_type=None):
        rt = (reg_type or self.default_reg).lower()
        if rt == "f2":
            return L.REG_F2
        if rt == "n3":
            return L.REG_N3_ABS if self.reg_abs else L.REG_N3
        raise NotImplementedError("Unknown regularizer type: %s" % rt)


class Complex(DistMult):
    """pointwise.py:122-202.  energy = -Re(<h, r, conj(t)>)."""
    kernel_name = "complex"

    def __init__(self, **kwargs):
        PointwiseModel.__init__(self, self.__class__.__name__.lower())
        self.__dict__.update(self.load_params(["tot_entity", "tot_relation", "hidden_size", "lmbda"], kwargs))
        k = self.hidden_size
        self.ent_embeddings_real = NamedEmbedding("emb_e_real", self.tot_entity, k)
        self.ent_embeddings_img = NamedEmbedding("emb_e_img", self.tot_entity, k)
        self.rel_embeddings_real = NamedEmbedding("emb_rel_real", self.tot_relation, k)
        self.rel_embeddings_img = NamedEmbedding("emb_rel_img", self.tot_relation, k)
        _xavier(self.ent_embeddings_real, self.ent_embeddings_img, self.rel_embeddings_real, self.rel_embeddings_img)
        self.parameter_list = [self.ent_embeddings_real, self.ent_embeddings_img, self.rel_embeddings_real,
                               self.rel_embeddings_img]
        self.loss = Criterion.pointwise_logistic

    def embed(self, h, r, t):
        return (self.ent_embeddings_real(h), self.ent_embeddings_img(h), self.rel_embeddings_real(r),
                self.rel_embeddings_img(r), self.ent_embeddings_real(t), self.ent_embeddings_img(t))


class ComplexN3(Complex):
    """pointwise.py:205-238.  Complex with the nuclear 3-norm (|x|^3) regulariser by default."""
    default_reg, reg_abs = "N3", True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.model_name = "complexn3"


class ANALOGY(DistMult):
    """pointwise.py:13-119.  DistMult term on k-dim tables + ComplEx term on k/2-dim tables."""
    kernel_name = "analogy"

    def __init__(self, **kwargs):
        PointwiseModel.__init__(self, self.__class__.__name__.lower())
        self.__dict__.update(self.load_params(["tot_entity", "tot_relation", "hidden_size", "lmbda"], kwargs))
        k = self.hidden_size
        self.ent_embeddings = NamedEmbedding("ent_embedding", self.tot_entity, k)
        self.rel_embeddings = NamedEmbedding("rel_embedding", self.tot_relation, k)
        self.ent_embeddings_real = NamedEmbedding("emb_e_real", self.tot_entity, k // 2)
        self.ent_embeddings_img = NamedEmbedding("emb_e_img", self.tot_entity, k // 2)
        self.rel_embeddings_real = NamedEmbedding("emb_rel_real", self.tot_relation, k // 2)
        self.rel_embeddings_img = NamedEmbedding("emb_rel_img", self.tot_relation, k // 2)
        self.parameter_list = [self.ent_embeddings, self.rel_embeddings, self.ent_embeddings_real,
                               self.ent_embeddings_img, self.rel_embeddings_real, self.rel_embeddings_img]
        _xavier(*self.parameter_list)
        self.loss = Criterion.pointwise_logistic

    def embed_complex(self, h, r, t):
        return (self.ent_embeddings_real(h), self.ent_embeddings_img(h), self.rel_embeddings_real(r),
                self.rel_embeddings_img(r), self.ent_embeddings_real(t), self.ent_embeddings_img(t))

    def reg_rows(self, h, r, t):
        return tuple(self.embed_complex(h, r, t)) + tuple(self.embed(h, r, t))


class CP(DistMult):
    """pointwise.py:320-387.  Canonical tensor decomposition: separate subject / object entity tables."""
    kernel_name = "cp"
    default_reg, reg_abs = "N3", False

    def __init__(self, **kwargs):
        PointwiseModel.__init__(self, self.__class__.__name__.lower())
        self.__dict__.update(self.load_params(["tot_entity", "tot_relation", "hidden_size", "lmbda"], kwargs))
        k = self.hidden_size
        self.sub_embeddings = NamedEmbedding("sub_embedding", self.tot_entity, k)
        self.rel_embeddings = NamedEmbedding("rel_embedding", self.tot_relation, k)
        self.obj_embeddings = NamedEmbedding("obj_embedding", self.tot_entity, k)
        _xavier(self.sub_embeddings, self.rel_embeddings, self.obj_embeddings)
        self.parameter_list = [self.sub_embeddings, self.rel_embeddings, self.obj_embeddings]
        self.loss = Criterion.pointwise_logistic

    def embed(self, h, r, t):
        return self.sub_embeddings(h), self.rel_embeddings(r), self.obj_embeddings(t)


class SimplE(DistMult):
    """pointwise.py:461-546.  energy = -clamp(<head[h], rel[r], tail[t]> + <head[t], rel_inv[r], tail[h]> / 2, +-20)."""
    kernel_name = "simple"

    def __init__(self, **kwargs):
        PointwiseModel.__init__(self, self.__class__.__name__.lower())
        self.__dict__.update(self.load_params(["tot_entity", "tot_relation", "hidden_size", "lmbda"], kwargs))
        k = self.hidden_size
        self.tot_train_triples = kwargs["tot_train_triples"]
        self.batch_size = kwargs["batch_size"]
        self.ent_head_embeddings = NamedEmbedding("ent_head_embedding", self.tot_entity, k)
        self.ent_tail_embeddings = NamedEmbedding("ent_tail_embedding", self.tot_entity, k)
        self.rel_embeddings = NamedEmbedding("rel_embedding", self.tot_relation, k)
        self.rel_inv_embeddings = NamedEmbedding("rel_inv_embedding", self.tot_relation, k)
        self.parameter_list = [self.ent_head_embeddings, self.ent_tail_embeddings, self.rel_embeddings,
                               self.rel_inv_embeddings]
        _xavier(*self.parameter_list)
        self.loss = Criterion.pointwise_logistic

    def embed(self, h, r, t):
        return (self.ent_head_embeddings(h), self.ent_head_embeddings(t), self.rel_embeddings(r),
                self.rel_inv_embeddings(r), self.ent_tail_embeddings(t), self.ent_tail_embeddings(h))

    def get_reg(self, h, r, t, reg_type="F2"):
        """pointwise.py:528-536: the reference hands the ID tensors to get_reg and regularises THEM -- a constant
        lmbda * (sum h^p + sum r^p + sum t^p) in float32 with no gradient.  Kept, so losses match."""
        rt = reg_type.lower()
        if rt not in ("f2", "n3"):
            raise NotImplementedError("Unknown regularizer type: %s" % reg_type)
        p = 2 if rt == "f2" else 3
        term = torch.sum(h.float() ** p, -1) + torch.sum(r.float() ** p, -1) + torch.sum(t.float() ** p, -1)
        return self.lmbda * torch.mean(term)

    def kernel_reg_type(self, reg_type="F2"):
        return L.REG_ID_F2 if reg_type.lower() == "f2" else L.REG_ID_N3  # loss constant only; no parameter gradient


class SimplE_ignr(SimplE):
    """pointwise.py:549-592.  Same tables; both terms summed without the 1/2."""
    kernel_name = "simple_ignr"

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.model_name = "simple_ignr"

    def embed(self, h, r, t):
        cat = lambda e1, i1, e2, i2: torch.cat([e1.weight.index_select(0, i1), e2.weight.index_select(0, i2)], 1)
        return (cat(self.ent_head_embeddings, h, self.ent_head_embeddings, t),
                cat(self.rel_embeddings, r, self.rel_inv_embeddings, r),
                cat(self.ent_tail_embeddings, t, self.ent_tail_embeddings, h))


class QuatE(DistMult):
    """pointwise.py:595-768.  energy = -sum((h (x) r/|r|) . t) with element-wise quaternions (s, x, y, z)."""
    kernel_name = "quate"
    default_reg, reg_abs = "N3", True

    def __init__(self, **kwargs):
        PointwiseModel.__init__(self, self.__class__.__name__.lower())
        self.__dict__.update(self.load_params(["tot_entity", "tot_relation", "hidden_size", "lmbda"], kwargs))
        k = self.hidden_size
        for c in "sxyz":
            setattr(self, "ent_%s_embedding" % c, NamedEmbedding("ent_%s_embedding" % c, self.tot_entity, k))
        # the reference overwrites the four rel_{s,x,y,z} weights with _quaternion_init(tot_entity, k) arrays before
        # the Xavier pass (pointwise.py:653-668), so those tables (and its checkpoints) carry tot_entity rows
        for c in "sxyz":
            setattr(self, "rel_%s_embedding" % c, NamedEmbedding("rel_%s_embedding" % c, self.tot_entity, k))
        self.rel_w_embedding = NamedEmbedding("rel_w_embedding", self.tot_relation, k)
        self.fc = nn.Linear(100, 50, bias=False)  # unused by forward; present in the reference's state_dict
        self.ent_dropout = nn.Dropout(0)
        self.rel_dropout = nn.Dropout(0)
        self.bn = nn.BatchNorm1d(k)
        self.parameter_list = [getattr(self, "%s_%s_embedding" % (a, c)) for a in ("ent", "rel") for c in "sxyz"]
        self.parameter_list.append(self.rel_w_embedding)
        _xavier(*self.parameter_list)
        self.loss = Criterion.pointwise_logistic

    def embed(self, h, r, t):
        e = [getattr(self, "ent_%s_embedding" % c) for c in "sxyz"]
        q = [getattr(self, "rel_%s_embedding" % c) for c in "sxyz"]
        return tuple(x(h) for x in e) + tuple(x(t) for x in e) + tuple(x(r) for x in q)

    def get_reg(self, h, r, t, reg_type=None):
        rt = (reg_type or self.default_reg).lower()
        if rt not in ("f2", "n3"):
            raise NotImplementedError("Unknown regularizer type: %s" % rt)
        p = 2 if rt == "f2" else 3
        return self.lmbda * sum(torch.mean(torch.abs(x) ** p) for x in self.embed(h, r, t))

    def kernel_lmbda(self):
        return self.lmbda / self.hidden_size  # means over all B*k elements, not over the B rows

    def kernel_reg_type(self, reg_type=None):
        rt = (reg_type or self.default_reg).lower()
        if rt == "f2":
            return L.REG_F2
        if rt == "n3":
            return L.REG_N3_ABS
        raise NotImplementedError("Unknown regularizer type: %s" % rt)


class OctonionE(DistMult):
    """pointwise.py:772-1001.  energy = -sum(o(h, r / |r|) . t) with element-wise octonions of 8 components (the product built from
    quaternion products and conjugates, _omult).  rel_w_embedding is in parameter_list and the state dict but unused by forward.

    The kernels take the 8 entity and the 8 relation tables as two component blocks (include/kge_hip.h, KGE_OCTONIONE).  The
    model keeps its tables in that layout -- at construction and after every .to() / .cuda() -- so descriptors pass them by
    address; tables moved out of it (a caller re-binding .data) still work through a packed copy (kernels.octonion_desc)."""
    kernel_name = "octonione"
    default_reg, reg_abs = "N3", True

    def __init__(self, **kwargs):
        PointwiseModel.__init__(self, self.__class__.__name__.lower())
        self.__dict__.update(self.load_params(["tot_entity", "tot_relation", "hidden_size", "lmbda"], kwargs))
        k = self.hidden_size
        for i in range(1, 9):
            setattr(self, "ent_embedding_%d" % i, NamedEmbedding("ent_embedding_%d" % i, self.tot_entity, k))
        for i in range(1, 9):
            setattr(self, "rel_embedding_%d" % i, NamedEmbedding("rel_embedding_%d" % i, self.tot_relation, k))
        self.rel_w_embedding = NamedEmbedding("rel_w_embedding", self.tot_relation, k)
        self.parameter_list = ([getattr(self, "ent_embedding_%d" % i) for i in range(1, 9)]
                               + [getattr(self, "rel_embedding_%d" % i) for i in range(1, 9)] + [self.rel_w_embedding])
        _xavier(*self.parameter_list)
        self.loss = Criterion.pointwise_logistic
        self._to_blocks()

    def _to_blocks(self):
        """Re-home ent_embedding_1..8 and rel_embedding_1..8 into one component block each (segments rounded up to 4 floats)."""
        for group in (self.parameter_list[0:8], self.parameter_list[8:16]):
            w = [e.weight for e in group]
            if w[0].dtype != torch.float32:
                continue
            stride = (w[0].numel() + 3) // 4 * 4
            if all(x.device == w[0].device and x.is_contiguous() and x.data_ptr() == w[0].data_ptr() + 4 * c * stride
                   for c, x in enumerate(w)):
                continue
            blk = torch.zeros(8 * stride, dtype=torch.float32, device=w[0].device)
            for c, x in enumerate(w):
                v = blk[c * stride:c * stride + x.numel()].view_as(x)
                v.copy_(x.data)
                x.data = v

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._to_blocks()   # .to() / .cuda() move every table on its own
        return out

    def make_desc(self, weights=None, grads=None):
        if weights is None:
            weights = [p.weight for p in self.parameter_list]
        return K.octonion_desc(list(weights), None if grads is None else list(grads), tot_entity=self.tot_entity,
                               tot_relation=self.tot_relation, dim=self.hidden_size)

    def embed(self, h, r, t):
        e = self.parameter_list[0:8]
        q = self.parameter_list[8:16]
        return tuple(x(h) for x in e) + tuple(x(t) for x in e) + tuple(x(r) for x in q)

    def get_reg(self, h, r, t, reg_type="N3"):
        """pointwise.py:894-956: lmbda * sum over the 24 gathered row sets of mean(|x|^p) (means over B * d; raw r, rel_w excluded)."""
        rt = reg_type.lower()
        if rt not in ("f2", "n3"):
            raise NotImplementedError("Unknown regularizer type: %s" % reg_type)
        p = 2 if rt == "f2" else 3
        return self.lmbda * sum(torch.mean(torch.abs(x) ** p) for x in self.embed(h, r, t))

    def kernel_lmbda(self):
        return self.lmbda / self.hidden_size  # means over all B*k elements, not over the B rows

    def kernel_reg_type(self, reg_type=None):
        rt = (reg_type or self.default_reg).lower()
        if rt == "f2":
            return L.REG_F2
        if rt == "n3":
            return L.REG_N3_ABS
        raise NotImplementedError("Unknown regularizer type: %s" % rt)


class ConvKB(PointwiseModel):
    """pointwise.py:241-318.  preds = fc1(cat_j conv_j(stack(h, r, t))) with NO activation and NO dropout in between (the published
    ConvKB has both; this follows the reference), so the score is affine in the three rows: the kernels collapse the filters and
    fc1 into three vectors and a constant (csrc/kge_convkb.hip).

    conv_list is a plain Python list, as in the reference: the filters are in neither parameters() nor state_dict(), no optimiser
    steps them, and they are built on the constructor's `device`.  Trained state is the two tables plus fc1."""
    kernel_name = "convkb"

    def __init__(self, **kwargs):
        super().__init__(self.__class__.__name__.lower())
        self.__dict__.update(self.load_params(["tot_entity", "tot_relation", "hidden_size", "num_filters", "filter_sizes", "device"],
                                              kwargs))
        k, F = self.hidden_size, self.num_filters
        self.filter_sizes = [int(s) for s in self.filter_sizes]
        self.ent_embeddings = NamedEmbedding("ent_embedding", self.tot_entity, k)
        self.rel_embeddings = NamedEmbedding("rel_embedding", self.tot_relation, k)
        _xavier(self.ent_embeddings, self.rel_embeddings)
        self.parameter_list = [self.ent_embeddings, self.rel_embeddings]
        self.conv_list = [nn.Conv2d(1, F, (3, s), stride=(1, 1)).to(self.device) for s in self.filter_sizes]
        self.fc1 = nn.Linear(in_features=F * sum(k - s + 1 for s in self.filter_sizes), out_features=1, bias=True)
        self.loss = Criterion.pointwise_logistic
        self._packed = None

    def trainable_tensors(self):
        return [self.ent_embeddings.weight, self.rel_embeddings.weight, self.fc1.weight, self.fc1.bias]

    def packed_filters(self, device):
        """(conv_w, conv_b) on `device`: the flattened conv_list[j].weight / .bias tensors concatenated in list order.  Rebuilt when
        the tables moved to another device or a filter was written to."""
        stamp = (torch.device(device), tuple((c.weight._version, c.bias._version) for c in self.conv_list))
        if self._packed is None or self._packed[0] != stamp:
            w = torch.cat([c.weight.detach().reshape(-1) for c in self.conv_list]).to(device=device, dtype=torch.float32).contiguous()
            b = torch.cat([c.bias.detach().reshape(-1) for c in self.conv_list]).to(device=device, dtype=torch.float32).contiguous()
            self._packed = (stamp, w, b)
        return self._packed[1], self._packed[2]

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._packed = None   # .to() / .cuda() moved the tables; the packed filters follow them at the next descriptor
        return out

    def make_desc(self, weights=None, grads=None):
        if weights is None:
            weights = self.trainable_tensors()
        weights = list(weights)
        conv_w, conv_b = self.packed_filters(weights[0].device)
        return K.convkb_desc(weights, None if grads is None else list(grads), tot_entity=self.tot_entity,
                             tot_relation=self.tot_relation, dim=self.hidden_size, num_filters=self.num_filters,
                             filter_sizes=self.filter_sizes, conv_w=conv_w, conv_b=conv_b)

    def embed(self, h, r, t):
        return self.ent_embeddings(h), self.rel_embeddings(r), self.ent_embeddings(t)

    def forward(self, h, r, t):
        return torch.ops.kge.convkb_score(self._kge_op_key, h, r, t, self.trainable_tensors())

    def kernel_lmbda(self):
        return 0.0

    def kernel_reg_type(self, reg_type=None):
        return L.REG_NONE


class MuRP(PointwiseModel):
    """pointwise.py:1004-1133, float64 throughout.  preds = -(d(u_m, v_m)^2 - bs[h] - bo[t]) with u_m the head mapped to the tangent
    space, scaled by wu[r] and mapped back, v_m = p_sum(t, r), all through the reference's own maps (csrc/kge_murp.hip):
    arsech(x) = log((1 + sqrt(1 - x^2)) / x) where the Poincare ball has artanh, 1 / cosh where it has tanh.  They are what the
    reference's checkpoints were trained with and are kept.  preds is a logit (higher = more plausible); the loss is BCE-with-logits.

    Tables, names, dtypes, padding_idx and the order of the random draws are the reference's, so the initial state under given torch
    and numpy seeds is bit-identical to it.  state_dict order: wu, bs, bo, ent_embeddings.weight, rel_embeddings.weight;
    parameter_list holds the two embeddings only; all five are trained (trainable_tensors).  `lmbda` is required and unused.

    rank_order (class attribute, default 0; set it on an instance): the order predict_*_rank lists and the Evaluator's ranks use.
    0 = ascending score, as the reference's predict_*_rank return them (the least plausible candidate first): a rank is the true
    entity's position in that list.  1 = most plausible first.  The reference's MetricCalculator walks a list from its END, so the
    metrics the reference reports for MuRP are the rank_order = 1 ranks.  topk is ignored, as in the reference: the lists are full."""
    kernel_name = "murp"
    rank_order = 0
    higher_is_better = True   # preds is a logit; rank_order does not enter the batched link prediction

    def __init__(self, **kwargs):
        super().__init__(self.__class__.__name__.lower())
        self.__dict__.update(self.load_params(["tot_entity", "tot_relation", "hidden_size", "lmbda"], kwargs))
        k = self.hidden_size
        self.device = kwargs["device"]
        # (the draws in the reference's order: each nn.Embedding draws its own fp32 init before its data is replaced)
        self.ent_embeddings = NamedEmbedding("ent_embedding", self.tot_entity, k, padding_idx=0)
        self.ent_embeddings.weight.data = 1e-3 * torch.randn((self.tot_entity, k), dtype=torch.double, device=self.device)
        self.rel_embeddings = NamedEmbedding("rel_embedding", self.tot_relation, k, padding_idx=0)
        self.rel_embeddings.weight.data = 1e-3 * torch.randn((self.tot_relation, k), dtype=torch.double, device=self.device)
        self.wu = nn.Parameter(torch.tensor(np.random.uniform(-1, 1, (self.tot_relation, k)), dtype=torch.double, requires_grad=True,
                                            device=self.device))
        self.bs = nn.Parameter(torch.zeros(self.tot_entity, dtype=torch.double, requires_grad=True, device=self.device))
        self.bo = nn.Parameter(torch.zeros(self.tot_entity, dtype=torch.double, requires_grad=True, device=self.device))
        self.parameter_list = [self.ent_embeddings, self.rel_embeddings]
        self.loss = Criterion.pointwise_bce

    def trainable_tensors(self):
        return [self.wu, self.bs, self.bo, self.ent_embeddings.weight, self.rel_embeddings.weight]

    def make_desc(self, weights=None, grads=None):
        if weights is None:
            weights = self.trainable_tensors()
        return K.murp_desc(list(weights), None if grads is None else list(grads), tot_entity=self.tot_entity,
                           tot_relation=self.tot_relation, dim=self.hidden_size, rank_order=self.rank_order)

    def embed(self, h, r, t):
        return self.ent_embeddings(h), self.rel_embeddings(r), self.ent_embeddings(t)

    def forward(self, h, r, t):
        return torch.ops.kge.murp_score(self._kge_op_key, h, r, t, self.trainable_tensors())

    def _ranked(self, scores):
        # (stable: candidates that tie -- rows saturated at the last clamp -- keep their id order, in either direction)
        return torch.sort(scores, descending=bool(self.rank_order), stable=True)[1]

    def predict_tail_rank(self, h, r, topk=-1):
        del topk
        return self._ranked(self._sweep(h, r, torch.zeros_like(h), 0))

    def predict_head_rank(self, t, r, topk=-1):
        del topk
        return self._ranked(self._sweep(torch.zeros_like(t), r, t, 1))

    def predict_rel_rank(self, h, t, topk=-1):
        del topk
        rel = torch.arange(self.tot_relation, dtype=torch.int64, device=h.device)
        with torch.no_grad():
            return self._ranked(K.murp_score_forward(self.make_desc(), h.view(-1)[:1].expand(rel.numel()).contiguous(), rel,
                                                     t.view(-1)[:1].expand(rel.numel()).contiguous()))

    def kernel_lmbda(self):
        return 0.0

    def kernel_reg_type(self, reg_type=None):
        return L.REG_NONE
