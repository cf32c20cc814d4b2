"""Drop-in projection (1-N) models mirroring pykg2vec/models/projection.py, scored by HIP kernels.  TuckER and ProjE_pointwise are the
models of that family whose body is no convolution stack.  TuckER: two L2 normalisations and a contraction with the shared core
(csrc/kge_tucker.hip) in front of the 1-N head (csrc/kge_head.hip).  ProjE_pointwise: a pointwise tanh body whose loss reads only the
labelled columns of the 1-N product (csrc/kge_proje.hip); it is the one model here that trains with sampled negatives on this path.
ConvE, InteractE, HypER and AcrE keep their PyTorch layers and call the head themselves."""
import torch

from . import _lib as L  # noqa: F401
from . import kernels as K
from . import ops  # noqa: F401  (registers torch.ops.kge.*)
from .criterion import Criterion
from .kgmeta import NamedEmbedding, ProjectionModel


class TuckER(ProjectionModel):
    """projection.py:259-344.  forward(e, r, direction) = sigmoid(normalize(normalize(ent[e]) M_r) @ ent.T) with M_r = rel[r] . W and the
    reference's three dropouts.  The dropout masks come from Philox counters keyed by (dropout_seed, dropout_offset) instead of
    torch's generator (include/kge_hip.h spells the counters out): forward() under train() advances dropout_offset by one per call, so
    that successive calls draw fresh masks and a run is reproducible from dropout_seed; under eval() nothing is drawn."""
    kernel_name = "tucker"

    def __init__(self, **kwargs):
        super().__init__(self.__class__.__name__.lower())
        param_list = ["tot_entity", "tot_relation", "ent_hidden_size", "rel_hidden_size", "lmbda", "input_dropout", "hidden_dropout1",
                      "hidden_dropout2"]
        self.__dict__.update(self.load_params(param_list, kwargs))
        self.d1, self.d2 = int(self.ent_hidden_size), int(self.rel_hidden_size)
        # (the reference replaces the three rates by nn.Dropout modules of the same names; here the rates stay numbers)
        self.dropouts = (float(self.input_dropout), float(self.hidden_dropout1), float(self.hidden_dropout2))
        self.ent_embeddings = NamedEmbedding("ent_embedding", self.tot_entity, self.d1)
        self.rel_embeddings = NamedEmbedding("rel_embedding", self.tot_relation, self.d2)
        self.W = NamedEmbedding("W", self.d2, self.d1 * self.d1)
        for p in (self.ent_embeddings, self.rel_embeddings, self.W):
            torch.nn.init.xavier_uniform_(p.weight)
        self.parameter_list = [self.ent_embeddings, self.rel_embeddings, self.W]
        self.loss = Criterion.multi_class_bce
        self.dropout_seed = int(kwargs.get("seed", 0) or 0)
        self.dropout_offset = 0

    def make_desc(self, weights=None, grads=None, train=None, seed=None, offset=None):
        if weights is None:
            weights = self.trainable_tensors()
        return K.tucker_desc(list(weights), None if grads is None else list(grads), tot_entity=self.tot_entity,
                             tot_relation=self.tot_relation, d1=self.d1, d2=self.d2, dropouts=self.dropouts,
                             train=self.training if train is None else train, seed=self.dropout_seed if seed is None else seed,
                             offset=self.dropout_offset if offset is None else offset)

    def fused_projection_step(self, K, desc, h, r, t, hr_t_csr, tr_h_csr, neg, config, loss_buf):
        K.tucker_train_bce(desc, h, r, t, *hr_t_csr, *tr_h_csr, getattr(config, "label_smoothing", None), loss_buf)

    def forward(self, e1, r, direction="head"):
        assert direction in ("head", "tail"), "Unknown forward direction"
        offset = -1   # eval(): no dropout
        if self.training and any(p > 0.0 for p in self.dropouts):
            offset = self.dropout_offset
            self.dropout_offset += 1
        x, _saved = torch.ops.kge.tucker_body(self._kge_op_key, e1, r, self.dropout_seed, offset, self.trainable_tensors())
        return torch.ops.kge.one_to_n_scores(x, self.ent_embeddings.weight, None, False)

    def predict_tail_rank(self, e, r, topk=-1):
        _, rank = torch.topk(-self.forward(e, r, direction="tail"), k=topk)
        return rank

    def predict_head_rank(self, e, r, topk=-1):
        _, rank = torch.topk(-self.forward(e, r, direction="head"), k=topk)
        return rank


class ProjE_pointwise(ProjectionModel):
    """projection.py:128-257.  forward(e, r, er_e2, direction) is the SCALAR loss of one direction against the dense label rows er_e2 in
    {-1, 0, +1}: x = dropout(tanh(ent[e] o De_s + rel[r] o Dr_s + bc_s)), s = sigmoid(x @ ent.T), loss = -sum log(clamp(s)) [y = +1]
    - sum log(clamp(1 - s)) [y = -1]; "tail" uses f1 (De1 / Dr1 / bc1), "head" f2.  The reference draws this dropout with train=True
    whatever the module's mode, and so does forward() here: whenever hidden_dropout > 0 it draws the Philox mask of (dropout_seed,
    dropout_offset) (include/kge_hip.h spells the counters out) and advances dropout_offset by one.  The ranking calls draw nothing.
    The Trainer does not go through forward(): its fused step (kge_proje_train) reads the labelled columns only."""
    kernel_name = "proje"
    dropout_in_eval = True   # the reference's torch.dropout(..., train=True)
    label_negatives = True   # the -1 labels the reference writes for neg_rate > 0 are the model (loss = Criterion.multi_class)

    def __init__(self, **kwargs):
        super().__init__(self.__class__.__name__.lower())
        param_list = ["tot_entity", "tot_relation", "hidden_size", "lmbda", "hidden_dropout"]
        self.__dict__.update(self.load_params(param_list, kwargs))
        k = int(self.hidden_size)
        self.ent_embeddings = NamedEmbedding("ent_embedding", self.tot_entity, k)
        self.rel_embeddings = NamedEmbedding("rel_embedding", self.tot_relation, k)
        self.bc1 = NamedEmbedding("bc1", 1, k)
        self.De1 = NamedEmbedding("De1", 1, k)
        self.Dr1 = NamedEmbedding("Dr1", 1, k)
        self.bc2 = NamedEmbedding("bc2", 1, k)
        self.De2 = NamedEmbedding("De2", 1, k)
        self.Dr2 = NamedEmbedding("Dr2", 1, k)
        self.parameter_list = [self.ent_embeddings, self.rel_embeddings, self.bc1, self.De1, self.Dr1, self.bc2, self.De2, self.Dr2]
        for p in self.parameter_list:
            torch.nn.init.xavier_uniform_(p.weight)
        self._device = kwargs.get("device")   # the reference requires the kwarg; here it defaults to where the weights live
        self.loss = Criterion.multi_class
        self.dropout_seed = int(kwargs.get("seed", 0) or 0)
        self.dropout_offset = 0

    @property
    def device(self):
        return self._device if self._device is not None else self.ent_embeddings.weight.device

    def make_desc(self, weights=None, grads=None, train=None, seed=None, offset=None):
        if weights is None:
            weights = self.trainable_tensors()
        return K.proje_desc(list(weights), None if grads is None else list(grads), tot_entity=self.tot_entity,
                            tot_relation=self.tot_relation, dim=int(self.hidden_size), hidden_dropout=float(self.hidden_dropout),
                            train=True if train is None else train, seed=self.dropout_seed if seed is None else seed,
                            offset=self.dropout_offset if offset is None else offset)

    def fused_projection_step(self, K, desc, h, r, t, hr_t_csr, tr_h_csr, neg, config, loss_buf):
        K.proje_train(desc, h, r, t, *hr_t_csr, *tr_h_csr, neg, self.lmbda, loss_buf)

    def get_reg(self, h, r, t):
        return self.lmbda * (torch.sum(torch.abs(self.De1.weight) + torch.abs(self.Dr1.weight)) +
                             torch.sum(torch.abs(self.De2.weight) + torch.abs(self.Dr2.weight)) +
                             torch.sum(torch.abs(self.ent_embeddings.weight)) + torch.sum(torch.abs(self.rel_embeddings.weight)))

    def _body(self, e, r, side, offset):
        return torch.ops.kge.proje_body(self._kge_op_key, e, r, side, self.dropout_seed, offset, self.trainable_tensors())

    def forward(self, e, r, er_e2, direction="tail"):
        assert direction in ("head", "tail"), "Unknown forward direction"
        offset = -1
        if float(self.hidden_dropout) > 0.0:   # torch.dropout(..., train=True): drawn under eval() too
            offset = self.dropout_offset
            self.dropout_offset += 1
        x = self._body(e, r, 0 if direction == "tail" else 1, offset)
        s = torch.ops.kge.one_to_n_scores(x, self.ent_embeddings.weight, None, False)
        zero = torch.zeros(1, dtype=s.dtype, device=s.device)
        left = -torch.sum(torch.log(torch.clamp(s, 1e-10, 1.0)) * torch.max(zero, er_e2))
        right = -torch.sum(torch.log(torch.clamp(1 - s, 1e-10, 1.0)) * torch.max(zero, torch.neg(er_e2)))
        return left + right

    def f1(self, h, r):
        """tanh(h o De1 + r o Dr1 + bc1) on embedding ROWS h, r [m, k] (the reference's signature; plain torch, as g is)."""
        return torch.tanh(h * self.De1.weight + r * self.Dr1.weight + self.bc1.weight)

    def f2(self, t, r):
        return torch.tanh(t * self.De2.weight + r * self.Dr2.weight + self.bc2.weight)

    @staticmethod
    def g(f, w):
        return torch.sigmoid(torch.matmul(f, w.T))

    def _predict(self, e, r, side, topk):
        x = self._body(e.view(-1), r.view(-1), side, -1)
        s = torch.ops.kge.one_to_n_scores(x, self.ent_embeddings.weight, None, False)
        _, rank = torch.topk(-s, k=topk)
        return rank

    def predict_tail_rank(self, h, r, topk=-1):
        return self._predict(h, r, 0, topk)

    def predict_head_rank(self, t, r, topk=-1):
        return self._predict(t, r, 1, topk)
