"""Drop-in projection (1-N) models mirroring pykg2vec/models/projection.py, scored by HIP kernels.  TuckER is the one model of that
family whose body is no convolution stack: two L2 normalisations and a contraction with the shared core (csrc/kge_tucker.hip), in
front of the 1-N head (csrc/kge_head.hip).  ConvE, InteractE, HypER and AcrE keep their PyTorch layers and call the head
themselves."""
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
