"""Model base classes mirroring pykg2vec/models/KGMeta.py:14-80 and models/Domain.py:8-17, with `forward`
routed to the HIP scorer through the custom op `kge::score` (ops.py; dense gradients, like nn.Embedding(sparse=False))."""
import torch
import torch.nn as nn

from . import kernels as K
from . import ops
from .common import TrainingStrategy


class NamedEmbedding(nn.Embedding):
    """nn.Embedding carrying a human-readable `.name` (models/Domain.py:8-17)."""

    def __init__(self, name, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._name = name

    @property
    def name(self):
        return self._name


class Model:
    """KGMeta.Model (models/KGMeta.py:14-38)."""

    kernel_name = None  # key into kernels.MODEL_IDS

    def load_params(self, param_list, kwargs):
        for param_name in param_list:
            if param_name not in kwargs:
                raise Exception("hyperparameter %s not found!" % param_name)
            self.database[param_name] = kwargs[param_name]
        return self.database

    def get_reg(self, h, r, t, **kwargs):
        return 0.0

    # ---- HIP plumbing
    def desc_kwargs(self):
        raise NotImplementedError

    def trainable_tensors(self):
        """The tensors a Trainer re-homes into its flat parameter buffer and steps, in descriptor order: the weights of
        `parameter_list`, unless a model trains more than its tables (ConvKB: fc1)."""
        return [p.weight for p in self.parameter_list]

    def make_desc(self, weights=None, grads=None):
        if weights is None:
            weights = [p.weight for p in self.parameter_list]
        return K.make_desc(self.kernel_name, list(weights), None if grads is None else list(grads),
                           tot_entity=self.tot_entity, tot_relation=self.tot_relation, **self.desc_kwargs())

    def forward(self, h, r, t):
        """Energies of the triples (h, r, t) through the dispatcher-registered op `kge::score` (ops.py): differentiable w.r.t. the
        tables (dense gradients, like nn.Embedding(sparse=False)), visible to torch.ops / torch.compile."""
        return torch.ops.kge.score(self._kge_op_key, h, r, t, [p.weight for p in self.parameter_list])

    def _register_op_handle(self):
        """The integer handle torch.ops.kge.score finds this model by: taken once per object (construction, unpickling, deepcopy),
        so that forward() reads a plain attribute -- a constant for torch.compile -- instead of touching the weak registry."""
        self.__dict__.pop("_kge_op_key", None)
        ops.register_model(self)

    def _restore(self, state):   # unpickling / deepcopy: the copy is a new object and needs its own handle
        nn.Module.__setstate__(self, state)
        self._register_op_handle()

    # ---- the reference Evaluator's optional hooks (utils/evaluator.py:250-252,263-265): candidate ids by
    # descending energy, shape [1, topk]; served by the sweep kernels instead of forward() over E id tensors.
    def _sweep(self, h, r, t, side):
        """float32 [E]: energies of (h, r, e) (side 0) or of (e, r, t) (side 1) for every entity e -- ONE sweep (round 5 ran both
        and threw one away); the id of the swept position is a placeholder the kernel never reads."""
        h0, r0, t0 = h.view(-1)[0], r.view(-1)[0], t.view(-1)[0]
        trip = torch.stack([h0, r0, t0]).view(1, 3).contiguous()
        return K.eval_sweep_scores_side(self.make_desc(), trip, side)[0]

    higher_is_better = False   # what forward() / score_rows return: an energy (lower = more plausible) or a logit / probability

    def score_rows(self, queries, side):
        """[n, E] scores of int64 `queries` [n, 3] against every entity e, no gradient, the model's evaluation form: side 0 scores
        (h_i, r_i, e), side 1 scores (e, r_i, t_i); the id in the swept column is a placeholder.  Rows may be a strided view.
        The one place the batched link prediction (Evaluator.predict_*) gets its rows from."""
        assert side in (0, 1), "side 0 = tails, 1 = heads"
        queries = queries.contiguous()
        with torch.no_grad():
            if self.kernel_name == "rescal":   # the reference's forward renormalises both tables during eval too, as rank_all does
                K.rescal_normalize(self.ent_embeddings.weight.data, self.rel_matrices.weight.data, self.hidden_size)
            desc = self.make_desc()
            if self.kernel_name != "transr":
                return K.eval_sweep_scores_side(desc, queries, side)
            # TransR's sweep projects the candidates by ONE relation matrix per call: a call per relation (one host read of the
            # distinct relations), rows scattered back
            out = torch.empty((queries.shape[0], int(self.tot_entity)), dtype=torch.float32, device=queries.device)
            for rel in torch.unique(queries[:, 1]).tolist():
                idx = torch.nonzero(queries[:, 1] == rel).view(-1)
                out[idx] = K.eval_sweep_scores_side(desc, queries[idx].contiguous(), side)
            return out

    # ---- the rows of the nearest-neighbour search (Evaluator.nearest_*): what "the embedding of entity e" is, per model
    # THE rule, by NamedEmbedding name: a table of parameter_list is entity-indexed when its name starts with one of the first
    # prefixes or is one of the first names, relation-indexed likewise with the second.  Every model, by hand: TransE / TransM /
    # HoLE / DistMult / ConvKB / MuRP / TuckER / ConvE / HypER / InteractE / AcrE / ProjE take ent_embedding(s) | rel_embedding(s)
    # (ConvE's b [1, E], ProjE's bc / De / Dr, TuckER's W, HypER's filters are neither); TransR + rel_matrix, Rescal rel_matrices
    # (the flattened matrices); TransH + w (the normal vectors); TransD + ent_mappings | rel_mappings; RotatE
    # ent_embeddings_real, ent_embeddings_imag | rel_embeddings_real; KG2E ent_embeddings_mu, _sigma | rel_embeddings_mu, _sigma;
    # Complex(N3) emb_e_real, emb_e_img | emb_rel_real, emb_rel_img; ANALOGY all three of each; CP sub_embedding, obj_embedding |
    # rel_embedding; SimplE(_ignr) ent_head_, ent_tail_embedding | rel_, rel_inv_embedding; QuatE ent_{s,x,y,z}_embedding |
    # rel_{s,x,y,z,w}_embedding; OctonionE ent_embedding_1..8 | rel_embedding_1..8, rel_w_embedding; NTN / SLM / SME(_BL)
    # ent_embedding | rel_embedding (mr*, br, mu*, mv*, bu, bv are indexed by neither).
    _MATRIX_RULE = {"entity": (("ent_", "emb_e_"), ("sub_embedding", "obj_embedding")),
                    "relation": (("rel_", "emb_rel_"), ("w",))}

    def _index_matrix(self, kind, tables):
        prefixes, names = self._MATRIX_RULE[kind]
        rows = int(self.tot_entity if kind == "entity" else self.tot_relation)
        by_name = {p.name: p for p in self.parameter_list}
        if tables is None:
            picked = [p for p in self.parameter_list if p.name.startswith(prefixes) or p.name in names]
        else:
            missing = [n for n in tables if n not in by_name]
            if missing:
                raise KeyError("%s has no table named %s (it has %s)" % (type(self).__name__, missing, sorted(by_name)))
            picked = [by_name[n] for n in tables]
        if not picked:
            raise ValueError("%s has no %s-indexed table" % (type(self).__name__, kind))
        parts = []
        for p in picked:
            w = p.weight.detach()
            if w.shape[0] < rows:
                raise ValueError("table %s has %d rows, fewer than the %d %s ids" % (p.name, w.shape[0], rows, kind))
            # a table with more rows than ids (the reciprocal relations of ConvE / AcrE behind the relations): the ids' own rows
            parts.append(w[:rows].to(torch.float32))
        return parts[0] if len(parts) == 1 else torch.cat(parts, 1)

    def entity_matrix(self, tables=None):
        """float32 [tot_entity, D]: the model's entity-indexed tables of parameter_list (picked by name, _MATRIX_RULE), concatenated
        along the columns in that order; a single float32 table is returned as it is, without a copy.  tables: explicit
        NamedEmbedding names instead.  MuRP's float64 tables are converted to float32 for the search."""
        return self._index_matrix("entity", tables)

    def relation_matrix(self, tables=None):
        """entity_matrix for the relation-indexed tables: float32 [tot_relation, D]."""
        return self._index_matrix("relation", tables)

    def predict_tail_rank(self, h, r, topk=-1):
        _, rank = torch.topk(self._sweep(h, r, torch.zeros_like(h), 0), k=topk)
        return rank.view(1, -1)

    def predict_head_rank(self, t, r, topk=-1):
        _, rank = torch.topk(self._sweep(torch.zeros_like(t), r, t, 1), k=topk)
        return rank.view(1, -1)


class PairwiseModel(nn.Module, Model):
    forward = Model.forward  # nn.Module.forward precedes Model.forward in the MRO
    __setstate__ = Model._restore

    def __init__(self, model_name):
        super().__init__()
        self.model_name = model_name
        self.training_strategy = TrainingStrategy.PAIRWISE_BASED
        self.database = {}
        self._register_op_handle()


class PointwiseModel(nn.Module, Model):
    forward = Model.forward
    __setstate__ = Model._restore

    def __init__(self, model_name):
        super().__init__()
        self.model_name = model_name
        self.training_strategy = TrainingStrategy.POINTWISE_BASED
        self.database = {}
        self._register_op_handle()


class ProjectionModel(nn.Module, Model):
    """The base of the 1-N models (models/KGMeta.py: ProjectionModel): forward(e, r, direction) returns [B, E] predictions."""
    __setstate__ = Model._restore
    dropout_in_eval = False   # True: the model draws its dropout masks whatever the module's mode
    label_negatives = False   # True: the loss reads sampled negatives as -1 labels (the generator draws them); else neg_rate > 0 is refused
    higher_is_better = True   # forward() / score_rows return sigmoid probabilities

    def _eval_body(self, e, r, side):
        """x [n, k]: the model's body in evaluation form (no dropout, running statistics) whatever self.training says; nothing is
        drawn and dropout_offset does not move."""
        raise NotImplementedError("%s has no evaluation body" % type(self).__name__)

    def _head_bias(self):
        return None

    def score_rows(self, queries, side):
        """Model.score_rows for the 1-N models: the evaluation-form body of (h_i, r_i) (side 0) or (t_i, r_i) (side 1) + the head."""
        assert side in (0, 1), "side 0 = tails, 1 = heads"
        e, r = queries[:, 2 if side else 0].contiguous(), queries[:, 1].contiguous()
        with torch.no_grad():
            return torch.ops.kge.one_to_n_scores(self._eval_body(e, r, side), self.ent_embeddings.weight, self._head_bias(), False)

    def fused_projection_step(self, K, desc, h, r, t, hr_t_csr, tr_h_csr, neg, config, loss_buf):
        """One training step in ONE library call: adds to loss_buf and to the descriptor's gradients.  hr_t_csr / tr_h_csr: the
        label CSRs of the batch; neg: the batch's negative label ids where label_negatives, else None."""
        raise NotImplementedError("%s has no fused projection step" % type(self).__name__)

    def __init__(self, model_name):
        super().__init__()
        self.model_name = model_name
        self.training_strategy = TrainingStrategy.PROJECTION_BASED
        self.database = {}
        self._register_op_handle()
