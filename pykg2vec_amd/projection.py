"""Drop-in projection (1-N) models mirroring pykg2vec/models/projection.py, scored by HIP kernels.  TuckER: two L2 normalisations and a contraction with the shared core
(csrc/kge_tucker.hip) in front of the 1-N head (csrc/kge_head.hip).  ProjE_pointwise: a pointwise tanh body whose loss reads only the
labelled columns of the 1-N product (csrc/kge_proje.hip); it is the one model here that trains with sampled negatives on this path.
ConvE: batch norm, a 3 x 3 convolution, a fully connected layer on the matrix cores and two more batch norms (csrc/kge_conve.hip) in
front of the head with its bias b; its torch layers are holders of parameters and buffers only.  HypER: the same stack with a
convolution filter that a second linear layer computes per row from the relation embedding, and padding_idx = 0 on both tables
(csrc/kge_hyper.hip).  InteractE: chequer permutations of [ent[e] | rel[r]], a depthwise convolution with circular padding whose
filters the permutations share, and the same fc / batch-norm tail (csrc/kge_interacte.hip).  AcrE: three dilated 3 x 3 convolutions
chained with a residual, the two channel-mixing ones as implicit GEMMs on the matrix cores, and the same tail (csrc/kge_acre.hip); in
its parallel way three convolutions of the same input feed a shared 1600 -> 400 gate, a GEMM over the (row, channel) pairs."""
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

    def _eval_body(self, e, r, side):
        return torch.ops.kge.tucker_body(self._kge_op_key, e, r, self.dropout_seed, -1, self.trainable_tensors())[0]

    def predict_tail_rank(self, e, r, topk=-1):
        _, rank = torch.topk(-self.forward(e, r, direction="tail"), k=topk)
        return rank

    def predict_head_rank(self, e, r, topk=-1):
        _, rank = torch.topk(-self.forward(e, r, direction="head"), k=topk)
        return rank


class Conv1NModel(ProjectionModel):
    """What ConvE, HypER, InteractE and AcrE share on the host: three batch norms bn0 / bn1 / bn2 whose running buffers the training
    form updates, one descriptor builder K.<kernel_name>_desc fed from make_desc, one body op torch.ops.kge.<kernel_name>_body in front
    of the 1-N head, one fused step K.<kernel_name>_train_bce.  A subclass supplies its constructor, trainable_tensors() in
    state-dict order, _geometry() (the model's own keywords of its descriptor builder) and _head_bias(); ConvE also its _direction."""

    def _geometry(self):
        raise NotImplementedError

    def _head_bias(self):
        raise NotImplementedError

    def _direction(self, direction, e):
        """The body op's direction argument: the mask row of the call's first row (the "head" rows follow the "tail" rows)."""
        return 0 if direction == "tail" else e.numel()

    def _norms(self):
        return (self.bn0, self.bn1, self.bn2)

    def running_buffers(self):
        return [t for bn in self._norms() for t in (bn.running_mean, bn.running_var)]

    def make_desc(self, weights=None, grads=None, train=None, seed=None, offset=None):
        if weights is None:
            weights = self.trainable_tensors()
        norms = self._norms()
        return getattr(K, self.kernel_name + "_desc")(
            list(weights), self.running_buffers(), None if grads is None else list(grads), tot_entity=self.tot_entity,
            tot_relation=self.tot_relation, dropouts=self.dropouts, eps=[bn.eps for bn in norms], momentum=[bn.momentum for bn in norms],
            train=self.training if train is None else train, seed=self.dropout_seed if seed is None else seed,
            offset=self.dropout_offset if offset is None else offset, **self._geometry())

    def _count_batches(self, calls):
        for bn in self._norms():
            bn.num_batches_tracked += calls

    def fused_projection_step(self, K, desc, h, r, t, hr_t_csr, tr_h_csr, neg, config, loss_buf):
        getattr(K, self.kernel_name + "_train_bce")(desc, h, r, t, *hr_t_csr, *tr_h_csr, getattr(config, "label_smoothing", None), loss_buf)
        self._count_batches(2)   # the step is two training forwards

    def embed(self, h, r, t):
        return self.ent_embeddings(h), self.rel_embeddings(r), self.ent_embeddings(t)

    def embed2(self, e, r):
        return self.ent_embeddings(e), self.rel_embeddings(r)

    def forward(self, e, r, direction="tail"):
        assert direction in ("head", "tail"), "Unknown forward direction"
        offset = -1   # eval(): running statistics, no dropout (ConvE: no bn2 either)
        if self.training:
            offset = self.dropout_offset
            if any(p > 0.0 for p in self.dropouts):
                self.dropout_offset += 1
        body = getattr(torch.ops.kge, self.kernel_name + "_body")
        x, _saved = body(self._kge_op_key, e, r, self._direction(direction, e), self.dropout_seed, offset, self.trainable_tensors())
        if self.training:
            self._count_batches(1)
        return torch.ops.kge.one_to_n_scores(x, self.ent_embeddings.weight, self._head_bias(), False)

    def _eval_body(self, e, r, side):
        body = getattr(torch.ops.kge, self.kernel_name + "_body")
        return body(self._kge_op_key, e, r, self._direction("head" if side else "tail", e), self.dropout_seed, -1, self.trainable_tensors())[0]

    def predict_tail_rank(self, e, r, topk=-1):
        _, rank = torch.topk(-self.forward(e, r, direction="tail"), k=topk)
        return rank

    def predict_head_rank(self, e, r, topk=-1):
        _, rank = torch.topk(-self.forward(e, r, direction="head"), k=topk)
        return rank


class ConvE(Conv1NModel):
    """projection.py:12-125.  forward(e, r, direction) = sigmoid(x @ ent.T + b) with x = relu(bn2(hdrop(fc(flatten(fdrop(relu(bn1(conv(
    idrop(bn0(img)))))))))) and img the [h2, h1] view of ent[e] stacked on that of rel[r] ("tail") or rel[r + tot_relation] ("head").  The
    torch layers (bn0, conv2d_1, bn1, fc, bn2) hold parameters and buffers only, so state_dict() has the reference's keys and shapes and
    loads a reference checkpoint; the arithmetic is csrc/kge_conve.hip.  Under train() a forward normalises with the statistics of its
    own rows, updates the six running buffers and the three num_batches_tracked counters as torch does (under no_grad too), and draws the
    Philox masks of (dropout_seed, dropout_offset) instead of torch's generator (include/kge_hip.h spells the counters out), the mask
    rows of the "head" direction following those of the "tail" direction; with any rate > 0 it then advances dropout_offset by one, as
    TuckER does.  Under eval() bn0 and bn1 use the running buffers, bn2 is skipped (the reference's `if self.training`), nothing is drawn
    and nothing is written."""
    kernel_name = "conve"
    TENSORS = ("ent_embeddings.weight", "rel_embeddings.weight", "b.weight", "bn0.weight", "bn0.bias", "conv2d_1.weight", "conv2d_1.bias",
               "bn1.weight", "bn1.bias", "fc.weight", "fc.bias", "bn2.weight", "bn2.bias")   # descriptor order = state-dict order

    def __init__(self, **kwargs):
        super().__init__(self.__class__.__name__.lower())
        param_list = ["tot_entity", "tot_relation", "hidden_size", "hidden_size_1", "lmbda", "input_dropout", "feature_map_dropout",
                      "hidden_dropout"]
        self.__dict__.update(self.load_params(param_list, kwargs))
        k, h1 = int(self.hidden_size), int(self.hidden_size_1)
        self.hidden_size_2 = k // h1
        # (the reference replaces the three rates by nn.Dropout modules inp_drop / feat_drop / hidden_drop; here the rates stay numbers)
        self.dropouts = (float(self.input_dropout), float(self.feature_map_dropout), float(self.hidden_dropout))
        self.ent_embeddings = NamedEmbedding("ent_embedding", self.tot_entity, k)       # N(0, 1), as the reference leaves them
        self.rel_embeddings = NamedEmbedding("rel_embedding", self.tot_relation * 2, k)  # every relation and its reciprocal
        self.b = NamedEmbedding("b", 1, self.tot_entity)
        self.bn0 = torch.nn.BatchNorm2d(1)
        self.conv2d_1 = torch.nn.Conv2d(1, 32, (3, 3), stride=(1, 1))
        self.bn1 = torch.nn.BatchNorm2d(32)
        # (max(..., 1): a geometry the library refuses must still construct, so that the refusal is the library's sentence)
        self.fc = torch.nn.Linear(max((2 * self.hidden_size_2 - 2) * (h1 - 2) * 32, 1), k)
        self.bn2 = torch.nn.BatchNorm1d(k)
        self.parameter_list = [self.ent_embeddings, self.rel_embeddings, self.b]
        self.loss = Criterion.multi_class_bce
        self.dropout_seed = int(kwargs.get("seed", 0) or 0)
        self.dropout_offset = 0

    def trainable_tensors(self):
        return [self.ent_embeddings.weight, self.rel_embeddings.weight, self.b.weight, self.bn0.weight, self.bn0.bias, self.conv2d_1.weight,
                self.conv2d_1.bias, self.bn1.weight, self.bn1.bias, self.fc.weight, self.fc.bias, self.bn2.weight, self.bn2.bias]

    def _geometry(self):
        return dict(hidden_size=int(self.hidden_size), hidden_size_1=int(self.hidden_size_1))

    def _head_bias(self):
        return self.b.weight

    def _direction(self, direction, e):
        """side: 0 reads rel[r], 1 rel[r + tot_relation]; the mask rows of side 1 follow those of side 0."""
        return 0 if direction == "tail" else 1


class HypER(Conv1NModel):
    """projection.py:508-618.  forward(e, r, direction) = sigmoid(x @ ent.T + b) with x = relu(bn2(hdrop(fc(flatten(fdrop(bn1(conv(
    idrop(bn0(ent[e])), filt)))))))) and filt = fc1(rel[r]) viewed [32, 9]: a 1 x 9 filter per row and channel (the reference's grouped
    convolution and permutes are exactly this).  There is one relation table: `direction` selects no relation row, only the mask rows.
    The torch layers (bn0, bn1, bn2, fc, fc1) hold parameters and buffers only, so state_dict() has the reference's keys, order and
    shapes (the bare parameter b first) and loads a reference checkpoint; the arithmetic is csrc/kge_hyper.hip.  Both embeddings are built
    with padding_idx = 0 and then overwritten by xavier_uniform_, as the reference does: row 0 is an ordinary row in the forward, the
    lookup's gradient of id 0 is dropped (grad of rel row 0 is zero; grad of ent row 0 is the head's share only).  Under train() a
    forward normalises with the statistics of its own rows, updates the six running buffers and the three num_batches_tracked counters
    as torch does, and draws the Philox masks of (dropout_seed, dropout_offset), the mask rows of the "head" direction following those of
    the "tail" direction; with any rate > 0 it then advances dropout_offset by one.  Under eval() all three batch norms use the running
    buffers (bn2 too, unlike ConvE), nothing is drawn and nothing is written."""
    kernel_name = "hyper"
    TENSORS = ("b", "ent_embeddings.weight", "rel_embeddings.weight", "bn0.weight", "bn0.bias", "bn1.weight", "bn1.bias", "bn2.weight",
               "bn2.bias", "fc.weight", "fc.bias", "fc1.weight", "fc1.bias")   # descriptor order = state-dict order

    def __init__(self, **kwargs):
        super().__init__(self.__class__.__name__.lower())
        param_list = ["tot_entity", "tot_relation", "ent_hidden_size", "rel_hidden_size", "input_dropout", "hidden_dropout",
                      "feature_map_dropout"]
        self.__dict__.update(self.load_params(param_list, kwargs))
        self._device = kwargs.get("device")   # the reference requires the kwarg; here it defaults to where the weights live
        self.filt_h, self.filt_w, self.in_channels, self.out_channels = 1, 9, 1, 32
        D, Dr = int(self.ent_hidden_size), int(self.rel_hidden_size)
        # (the reference replaces the three rates by nn.Dropout modules inp_drop / feature_map_drop / hidden_drop; here they stay numbers)
        self.dropouts = (float(self.input_dropout), float(self.feature_map_dropout), float(self.hidden_dropout))
        self.ent_embeddings = NamedEmbedding("ent_embeddings", self.tot_entity, D, padding_idx=0)
        self.rel_embeddings = NamedEmbedding("rel_embeddings", self.tot_relation, Dr, padding_idx=0)
        self.bn0 = torch.nn.BatchNorm2d(self.in_channels)
        self.bn1 = torch.nn.BatchNorm2d(self.out_channels)
        self.bn2 = torch.nn.BatchNorm1d(D)
        self.register_parameter("b", torch.nn.Parameter(torch.zeros(self.tot_entity)))
        # (max(..., 1): a geometry the library refuses must still construct, so that the refusal is the library's sentence)
        self.fc = torch.nn.Linear(max((D - self.filt_w + 1) * self.out_channels, 1), D)
        self.fc1 = torch.nn.Linear(Dr, self.in_channels * self.out_channels * self.filt_h * self.filt_w)
        torch.nn.init.xavier_uniform_(self.ent_embeddings.weight.data)   # (overwrites the zero row of padding_idx, as the reference does)
        torch.nn.init.xavier_uniform_(self.rel_embeddings.weight.data)
        self.parameter_list = [self.ent_embeddings, self.rel_embeddings]
        self.loss = Criterion.multi_class_bce
        self.dropout_seed = int(kwargs.get("seed", 0) or 0)
        self.dropout_offset = 0

    @property
    def device(self):
        return self._device if self._device is not None else self.ent_embeddings.weight.device

    def trainable_tensors(self):
        return [self.b, self.ent_embeddings.weight, self.rel_embeddings.weight, self.bn0.weight, self.bn0.bias, self.bn1.weight,
                self.bn1.bias, self.bn2.weight, self.bn2.bias, self.fc.weight, self.fc.bias, self.fc1.weight, self.fc1.bias]

    def _geometry(self):
        return dict(ent_hidden_size=int(self.ent_hidden_size), rel_hidden_size=int(self.rel_hidden_size))

    def _head_bias(self):
        return self.b


class InteractE(Conv1NModel):
    """projection.py:347-505.  forward(e, r, direction) = sigmoid(x @ ent.T + bias) with x = relu(bn2(hdrop(fc(flatten(fdrop(relu(bn1(
    conv(idrop(bn0(img)))))))))), img the feature_permutation chequer permutations of [ent[e] | rel[r]] viewed [2 reshape_width,
    reshape_height], and conv the depthwise convolution with circular padding whose num_filters filters are shared by the
    permutations.  There is one relation table: `direction` selects no relation row, only the mask rows.  The torch layers (bn0, bn1,
    bn2, fc) hold parameters and buffers only, so state_dict() has the reference's keys, order and shapes (the bare parameters bias and
    conv_filt first) and loads a reference checkpoint; the arithmetic is csrc/kge_interacte.hip.  chequer_perm is a plain attribute
    (not in state_dict(), as in the reference) drawn by _get_chequer_perm with the reference's np.random calls in the reference's
    order; `m.chequer_perm = tensor` loads another model's.  Its int32 device copy and inverse are cached and rebuilt when the
    attribute is reassigned, changed in place or the weights move; a row that is no permutation of [0, 2 hidden_size) is refused
    there.  Under train() a forward normalises with the statistics of its own rows, updates the six running buffers and the three
    num_batches_tracked counters as torch does, and draws the Philox masks of (dropout_seed, dropout_offset), the mask rows of the
    "head" direction following those of the "tail" direction; with any rate > 0 it then advances dropout_offset by one.  Under
    eval() all three batch norms use the running buffers, nothing is drawn and nothing is written."""
    kernel_name = "interacte"
    TENSORS = ("bias", "conv_filt", "ent_embeddings.weight", "rel_embeddings.weight", "bn0.weight", "bn0.bias", "bn1.weight", "bn1.bias",
               "bn2.weight", "bn2.bias", "fc.weight", "fc.bias")   # descriptor order = state-dict order

    def __init__(self, **kwargs):
        super().__init__(self.__class__.__name__.lower())
        param_list = ["tot_entity", "tot_relation", "hidden_size", "input_dropout", "hidden_dropout", "feature_map_dropout",
                      "feature_permutation", "num_filters", "kernel_size", "reshape_height", "reshape_width"]
        self.__dict__.update(self.load_params(param_list, kwargs))
        self.hidden_size = self.reshape_width * self.reshape_height
        self._device = kwargs.get("device")   # the reference requires the kwarg; here it defaults to where the weights live
        k, P, NF, ks = int(self.hidden_size), int(self.feature_permutation), int(self.num_filters), int(self.kernel_size)
        # (the reference replaces the three rates by nn.Dropout modules inp_drop / feature_map_drop / hidden_drop; here they stay numbers)
        self.dropouts = (float(self.input_dropout), float(self.feature_map_dropout), float(self.hidden_dropout))
        self.ent_embeddings = NamedEmbedding("ent_embeddings", self.tot_entity, k, padding_idx=None)
        self.rel_embeddings = NamedEmbedding("rel_embeddings", self.tot_relation, k, padding_idx=None)
        self.bn0 = torch.nn.BatchNorm2d(P)
        self.padding = 0
        self.bn1 = torch.nn.BatchNorm2d(NF * P)
        self.flat_sz = self.reshape_height * 2 * self.reshape_width * NF * P
        self.bn2 = torch.nn.BatchNorm1d(k)
        self.fc = torch.nn.Linear(self.flat_sz, k)
        self._perm_cache = None
        self.chequer_perm = self._get_chequer_perm()
        self.register_parameter("bias", torch.nn.Parameter(torch.zeros(self.tot_entity)))
        self.register_parameter("conv_filt", torch.nn.Parameter(torch.zeros(NF, 1, ks, ks)))
        torch.nn.init.xavier_uniform_(self.ent_embeddings.weight)
        torch.nn.init.xavier_uniform_(self.rel_embeddings.weight)
        torch.nn.init.xavier_uniform_(self.conv_filt)
        self.parameter_list = [self.ent_embeddings, self.rel_embeddings]
        self.loss = Criterion.multi_class_bce
        self.dropout_seed = int(kwargs.get("seed", 0) or 0)
        self.dropout_offset = 0

    @property
    def device(self):
        return self._device if self._device is not None else self.ent_embeddings.weight.device

    def _get_chequer_perm(self):
        """The reference's draw (projection.py:468-505): all entity permutations first, then all relation ones, from np.random."""
        import numpy as np
        k, P = int(self.hidden_size), int(self.feature_permutation)
        ent_perm = np.int32([np.random.permutation(k) for _ in range(P)])
        rel_perm = np.int32([np.random.permutation(k) for _ in range(P)])
        comb_idx = []
        for p in range(P):
            temp, idx = [], 0
            for i in range(int(self.reshape_height)):
                for _ in range(int(self.reshape_width)):
                    pair = [ent_perm[p, idx], rel_perm[p, idx] + k]
                    temp += pair if (p + i) % 2 == 0 else pair[::-1]   # the chequer: the entity value leads where p + i is even
                    idx += 1
            comb_idx.append(temp)
        return torch.LongTensor(np.int32(comb_idx).reshape(P, 2 * k))

    def _perms(self):
        """The cached (perm, inv_perm) int32 device pair of chequer_perm (K.interacte_perm checks the permutation rows)."""
        cp, dev = self.chequer_perm, self.ent_embeddings.weight.device
        key = (id(cp), getattr(cp, "_version", None), getattr(cp, "device", None), dev)
        if self._perm_cache is None or self._perm_cache[0] != key:
            # (the cache holds cp itself, so that its id cannot be reused by another tensor while the entry lives)
            self._perm_cache = (key, cp, K.interacte_perm(cp, int(self.feature_permutation), int(self.hidden_size), dev))
        return self._perm_cache[2]

    def trainable_tensors(self):
        return [self.bias, self.conv_filt, self.ent_embeddings.weight, self.rel_embeddings.weight, self.bn0.weight, self.bn0.bias,
                self.bn1.weight, self.bn1.bias, self.bn2.weight, self.bn2.bias, self.fc.weight, self.fc.bias]

    def _geometry(self):
        return dict(reshape_height=int(self.reshape_height), reshape_width=int(self.reshape_width),
                    feature_permutation=int(self.feature_permutation), num_filters=int(self.num_filters),
                    kernel_size=int(self.kernel_size), perms=self._perms())

    def _head_bias(self):
        return self.bias


class AcrE(Conv1NModel):
    """projection.py:621-746.  forward(e, r, direction) = sigmoid(x @ ent.T + bias) with x = relu(bn2(hdrop(fc(flatten(fdrop(relu(bn1(
    c))))))), y0 = idrop(bn0(img)), img the [10, 20] view of ent[e] stacked on that of rel[r] (hidden_size is 200 by construction), and
    c = conv3(conv2(conv1(y0))) + y0 in the "serial" way: three 3 x 3 convolutions with dilations first / second / third_atrous and as
    much zero padding, 1 -> in_channels -> in_channels -> in_channels, with no nonlinearity between them.  The "parallel" way (three
    1 -> in_channels convolutions of y0 and a shared 1600 -> 400 gate, c[ch] = [y0 | z1[ch] | z2[ch] | z3[ch]] W_gate_e^T + b, in
    place of the chain and the residual) runs on the same kernels before z1 and after c.  There is one relation table of
    2 tot_relation rows: `direction` selects no relation row, only the mask rows.  The torch layers (bn0, bn1, bn2, fc, conv1, conv2,
    conv3, W_gate_e) hold parameters and buffers only, so state_dict() has the reference's keys, order and shapes (the bare parameter
    bias first) and loads a reference checkpoint; the arithmetic is csrc/kge_acre.hip.  Under train() a forward normalises with the
    statistics of its own rows, updates the six running buffers and the three num_batches_tracked counters as torch does, and draws
    the Philox masks of (dropout_seed, dropout_offset), the mask rows of the "head" direction following those of the "tail"
    direction; with any rate > 0 it then advances dropout_offset by one.  Under eval() all three batch norms use the running buffers,
    nothing is drawn and nothing is written."""
    kernel_name = "acre"

    def __init__(self, **kwargs):
        super().__init__(self.__class__.__name__.lower())
        param_list = ["tot_entity", "tot_relation", "hidden_size", "input_dropout", "hidden_dropout", "feature_map_dropout",
                      "in_channels", "way", "first_atrous", "second_atrous", "third_atrous", "acre_bias"]
        self.__dict__.update(self.load_params(param_list, kwargs))
        k, C = int(self.hidden_size), int(self.in_channels)
        # (the reference replaces the three rates by nn.Dropout modules inp_drop / feature_map_drop / hidden_drop; here they stay numbers)
        self.dropouts = (float(self.input_dropout), float(self.feature_map_dropout), float(self.hidden_dropout))
        self.ent_embeddings = NamedEmbedding("ent_embedding", self.tot_entity, k, padding_idx=None)
        self.rel_embeddings = NamedEmbedding("rel_embedding", self.tot_relation * 2, k, padding_idx=None)
        self.bn0 = torch.nn.BatchNorm2d(1)
        self.bn1 = torch.nn.BatchNorm2d(C)
        self.bn2 = torch.nn.BatchNorm1d(k)
        self.fc = torch.nn.Linear(C * 400, k)
        self.padding = 0
        a1, a2, a3, cb = int(self.first_atrous), int(self.second_atrous), int(self.third_atrous), bool(self.acre_bias)
        Cin = C if self.way == "serial" else 1   # (as the reference: every way but "serial" is the parallel one)
        self.conv1 = torch.nn.Conv2d(1, C, (3, 3), 1, a1, bias=cb, dilation=a1)
        self.conv2 = torch.nn.Conv2d(Cin, C, (3, 3), 1, a2, bias=cb, dilation=a2)
        self.conv3 = torch.nn.Conv2d(Cin, C, (3, 3), 1, a3, bias=cb, dilation=a3)
        if self.way != "serial":
            self.W_gate_e = torch.nn.Linear(1600, 400)
        self.register_parameter("bias", torch.nn.Parameter(torch.zeros(self.tot_entity)))
        torch.nn.init.xavier_uniform_(self.ent_embeddings.weight.data)
        torch.nn.init.xavier_uniform_(self.rel_embeddings.weight.data)
        self.parameter_list = [self.ent_embeddings, self.rel_embeddings]
        self.loss = Criterion.multi_class_bce
        self.dropout_seed = int(kwargs.get("seed", 0) or 0)
        self.dropout_offset = 0

    def trainable_tensors(self):
        """The parameters in state-dict order: the conv biases only with acre_bias, the gate only in the parallel way."""
        t = [self.bias, self.ent_embeddings.weight, self.rel_embeddings.weight, self.bn0.weight, self.bn0.bias, self.bn1.weight,
             self.bn1.bias, self.bn2.weight, self.bn2.bias, self.fc.weight, self.fc.bias]
        for conv in (self.conv1, self.conv2, self.conv3):
            t.append(conv.weight)
            if conv.bias is not None:
                t.append(conv.bias)
        if self.way != "serial":
            t += [self.W_gate_e.weight, self.W_gate_e.bias]
        return t

    def _geometry(self):
        return dict(hidden_size=int(self.hidden_size), in_channels=int(self.in_channels), way=0 if self.way == "serial" else 1,
                    first_atrous=int(self.first_atrous), second_atrous=int(self.second_atrous), third_atrous=int(self.third_atrous),
                    acre_bias=bool(self.acre_bias))

    def _head_bias(self):
        return self.bias


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

    def _eval_body(self, e, r, side):
        return self._body(e, r, side, -1)

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
