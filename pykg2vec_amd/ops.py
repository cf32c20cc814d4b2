"""Dispatcher-registered custom ops over the C ABI (BASELINE.json north_star: "exposed to the existing Trainer/Evaluator via a
PyTorch-ROCm custom op that keeps each model's forward()/embed() signature").

  torch.ops.kge.score(key, h, r, t, weights) -> float32 [N]        Model.forward of models/pairwise.py / pointwise.py
  torch.ops.kge.score_backward(key, h, r, t, dscore, weights) -> dense gradients of `weights` (nn.Embedding(sparse=False) semantics)
  torch.ops.kge.convkb_score(key, h, r, t, weights) -> float32 [N]   ConvKB.forward (models/pointwise.py:302-318); weights = ent, rel, fc1.weight, fc1.bias
  torch.ops.kge.convkb_score_backward(key, h, r, t, dscore, weights) -> their dense gradients (the filters are fixed inputs)
  torch.ops.kge.murp_score(key, h, r, t, weights) -> float64 [N]     MuRP.forward (models/pointwise.py:1081-1102); weights = wu, bs, bo, ent, rel (float64)
  torch.ops.kge.murp_score_backward(key, h, r, t, dscore, weights) -> their dense gradients (rows 0 of ent and rel get none: padding_idx = 0)
  torch.ops.kge.tucker_body(key, e, r, seed, offset, weights) -> (x float32 [N, d1], saved)   the body of TuckER.forward (models/projection.py:321-334); weights = ent, rel, W
  torch.ops.kge.tucker_body_backward(key, e, r, seed, offset, dx, saved, weights) -> their dense gradients
  torch.ops.kge.proje_body(key, e, r, side, seed, offset, weights) -> x float32 [N, k]   tanh(ent[e] o De_s + rel[r] o Dr_s + bc_s) with dropout: f1 / f2 of ProjE_pointwise (models/projection.py:212-228); weights = its parameter_list
  torch.ops.kge.proje_body_backward(key, e, r, side, seed, offset, dx, weights) -> their dense gradients
  torch.ops.kge.conve_body(key, e, r, side, seed, offset, weights) -> (x float32 [N, k], saved)   the body of ConvE.forward (models/projection.py:86-99, 104-113) up to the head; weights = its 13 tensors in state-dict order; the training form updates the model's running buffers, a write outside the op's schema: eager execution only
  torch.ops.kge.conve_body_backward(key, e, r, side, seed, offset, dx, saved, weights) -> their dense gradients (b's is the head's: zero here)
  torch.ops.kge.hyper_body(key, e, r, row0, seed, offset, weights) -> (x float32 [N, D], saved)   the body of HypER.forward (models/projection.py:583-606) up to the head; weights = its 13 tensors in state-dict order (b first); row0 = the mask row of the call's first row; the training form updates the model's running buffers, a write outside the op's schema: eager execution only
  torch.ops.kge.hyper_body_backward(key, e, r, row0, seed, offset, dx, saved, weights) -> their dense gradients (b's is the head's: zero here; the lookup gradients of id 0 are dropped, padding_idx = 0)
  torch.ops.kge.interacte_body(key, e, r, row0, seed, offset, weights) -> (x float32 [N, k], saved)   the body of InteractE.forward (models/projection.py:425-442) up to the head; weights = its 12 tensors in state-dict order (bias and conv_filt first); the chequer permutations are the model's; row0 and the running-buffer write as in hyper_body: eager execution only
  torch.ops.kge.interacte_body_backward(key, e, r, row0, seed, offset, dx, saved, weights) -> their dense gradients (bias's is the head's: zero here)
  torch.ops.kge.acre_body(key, e, r, row0, seed, offset, weights) -> (x float32 [N, 200], saved)   the body of AcrE.forward (models/projection.py:706-734) up to the head; weights = its parameters in state-dict order (bias first); the way and the dilations are the model's; row0 and the running-buffer write as in hyper_body: eager execution only
  torch.ops.kge.acre_body_backward(key, e, r, row0, seed, offset, dx, saved, weights) -> their dense gradients (bias's is the head's: zero here)
  torch.ops.kge.one_to_n_scores(x, ent, bias, bf16) -> float32 [B, E]  the projection models' 1-N head (models/projection.py:100-102)
  torch.ops.kge.one_to_n_scores_backward(x, ent, preds, dpreds, need_bias) -> (dx, g_ent, g_bias)

Registered with torch.library.custom_op (schema, fake-tensor kernels, autograd formulas), so the scorer is visible to torch.ops,
torch.library.opcheck and torch.compile (no graph break at `model(h, r, t)`).  The CUDA-key implementations call libkge_hip.so through
pykg2vec_amd.kernels; there is no CPU implementation (a CPU tensor raises, as everywhere in this package).

`key` names the model a call scores with: an integer handle into a weak registry of live model objects (a custom-op argument can only
be a tensor, a number, a string or lists of those; the descriptor needs the model's kernel id, entity / relation counts and
hyper-parameters, which are fixed per model object and therefore trace as a constant)."""
import itertools
import weakref
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from . import kernels as K

_models = weakref.WeakValueDictionary()
_next_key = itertools.count(1)


def register_model(model):
    """Handle of `model` for torch.ops.kge.score (idempotent; the registry holds the model weakly)."""
    key = getattr(model, "_kge_op_key", None)
    if key is None or _models.get(key) is not model:
        key = next(_next_key)
        _models[key] = model
        model._kge_op_key = key
    return key


def _model(key):
    m = _models.get(int(key))
    if m is None:
        raise RuntimeError("kge::score: model handle %d is not (or no longer) registered" % int(key))
    return m


@torch.library.custom_op("kge::score", mutates_args=(), device_types="cuda")
def score(key: int, h: Tensor, r: Tensor, t: Tensor, weights: List[Tensor]) -> Tensor:
    m = _model(key)
    return K.score_forward(m.make_desc(list(weights)), h.contiguous(), r.contiguous(), t.contiguous())


@score.register_fake
def _(key, h, r, t, weights):
    return h.new_empty((h.numel(),), dtype=torch.float32)


@score.register_kernel("cpu")
def _(key, h, r, t, weights):     # loud, like every other entry of the package: there is no CPU scorer
    raise L.KgeHipError("kge::score: ids and tables must live on the HIP device (got %s); the HIP path has no CPU fallback" % h.device)


@torch.library.custom_op("kge::score_backward", mutates_args=(), device_types="cuda")
def score_backward(key: int, h: Tensor, r: Tensor, t: Tensor, dscore: Tensor, weights: List[Tensor]) -> List[Tensor]:
    m = _model(key)
    grads = [torch.zeros_like(w) for w in weights]
    K.score_backward(m.make_desc(list(weights), grads), h.contiguous(), r.contiguous(), t.contiguous(), dscore.contiguous())
    return grads


@score_backward.register_fake
def _(key, h, r, t, dscore, weights):
    return [torch.empty_like(w) for w in weights]


def _score_setup(ctx, inputs, output):
    key, h, r, t, weights = inputs
    ctx.key = key
    ctx.n_weights = len(weights)
    ctx.save_for_backward(h, r, t, *weights)


def _score_backward(ctx, dscore):
    h, r, t, *weights = ctx.saved_tensors
    return None, None, None, None, score_backward(ctx.key, h, r, t, dscore, weights)


score.register_autograd(_score_backward, setup_context=_score_setup)


# ConvKB has its own descriptor and entry points (include/kge_hip.h: kge_convkb_*): the same op pair under its own names
@torch.library.custom_op("kge::convkb_score", mutates_args=(), device_types="cuda")
def convkb_score(key: int, h: Tensor, r: Tensor, t: Tensor, weights: List[Tensor]) -> Tensor:
    m = _model(key)
    return K.convkb_score_forward(m.make_desc(list(weights)), h.contiguous(), r.contiguous(), t.contiguous())


@convkb_score.register_fake
def _(key, h, r, t, weights):
    return h.new_empty((h.numel(),), dtype=torch.float32)


@convkb_score.register_kernel("cpu")
def _(key, h, r, t, weights):
    raise L.KgeHipError("kge::convkb_score: ids and tables must live on the HIP device (got %s); the HIP path has no CPU fallback" % h.device)


@torch.library.custom_op("kge::convkb_score_backward", mutates_args=(), device_types="cuda")
def convkb_score_backward(key: int, h: Tensor, r: Tensor, t: Tensor, dscore: Tensor, weights: List[Tensor]) -> List[Tensor]:
    m = _model(key)
    grads = [torch.zeros_like(w) for w in weights]
    K.convkb_score_backward(m.make_desc(list(weights), grads), h.contiguous(), r.contiguous(), t.contiguous(), dscore.contiguous())
    return grads


@convkb_score_backward.register_fake
def _(key, h, r, t, dscore, weights):
    return [torch.empty_like(w) for w in weights]


def _convkb_backward(ctx, dscore):
    h, r, t, *weights = ctx.saved_tensors
    return None, None, None, None, convkb_score_backward(ctx.key, h, r, t, dscore, weights)


convkb_score.register_autograd(_convkb_backward, setup_context=_score_setup)


# MuRP has its own descriptor and entry points too (include/kge_hip.h: kge_murp_*), in float64
@torch.library.custom_op("kge::murp_score", mutates_args=(), device_types="cuda")
def murp_score(key: int, h: Tensor, r: Tensor, t: Tensor, weights: List[Tensor]) -> Tensor:
    m = _model(key)
    return K.murp_score_forward(m.make_desc(list(weights)), h.contiguous(), r.contiguous(), t.contiguous())


@murp_score.register_fake
def _(key, h, r, t, weights):
    return h.new_empty((h.numel(),), dtype=torch.float64)


@murp_score.register_kernel("cpu")
def _(key, h, r, t, weights):
    raise L.KgeHipError("kge::murp_score: ids and tables must live on the HIP device (got %s); the HIP path has no CPU fallback" % h.device)


@torch.library.custom_op("kge::murp_score_backward", mutates_args=(), device_types="cuda")
def murp_score_backward(key: int, h: Tensor, r: Tensor, t: Tensor, dscore: Tensor, weights: List[Tensor]) -> List[Tensor]:
    m = _model(key)
    grads = [torch.zeros_like(w) for w in weights]
    K.murp_score_backward(m.make_desc(list(weights), grads), h.contiguous(), r.contiguous(), t.contiguous(), dscore.contiguous())
    return grads


@murp_score_backward.register_fake
def _(key, h, r, t, dscore, weights):
    return [torch.empty_like(w) for w in weights]


def _murp_backward(ctx, dscore):
    h, r, t, *weights = ctx.saved_tensors
    return None, None, None, None, murp_score_backward(ctx.key, h, r, t, dscore, weights)


murp_score.register_autograd(_murp_backward, setup_context=_score_setup)


# TuckER's body (include/kge_hip.h: kge_tucker_body_*).  seed / offset key the dropout masks the two ops recompute; the model's
# train / eval state is read from the model object when the forward runs and travels to the backward as offset < 0 = eval.
@torch.library.custom_op("kge::tucker_body", mutates_args=(), device_types="cuda")
def tucker_body(key: int, e: Tensor, r: Tensor, seed: int, offset: int, weights: List[Tensor]) -> Tuple[Tensor, Tensor]:
    m = _model(key)
    return K.tucker_body_forward(m.make_desc(list(weights), train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(), r.contiguous())


@tucker_body.register_fake
def _(key, e, r, seed, offset, weights):
    n, d1 = e.numel(), weights[0].shape[1]
    return weights[0].new_empty((n, d1)), weights[0].new_empty((max(1, n * (2 * d1 + 2)),))


@tucker_body.register_kernel("cpu")
def _(key, e, r, seed, offset, weights):
    raise L.KgeHipError("kge::tucker_body: ids and tables must live on the HIP device (got %s); the HIP path has no CPU fallback" % e.device)


@torch.library.custom_op("kge::tucker_body_backward", mutates_args=(), device_types="cuda")
def tucker_body_backward(key: int, e: Tensor, r: Tensor, seed: int, offset: int, dx: Tensor, saved: Tensor, weights: List[Tensor]) -> List[Tensor]:
    m = _model(key)
    grads = [torch.zeros_like(w) for w in weights]
    K.tucker_body_backward(m.make_desc(list(weights), grads, train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                           r.contiguous(), dx.contiguous(), saved)
    return grads


@tucker_body_backward.register_fake
def _(key, e, r, seed, offset, dx, saved, weights):
    return [torch.empty_like(w) for w in weights]


def _tucker_setup(ctx, inputs, output):
    key, e, r, seed, offset, weights = inputs
    ctx.key, ctx.seed, ctx.offset = key, seed, offset
    ctx.save_for_backward(e, r, output[1], *weights)
    ctx.mark_non_differentiable(output[1])


def _tucker_backward(ctx, dx, _dsaved):
    e, r, saved, *weights = ctx.saved_tensors
    return None, None, None, None, None, tucker_body_backward(ctx.key, e, r, ctx.seed, ctx.offset, dx, saved, weights)


tucker_body.register_autograd(_tucker_backward, setup_context=_tucker_setup)


# ProjE_pointwise's body (include/kge_hip.h: kge_proje_body_*).  side 0 = f1 (the tail direction), 1 = f2; offset < 0 = no dropout.  The
# backward recomputes the body from the tables: nothing but the ids is saved.
@torch.library.custom_op("kge::proje_body", mutates_args=(), device_types="cuda")
def proje_body(key: int, e: Tensor, r: Tensor, side: int, seed: int, offset: int, weights: List[Tensor]) -> Tensor:
    m = _model(key)
    return K.proje_body_forward(m.make_desc(list(weights), train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                                r.contiguous(), side)


@proje_body.register_fake
def _(key, e, r, side, seed, offset, weights):
    return weights[0].new_empty((e.numel(), weights[0].shape[1]))


@proje_body.register_kernel("cpu")
def _(key, e, r, side, seed, offset, weights):
    raise L.KgeHipError("kge::proje_body: ids and tables must live on the HIP device (got %s); the HIP path has no CPU fallback" % e.device)


@torch.library.custom_op("kge::proje_body_backward", mutates_args=(), device_types="cuda")
def proje_body_backward(key: int, e: Tensor, r: Tensor, side: int, seed: int, offset: int, dx: Tensor, weights: List[Tensor]) -> List[Tensor]:
    m = _model(key)
    grads = [torch.zeros_like(w) for w in weights]
    K.proje_body_backward(m.make_desc(list(weights), grads, train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                          r.contiguous(), side, dx.contiguous())
    return grads


@proje_body_backward.register_fake
def _(key, e, r, side, seed, offset, dx, weights):
    return [torch.empty_like(w) for w in weights]


def _proje_setup(ctx, inputs, output):
    key, e, r, side, seed, offset, weights = inputs
    ctx.key, ctx.side, ctx.seed, ctx.offset = key, side, seed, offset
    ctx.save_for_backward(e, r, *weights)


def _proje_backward(ctx, dx):
    e, r, *weights = ctx.saved_tensors
    return None, None, None, None, None, None, proje_body_backward(ctx.key, e, r, ctx.side, ctx.seed, ctx.offset, dx, weights)


proje_body.register_autograd(_proje_backward, setup_context=_proje_setup)


# The bodies of the conv 1-N models (include/kge_hip.h: kge_<stem>_body_* for conve, hyper, interacte, acre), one registration for all.
# offset < 0 = the eval form (running statistics, no draws).  The training form updates the model's running buffers (found through
# the model handle, not passed as tensors).  That write is not in the op's schema (mutates_args is empty), so the ops are for eager
# execution only: under torch.compile or functionalisation the update is invisible, and a training-form call whose outputs are
# unused could be dropped together with it.
def _register_conv_1n(stem, direction, ent_slot, saved_floats):
    """Defines kge::<stem>_body and kge::<stem>_body_backward with their fake kernels, CPU refusal and autograd formula, and returns
    the pair.  direction: the schema's name of the direction argument, "side" (ConvE: 0 / 1, which also picks the relation half; the
    mask rows start at side * n) or "row0" (the mask row of the call's first row); ent_slot: where the entity table stands in
    `weights`, its width is x's; saved_floats(n, weights): the size of `saved`, the library's kge_<stem>_saved_floats restated on
    shapes for the fake kernel (tests/test_conv_1n_host.py holds the two together)."""
    forward, backward = getattr(K, stem + "_body_forward"), getattr(K, stem + "_body_backward")

    def rows(e, d):     # the direction as K.<stem>_body_* take it: ConvE's side in front, row0 by keyword
        return ((d,), d * e.numel()) if direction == "side" else ((), d)

    def desc(key, weights, grads, seed, offset):
        return _model(key).make_desc(list(weights), grads, train=offset >= 0, seed=seed, offset=max(offset, 0))

    @torch.library.custom_op("kge::%s_body" % stem, mutates_args=(), device_types="cuda",
                             schema="(SymInt key, Tensor e, Tensor r, SymInt %s, SymInt seed, SymInt offset, Tensor[] weights) -> (Tensor, Tensor)"
                             % direction)
    def body(key: int, e: Tensor, r: Tensor, d: int, seed: int, offset: int, weights: List[Tensor]) -> Tuple[Tensor, Tensor]:
        lead, row0 = rows(e, d)
        return forward(desc(key, weights, None, seed, offset), e.contiguous(), r.contiguous(), *lead, row0=row0)

    @body.register_fake
    def _(key, e, r, d, seed, offset, weights):
        ent, n = weights[ent_slot], e.numel()
        return ent.new_empty((n, ent.shape[1])), ent.new_empty((saved_floats(n, weights),))

    @body.register_kernel("cpu")
    def _(key, e, r, d, seed, offset, weights):
        raise L.KgeHipError("kge::%s_body: ids and tables must live on the HIP device (got %s); the HIP path has no CPU fallback" % (stem, e.device))

    @torch.library.custom_op("kge::%s_body_backward" % stem, mutates_args=(), device_types="cuda",
                             schema="(SymInt key, Tensor e, Tensor r, SymInt %s, SymInt seed, SymInt offset, Tensor dx, Tensor saved, "
                                    "Tensor[] weights) -> Tensor[]" % direction)
    def body_backward(key: int, e: Tensor, r: Tensor, d: int, seed: int, offset: int, dx: Tensor, saved: Tensor,
                      weights: List[Tensor]) -> List[Tensor]:
        grads = [torch.zeros_like(w) for w in weights]
        lead, row0 = rows(e, d)
        backward(desc(key, weights, grads, seed, offset), e.contiguous(), r.contiguous(), *lead, dx.contiguous(), saved, row0=row0)
        return grads

    @body_backward.register_fake
    def _(key, e, r, d, seed, offset, dx, saved, weights):
        return [torch.empty_like(w) for w in weights]

    def setup(ctx, inputs, output):
        key, e, r, d, seed, offset, weights = inputs
        ctx.key, ctx.direction, ctx.seed, ctx.offset = key, d, seed, offset
        ctx.save_for_backward(e, r, output[1], *weights)
        ctx.mark_non_differentiable(output[1])

    def autograd(ctx, dx, _dsaved):
        e, r, saved, *weights = ctx.saved_tensors
        return None, None, None, None, None, None, body_backward(ctx.key, e, r, ctx.direction, ctx.seed, ctx.offset, dx, saved, weights)

    body.register_autograd(autograd, setup_context=setup)
    return body, body_backward


# ConvE: side 0 = the tail direction, 1 = the head direction (rel[r + tot_relation]), and eval skips bn2.  The mask rows of a call start
# at side * n: the head direction's rows follow the tail direction's, as in the fused step, so that the two forward calls of a training
# step under one (seed, offset) draw the step's masks.  saved: the fc input [n, F], u [n, k] and the statistics 66 + 2 k.
conve_body, conve_body_backward = _register_conv_1n(
    "conve", "side", 0, lambda n, w: n * (w[9].shape[1] + w[0].shape[1]) + 66 + 2 * w[0].shape[1])

# HypER: there is one relation table, so a direction selects nothing but the mask rows: row0 = 0 for the tail direction and n for the
# head direction, so that the two forward calls of a training step under one (seed, offset) draw the fused step's masks.  Eval uses
# the running statistics in all three batch norms.  saved: as ConvE's and the per-row filter [n, 288].
hyper_body, hyper_body_backward = _register_conv_1n(
    "hyper", "row0", 1, lambda n, w: n * (w[9].shape[1] + w[1].shape[1] + 288) + 66 + 2 * w[1].shape[1])

# InteractE: row0 as in kge::hyper_body.  The chequer permutations are the model's (found through `key`), not an operand.  saved: the
# fc input, u, the feature-map factors [n, C] and the statistics 2 P + 2 C + 2 k (P = bn0's width, C = bn1's).
interacte_body, interacte_body_backward = _register_conv_1n(
    "interacte", "row0", 2,
    lambda n, w: n * (w[10].shape[1] + w[2].shape[1] + w[6].shape[0]) + 2 * w[4].shape[0] + 2 * w[6].shape[0] + 2 * w[2].shape[1])

# AcrE: row0 as in kge::hyper_body.  weights: the model's parameters in state-dict order (bias first; the conv biases only with
# acre_bias, the gate only in the parallel way); the way and the dilations are the model's (found through `key`).  saved: c, z_1, z_2
# [n, 400 C] each, in the parallel way z_3 too, then u, the factors [n, C] and the statistics 2 + 2 C + 2 k.  The weight count tells
# the way: 11 + 3 or 11 + 6 tensors in the serial way, the gate's two more in the parallel way.
acre_body, acre_body_backward = _register_conv_1n(
    "acre", "row0", 1,
    lambda n, w: n * ((4 if len(w) in (16, 19) else 3) * w[9].shape[1] + w[1].shape[1] + w[5].shape[0]) + 2 + 2 * w[5].shape[0]
    + 2 * w[1].shape[1])


@torch.library.custom_op("kge::one_to_n_scores", mutates_args=(), device_types="cuda")
def one_to_n_scores(x: Tensor, ent: Tensor, bias: Optional[Tensor], bf16: bool) -> Tensor:
    b = None if bias is None else bias.contiguous().view(-1)
    return K.head_1n_forward(x.contiguous(), ent.contiguous(), b, precision="bf16" if bf16 else "f32")


@one_to_n_scores.register_fake
def _(x, ent, bias, bf16):
    return x.new_empty((x.shape[0], ent.shape[0]), dtype=torch.float32)


@torch.library.custom_op("kge::one_to_n_scores_backward", mutates_args=(), device_types="cuda")
def one_to_n_scores_backward(x: Tensor, ent: Tensor, preds: Tensor, dpreds: Tensor, need_bias: bool) -> Tuple[Tensor, Tensor, Tensor]:
    dx, g_ent, g_bias = K.head_1n_backward(x.contiguous(), ent.contiguous(), preds.contiguous(), dpreds.contiguous(), need_bias=need_bias)
    return dx, g_ent, (g_bias if need_bias else ent.new_zeros((ent.shape[0],)))


@one_to_n_scores_backward.register_fake
def _(x, ent, preds, dpreds, need_bias):
    return torch.empty_like(x), torch.empty_like(ent), ent.new_empty((ent.shape[0],))


def _head_setup(ctx, inputs, output):
    x, ent, bias, bf16 = inputs
    ctx.has_bias = bias is not None
    ctx.bias_shape = None if bias is None else bias.shape
    ctx.save_for_backward(x, ent, output)


def _head_backward(ctx, dpreds):
    x, ent, preds = ctx.saved_tensors
    dx, g_ent, g_bias = one_to_n_scores_backward(x, ent, preds, dpreds, ctx.has_bias)
    return dx, g_ent, (g_bias.view(ctx.bias_shape) if ctx.has_bias else None), None


one_to_n_scores.register_autograd(_head_backward, setup_context=_head_setup)
