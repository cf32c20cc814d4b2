"""Dispatcher-registered custom ops over the C ABI (BASELINE.json north_star: "exposed to the existing Trainer/Evaluator via a
PyTorch-ROCm custom op that keeps each model's forward()/embed() signature").

  torch.ops.kge.score(key, h, r, t, weights) -> float32 [N]        Model.forward of models/pairwise.py / pointwise.py
  torch.ops.kge.score_backward(key, h, r, t, dscore, weights) -> dense gradients of `weights` (nn.Embedding(sparse=False) semantics)
  torch.ops.kge.convkb_score(key, h, r, t, weights) -> float32 [N]   ConvKB.forward (models/pointwise.py:302-318); weights = ent, rel, fc1.weight, fc1.bias
  torch.ops.kge.convkb_score_backward(key, h, r, t, dscore, weights) -> their dense gradients (the filters are fixed inputs)
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


# ConvE's body (include/kge_hip.h: kge_conve_body_*).  side 0 = the tail direction, 1 = the head direction; offset < 0 = the eval form
# (running statistics, no bn2, no draws).  The mask rows of a call start at side * n: the head direction's rows follow the tail
# direction's, as in the fused step, so that the two forward calls of a training step under one (seed, offset) draw the step's masks.
# The training form updates the model's running buffers (found through the model handle, not passed as tensors).  That write is not
# in the op's schema (mutates_args is empty), so the op is for eager execution only: under torch.compile or functionalisation the
# update is invisible, and a training-form call whose outputs are unused could be dropped together with it.
@torch.library.custom_op("kge::conve_body", mutates_args=(), device_types="cuda")
def conve_body(key: int, e: Tensor, r: Tensor, side: int, seed: int, offset: int, weights: List[Tensor]) -> Tuple[Tensor, Tensor]:
    m = _model(key)
    return K.conve_body_forward(m.make_desc(list(weights), train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                                r.contiguous(), side, row0=side * e.numel())


@conve_body.register_fake
def _(key, e, r, side, seed, offset, weights):
    n, k = e.numel(), weights[0].shape[1]
    return weights[0].new_empty((n, k)), weights[0].new_empty((n * (weights[9].shape[1] + k) + 66 + 2 * k,))


@conve_body.register_kernel("cpu")
def _(key, e, r, side, seed, offset, weights):
    raise L.KgeHipError("kge::conve_body: ids and tables must live on the HIP device (got %s); the HIP path has no CPU fallback" % e.device)


@torch.library.custom_op("kge::conve_body_backward", mutates_args=(), device_types="cuda")
def conve_body_backward(key: int, e: Tensor, r: Tensor, side: int, seed: int, offset: int, dx: Tensor, saved: Tensor,
                        weights: List[Tensor]) -> List[Tensor]:
    m = _model(key)
    grads = [torch.zeros_like(w) for w in weights]
    K.conve_body_backward(m.make_desc(list(weights), grads, train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                          r.contiguous(), side, dx.contiguous(), saved, row0=side * e.numel())
    return grads


@conve_body_backward.register_fake
def _(key, e, r, side, seed, offset, dx, saved, weights):
    return [torch.empty_like(w) for w in weights]


def _conve_setup(ctx, inputs, output):
    key, e, r, side, seed, offset, weights = inputs
    ctx.key, ctx.side, ctx.seed, ctx.offset = key, side, seed, offset
    ctx.save_for_backward(e, r, output[1], *weights)
    ctx.mark_non_differentiable(output[1])


def _conve_backward(ctx, dx, _dsaved):
    e, r, saved, *weights = ctx.saved_tensors
    return None, None, None, None, None, None, conve_body_backward(ctx.key, e, r, ctx.side, ctx.seed, ctx.offset, dx, saved, weights)


conve_body.register_autograd(_conve_backward, setup_context=_conve_setup)


# HypER's body (include/kge_hip.h: kge_hyper_body_*).  There is one relation table, so a direction selects nothing but the mask rows:
# row0 = 0 for the tail direction and n for the head direction, so that the two forward calls of a training step under one (seed,
# offset) draw the fused step's masks.  offset < 0 = the eval form (running statistics in all three batch norms, no draws).  Like
# kge::conve_body, the training form updates the model's running buffers, a write outside the op's schema (mutates_args is empty):
# eager execution only.
@torch.library.custom_op("kge::hyper_body", mutates_args=(), device_types="cuda")
def hyper_body(key: int, e: Tensor, r: Tensor, row0: int, seed: int, offset: int, weights: List[Tensor]) -> Tuple[Tensor, Tensor]:
    m = _model(key)
    return K.hyper_body_forward(m.make_desc(list(weights), train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                                r.contiguous(), row0=row0)


@hyper_body.register_fake
def _(key, e, r, row0, seed, offset, weights):
    n, D = e.numel(), weights[1].shape[1]
    return weights[1].new_empty((n, D)), weights[1].new_empty((n * (weights[9].shape[1] + D + 288) + 66 + 2 * D,))


@hyper_body.register_kernel("cpu")
def _(key, e, r, row0, seed, offset, weights):
    raise L.KgeHipError("kge::hyper_body: ids and tables must live on the HIP device (got %s); the HIP path has no CPU fallback" % e.device)


@torch.library.custom_op("kge::hyper_body_backward", mutates_args=(), device_types="cuda")
def hyper_body_backward(key: int, e: Tensor, r: Tensor, row0: int, seed: int, offset: int, dx: Tensor, saved: Tensor,
                        weights: List[Tensor]) -> List[Tensor]:
    m = _model(key)
    grads = [torch.zeros_like(w) for w in weights]
    K.hyper_body_backward(m.make_desc(list(weights), grads, train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                          r.contiguous(), dx.contiguous(), saved, row0=row0)
    return grads


@hyper_body_backward.register_fake
def _(key, e, r, row0, seed, offset, dx, saved, weights):
    return [torch.empty_like(w) for w in weights]


def _hyper_setup(ctx, inputs, output):
    key, e, r, row0, seed, offset, weights = inputs
    ctx.key, ctx.row0, ctx.seed, ctx.offset = key, row0, seed, offset
    ctx.save_for_backward(e, r, output[1], *weights)
    ctx.mark_non_differentiable(output[1])


def _hyper_backward(ctx, dx, _dsaved):
    e, r, saved, *weights = ctx.saved_tensors
    return None, None, None, None, None, None, hyper_body_backward(ctx.key, e, r, ctx.row0, ctx.seed, ctx.offset, dx, saved, weights)


hyper_body.register_autograd(_hyper_backward, setup_context=_hyper_setup)


# InteractE's body (include/kge_hip.h: kge_interacte_body_*).  As in kge::hyper_body there is one relation table, row0 = 0 for the tail
# direction and n for the head direction, offset < 0 = the eval form, and the training form updates the model's running buffers, a
# write outside the op's schema: eager execution only.  The chequer permutations are the model's (found through `key`), not an operand.
@torch.library.custom_op("kge::interacte_body", mutates_args=(), device_types="cuda")
def interacte_body(key: int, e: Tensor, r: Tensor, row0: int, seed: int, offset: int, weights: List[Tensor]) -> Tuple[Tensor, Tensor]:
    m = _model(key)
    return K.interacte_body_forward(m.make_desc(list(weights), train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                                    r.contiguous(), row0=row0)


@interacte_body.register_fake
def _(key, e, r, row0, seed, offset, weights):
    n, k, P, C = e.numel(), weights[2].shape[1], weights[4].shape[0], weights[6].shape[0]
    return weights[2].new_empty((n, k)), weights[2].new_empty((n * (weights[10].shape[1] + k + C) + 2 * P + 2 * C + 2 * k,))


@interacte_body.register_kernel("cpu")
def _(key, e, r, row0, seed, offset, weights):
    raise L.KgeHipError("kge::interacte_body: ids and tables must live on the HIP device (got %s); the HIP path has no CPU fallback" % e.device)


@torch.library.custom_op("kge::interacte_body_backward", mutates_args=(), device_types="cuda")
def interacte_body_backward(key: int, e: Tensor, r: Tensor, row0: int, seed: int, offset: int, dx: Tensor, saved: Tensor,
                            weights: List[Tensor]) -> List[Tensor]:
    m = _model(key)
    grads = [torch.zeros_like(w) for w in weights]
    K.interacte_body_backward(m.make_desc(list(weights), grads, train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                              r.contiguous(), dx.contiguous(), saved, row0=row0)
    return grads


@interacte_body_backward.register_fake
def _(key, e, r, row0, seed, offset, dx, saved, weights):
    return [torch.empty_like(w) for w in weights]


def _interacte_setup(ctx, inputs, output):
    key, e, r, row0, seed, offset, weights = inputs
    ctx.key, ctx.row0, ctx.seed, ctx.offset = key, row0, seed, offset
    ctx.save_for_backward(e, r, output[1], *weights)
    ctx.mark_non_differentiable(output[1])


def _interacte_backward(ctx, dx, _dsaved):
    e, r, saved, *weights = ctx.saved_tensors
    return None, None, None, None, None, None, interacte_body_backward(ctx.key, e, r, ctx.row0, ctx.seed, ctx.offset, dx, saved, weights)


interacte_body.register_autograd(_interacte_backward, setup_context=_interacte_setup)


# AcrE's body (include/kge_hip.h: kge_acre_body_*).  As in kge::interacte_body there is one relation table, row0 = 0 for the tail
# direction and n for the head direction, offset < 0 = the eval form, and the training form updates the model's running buffers, a
# write outside the op's schema: eager execution only.  weights: the model's parameters in state-dict order (bias first; the conv
# biases only with acre_bias, the gate only in the parallel way); the way and the dilations are the model's (found through `key`).
@torch.library.custom_op("kge::acre_body", mutates_args=(), device_types="cuda")
def acre_body(key: int, e: Tensor, r: Tensor, row0: int, seed: int, offset: int, weights: List[Tensor]) -> Tuple[Tensor, Tensor]:
    m = _model(key)
    return K.acre_body_forward(m.make_desc(list(weights), train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                               r.contiguous(), row0=row0)


@acre_body.register_fake
def _(key, e, r, row0, seed, offset, weights):
    n, k, C = e.numel(), weights[1].shape[1], weights[5].shape[0]
    layers = 4 if tuple(weights[-1].shape) == (400,) and weights[-2].dim() == 2 else 3   # the parallel way (the gate comes last) saves z_3 too
    return weights[1].new_empty((n, k)), weights[1].new_empty((n * (layers * weights[9].shape[1] + k + C) + 2 + 2 * C + 2 * k,))


@acre_body.register_kernel("cpu")
def _(key, e, r, row0, seed, offset, weights):
    raise L.KgeHipError("kge::acre_body: ids and tables must live on the HIP device (got %s); the HIP path has no CPU fallback" % e.device)


@torch.library.custom_op("kge::acre_body_backward", mutates_args=(), device_types="cuda")
def acre_body_backward(key: int, e: Tensor, r: Tensor, row0: int, seed: int, offset: int, dx: Tensor, saved: Tensor,
                       weights: List[Tensor]) -> List[Tensor]:
    m = _model(key)
    grads = [torch.zeros_like(w) for w in weights]
    K.acre_body_backward(m.make_desc(list(weights), grads, train=offset >= 0, seed=seed, offset=max(offset, 0)), e.contiguous(),
                         r.contiguous(), dx.contiguous(), saved, row0=row0)
    return grads


@acre_body_backward.register_fake
def _(key, e, r, row0, seed, offset, dx, saved, weights):
    return [torch.empty_like(w) for w in weights]


def _acre_setup(ctx, inputs, output):
    key, e, r, row0, seed, offset, weights = inputs
    ctx.key, ctx.row0, ctx.seed, ctx.offset = key, row0, seed, offset
    ctx.save_for_backward(e, r, output[1], *weights)
    ctx.mark_non_differentiable(output[1])


def _acre_backward(ctx, dx, _dsaved):
    e, r, saved, *weights = ctx.saved_tensors
    return None, None, None, None, None, None, acre_body_backward(ctx.key, e, r, ctx.row0, ctx.seed, ctx.offset, dx, saved, weights)


acre_body.register_autograd(_acre_backward, setup_context=_acre_setup)


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
