"""Host-side answers of libkge_hip.so that need no GPU: workspace sizes and the refusals an entry point issues before its
first HIP call, for all 21 model ids.  tests/test_host_cpu.py compares what the library in the tree answers with
tests/golden/host_answers.json, which this script recorded from a build of commit d1db425 (the last one that routed models
through `if (m->model == ...)` ladders), so equal answers mean equal routing:

    make -C pykg2vec_amd/csrc                      # in a checkout of d1db425
    KGE_HIP_LIB=<that checkout>/pykg2vec_amd/libkge_hip.so python tools/host_answers.py tests/golden/host_answers.json

Every call below hands the library dummy pointers, so it must be refused before anything is launched.  That is so by
construction: a hidden size of 4096 is beyond every launcher's limit, and a NULL workspace is only handed to launchers that
check it.  A call that comes back with anything but -1 (a launch that was tried returns -2) stops the recording.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RECORDED_FROM = "d1db425"
MODELS = ("transe", "transh", "transd", "rotate", "rescal", "ntn", "distmult", "complex", "analogy", "transm", "cp", "simple",
          "simple_ignr", "quate", "transr", "slm", "sme", "sme_bl", "kg2e", "hole", "octonione")   # enum kge_model order
# (E, R, dim, n); the last hidden size is not a multiple of 4
SHAPES = ((1000, 20, 32, 64), (14951, 1345, 100, 1024), (500, 7, 50, 33))
REL_DIMS = {"transr": (20, 64, 30), "ntn": (20, 64, 30), "slm": (20, 64, 30)}   # rel_dim != dim, one per shape
GROUPED = ("transh", "transd", "transr")
# which launchers check what, read off the launchers themselves (the dummy-pointer calls rely on it)
SCORER_WS = ("rescal", "ntn", "transr", "slm", "sme", "sme_bl")                 # scorers that refuse a NULL workspace
OWN_RANK = ("ntn", "slm", "sme", "sme_bl", "kg2e", "hole", "octonione")         # rank launchers with a hidden-size limit
ROW_KERNELS = ("transe", "transh", "transd", "rotate", "distmult", "complex", "analogy", "transm", "cp", "simple", "simple_ignr",
               "quate", "kg2e")
BIG = 4096
FAKE, FAKE2 = ctypes.c_void_p(16), ctypes.c_void_p(32)   # never dereferenced
ROOMY = 1 << 62


def desc(_lib, model, E, R, dim, rel_dim):
    d = _lib.ModelDesc()
    d.model, d.tot_entity, d.tot_relation, d.dim, d.rel_dim, d.margin = MODELS.index(model), E, R, dim, rel_dim, 1.0
    for i in range(_lib.KGE_MAX_TABLES):
        d.tables[i] = d.grads[i] = 16
    return d


def sizes(_lib, lib):
    out = []
    for k, (E, R, dim, n) in enumerate(SHAPES):
        for model in MODELS:
            for rel_dim in (dim,) + ((REL_DIMS[model][k],) if model in REL_DIMS else ()):
                d = ctypes.byref(desc(_lib, model, E, R, dim, rel_dim))
                row = dict(model=model, E=E, R=R, dim=dim, rel_dim=rel_dim, n=n, workspace=lib.kge_workspace_bytes(d, n),
                           eval_workspace=lib.kge_eval_workspace_bytes(d, n))
                if model in GROUPED:
                    row["eval_grouped_workspace"] = {str(g): lib.kge_eval_grouped_workspace_bytes(d, n, g) for g in (1, 3)}
                out.append(row)
    return out


def refusals(_lib, lib):
    n = 4
    calls = {
        "kge_score_forward": lambda d, ws, nb, **_: lib.kge_score_forward(d, FAKE, FAKE, FAKE, n, FAKE, ws, nb, None),
        "kge_score_backward": lambda d, ws, nb, **_: lib.kge_score_backward(d, FAKE, FAKE, FAKE, n, FAKE, ws, nb, None),
        "kge_train_pairwise_hinge": lambda d, ws, nb, nr=FAKE2, **_: lib.kge_train_pairwise_hinge(
            d, FAKE, FAKE, FAKE, FAKE, nr, FAKE, n, 1.0, ws, nb, FAKE, None),
        "kge_train_pointwise_logistic": lambda d, ws, nb, **_: lib.kge_train_pointwise_logistic(
            d, FAKE, FAKE, FAKE, FAKE, n, 1, 0.0, 0, FAKE, None),
        "kge_eval_ranks": lambda d, ws, nb, **_: lib.kge_eval_ranks(d, FAKE, n, None, None, None, None, ws, nb, FAKE, None),
        "kge_eval_sweep_scores_side": lambda d, ws, nb, **_: lib.kge_eval_sweep_scores_side(d, FAKE, n, 0, ws, nb, FAKE, None),
    }
    plan = []   # (entry point, model, case, hidden size, workspace, workspace bytes, extra)
    for model in MODELS:
        rank_entries = ("kge_eval_ranks", "kge_eval_sweep_scores_side")
        # hidden size beyond every limit, roomy dummy workspace
        for entry in ("kge_score_forward", "kge_score_backward", "kge_train_pairwise_hinge", "kge_train_pointwise_logistic"):
            plan.append((entry, model, "hidden size 4096", BIG, FAKE, ROOMY, {}))
        if model in ("rescal", "transr"):   # nr == pr: the one-launch / two-launch shortcut must decline this shape
            plan.append(("kge_train_pairwise_hinge", model, "hidden size 4096, shared relation ids", BIG, FAKE, ROOMY, dict(nr=FAKE)))
        if model in OWN_RANK:
            plan += [(entry, model, "hidden size 4096", BIG, FAKE, ROOMY, {}) for entry in rank_entries]
        # valid hidden size, no workspace / a workspace of 64 bytes
        if model in SCORER_WS:
            plan += [(entry, model, "no workspace", 32, None, 0, {}) for entry in ("kge_score_forward", "kge_score_backward")]
        if model not in ROW_KERNELS:
            plan.append(("kge_train_pairwise_hinge", model, "no workspace", 32, None, 0, {}))
        plan += [(entry, model, "no workspace", 32, None, 0, {}) for entry in rank_entries]
        plan.append(("kge_eval_ranks", model, "64-byte workspace", 32, FAKE, 64, {}))
    out = []
    for entry, model, case, dim, ws, nb, extra in plan:
        rc = calls[entry](ctypes.byref(desc(_lib, model, 1000, 20, dim, dim)), ws, nb, **extra)
        err = lib.kge_last_error().decode()
        if rc != -1:
            raise RuntimeError("%s (%s, %s) was not refused before its first HIP call: rc %d, %r" % (entry, model, case, rc, err))
        out.append(dict(entry=entry, model=model, case=case, rc=rc, error=err))
    return out


def collect():
    """What the library that pykg2vec_amd._lib loads answers (KGE_HIP_LIB selects another build)."""
    if os.environ.get("KGE_DEBUG_IDS", "0") not in ("", "0"):
        raise RuntimeError("KGE_DEBUG_IDS reads the id arrays: unset it for the dummy-pointer calls")
    from pykg2vec_amd import _lib
    lib = _lib.load()
    return dict(recorded_from=RECORDED_FROM, sizes=sizes(_lib, lib), refusals=refusals(_lib, lib))


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(collect(), f, indent=1)
        f.write("\n")
