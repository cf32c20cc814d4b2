#!/usr/bin/env python
"""Dev tool: bit-for-bit A/B of two builds of the library on the conv 1-N bodies (ConvE, HypER, InteractE, AcrE serial and parallel),
for changes that must not move a single result bit (the shared tail of csrc/kge_conv_tail.h).

    KGE_HIP_LIB=<library A> python tools/conv_tail_ab.py dump A.npz      (GPU; one fresh process per library)
    KGE_HIP_LIB=<library B> python tools/conv_tail_ab.py dump B.npz
    python tools/conv_tail_ab.py compare A.npz B.npz                     (CPU; exit status 1 unless every array is equal byte for byte)
    python tools/conv_tail_ab.py compare A.npz B.npz A2.npz              (A2: a second dump of library A from another process.  Arrays on
                                                                          which A differs from ITSELF are listed as not reproducible and
                                                                          are not held against B; every other array must be equal)

`dump` runs, on the shapes and seeds of the "other shapes" and duplicate-id cases of tests/test_hip_<model>.py (two rows, 70 rows = a
partial second row tile, several F splits, widths off the 16 / 64 / 128 tiles, repeated ids and id 0 in the scatter), with dropout off
and with all three rates at 0.2:
    * one fused step (kge_<model>_train_bce): loss buffer, every gradient, the six running buffers
    * one body forward / backward pair of the head direction's rows with row0 = B > 0: x, saved, every gradient, the running buffers
    * one rank pass (kge_<model>_eval_ranks) over the batch's triples: ranks and tie counts
The batches stay below 150 rows, where the head's loss is deterministic as well."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RATES = ((0.0, 0.0, 0.0), (0.2, 0.2, 0.2))
SEED, OFFSET, LS = (7 << 32) | 9, 5, 0.1
MODELS = ("conve", "hyper", "interacte", "acre", "acre_parallel")


def cases(T):
    out = dict(T.SHAPES)
    if hasattr(T, "DUP"):
        out["dup"] = T.DUP
    return out


def dump_model(name, out):
    import importlib
    import torch
    from pykg2vec_amd import kernels as K
    T = importlib.import_module("test_hip_" + name)
    stem = "acre" if name.startswith("acre") else name
    fwd, bwd = getattr(K, stem + "_body_forward"), getattr(K, stem + "_body_backward")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda()
    put = lambda key, v: out.__setitem__(key, v.detach().cpu().numpy().copy())
    for case, shape in sorted(cases(T).items()):
        prob = T.problem(**shape)
        lead, (h, r, t, y1, y2) = prob[:-5], prob[-5:]     # (P,) or (P, G)
        B = len(h)
        assert B < 150
        for rates in RATES:
            tag = "%s/%s/p%g" % (name, case, rates[0])
            loss, gs, bufs = T.fused(*lead, h, r, t, y1, y2, rates, SEED, OFFSET, LS, raw=True)
            put(tag + "/step/loss", loss)
            for i, g in enumerate(gs):
                put(tag + "/step/grad%d" % i, g)
            for i, b in enumerate(bufs):
                put(tag + "/step/buf%d" % i, b)
            # the head direction alone: rows B .. 2B-1 of the step's mask rows
            m = T.model_for(*lead, rates, counters=2)
            m.train()
            ws = m.trainable_tensors()
            gs = [torch.zeros_like(w) for w in ws]
            d = m.make_desc(ws, gs, train=True, seed=SEED, offset=OFFSET)
            side = (1,) if name == "conve" else ()
            x, saved = fwd(d, dev(t), dev(r), *side, row0=B)
            dx = torch.from_numpy(np.random.default_rng(B).normal(size=tuple(x.shape)).astype(np.float32)).cuda()
            bwd(d, dev(t), dev(r), *side, dx, saved, row0=B)
            put(tag + "/body/x", x)
            put(tag + "/body/saved", saved)
            for i, g in enumerate(gs):
                put(tag + "/body/grad%d" % i, g)
            for i, b in enumerate(m.running_buffers()):
                put(tag + "/body/buf%d" % i, b)
            m.eval()
            E, R = m.ent_embeddings.weight.shape[0], int(shape["R"])
            trip = dev(np.stack([h, np.asarray(r) % R, t], axis=1))     # (AcrE's duplicate case names rows of the second half of its table)
            csr = K.filter_csr_build(trip, trip, E, R)
            ties = torch.zeros((2, B), dtype=torch.int32, device="cuda")
            put(tag + "/ranks", K.eval_ranks(m.make_desc(train=False), trip, *csr, ties=ties))
            put(tag + "/ties", ties)
        print(name, case, "done", flush=True)


def dump(path):
    import torch
    assert torch.cuda.is_available(), "dump needs the GPU"
    from pykg2vec_amd import _lib
    out = {}
    for name in MODELS:
        dump_model(name, out)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("library %s: %d arrays -> %s" % (_lib.LIB_PATH, len(out), path))


def differing(A, B):
    bad = sorted(set(A.files) ^ set(B.files))
    for key in sorted(set(A.files) & set(B.files)):
        x, y = A[key], B[key]
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(key)
    return bad


def compare(a, b, a2=None):
    A, B = np.load(a), np.load(b)
    bad = differing(A, B)
    print("%d arrays in %s, %d in %s: %s" % (len(A.files), a, len(B.files), b, "all equal byte for byte" if not bad else "%d DIFFER" % len(bad)))
    if a2 is not None:
        noisy = set(differing(A, np.load(a2)))
        print("%d arrays differ between %s and %s, two dumps of ONE library: not reproducible, not held against %s" % (len(noisy), a, a2, b))
        for key in sorted(noisy):
            print("  not reproducible:", key)
        bad = [key for key in bad if key not in noisy]
        print("%d of the reproducible arrays differ" % len(bad))
    for key in bad:
        print("  differs:", key)
    return 1 if bad or not A.files else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) in (4, 5) and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
