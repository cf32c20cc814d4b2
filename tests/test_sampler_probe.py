"""The device samplers (kge_corrupt: k_sample; kge_pull_sample: pull_sample_one) against oracle/sampler_oracle.py on train sets built
to make the membership probe work and the redraw loop turn: every (h, r) has 8 of its E tails in train, so a tail corruption is
rejected with probability 8 / E and a head corruption likewise, while every pair keeps E - 8 free candidates on either side.

  small    E = 12, R = 3: 288 triples, 1 024 slots; two draws in three are rejected
  tiny     E = 12, R = 3, the 8 tails of ONE (h, r): 8 triples, the 16-slot table (load 0.5; a 16-slot group is the whole table)
  half     E = 16, R = 4: 512 triples, 1 024 slots (load 0.5: the longest runs kernels.triple_set_build allows)
  quarter  the same plus a ninth tail of one (h, r): 513 triples, 2 048 slots (load 0.25)

(12 * 3 * 12 = 432 distinct triples cannot make n = 512, hence E = 16, R = 4 for the last two.)  Integer work: no tolerance."""
import functools

import numpy as np
import pytest

import sampler_oracle as so

N_PAIRS = 601   # three 256-thread blocks, the last one partial
SEED, OFFSET = 2 ** 40 + 17, 2 ** 33 + 5


def _train(name):
    E, R = (12, 3) if name in ("small", "tiny") else (16, 4)
    rows = [(h, r, (h + r + k) % E) for h in range(E) for r in range(R) for k in range(8)]
    if name == "tiny":
        rows = [(3, 1, t) for t in (0, 2, 3, 5, 7, 8, 10, 11)]
    if name == "quarter":
        rows.append((5, 2, (5 + 2 + 8) % E))
    train = np.asarray(rows, dtype=np.int64)
    assert len({tuple(x) for x in rows}) == len(rows) == {"small": 288, "tiny": 8, "half": 512, "quarter": 513}[name]
    return E, R, train


class _CountingSet(set):
    rejected = 0

    def __contains__(self, x):
        hit = set.__contains__(self, x)
        self.rejected += int(hit)
        return hit


@functools.lru_cache(maxsize=None)
def _case(name, bern):
    """(E, R, train, positives, bern table, oracle negatives, rejected draws): computed once per set, shared, never written to."""
    E, R, train = _train(name)
    pos = train[(np.arange(N_PAIRS) * 7) % len(train)]
    prob = np.linspace(0.1, 0.9, R).astype(np.float32) if bern else None
    train_set = _CountingSet(tuple(map(int, x)) for x in train)
    neg = so.corrupt(pos[:, 0], pos[:, 1], pos[:, 2], 1, E, prob, train_set, SEED, OFFSET)
    for a in (train, pos) + neg:
        a.setflags(write=False)
    return E, R, train, pos, prob, neg, train_set.rejected


CASES = [(n, b) for n in ("small", "tiny", "half", "quarter") for b in (False, True)]


@pytest.mark.parametrize("name,bern", CASES)
def test_oracle_terminates_and_rejects_often(name, bern):
    E, R, train, pos, prob, (nh, nr, nt), rejected = _case(name, bern)
    train_set = {tuple(map(int, x)) for x in train}
    assert not any((int(a), int(b), int(c)) in train_set for a, b, c in zip(nh, nr, nt))
    assert np.array_equal(nr, pos[:, 1]) and np.all((nh == pos[:, 0]) != (nt == pos[:, 2]))
    # 8 of E candidates are taken on the corrupted side: 8 / (E - 8) rejections per pair are expected (2 or 1); 0.4 per pair is far
    # below either and far above what a sparse set gives
    assert rejected > 0.4 * N_PAIRS, rejected


@pytest.mark.gpu
@pytest.mark.parametrize("name,bern", CASES)
def test_device_samplers_equal_the_oracle_on_crowded_sets(name, bern):
    import torch
    import hip_util
    from pykg2vec_amd import _lib as L
    from pykg2vec_amd import kernels as K
    from pykg2vec_amd.generator import PullIndex
    E, R, train, pos, prob, (rh, rr, rt), _ = _case(name, bern)
    pos, train = pos.copy(), train.copy()    # (the shared arrays are read-only; torch wants writable memory)
    slots = K.triple_set_build(hip_util.dev(train))
    assert slots.numel() == {"small": 1024, "tiny": 16, "half": 1024, "quarter": 2048}[name]
    bp = torch.from_numpy(prob.copy()).cuda() if bern else None
    ph, pr, pt = (hip_util.dev(pos[:, i]) for i in range(3))
    # kge_corrupt (k_sample)
    nh, nr, nt = (x.cpu().numpy() for x in K.corrupt(ph, pr, pt, 1, E, bp, slots, SEED, OFFSET))
    assert np.array_equal(nh, rh) and np.array_equal(nr, rr) and np.array_equal(nt, rt)
    train_set = {tuple(map(int, x)) for x in train}
    assert not any((int(a), int(b), int(c)) in train_set for a, b, c in zip(nh, nr, nt))
    # kge_pull_sample (pull_sample_one): same draws, registered with the corrupting entity
    idx = PullIndex([pos], E, R, "cuda")
    pairs, inc = idx.batch(0)[0], idx.batch(0)[1]
    lists = K.PullListSet(N_PAIRS, E, "cuda")
    K.pull_sample(pairs, idx.inv(0), E, bp, slots, SEED, OFFSET, lists)
    torch.cuda.synchronize()
    pc = lists.pc.cpu().numpy()
    c, tail, first = pc & 0xFFFFFF, (pc >> 24) & 1, (pc >> 27) & 1
    assert np.array_equal(np.where(tail == 1, pos[:, 0], c), nh) and np.array_equal(np.where(tail == 1, c, pos[:, 2]), nt)
    count, head, nxt = lists.count.cpu().numpy(), lists.head.cpu().numpy(), lists.next.cpu().numpy()
    bucket = lists.bucket.cpu().numpy().reshape(E, L.PULL_BUCKET)
    dbucket = lists.dbucket.cpu().numpy().reshape(E, L.PULL_BUCKET, 4)
    assert np.array_equal(count, np.bincount(c, minlength=E))
    long_lists = 0
    for e in range(E):
        want = set(np.nonzero(c == e)[0].tolist())
        got = bucket[e, :min(count[e], L.PULL_BUCKET)].tolist()
        for q, i in enumerate(got):
            assert dbucket[e, q].tolist() == [pos[i, 0], pos[i, 1], pos[i, 2], i | int(tail[i]) << 24 | 3 << 25]
        i, chain = int(head[e]), []
        while i >= 0:
            chain.append(i)
            assert len(chain) <= N_PAIRS, "overflow chain of entity %d does not end" % e
            i = int(nxt[i])
        long_lists += bool(chain)
        assert len(got) + len(chain) == count[e] and set(got) | set(chain) == want, e
        assert first[list(want)].sum() == (1 if want else 0), e          # exactly one first registrant per drawn entity
    assert long_lists > 0                                                # 601 pairs over at most 16 entities: the chain is in use
    # the static visit descriptors, filed at the pair's three incidence positions
    sdesc, inv = lists.sdesc.cpu().numpy(), idx.inv(0).cpu().numpy()
    assert np.array_equal(inc.cpu().numpy()[inv], (4 * np.arange(N_PAIRS)[:, None] + np.arange(3)).ravel())
    for role in range(3):
        want = np.stack([pos[:, 0], pos[:, 1], pos[:, 2], c | tail << 24 | role << 25], 1)
        assert np.array_equal(sdesc[inv[3 * np.arange(N_PAIRS) + role]], want), role
