"""The epoch cursor the owner-computes paths share (pykg2vec_amd/state.py: OwnerRunState.run_steps), driven without a GPU by a
stub generator and a recording `run`.  5 batches per epoch, B = 4, neg_rate 1: a batch consumes 4 Philox counters.  Every
expected tuple below is written out from the protocol: the first step of a call samples stand-alone unless the current list
set was sampled for (that batch, that offset); the sampler of the following batch rides in every step, after the last step
of a call as sample_after_last = 1 (the next batch of the epoch) or 2 (batch 0 of the next epoch); the list set flips once per
carried sampler; `ready` names the batch and offset the current set was sampled for."""
import types

import pytest

from pykg2vec_amd.state import OwnerRunState, PullState

N_BATCHES, B = 5, 4


class StubLists:
    def __init__(self):
        self.clears = 0

    def clear(self):
        self.clears += 1


class StubGenerator:
    neg_rate = 1

    def __init__(self):
        self._batch_idx = self._pending = self._draws = 0

    def start_one_epoch(self, num_batch):
        self._pending, self._batch_idx = num_batch, 0

    def stop(self):
        self._pending = 0

    def counters(self):
        return self._batch_idx, self._pending, self._draws


class Harness:
    def __init__(self, kind):
        self.kind = kind
        lists = [StubLists(), StubLists()]
        if kind == "pull":   # the pull state without its device buffers: the cursor needs lists / cur_list / ready / cur only
            self.st = PullState.__new__(PullState)
            OwnerRunState.__init__(self.st, lists)
            self.st.cur = 0
        else:
            self.st = OwnerRunState(lists)
        self.gen = StubGenerator()
        self.index = types.SimpleNamespace(n_batches=N_BATCHES, batch_size=B)
        self.flat = types.SimpleNamespace(step=0)
        self.calls = []

    def run(self, first_batch, n_steps, *rest):
        if self.kind == "pull":   # kge_pull_run also takes the table half the first step reads
            assert rest[0] == self.st.cur
            rest = rest[1:]
        cur_list, lists_ready, first_opt_step, first_offset, sample_after_last = rest
        assert first_opt_step == self.flat.step + 1
        self.calls.append((first_batch, n_steps, cur_list, lists_ready, first_offset, sample_after_last))

    def step(self, n):
        self.st.run_steps(self.gen, self.index, n, self.flat, self.run)
        return self.calls[-1]

    def state(self):
        """(cur_list, ready, optimiser steps taken, clears of list set 0 / 1[, table half])"""
        s = (self.st.cur_list, self.st.ready, self.flat.step, self.st.lists[0].clears, self.st.lists[1].clears)
        return s + ((self.st.cur,) if self.kind == "pull" else ())


def expect(h, state, cur):
    assert h.state() == state + ((cur,) if h.kind == "pull" else ())


@pytest.fixture(params=["pull", "owner"])
def h(request):
    return Harness(request.param)


def test_two_epochs_in_chunks(h):
    h.gen.start_one_epoch(N_BATCHES)
    assert h.step(1) == (0, 1, 0, False, 0, 1)
    expect(h, (1, (1, 4), 1, 0, 0), 1)
    assert h.step(2) == (1, 2, 1, True, 4, 1)
    expect(h, (1, (3, 12), 3, 0, 0), 1)
    assert h.step(2) == (3, 2, 1, True, 12, 2)      # ends the epoch: batch 0 of the next one rides in its last step
    expect(h, (1, (0, 20), 5, 0, 0), 1)
    assert h.gen.counters() == (5, 0, 20)
    h.gen.start_one_epoch(N_BATCHES)
    assert h.step(5) == (0, 5, 1, True, 20, 2)
    expect(h, (0, (0, 40), 10, 0, 0), 0)
    assert h.gen.counters() == (5, 0, 40)
    assert len(h.calls) == 4


def test_abandoned_epoch_discards_the_stale_list_set_once(h):
    h.gen.start_one_epoch(N_BATCHES)
    assert h.step(3) == (0, 3, 0, False, 0, 1)
    expect(h, (1, (3, 12), 3, 0, 0), 1)
    h.gen.stop()
    h.gen.start_one_epoch(N_BATCHES)
    assert h.step(5) == (0, 5, 1, False, 12, 2)     # the set sampled for batch 3 is cleared and batch 0 sampled stand-alone
    expect(h, (0, (0, 32), 8, 0, 1), 0)
    h.gen.start_one_epoch(N_BATCHES)
    assert h.step(2) == (0, 2, 0, True, 32, 1)      # `ready` was rebuilt: nothing more is cleared
    expect(h, (0, (2, 40), 10, 0, 1), 0)


@pytest.mark.parametrize("pending, taken, asked", [(N_BATCHES, 3, 3), (N_BATCHES + 1, 0, N_BATCHES + 1)])
def test_more_steps_than_remain_raise_and_change_nothing(h, pending, taken, asked):
    """More than the generator has pending, or more than the index has batches."""
    h.gen.start_one_epoch(pending)
    if taken:
        h.step(taken)
    counters, state, calls = h.gen.counters(), h.state(), list(h.calls)
    with pytest.raises(StopIteration):
        h.st.run_steps(h.gen, h.index, asked, h.flat, h.run)
    assert (h.gen.counters(), h.state(), h.calls) == (counters, state, calls)
