"""Block operations and multi-sequence groups in the worker, on the scripted engine double (no GPU): the three block lists of
ExecuteModelRequest reach the engine in the reference's order (vllm/worker/worker.py, execute_worker: swap in, swap out, copy)
in front of the step; a prompt with n = 3 takes three slots and returns three samples; the samples' sequence ids are bound on
the next step by their last token; a single-sequence run makes exactly the engine calls it always made."""
from types import SimpleNamespace

import pytest

from qspec_amd.spec_decode import worker as W
from qspec_amd.spec_decode.worker import ExecuteModelRequest, SequenceData, SequenceGroupMetadata

from test_worker_cpu import FakeEngine, decode, make_worker, prompt


class BlockEngine(FakeEngine):
    """The scripted engine plus the calls this feature adds, recorded in self.calls."""
    first_tokens = None   # slot -> first token (default: the double's 1000 + slot)

    def swap_in(self, pairs):
        self.calls.append(("swap_in", list(pairs)))

    def swap_out(self, pairs):
        self.calls.append(("swap_out", list(pairs)))

    def copy_blocks(self, pairs):
        self.calls.append(("copy", list(pairs)))

    def set_block_table(self, slot, blocks):
        super().set_block_table(slot, blocks)
        self.calls.append(("table", slot, tuple(blocks)))

    def add_sequences_to(self, slots, prompts, block_tables=None, sample_slots=None):
        for i, (b, p) in enumerate(zip(slots, prompts)):
            table = None if block_tables is None else block_tables[i]
            self.add_sequence(b, p, table)
            for c in (sample_slots[i] if sample_slots else ()):
                assert self._len_ub[c] == 0
                self.calls.append(("sample", b, c))
                self._len_ub[c] = len(p) + 1
                self.gen_tokens[c, 0] = 1000 + c
        for b, t in (self.first_tokens or {}).items():
            self.gen_tokens[b, 0] = t


def block_worker(**kw):
    w = make_worker(**kw)
    w._engine_factory = BlockEngine
    nb, _ = w.determine_num_available_blocks()
    w.initialize_cache(nb, 0)
    return w


def group_prompt(rid, seq_id, n_tokens, n, blocks=None, **sp):
    sg = prompt(rid, seq_id, n_tokens, blocks)
    sg.sampling_params = W.SamplingParams(temperature=1.0, n=n, **sp)
    return sg


def test_block_lists_reach_the_engine_in_order_before_the_step():
    w = block_worker()
    sg = prompt("a", 1, 5)
    req = ExecuteModelRequest([sg], blocks_to_copy=[(1, 2)], blocks_to_swap_out=[(3, 0)], blocks_to_swap_in=[(1, 4)])
    w.execute_model(req)
    assert w.engine.calls == [("swap_in", [(1, 4)]), ("swap_out", [(3, 0)]), ("copy", [(1, 2)]), ("add", 0, 5, None)]
    w.engine.calls.clear()
    w.execute_model(ExecuteModelRequest([decode(sg)], num_lookahead_slots=3, blocks_to_copy=[(0, 7), (0, 8)]))
    assert w.engine.calls == [("copy", [(0, 7), (0, 8)]), ("step", (0,))]
    w.engine.calls.clear()
    w.execute_model(ExecuteModelRequest([decode(sg)], num_lookahead_slots=0, blocks_to_swap_out=[(2, 1)]))
    assert w.engine.calls == [("swap_out", [(2, 1)]), ("step_no_spec", (0,))]


def test_empty_block_lists_make_no_call_and_an_older_engine_double_keeps_working():
    w = make_worker()                       # FakeEngine itself: it has none of the three methods
    sg = prompt("a", 1, 5)
    w.execute_model(ExecuteModelRequest([sg], blocks_to_swap_in=[], blocks_to_swap_out=[], blocks_to_copy=[]))
    w.execute_model(ExecuteModelRequest([decode(sg)], num_lookahead_slots=3))
    assert w.engine.calls == [("add", 0, 5, None), ("step", (0,))]
    with pytest.raises(AttributeError):     # asked for, and missing: an error, never silently skipped
        w.execute_model(ExecuteModelRequest([decode(sg)], num_lookahead_slots=3, blocks_to_copy=[(0, 1)]))


def test_clone_carries_the_block_lists():
    req = ExecuteModelRequest([], blocks_to_swap_in=[(1, 2)], blocks_to_swap_out=[(3, 4)], blocks_to_copy=[(5, 6), (5, 7)])
    c = req.clone([])
    assert c.blocks_to_swap_in == [(1, 2)] and c.blocks_to_swap_out == [(3, 4)] and c.blocks_to_copy == [(5, 6), (5, 7)]
    assert ExecuteModelRequest([]).blocks_to_copy == [] and ExecuteModelRequest([]).clone([]).blocks_to_swap_in == []


def _admit_group(w, first_tokens=None):
    w.engine.first_tokens = first_tokens
    sg = group_prompt("g", 7, 20, 3, blocks=[0, 1])
    out = w.execute_model(ExecuteModelRequest([sg]))
    return sg, out


def test_prompt_of_a_group_takes_n_slots_and_returns_n_samples_of_the_parent():
    w = block_worker()
    sg, out = _admit_group(w)
    assert w.engine.calls == [("add", 0, 20, (0, 1)), ("sample", 0, 1), ("sample", 0, 2)]
    assert [v > 0 for v in w.engine._len_ub] == [True, True, True, False]
    assert len(out) == 1 and len(out[0].outputs) == 1
    samples = out[0].outputs[0].samples
    assert [s.parent_seq_id for s in samples] == [7, 7, 7]
    assert [s.output_token for s in samples] == [1000, 1001, 1002]
    assert w.scorer_calls == 1                                     # ONE prompt pass
    # a second, single-sequence prompt takes the one slot left
    w.execute_model(ExecuteModelRequest([prompt("s", 30, 4)]))
    assert w._slots == {"g": 0, "s": 3}


@pytest.mark.parametrize("firsts, last_tokens, want", [
    ({0: 50, 1: 60, 2: 70}, {7: 50, 12: 70, 11: 60}, {7: 0, 11: 1, 12: 2}),     # bound by the last token
    ({0: 50, 1: 50, 2: 50}, {7: 50, 11: 50, 12: 50}, {7: 0, 11: 1, 12: 2}),     # a three-way tie: ascending id, ascending sample
    ({0: 50, 1: 60, 2: 50}, {7: 50, 11: 50, 12: 60}, {7: 0, 11: 2, 12: 1}),     # a tie with the parent: it keeps its slot
])
def test_next_step_binds_each_sequence_id_by_its_last_token_and_uploads_its_table(firsts, last_tokens, want):
    w = block_worker()
    sg, _ = _admit_group(w, firsts)
    seqs = {q: SequenceData(list(range(20)), [t]) for q, t in last_tokens.items()}
    tables = {7: [0, 1], 11: [0, 5], 12: [0, 6]}
    step = SequenceGroupMetadata("g", False, seqs, block_tables=tables, sampling_params=sg.sampling_params)
    w.engine.calls.clear()
    w.engine.out_script = lambda i, slots: {b: [100 + b, -1, -1, -1] for b in slots}
    outs = w.execute_model(ExecuteModelRequest([step], num_lookahead_slots=3, blocks_to_copy=[(1, 5), (1, 6)]))
    order = [want[q] for q in seqs]                               # rows: the group's sequences in seq_data order
    assert w.engine.calls[0] == ("copy", [(1, 5), (1, 6)]) and w.engine.calls[-1] == ("step", tuple(order))
    assert sorted(c for c in w.engine.calls if c[0] == "table") == sorted(("table", want[q], tuple(tables[q])) for q in seqs)
    assert {q: w.engine.block_tables[want[q]] for q in seqs} == tables
    assert len(outs) == 1 and len(outs[0].outputs) == 1           # one output per GROUP, one sample per sequence
    got = outs[0].outputs[0].samples
    assert [s.parent_seq_id for s in got] == list(seqs) and [s.output_token for s in got] == [100 + b for b in order]
    assert w._request_id_seq_id_mapping["g"] == {7, 11, 12}
    # the binding holds on the following step (the last tokens are other ones by then)
    for q, b in want.items():
        seqs[q].output_token_ids.append(100 + b)
    w.execute_model(ExecuteModelRequest([step], num_lookahead_slots=3))
    assert w.engine.calls[-1] == ("step", tuple(order))
    # a sequence nobody sampled is refused
    seqs[99] = SequenceData(list(range(20)), [1])
    with pytest.raises((KeyError, ValueError)):
        w.execute_model(ExecuteModelRequest([step], num_lookahead_slots=3))


def test_finished_group_frees_all_of_its_slots():
    w = block_worker()
    _admit_group(w)
    w.execute_model(ExecuteModelRequest([prompt("s", 30, 4)]))
    w.engine.calls.clear()
    w.execute_model(ExecuteModelRequest([], finished_requests_ids=["g"]))
    assert sorted(w.engine.calls) == [("free", 0), ("free", 1), ("free", 2)]
    assert w._slots == {"s": 3} and [v > 0 for v in w.engine._len_ub] == [False, False, False, True]
    w.execute_model(ExecuteModelRequest([group_prompt("h", 40, 6, 3)]))           # and the next group takes them
    assert [v > 0 for v in w.engine._len_ub] == [True] * 4


def test_group_that_needs_more_slots_than_are_free_is_refused_with_nothing_admitted():
    w = block_worker()
    w.execute_model(ExecuteModelRequest([prompt("s", 30, 4)]))
    w.engine.calls.clear()
    with pytest.raises(RuntimeError, match="no free sequence slot for request g"):
        w.execute_model(ExecuteModelRequest([prompt("t", 31, 4), group_prompt("g", 7, 20, 4)]))
    assert w.engine.calls == [] and w._slots == {"s": 0} and w.engine._len_ub[1:] == [0, 0, 0]
    w.execute_model(ExecuteModelRequest([group_prompt("g", 7, 20, 1, best_of=3)]))    # best_of counts: three fit
    assert [v > 0 for v in w.engine._len_ub] == [True] * 4


def test_beam_search_is_still_refused():
    w = make_worker()
    sp = SimpleNamespace(use_beam_search=True, n=2, best_of=2, temperature=0.0, top_k=-1, top_p=1.0, seed=None, logprobs=None,
                         prompt_logprobs=None)
    beam = SequenceGroupMetadata("b", True, {1: SequenceData([1, 2, 3]), 2: SequenceData([1, 2, 3])}, sampling_params=sp)
    with pytest.raises(NotImplementedError):
        w.execute_model(ExecuteModelRequest([beam]))
    assert w._slots == {} and w.engine._len_ub == [0, 0, 0, 0]


def test_pair_validation_is_a_pure_function():
    from qspec_amd.ops import validate_block_pairs as v
    assert v([(0, 5), (0, 6), (23, 7)], 24, 24) == [(0, 5), (0, 6), (23, 7)]       # one src may feed several dst
    assert v([], 24, 24) == []
    assert v([[1, 2]], 24, 24) == [(1, 2)]
    for bad in ([(24, 0)], [(-1, 0)], [(0, 24)], [(0, -1)]):                        # out of range
        with pytest.raises(ValueError, match="outside"):
            v(bad, 24, 24)
    with pytest.raises(ValueError, match="twice"):                                  # a dst twice
        v([(0, 3), (1, 3)], 24, 24)
    for bad in ([(0, 1), (1, 2)], [(4, 4)], [(0, 1), (2, 0)]):                      # a dst that is also a src
        with pytest.raises(ValueError, match="src and dst"):
            v(bad, 24, 24)
    # two id spaces (swaps): each side has its own range, and equal numbers on both sides are no alias
    assert v([(3, 3), (5, 0)], 24, 8, same_space=False) == [(3, 3), (5, 0)]
    with pytest.raises(ValueError, match="outside"):
        v([(3, 8)], 24, 8, same_space=False)
    with pytest.raises(ValueError, match="twice"):
        v([(3, 1), (4, 1)], 24, 8, same_space=False)
    with pytest.raises(ValueError):
        v([(1, 2, 3)], 24, 24)


# what a single-sequence run asks of the engine, recorded before block operations and groups existed: nothing may move
SINGLE_SEQUENCE_CALLS = [
    ("add", 0, 5, (3, 4)), ("add", 1, 9, None),
    ("step", (1, 0)),
    ("step_no_spec", (0,)),
    ("add", 2, 4, None), ("step_no_spec", (1,)),
    ("free", 0),
    ("add", 0, 6, None),
    ("free", 1), ("add", 1, 10, None),
    ("step", (0, 2, 1)),
]


def test_single_sequence_run_makes_exactly_the_engine_calls_it_always_made():
    w = make_worker()
    a, b = prompt("a", 10, 5, [3, 4]), prompt("b", 11, 9)
    w.execute_model(ExecuteModelRequest([a, b]))
    w.execute_model(ExecuteModelRequest([decode(b), decode(a)], num_lookahead_slots=3))
    w.execute_model(ExecuteModelRequest([decode(a)], num_lookahead_slots=0))
    c = prompt("c", 12, 4)
    w.execute_model(ExecuteModelRequest([c, decode(b)], num_lookahead_slots=0))               # a prompt beside a decode row
    d = prompt("d", 13, 6)
    w.execute_model(ExecuteModelRequest([d], finished_requests_ids=["a"]))                    # takes the freed slot
    b2 = SequenceGroupMetadata("b", True, {11: SequenceData(list(range(9)), [7])})            # recomputation of "b"
    w.execute_model(ExecuteModelRequest([b2]))
    b2.seq_data[11].output_token_ids.append(1001)                                             # (the scheduler appends its token)
    w.execute_model(ExecuteModelRequest([decode(d), decode(c), decode(b2)], num_lookahead_slots=3))
    assert w.engine.calls == SINGLE_SEQUENCE_CALLS
    assert w._slots == {"c": 2, "d": 0, "b": 1}
