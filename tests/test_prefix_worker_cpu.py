"""The worker's scheduling of prefix-cache hits and chunked prefill, against a scripted engine double that records
(slot, computed, chunk) per admission: the translation of the scheduler's fields (model_runner.py:488-590), a prompt in three
chunks, continuation against recomputation, aborts, n > 1, and prompt chunks inside a speculative step."""
import pytest
import torch

from qspec_amd.spec_decode.worker import (ExecuteModelRequest, SamplingParams, SequenceData, SequenceGroupMetadata,
                                          SpeculativeConfig, create_spec_worker)
from test_worker_cpu import CFG, FakeEngine, fake_memory_probe, make_worker

BS = 16


class ChunkEngine(FakeEngine):
    """FakeEngine + the chunked admission surface: windows = [(slot, c, q)] in call order."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.block_size = BS
        self.windows, self.prefill, self.held = [], {}, {}

    def is_prefilling(self, slot):
        return slot in self.prefill

    def num_computed_tokens(self, slot):
        return self.prefill.get(slot, (None, 0))[1]

    def add_sequences_to(self, slots, prompts, block_tables=None, sample_slots=None, num_computed_tokens=None,
                         token_chunk_sizes=None):
        self.calls.append(("admit", tuple(slots), tuple(num_computed_tokens or ()), tuple(token_chunk_sizes or ())))
        for i, (b, p) in enumerate(zip(slots, prompts)):
            c = 0 if num_computed_tokens is None else num_computed_tokens[i]
            q = len(p) - c if token_chunk_sizes is None else token_chunk_sizes[i]
            extra = list(sample_slots[i]) if sample_slots else []
            if b in self.prefill:
                assert self.prefill[b][0] == list(p) and c >= self.prefill[b][1]
                extra = self.held.get(b, [])
            else:
                assert self._len_ub[b] == 0 and all(self._len_ub[x] == 0 for x in extra)
            self.windows.append((b, c, q))
            if c + q < len(p):
                self.prefill[b], self.held[b] = (list(p), c + q), extra
                continue
            self.prefill.pop(b, None)
            for x in [b] + extra:
                self._len_ub[x] = len(p) + 1
                self.gen_tokens[x, 0] = 1000 + x

    def free_slot(self, slot):
        super().free_slot(slot)
        self.prefill.pop(slot, None)

    def set_sampling_params(self, slot, temperature=0.0, top_k=-1, top_p=1.0, **kw):
        assert slot not in self.prefill


def worker(k=3, B=4, engine=ChunkEngine):
    w = create_spec_worker(model_config=CFG, model=object(), speculative_config=SpeculativeConfig(k), max_num_seqs=B,
                           max_model_len=512, block_size=BS, device="cpu", engine_factory=engine, disable_log_stats=True,
                           memory_probe=fake_memory_probe)
    w.init_device()
    w.initialize_cache(w.determine_num_available_blocks()[0], 0)
    return w


def chunk(rid, seq_id, n, computed=0, size=None, blocks=None, hit=None, do_sample=None, sp=None):
    data = SequenceData(list(range(n)))
    data.update_num_computed_tokens(computed)
    ends = computed + (size or n) >= n
    return SequenceGroupMetadata(rid, True, {seq_id: data}, block_tables={seq_id: blocks} if blocks else None,
                                 do_sample=ends if do_sample is None else do_sample, token_chunk_size=size,
                                 computed_block_nums=hit, sampling_params=sp)


def decode(sg, k=3):
    return SequenceGroupMetadata(sg.request_id, False, sg.seq_data, block_tables=sg.block_tables, num_speculative_tokens=k)


def test_mirror_dataclasses_default_to_nothing_computed():
    d = SequenceData([1, 2, 3])
    assert d.get_num_computed_tokens() == 0
    d.update_num_computed_tokens(2)
    assert d.get_num_computed_tokens() == 2 and d.get_len() == 3
    assert SequenceGroupMetadata("r", True, {0: d}).computed_block_nums is None


@pytest.mark.parametrize("n,computed,size,hit_blocks,want", [
    (100, 0, None, 0, (0, 100, True)),        # no hit
    (100, 0, None, 2, (32, 68, True)),        # a hit inside the prompt
    (100, 0, 48, 2, (32, 16, False)),         # a hit inside the chunk
    (100, 48, 48, 2, (48, 48, False)),        # a hit behind what is already computed
    (100, 0, 40, 3, (39, 1, False)),          # a hit past the chunk's end: the chunk's last token alone
    (64, 0, None, 4, (63, 1, True)),          # a block-aligned prompt fully hit: the last token alone
    (100, 96, 48, 0, (96, 4, True)),          # the last chunk is clipped to the prompt
])
def test_translation_of_the_scheduler_fields(n, computed, size, hit_blocks, want):
    w = worker()
    s = chunk("r", 5, n, computed, size, hit=list(range(hit_blocks)) or None)
    assert w._prompt_window(s) == want
    w2 = worker()
    w2.execute_model(ExecuteModelRequest([s], num_lookahead_slots=0))
    assert w2.engine.windows == [(0, want[0], want[1])]


def test_three_chunks_of_one_request_share_a_slot():
    w = worker()
    outs = []
    for computed, size in ((0, 64), (64, 64), (128, 64)):
        outs.append(w.execute_model(ExecuteModelRequest([chunk("r", 7, 150, computed, size, blocks=list(range(10)))])))
    assert w.engine.windows == [(0, 0, 64), (0, 64, 64), (0, 128, 22)]
    assert [len(o) for o in outs] == [1, 1, 1]
    assert [o[0].outputs[0].samples for o in outs[:2]] == [[], []] and outs[0][0].outputs[0].prompt_logprobs is None
    assert outs[2][0].token_ids() == [1000] and outs[2][0].outputs[0].samples[0].parent_seq_id == 7
    assert w._slots == {"r": 0} and ("free", 0) not in w.engine.calls
    assert w.scorer_calls == 3 and w.proposer_calls == 0


def test_continuation_against_recomputation():
    w = worker()
    w.execute_model(ExecuteModelRequest([chunk("r", 7, 150, 0, 64)]))
    # the scheduler counts other tokens than the engine holds: the request starts over
    w.execute_model(ExecuteModelRequest([chunk("r", 7, 150, 0, 64)]))
    assert ("free", 0) in w.engine.calls and w.engine.windows == [(0, 0, 64), (0, 0, 64)]
    w.execute_model(ExecuteModelRequest([chunk("r", 7, 150, 64, 64)]))
    assert w.engine.calls.count(("free", 0)) == 1 and w.engine.windows[-1] == (0, 64, 64)
    # a hit found later moves the context forward inside a continuation
    w.execute_model(ExecuteModelRequest([chunk("r", 7, 150, 128, 64, hit=list(range(9)))]))
    assert w.engine.windows[-1] == (0, 144, 6) and w.engine.calls.count(("free", 0)) == 1
    # a running request that comes back as a prompt is a recomputation, as ever
    w.execute_model(ExecuteModelRequest([chunk("r", 7, 150)]))
    assert w.engine.calls.count(("free", 0)) == 2 and w.engine.windows[-1] == (0, 0, 150)


def test_abort_mid_prefill_frees_the_slot():
    w = worker()
    w.execute_model(ExecuteModelRequest([chunk("r", 7, 150, 0, 64)]))
    assert w.engine.is_prefilling(0) and w._taken_slots() == {0}
    w.execute_model(ExecuteModelRequest([], finished_requests_ids=["r"]))
    assert not w.engine.is_prefilling(0) and w._slots == {} and w._taken_slots() == set()
    w.execute_model(ExecuteModelRequest([chunk("s", 8, 20)]))
    assert w._slots == {"s": 0}


def test_two_samples_hold_two_slots_from_the_first_chunk():
    w = worker()
    sp = SamplingParams(n=2)
    w.execute_model(ExecuteModelRequest([chunk("r", 7, 100, 0, 64, sp=sp)]))
    assert w._taken_slots() == {0, 1}
    out = w.execute_model(ExecuteModelRequest([chunk("s", 9, 10), chunk("r", 7, 100, 64, 64, sp=sp)]))
    assert w._slots == {"r": 0, "s": 2}
    assert out[0].outputs[0].samples[0].output_token == 1002
    assert [x.output_token for x in out[0].outputs[1].samples] == [1000, 1001]
    assert w.engine._len_ub[:3] == [101, 101, 11]


def test_do_sample_on_a_chunk_that_does_not_end_the_prompt_is_refused():
    w = worker()
    with pytest.raises(ValueError, match="do_sample"):
        w.execute_model(ExecuteModelRequest([chunk("r", 7, 150, 0, 64, do_sample=True)]))
    assert w.engine.windows == [] and w._slots == {}


def test_prompt_chunks_inside_a_speculative_step():
    k = 3
    w = worker(k=k)
    a = chunk("a", 1, 8)
    w.execute_model(ExecuteModelRequest([a]))
    w.engine.out_script = lambda step, slots: {0: [11, 12, -1, -1]}
    m0 = (w.engine.sampler.num_accepted_tokens, w.engine.sampler.num_emitted_tokens, w.engine.sampler.num_draft_tokens)
    b1, c1 = chunk("b", 2, 100, 0, 64), chunk("c", 3, 20)
    outs = w.execute_model(ExecuteModelRequest([b1, c1, decode(a)], num_lookahead_slots=k))
    # rows: b (not through) all -1, c [first token, -1 x k], a the cycle's; the list stops where every row is -1
    assert [o.token_ids() for o in outs] == [[-1, 1002, 11], [-1, -1, 12]]
    assert all(len(o.outputs) == 3 for o in outs)
    assert w.engine.windows == [(0, 0, 8), (1, 0, 64), (2, 0, 20)]
    assert w.engine.calls[-1] == ("step", (0,))                      # the proposer and the cycle never see the prompts
    assert w.proposer_calls == k and w.scorer_calls == 1 + 1 + 1
    assert (w.engine.sampler.num_accepted_tokens, w.engine.sampler.num_emitted_tokens, w.engine.sampler.num_draft_tokens) == m0
    assert w._seq_with_bonus_token_in_last_step == set()
    # c decodes with the next step, b ends its prompt in it
    w.engine.out_script = lambda step, slots: {0: [13, -1, -1, -1], 2: [21, 22, 23, 24]}
    outs = w.execute_model(ExecuteModelRequest([chunk("b", 2, 100, 64, 64), decode(c1), decode(a)], num_lookahead_slots=k))
    assert w.engine.calls[-1] == ("step", (2, 0)) and w.engine.windows[-1] == (1, 64, 36)
    assert [o.token_ids() for o in outs] == [[1001, 21, 13], [-1, 22, -1], [-1, 23, -1], [-1, 24, -1]]
    assert w._seq_with_bonus_token_in_last_step == {3}


def test_an_engine_without_the_keywords_never_sees_them():
    w = make_worker()                                                # test_worker_cpu.FakeEngine: the old signature
    s = chunk("r", 7, 40, 0, 40, blocks=[1, 2, 3])                   # token_chunk_size = the whole prompt, as vLLM sends it
    out = w.execute_model(ExecuteModelRequest([s], num_lookahead_slots=0))
    assert out[0].token_ids() == [1000] and w.engine.calls == [("add", 0, 40, (1, 2, 3))]
