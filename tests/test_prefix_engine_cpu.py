"""The engine's slot states around a partly computed prompt, on host tensors (tests/host_engine.HostEngine with the forward
and the first-token sampler stubbed): a prefilling slot is occupied for every admission, fork and count, survives sync_lens(),
is refused by step() / step_no_spec(), continues only with the same token list and a computed count that did not shrink, and
is dropped cleanly by free_slot()."""
from types import SimpleNamespace

import pytest
import torch

from host_engine import HostEngine


class _Model:
    def __init__(self):
        self.rows = []           # (positions, slot_mapping, ctx_lens, q_start, max_q_len, n_splits) per forward

    def forward(self, ids, pos, kv_caches, md, scratch, w4a4=False, **kw):
        assert not w4a4
        self.rows.append((pos.tolist(), md.slot_mapping.tolist(), md.ctx_lens.tolist(), md.q_start.tolist(), md.max_q_len, md.n_splits))
        return torch.zeros(ids.numel(), 8, dtype=torch.float16)


class PrefixHostEngine(HostEngine):
    def __init__(self, B=4, k=3, brought=False):
        super().__init__(B, k)
        self.cfg = SimpleNamespace(hidden_size=8, intermediate_size=16, q_size=256, kv_size=128, vocab_size=64,
                                   num_attention_heads=2, num_key_value_heads=1, head_dim=128)
        self.model, self.kv_caches, self._kv_fw = _Model(), [], {}
        self.max_model_len = self.blocks_per_seq * self.block_size
        if brought:              # fewer blocks than slots x max_model_len: every request brings its table
            self.num_blocks = 2 * self.blocks_per_seq
            self.block_tables = torch.zeros(B, self.blocks_per_seq, dtype=torch.int32)
            self._capacity = [0] * B
        else:
            self.block_tables = torch.arange(B * self.blocks_per_seq, dtype=torch.int32).view(B, self.blocks_per_seq)
            self._capacity = [self.max_model_len] * B
        self.firsts, self._prefill_scratch = [], None

    def _first_token(self, hs, scratch, slots, prompt_lens):
        self.firsts.append((list(slots), list(prompt_lens), hs.shape[0]))
        for b, T in zip(slots, prompt_lens):
            self.seq_lens[b] = T + 1
            self.gen_lens[b] = 1
            self._len_ub[b], self._gen_ub[b] = T + 1, 1
        self.n_active = len(self.active_slots())


P = list(range(40, 90))   # 50 tokens


def test_a_prefilling_slot_is_occupied_everywhere():
    e = PrefixHostEngine()
    e.add_sequence(1, P, num_computed_tokens=0, token_chunk_size=20, sample_slots=[3])
    assert e.is_prefilling(1) and e.num_computed_tokens(1) == 20 and e.firsts == []
    assert e._len_ub == [0, 0, 0, 0] and e.seq_lens.tolist() == [0, 0, 0, 0]      # the device still sees an empty slot
    assert e.active_slots() == [1] and e.n_active == 1
    for bad in (1, 3):                                                            # the slot itself and the one held for its sample
        with pytest.raises(ValueError):
            e.add_sequence(bad, [1, 2, 3])
        with pytest.raises(ValueError):
            e.add_sequences_to([0, bad], [[1, 2, 3], [4, 5, 6]])
        with pytest.raises(ValueError):
            e.add_sequence(0, [1, 2, 3], sample_slots=[bad])
    assert len(e.model.rows) == 1 and e._len_ub == [0, 0, 0, 0]                   # nothing was enqueued, nothing admitted
    e.add_sequence(0, [1, 2, 3])
    with pytest.raises(ValueError):
        e.fork_slot(0, 1)
    with pytest.raises(ValueError):
        e.set_sampling_params(1, logit_bias={3: 1.0})                             # the request's parameters are settled
    e.sync_lens()                                                                 # refreshes the bounds from the device ...
    assert e.is_prefilling(1) and e.active_slots() == [0, 1]                      # ... and the record is not one of them
    for step in (e.step, e.step_no_spec):
        with pytest.raises(ValueError, match="partly computed"):
            step(participants=[0, 1])


def test_chunks_continue_and_end_in_the_state_of_a_whole_prompt():
    e = PrefixHostEngine()
    e.add_sequence(2, P, token_chunk_size=20, sample_slots=[0])
    e.add_sequences_to([2, 1], [P, [7, 8, 9]], num_computed_tokens=[20, 0], token_chunk_sizes=[20, None])
    assert e.firsts == [([1], [3], 1)] and e.num_computed_tokens(2) == 40
    e.add_sequence(2, P, num_computed_tokens=40)
    assert e.firsts[-1] == ([2, 0], [50, 50], 2) and not e.is_prefilling(2) and not e._reserved
    assert e._len_ub == [51, 4, 51, 0] and e.n_active == 3
    pos = [r[0] for r in e.model.rows]
    assert pos == [list(range(20)), list(range(20, 40)) + [0, 1, 2], list(range(40, 50))]
    assert [r[2] for r in e.model.rows] == [[20], [40, 3], [50]] and e.model.rows[1][3] == [0, 20, 23]
    bt = e.block_tables[2].tolist()
    assert e.model.rows[2][1] == [bt[p // 16] * 16 + p % 16 for p in range(40, 50)]
    assert e.model.rows[0][5] == 1                                                # no context: the unsplit pass


def test_a_continuation_must_bring_the_same_tokens_and_no_smaller_count():
    e = PrefixHostEngine()
    e.add_sequence(0, P, token_chunk_size=20)
    n = len(e.model.rows)
    with pytest.raises(ValueError, match="another token list"):
        e.add_sequence(0, P[:-1] + [0], num_computed_tokens=20)
    with pytest.raises(ValueError, match="already computed"):
        e.add_sequence(0, P, num_computed_tokens=19)
    with pytest.raises(ValueError):
        e.add_sequences_to([1, 0], [[1, 2], P], num_computed_tokens=[0, 4])
    assert len(e.model.rows) == n and e.num_computed_tokens(0) == 20 and e._is_empty(1)
    e.add_sequence(0, P, num_computed_tokens=32, token_chunk_size=4)              # a hit found later: the caller vouches
    assert e.model.rows[-1][0] == [32, 33, 34, 35] and e.num_computed_tokens(0) == 36
    e.add_sequence(0, P, num_computed_tokens=99)                                  # everything hit: the last token alone
    assert e.model.rows[-1][0] == [49] and e.model.rows[-1][2] == [50] and e._len_ub[0] == 51


def test_computed_tokens_need_a_brought_block_table():
    e = PrefixHostEngine()
    with pytest.raises(ValueError, match="block table"):
        e.add_sequence(0, P, num_computed_tokens=16)
    with pytest.raises(ValueError, match="block table"):
        e.add_sequences_to([0, 1], [P, P], num_computed_tokens=[0, 16])
    assert e.model.rows == [] and e.active_slots() == []
    e.add_sequence(0, P, block_table=[5, 6, 7, 9], num_computed_tokens=16)
    assert e.model.rows[-1][0] == list(range(16, 50)) and e.model.rows[-1][2] == [50]
    assert e.model.rows[-1][1][:2] == [6 * 16, 6 * 16 + 1]
    b = PrefixHostEngine(brought=True)
    with pytest.raises(ValueError):
        b.add_sequence(0, P, token_chunk_size=20)                                 # no table at all: capacity 0


def test_prompt_logprobs_recompute_the_hit_without_writing_it():
    e = PrefixHostEngine()
    e._prompt_logprobs = lambda slot, hs, prompt, n: (torch.zeros(hs.shape[0]),) * 4 if slot is None else None
    e.add_sequence(0, P, block_table=[5, 6, 7, 9], num_computed_tokens=32, token_chunk_size=8, prompt_logprobs=3)
    pos, slots = e.model.rows[-1][0], e.model.rows[-1][1]
    assert pos == list(range(40)) and slots[:32] == [-1] * 32 and slots[32] == 7 * 16
    e.add_sequence(0, P, num_computed_tokens=40)
    assert e.model.rows[-1][0] == list(range(40, 50)) and min(e.model.rows[-1][1]) >= 0
    assert [t.shape[0] for t in e.take_prompt_logprobs(0)] == [49] * 4 and e.take_prompt_logprobs(0) is None


def test_free_slot_drops_a_prefilling_request():
    e = PrefixHostEngine()
    e.add_sequence(1, P, token_chunk_size=20, sample_slots=[2], block_table=[5, 6, 7, 9])
    e.free_slot(1)
    assert not e.is_prefilling(1) and not e._reserved and e.active_slots() == [] and e.n_active == 0
    assert e._bt_host[1] is None
    e.add_sequences_to([1, 2], [[1, 2, 3], [4, 5]])
    assert e._len_ub == [0, 4, 3, 0]
