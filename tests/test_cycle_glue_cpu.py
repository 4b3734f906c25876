"""The host references of the cycle glue (tests/cycle_cases.py) against a second, deliberately different model: every
sequence is a Python list of its tokens plus a dict position -> (block, offset), driven through several speculative cycles.
Also: the case builder really holds every class of row the GPU tests rely on."""
import itertools

import numpy as np
import pytest

import cycle_cases as cc

BLOCK_SIZES = (8, 16, 32)
KS = (1, 3, 7)


class Seq:
    """One sequence the way a host scheduler would keep it: its tokens, and where each position's KV lives."""

    def __init__(self, tokens, blocks, block_size):
        self.tokens = list(tokens)
        self.n_prompt = len(self.tokens)
        self.block_size = block_size
        self.kv = {}
        for n, blk in enumerate(blocks):
            for off in range(block_size):
                self.kv[n * block_size + off] = (int(blk), off)

    def slot(self, pos):
        entry = self.kv.get(pos)
        return -1 if entry is None else entry[0] * self.block_size + entry[1]

    def own_slots(self):
        return {b * self.block_size + o for b, o in self.kv.values()}


def _model_batch(case, rng, lens):
    seqs = []
    for b in range(case["B"]):
        L = max(int(lens[b]), 0)
        toks = rng.integers(0, case["vocab"], L).tolist()
        seqs.append(Seq(toks, case["block_tables"][b], case["block_size"]))
    return seqs


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("k", KS)
def test_references_follow_the_list_and_dict_model_over_cycles(bs, k):
    B, cycles, cap = 40, 6, cc.SEQ_SLOTS
    case = cc.build_batch(bs, k, B, seed=11)
    rng = np.random.default_rng([3, bs, k])
    lens = cc.cycle_start_lens(bs, k, B, seed=11)
    seqs = _model_batch(case, rng, lens)
    bt = case["block_tables"]
    seq_lens = np.array([len(s.tokens) for s in seqs], np.int32)
    last = np.array([s.tokens[-1] if s.tokens else 12345 for s in seqs], np.int64)
    gen_tokens = np.full((B, 6 * (k + 1) + k + 1), -1, np.int64)
    gen_lens = np.zeros(B, np.int32)
    refused = stepped = 0
    for cycle in range(cycles):
        # the host refuses a cycle whose positions L-1 .. L-1+k leave the table: the request is finished instead
        for b, s in enumerate(seqs):
            if s.tokens and len(s.tokens) - 1 + k >= cap:
                s.tokens, s.n_prompt = [], 0
                seq_lens[b], gen_lens[b] = 0, 0
                refused += 1
        mask = (rng.integers(0, 5, B) != 0).astype(np.int32)
        live = [b for b, s in enumerate(seqs) if s.tokens and mask[b]]
        stepped += len(live)
        used = {}

        def note(b, slot):
            assert slot >= 0
            used.setdefault(b, set()).add(int(slot))

        d = cc.prepare_draft(last, seq_lens, bt, bs, step_mask=mask)
        eff = d["eff_lens"]
        assert eff.tolist() == [len(s.tokens) * int(mask[b]) for b, s in enumerate(seqs)]
        for b in range(B):
            if b not in live:
                assert (d["tokens"][b], d["positions"][b], d["ctx_lens"][b], d["slots"][b]) == (0, 0, 1, -1)
        draft = rng.integers(0, case["vocab"], (B, k)).astype(np.int64)
        for i in range(k):
            for b in live:
                s, L = seqs[b], len(seqs[b].tokens)
                assert d["tokens"][b] == (s.tokens[-1] if i == 0 else draft[b, i - 1])
                assert d["positions"][b] == L - 1 + i and d["ctx_lens"][b] == L + i
                assert d["slots"][b] == s.slot(L - 1 + i)
                note(b, d["slots"][b])
            if i < k - 1:
                d = cc.advance_draft(d["tokens"], d["positions"], d["ctx_lens"], d["slots"], draft[:, i], bt, bs)
        v = cc.prepare_verify(last, draft, eff, bt, bs)
        for b in range(B):
            rows = slice(b * (k + 1), (b + 1) * (k + 1))
            if b in live:
                s, L = seqs[b], len(seqs[b].tokens)
                assert v["tokens"][rows].tolist() == [s.tokens[-1]] + draft[b].tolist()
                assert v["positions"][rows].tolist() == list(range(L - 1, L + k))
                assert v["slots"][rows].tolist() == [s.slot(p) for p in range(L - 1, L + k)]
                assert v["ctx_lens"][b] == L + k
                for sl in v["slots"][rows]:
                    note(b, sl)
            else:
                assert v["tokens"][rows].tolist() == [0] * (k + 1) and v["slots"][rows].tolist() == [-1] * (k + 1)
                assert v["positions"][rows].tolist() == list(range(k + 1)) and v["ctx_lens"][b] == k + 1
        # no two live rows share a slot, and every slot is one of the row's own
        for b, slots in used.items():
            assert slots <= seqs[b].own_slots()
        for a, b in itertools.combinations(used, 2):
            assert not (used[a] & used[b])
        # accept a random prefix; whatever follows the first -1 is not emitted
        out = np.full((B, k + 1), -1, np.int64)
        for b in live:
            n_acc = int(rng.integers(0, k + 1))
            out[b, :n_acc] = draft[b, :n_acc]
            out[b, n_acc] = int(rng.integers(0, case["vocab"]))
            if n_acc + 2 <= k and rng.integers(0, 2):
                out[b, n_acc + 2] = 777          # behind a -1: must not be appended
            seqs[b].tokens += list(itertools.takewhile(lambda t: t != -1, out[b].tolist()))
        c = cc.commit(out, seq_lens, last, gen_tokens, gen_lens)
        seq_lens, last, gen_tokens, gen_lens = c["seq_lens"], c["last_token"], c["gen_tokens"], c["gen_lens"]
        for b, s in enumerate(seqs):
            assert seq_lens[b] == len(s.tokens)
            if s.tokens:
                assert last[b] == s.tokens[-1]
                assert gen_tokens[b, :gen_lens[b]].tolist() == s.tokens[s.n_prompt:]
    assert refused >= 3 and stepped >= 2 * B        # the run really had rows reach the end, and really stepped


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("k", KS)
def test_safety_net_rules_follow_the_dict(bs, k):
    """Nothing refused: positions beyond the table are simply not in the dict (slot -1), and a draft row that meets one stays
    where it is from then on, its token being the last one sampled while it still had a slot."""
    for rotate in cc.rotations(6, bs, k):
        case = cc.build_batch(bs, k, 6, seed=5, rotate=rotate)
        B, bt = case["B"], case["block_tables"]
        rng = np.random.default_rng([9, bs, k, rotate])
        seqs = [Seq([0] * max(int(L), 0), bt[b], bs) for b, L in enumerate(case["seq_lens"])]
        d = cc.prepare_draft(case["last_token"], case["seq_lens"], bt, bs, step_mask=case["step_mask"])
        eff = d["eff_lens"]
        state = []                                  # per row: [token, position, has a slot]
        for b in range(B):
            L = int(case["seq_lens"][b]) * int(case["step_mask"][b])
            state.append([int(case["last_token"][b]), L - 1, True] if L > 0 else [0, 0, False])
            assert eff[b] == L
        for step in range(k + 2):
            for b in range(B):
                tok, pos, has = state[b]
                assert (d["tokens"][b], d["positions"][b], d["ctx_lens"][b]) == (tok, pos, pos + 1)
                assert d["slots"][b] == (seqs[b].slot(pos) if has else -1)
            sampled = rng.integers(0, case["vocab"], B).astype(np.int64)
            d = cc.advance_draft(d["tokens"], d["positions"], d["ctx_lens"], d["slots"], sampled, bt, bs)
            for b in range(B):
                if not state[b][2] or seqs[b].slot(state[b][1]) < 0:
                    state[b][2] = False
                    continue
                state[b][0] = int(sampled[b])
                if state[b][1] + 1 in seqs[b].kv:
                    state[b][1] += 1
                else:
                    state[b][2] = False
        draft = rng.integers(0, case["vocab"], (B, k)).astype(np.int64)
        v = cc.prepare_verify(case["last_token"], draft, eff, bt, bs)
        for b in range(B):
            L = int(eff[b])
            got = v["slots"][b * (k + 1):(b + 1) * (k + 1)].tolist()
            assert got == ([-1] * (k + 1) if L <= 0 else [seqs[b].slot(L - 1 + j) for j in range(k + 1)])


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B", [1, 6, 64, 65, 130])
def test_case_builder_holds_every_class(bs, k, B):
    seen = {}
    for rotate in cc.rotations(B, bs, k):
        case = cc.build_batch(bs, k, B, rotate=rotate)
        assert case["max_blocks"] * bs == cc.SEQ_SLOTS and case["block_tables"].shape == (B, case["max_blocks"])
        assert sorted(case["block_tables"].ravel().tolist()) == list(range(B * case["max_blocks"]))   # no shared block
        for name, rows in cc.row_classes(case).items():
            seen[name] = seen.get(name, 0) + len(rows)
        lens = {(int(L), int(m)) for L, m in zip(case["seq_lens"], case["step_mask"])}
        seen.setdefault("lens", set()).update(lens)
    cap = cc.SEQ_SLOTS
    for L in (1, bs, bs + 1, cap - k, cap - 1, cap, 0):
        assert (L, 1) in seen["lens"], L
    assert any(L < 0 for L, _ in seen["lens"])
    for name in ("empty", "masked", "block_last_slot", "crosses_block", "verify_past_table"):
        assert seen[name] > 0, name
    if k >= 2:
        assert seen["frozen_mid_draft"] > 0


def test_cycle_start_lens_reach_the_end_of_their_tables():
    for bs in BLOCK_SIZES:
        lens = cc.cycle_start_lens(bs, 3, 40)
        assert (lens == 0).sum() >= 3 and (lens == cc.SEQ_SLOTS - 3).sum() >= 3 and (lens == cc.SEQ_SLOTS - 2).sum() >= 3
        assert ((lens > 0) & (lens <= cc.SEQ_SLOTS - 3)).sum() >= 20


def test_commit_capacity_and_prefix_rule():
    out = np.array([[5, 6, 7, 8], [5, -1, 9, 9], [-1, 4, 4, 4], [1, 2, 3, -1]], np.int64)
    gen = np.full((4, 6), -7, np.int64)
    c = cc.commit(out, np.array([10, 10, 10, 10], np.int32), np.array([0, 0, 42, 0], np.int64), gen,
                  np.array([4, 0, 3, 5], np.int32))
    assert c["gen_tokens"].tolist() == [[-7, -7, -7, -7, 5, 6], [5, -7, -7, -7, -7, -7], [-7] * 6, [-7, -7, -7, -7, -7, 1]]
    assert c["gen_lens"].tolist() == [8, 1, 3, 8] and c["seq_lens"].tolist() == [14, 11, 10, 13]
    assert c["last_token"].tolist() == [8, 5, 42, 3]
    c = cc.commit(out, np.array([1, 1, 1, 1], np.int32), np.array([0, 0, 42, 0], np.int64))
    assert c["gen_tokens"] is None and c["gen_lens"] is None and c["seq_lens"].tolist() == [5, 2, 1, 4]


def test_snapshot_layout_and_error_words():
    i32, i64 = cc.snapshot([3, 4], [1, 2], [70, 80], [5, 6, 7], [11, 12])
    assert i32.tolist() == [3, 4, 1, 2] and i64.tolist() == [70, 80, 5, 6, 7, 11, 12]
    back = cc.restore(i32, i64, 2)
    assert [x.tolist() for x in back] == [[3, 4], [1, 2], [70, 80], [5, 6, 7], [11, 12]]
    assert cc.collect_error_words([], True) == (0, [])
    assert cc.collect_error_words([0, 6, -9, cc.I32_MIN + 1], False) == (6 | 9 | (2 ** 31 - 1), [0, 6, -9, cc.I32_MIN + 1])
    assert cc.collect_error_words([-4, None, 3], True) == (7, [0, None, 0])
