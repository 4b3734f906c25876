"""SlotSampling: everything a request's SamplingParams becomes on the device, one entry per engine slot.

The cycle reads these arrays at replay, so a change never re-captures a graph; the host mirrors exist so that a value is
uploaded only when it changes.  Nothing here touches the model or the KV cache; every kernel-free path runs on CPU tensors.
Three layers, each neutral -- and the last two unallocated -- until a request asks for it; level() orders them:
  1 sampling (sampler.py:216-316): temperature / top_k / top_p per slot and, as `v_` twins, per verify row; temperature 0 =
    greedy.  A seeded request draws from Philox keyed by (seed, seq_lens at the start of the cycle, stream, j, v) alone
    (include/qspec_hip.h, "seeded draws"); seq_seeded[b] == 0: the engine stream.
  2 logit processors (sampler.py:258-278; include/qspec_hip.h, "logit processors"): min_p, the penalties (fp16, as the reference
    holds them), min_tokens; the token table [B, V] (bit 31: in the prompt, low bits: output count), counted_len [B] (how many
    of gen_tokens[b][:gen_lens[b]] the table holds) and the processed-logits buffers.  INVARIANT: the catch-up is driven by
    gen_lens alone, so the engine's recover() -- which restores gen_lens to its value at the start of the failed cycle, i.e.
    to counted_len -- re-runs it without double counting.
  3 token constraints (include/qspec_hip.h, "token constraints"): logit_bias, allowed_token_ids, bad words in an
    ops.TokenConstraints (a deny bitmask, a sorted bias list, the multi-token words, the pre-admission tail).
  4 token guides (include/qspec_hip.h, "token guides"): guided decoding, a guides.TokenFSM per slot.  The resident guides sit
    in an ops.TokenGuides arena (allocated with the first guided request) placed by a guides.GuideArena: one copy per guide
    object, reference-counted by the slots.  gslot[b] = {state, g_len, miss, guided}: the state after g_len of
    gen_tokens[b][:gen_lens[b]].  INVARIANT (as counted_len's): the guide catch-up is driven by gen_lens alone -- it walks
    gen_tokens[b][g_len .. gen_lens) and sets g_len = gen_lens -- so recover(), which restores gen_lens to its value at the
    start of the failed cycle, i.e. to g_len, re-runs it without walking a token twice.  The outputs a re-admitted request had
    before its admission are walked on the host at admission (g_len = 0)."""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional, Sequence

import torch

from .. import ops
from .guides import GuideArena, TokenFSM


# The per-row arrays of one sampler call.  slot_ids: the slot of each sequence (None: sequence i is slot i); proc_out: where the
# pre-pass writes the processed logits (it and minp are None until a request first uses a logit processor)
Rows = namedtuple("Rows", "temp topk topp minp seeds seeded slot_ids proc_out")


class SlotSampling:
    _LP_NEUTRAL = (0.0, 0.0, 0.0, 1.0, 0, ())   # min_p, presence, frequency, repetition, min_tokens, stop ids

    def __init__(self, B: int, k: int, vocab_size: int, device, guide_states: int = 1024, guide_transitions: int = 1 << 24):
        self.B, self.k, self.vocab_size, self.device = B, k, vocab_size, torch.device(device)
        if int(guide_states) < 1 or int(guide_transitions) < 1:
            raise ValueError("guide_states / guide_transitions must be >= 1")
        self.guide_states, self.guide_transitions = int(guide_states), int(guide_transitions)
        self._g_host = None       # per slot None, or its TokenFSM; None until first used
        self.tg = self.guide_arena = None
        T, dev = B * (k + 1), self.device
        self.samp_temp = torch.zeros(B, dtype=torch.float32, device=dev)
        self.samp_topk = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.samp_topp = torch.ones(B, dtype=torch.float32, device=dev)
        self.v_samp_temp = torch.zeros(T, dtype=torch.float32, device=dev)     # the same, one row per verify token
        self.v_samp_topk = torch.full((T,), -1, dtype=torch.int32, device=dev)
        self.v_samp_topp = torch.ones(T, dtype=torch.float32, device=dev)
        self._samp_host = [(0.0, -1, 1.0)] * B
        self.seq_seed = torch.zeros(B, dtype=torch.int64, device=dev)
        self.seq_seeded = torch.zeros(B, dtype=torch.int32, device=dev)
        self._seed_host: List[Optional[int]] = [None] * B
        self._lp_host = None      # per slot (min_p, pres, freq, rep, min_tokens, stop ids); None until first used
        self.samp_minp = self.v_samp_minp = self.tok_table = self.counted_len = self.proc_logits_d = self.proc_logits_v = None
        self._tc_host = None      # per slot None, or (biases, allowed ids, bad words); None until first used
        self.tc = None

    def _lp(self, slot: int):
        return self._LP_NEUTRAL if self._lp_host is None else self._lp_host[slot]

    def _tc(self, slot: int):
        return None if self._tc_host is None else self._tc_host[slot]

    # ------------------------------------------------------------------ what the occupied slots ask for
    def sampling_on(self, occupied_slots: Sequence[int]) -> bool:
        return any(self._samp_host[b][0] >= 1e-5 for b in occupied_slots)

    def constraints_on(self, occupied_slots: Sequence[int]) -> bool:
        return self._tc_host is not None and any(self._tc_host[b] is not None for b in occupied_slots)

    def guides_on(self, occupied_slots: Sequence[int]) -> bool:
        return self._g_host is not None and any(self._g_host[b] is not None for b in occupied_slots)

    def processing_on(self, occupied_slots: Sequence[int]) -> bool:   # a non-neutral logit processor, or a token constraint
        return self.constraints_on(occupied_slots) or (
            self._lp_host is not None and any(self._lp_host[b] != self._LP_NEUTRAL for b in occupied_slots))

    def level(self, occupied_slots: Sequence[int]) -> int:
        """0 greedy, 1 sampling, 2 logit processors, 3 token constraints, 4 token guides"""
        if self.guides_on(occupied_slots):
            return 4
        return 3 if self.constraints_on(occupied_slots) else 2 if self.processing_on(occupied_slots) else \
            int(self.sampling_on(occupied_slots))

    # ------------------------------------------------------------------ the row sets of the sampler calls
    def draft_rows(self) -> Rows:   # one row per slot: a draft step, the non-speculative step
        return Rows(self.samp_temp, self.samp_topk, self.samp_topp, self.samp_minp, self.seq_seed, self.seq_seeded, None,
                    self.proc_logits_d)

    def verify_rows(self) -> Rows:   # k + 1 rows per slot
        return Rows(self.v_samp_temp, self.v_samp_topk, self.v_samp_topp, self.v_samp_minp, self.seq_seed, self.seq_seeded, None,
                    self.proc_logits_v)

    def gathered_rows(self, slots: Sequence[int], level: int, sampled: bool, like: torch.Tensor) -> Rows:
        """One row per listed slot, contiguous (admission); only what the call will read: the sampler's arrays when it samples,
        the slot ids and a buffer shaped like `like` for the pre-pass from level 2 on."""
        idx = torch.tensor(slots, dtype=torch.int64, device=self.device) if sampled else None
        g = lambda t, on=True: t[idx].contiguous() if sampled and on else None   # noqa: E731
        return Rows(g(self.samp_temp), g(self.samp_topk), g(self.samp_topp), g(self.samp_minp, level >= 2), g(self.seq_seed),
                    g(self.seq_seeded), torch.tensor(slots, dtype=torch.int32, device=self.device) if level >= 2 else None,
                    torch.empty_like(like) if level >= 2 else None)

    # ------------------------------------------------------------------ a request's parameters
    def set(self, slot: int, temperature: float = 0.0, top_k: int = -1, top_p: float = 1.0, seed: Optional[int] = None,
            min_p: float = 0.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0, repetition_penalty: float = 1.0,
            min_tokens: int = 0, stop_token_ids: Sequence[int] = (), logit_bias=None, allowed_token_ids=None,
            bad_words_token_ids=None, occupied: bool = False, guide: Optional[TokenFSM] = None) -> None:
        """QSpecEngine.set_sampling_params (its docstring is the contract).  occupied: a request sits in the slot."""
        stop = tuple(int(t) for t in stop_token_ids)
        vals = (float(min_p), float(presence_penalty), float(frequency_penalty), float(repetition_penalty))
        if len(stop) > ops.MAX_STOP_IDS:
            raise ValueError(f"{len(stop)} stop token ids: at most {ops.MAX_STOP_IDS} are supported")
        if not all(v == v and abs(v) != float("inf") for v in vals):
            raise ValueError("min_p and the penalties must be finite")
        if not 0.0 <= vals[0] <= 1.0:
            raise ValueError(f"min_p {min_p} outside [0, 1]")
        if not vals[3] > 0.0:
            raise ValueError(f"repetition_penalty {repetition_penalty} must be > 0")
        if int(min_tokens) < 0:
            raise ValueError(f"min_tokens {min_tokens} must be >= 0")
        want_tc = self._validate_constraints(slot, logit_bias, allowed_token_ids, bad_words_token_ids,
                                             stop if int(min_tokens) > 0 else (), occupied)
        self._validate_guide(slot, guide, occupied)
        if temperature < 1e-5:   # (min_p is reset for greedy requests, sampling_params.py:344; the rest applies to them too)
            temperature, top_k, top_p, seed = 0.0, -1, 1.0, None
            vals = (0.0,) + vals[1:]
        if int(min_tokens) == 0 or not stop:
            min_tokens, stop = 0, ()
        want_lp = vals + (int(min_tokens), stop)
        k1 = self.k + 1
        if want_lp != self._lp(slot):
            h = torch.tensor(vals[1:], dtype=torch.float16)   # what the kernels will read
            if float(h[2]) <= 0.0 or not bool(torch.isfinite(h).all()):
                raise ValueError("a penalty is outside the fp16 range")
            need = int(float(h[0]) != 0.0 or float(h[1]) != 0.0 or float(h[2]) != 1.0)
            if need and occupied and not self._lp_needs(slot):
                raise ValueError(f"slot {slot} is occupied: penalties are set before the request is admitted (its token "
                                 "table is built at admission)")
            self._ensure_processing()
            self.samp_minp[slot] = vals[0]
            self.v_samp_minp[slot * k1:(slot + 1) * k1] = vals[0]
            self.lp_pres[slot] = h[0]; self.lp_freq[slot] = h[1]; self.lp_rep[slot] = h[2]
            self.lp_min_tokens[slot] = int(min_tokens)
            row = torch.zeros(ops.MAX_STOP_IDS, dtype=torch.int32)
            if stop:
                row[:len(stop)] = torch.tensor(stop, dtype=torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32)
            self.lp_stop_ids[slot].copy_(row.to(self.device))
            self.lp_n_stop[slot] = len(stop)
            self.lp_need[slot] = need
            self._lp_host[slot] = want_lp
        if want_tc != self._tc(slot):
            self._ensure_processing()
            if self._tc_host is None:
                self.tc = ops.TokenConstraints(self.B, self.vocab_size, self.device)
                self._tc_host = [None] * self.B
            if want_tc is None:
                ops.token_constraints_set(self.tc, slot)           # flags off: the slot is unconstrained again
            else:
                ops.token_constraints_set(self.tc, slot, dict(want_tc[0]), want_tc[1], [list(w) for w in want_tc[2]])
            self._tc_host[slot] = want_tc
        if guide is not self._guide(slot):
            self._set_guide(slot, guide)
        want_seed = None if seed is None else int(seed) % (1 << 64)
        if self._seed_host[slot] != want_seed:
            self.seq_seed[slot] = 0 if want_seed is None else want_seed - (1 << 64) * (want_seed >= 1 << 63)
            self.seq_seeded[slot] = 0 if want_seed is None else 1
            self._seed_host[slot] = want_seed
        want = (float(temperature), int(top_k) if top_k and top_k > 0 else -1, float(top_p))
        if self._samp_host[slot] == want:
            return
        self.samp_temp[slot] = want[0]; self.samp_topk[slot] = want[1]; self.samp_topp[slot] = want[2]
        self.v_samp_temp[slot * k1:(slot + 1) * k1] = want[0]
        self.v_samp_topk[slot * k1:(slot + 1) * k1] = want[1]
        self.v_samp_topp[slot * k1:(slot + 1) * k1] = want[2]
        self._samp_host[slot] = want

    def clone_params(self, src: int, dst: int, seed_add: int = 0, occupied: bool = False) -> None:
        """The parameters of slot `src` set on slot `dst` (an additional sample of a request, a fork): the same values through
        set(), so the same canonical forms and the same uploads-only-on-change; a seeded request's seed becomes
        (seed + seed_add) mod 2^64."""
        temp, topk, topp = self._samp_host[src]
        seed = self._seed_host[src]
        min_p, pres, freq, rep, min_tokens, stop = self._lp(src)
        bias, allowed, words = self._tc(src) or ((), None, ())
        self.set(dst, temp, topk, topp, None if seed is None else (seed + seed_add) % (1 << 64), min_p, pres, freq, rep, min_tokens,
                 stop, dict(bias), allowed, [list(w) for w in words], occupied=occupied, guide=self._guide(src))

    def fork(self, src: int, dst: int) -> None:
        """Everything slot `src` holds here copied to the EMPTY slot `dst`: the parameters (same seed: a fork continues its
        parent's draws until the two diverge), the token-table row with counted_len and the output base, the pre-admission
        tail of the token constraints, the guide reference with its state and g_len.  Plain copies: forking is not on the
        step's critical path."""
        self.clone_params(src, dst)
        if self._lp_host is None:
            return
        if self._guide(src) is not None:   # (the same resident guide: the same arena rows)
            self.tg.gslot[dst].copy_(self.tg.gslot[src])
        self.tok_table[dst].copy_(self.tok_table[src])
        self.counted_len[dst] = self.counted_len[src]
        self.lp_gen_base[dst] = self.lp_gen_base[src]
        self._gen_base_host[dst] = self._gen_base_host[src]
        if self.tc is not None:
            self.tc.tail[dst].copy_(self.tc.tail[src])
            self.tc.meta[dst, 3] = self.tc.meta[src, 3]

    def _validate_constraints(self, slot: int, logit_bias, allowed_token_ids, bad_words_token_ids, stop: Sequence[int],
                              occupied: bool):
        """The canonical form of a request's token constraints -- (sorted (id, bias) pairs, sorted allowed ids or None, bad
        words) -- or None when it has none.  Raises ValueError; enqueues nothing."""
        if not logit_bias and allowed_token_ids is None and not bad_words_token_ids:
            return None
        V = self.vocab_size
        try:
            bias = {int(t): float(b) for t, b in (logit_bias or {}).items()}
        except (TypeError, ValueError) as exc:
            raise ValueError("logit_bias maps token ids (integers or strings of integers) to numbers") from exc
        allowed = None if allowed_token_ids is None else tuple(sorted(set(int(t) for t in allowed_token_ids)))
        words = []
        for w in (bad_words_token_ids or ()):
            w = tuple(int(t) for t in w)
            if not w:
                raise ValueError("an empty bad word")
            if w not in words:
                words.append(w)
        if allowed is not None and not allowed:
            raise ValueError("Empty allowed_token_ids provided")
        for name, ids in (("logit_bias", bias), ("allowed_token_ids", allowed or ()), ("bad_words_token_ids", [t for w in words for t in w])):
            bad = [t for t in ids if not 0 <= t < V]
            if bad:
                raise ValueError(f"{name} contains out-of-vocab token ids {bad[:8]} (vocabulary size {V})")
        if not all(b == b and abs(b) != float("inf") for b in bias.values()):
            raise ValueError("a logit_bias value is not finite")
        multi = [w for w in words if len(w) > 1]
        if len(bias) > ops.MAX_LOGIT_BIAS:
            raise ValueError(f"{len(bias)} logit_bias entries: at most {ops.MAX_LOGIT_BIAS} are supported")
        if len(multi) > ops.MAX_BAD_WORDS:
            raise ValueError(f"{len(multi)} multi-token bad words: at most {ops.MAX_BAD_WORDS} are supported")
        if any(len(w) > ops.MAX_BAD_WORD_LEN for w in multi):
            raise ValueError(f"a bad word is longer than {ops.MAX_BAD_WORD_LEN} tokens")
        single = set(w[0] for w in words if len(w) == 1)
        left = (set(allowed) if allowed is not None else None)
        n_left = len(left - single) if left is not None else V - len(single)
        if n_left <= 0:
            raise ValueError("every allowed token is a single-token bad word: the request could never emit a token")
        if stop:
            gone = single | set(int(t) for t in stop if 0 <= int(t) < V)
            if (len(left - gone) if left is not None else V - len(gone)) <= 0:
                raise ValueError("before min_tokens every allowed token is a bad word or a stop id: the request could never "
                                 "emit a token")
        want = (tuple(sorted(bias.items())), allowed, tuple(words))
        if want != self._tc(slot) and occupied:
            raise ValueError(f"slot {slot} is occupied: token constraints are set before the request is admitted")
        return want

    def _guide(self, slot: int) -> Optional[TokenFSM]:
        return None if self._g_host is None else self._g_host[slot]

    def _validate_guide(self, slot: int, guide, occupied: bool) -> None:
        """ValueError, nothing enqueued: not a TokenFSM, another vocabulary, an occupied slot, no room in the arena."""
        if guide is self._guide(slot):
            return
        if occupied:
            raise ValueError(f"slot {slot} is occupied: a guide is set before the request is admitted")
        if guide is None:
            return
        if not isinstance(guide, TokenFSM):
            raise ValueError("guide must be a TokenFSM (guides.TokenFSM.from_guide lowers a guide object)")
        if guide.vocab != self.vocab_size:
            raise ValueError(f"the guide was lowered for a vocabulary of {guide.vocab}, the model has {self.vocab_size}")
        arena = self.guide_arena or GuideArena(self.guide_states, self.guide_transitions)
        if arena.resident(guide) is None:
            old = self._guide(slot)   # (the slot's present guide is released first: its room counts when it has no other user)
            r = arena.resident(old) if old is not None else None
            if r is not None:
                r.refs -= 1
            try:
                arena.plan(guide)
            finally:
                if r is not None:
                    r.refs += 1

    def _set_guide(self, slot: int, guide: Optional[TokenFSM]) -> None:
        """Release the slot's guide, take a reference to the new one (built into the arena when it is not resident)."""
        old = self._guide(slot)
        if old is not None:
            self.guide_arena.release(old)
            self._g_host[slot] = None
        if guide is None:
            self.tg.set_slot(slot)
            return
        self._ensure_processing()
        if self.tc is None:   # the guided entry rides on the constrained one: its (all-zero) arrays exist
            self.tc = ops.TokenConstraints(self.B, self.vocab_size, self.device)
            self._tc_host = [None] * self.B
        if self.tg is None:
            self.tg = ops.TokenGuides(self.B, self.vocab_size, self.device, self.guide_states, self.guide_transitions)
            self.guide_arena = GuideArena(self.guide_states, self.guide_transitions)
            self._g_host = [None] * self.B
        r, fresh = self.guide_arena.acquire(guide)
        if fresh:
            ops.guide_build(self.tg, r.state_base, r.trans_base, guide.row_ptr, guide.tokens, guide.next_states)
        self._g_host[slot] = guide
        self.tg.set_slot(slot, r.state_base + guide.initial, r.state_base + guide.miss, guided=True)

    def _lp_needs(self, slot: int) -> bool:
        """The slot keeps token counts: one of its penalties is non-neutral (in fp16, as the kernels read it)."""
        _, pres, freq, rp, _, _ = self._lp(slot)
        h = torch.tensor((pres, freq, rp), dtype=torch.float16)
        return bool(float(h[0]) != 0.0 or float(h[1]) != 0.0 or float(h[2]) != 1.0)

    def _ensure_processing(self) -> None:
        if self._lp_host is not None:
            return
        B, T, V, f16, f32 = self.B, self.B * (self.k + 1), self.vocab_size, torch.float16, torch.float32
        z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=self.device)   # noqa: E731
        self.samp_minp, self.v_samp_minp = z(B, dtype=f32), z(T, dtype=f32)      # per slot, and one row per verify token
        self.lp_rep = torch.ones(B, dtype=f16, device=self.device)
        self.lp_freq, self.lp_pres = z(B, dtype=f16), z(B, dtype=f16)
        self.lp_min_tokens, self.lp_stop_ids, self.lp_n_stop = z(B), z(B, ops.MAX_STOP_IDS), z(B)
        self.lp_gen_base = z(B)   # outputs a re-admitted request had before its admission
        self.lp_need = z(B)       # the slot keeps token counts (a non-neutral penalty)
        self._gen_base_host = [0] * B
        self.tok_table, self.counted_len = ops.new_logit_table(B, V, self.device)
        self.proc_logits_d, self.proc_logits_v = z(B, V, dtype=f16), z(T, V, dtype=f16)   # draft / non-speculative rows, verify rows
        self._lp_host = [self._LP_NEUTRAL] * B

    # ------------------------------------------------------------------ admission and the pre-pass
    def admit_tokens(self, slot: int, tokens: Sequence[int], num_prompt_tokens: Optional[int]) -> None:
        """Admission: the outputs the request already has (recomputation), for a slot with penalties its table row, for a slot
        with token constraints the tail of those outputs (a bad word may straddle the admission)."""
        if self._lp_host is None:
            return
        npt = len(tokens) if num_prompt_tokens is None else int(num_prompt_tokens)
        base = len(tokens) - npt
        if self._tc(slot) is not None:
            ops.token_constraints_set_tail(self.tc, slot, list(tokens)[npt:])
        g = self._guide(slot)
        if g is not None:   # the outputs the request already has are walked here; gen_tokens starts empty: g_len = 0
            base_state = self.guide_arena.resident(g).state_base
            self.tg.set_slot(slot, base_state + g.advance(g.initial, list(tokens)[npt:]), base_state + g.miss, guided=True)
        if self._gen_base_host[slot] != base:
            self.lp_gen_base[slot] = base
            self._gen_base_host[slot] = base
        if self._lp_needs(slot):
            ids = torch.tensor(list(tokens), dtype=torch.int64, device=self.device)
            ops.logit_table_set_prompt(self.tok_table, self.counted_len, slot, ids[:npt].contiguous(),
                                       ids[npt:].contiguous() if base else None)

    def catch_up(self, gen_tokens, gen_lens) -> None:
        """The tokens committed since the last catch-up enter the table (idempotent: see the module docstring)."""
        ops.logit_table_catch_up(self.tok_table, self.counted_len, self.lp_need, gen_tokens, gen_lens)

    def guide_catch_up(self, gen_tokens, gen_lens) -> None:
        """The state of every guided slot advances over the tokens committed since (idempotent: see the module docstring)."""
        ops.guide_catch_up(*self.tg.arrays(), self.vocab_size, gen_tokens, gen_lens)

    def process(self, logits, out, rows_per_seq: int, j_base: int, draft_ids, active_lens, gen_tokens, gen_lens, slot_ids=None,
                constrained: bool = False, guided: bool = False):
        """The logits pre-pass in front of a sampler call (ops.process_logits, or its constrained / guided entry: same launches)."""
        T = logits.shape[0]
        shared = (logits, out[:T], self.tok_table, self.lp_rep, self.lp_freq, self.lp_pres, self.lp_min_tokens, self.lp_gen_base,
                  gen_lens, self.lp_stop_ids, self.lp_n_stop)
        rows = dict(draft_ids=draft_ids, rows_per_seq=rows_per_seq, j_base=j_base, slot_ids=slot_ids, active_lens=active_lens)
        if guided:
            return ops.process_logits_guided(*shared, *self.tc.arrays(), gen_tokens, *self.tg.arrays(), **rows)
        if constrained:
            return ops.process_logits_constrained(*shared, *self.tc.arrays(), gen_tokens, **rows)
        return ops.process_logits(*shared, **rows)
