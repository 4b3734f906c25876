"""Token guides: guided decoding as a finite automaton over token ids, lowered for the device (host side, numpy only).

The reference's engine lowers SamplingParams.guided_decoding (regex, JSON schema, choice) to an Outlines logits processor at index
0 of logits_processors (vllm/engine/llm_engine.py:1950-2009); its call
(vllm/model_executor/guided_decoding/outlines_logits_processors.py:34-93) keeps one automaton state per sequence, advanced over
the sequence's OUTPUT tokens, and masks every token the state does not allow.  Nothing here compiles a regex: a TokenFSM is built
from an automaton that already exists -- an Outlines-shaped RegexGuide read by attribute, any guide object enumerated through
get_next_instruction / get_next_state, a transition dictionary, or a set of token sequences (guided choice once tokenised).

A TokenFSM is a DFA in CSR form: states 0 .. S-1, per state its allowed tokens (ascending, distinct, < vocab, never empty) with a
next state each, an `initial` state and a `miss` state that every token not allowed in the current state leads to.  For a
lowered RegexGuide `miss` is its final state -1 renumbered: the only token it allows is eos_token_id, which leads back to it.

GuideArena is the host bookkeeping of the device arena the engine keeps its resident guides in (ops.TokenGuides holds the
tensors): one copy per guide object, reference-counted by the slots that use it, kept by a small LRU after the last release.
"""
from __future__ import annotations

from collections import OrderedDict, deque
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np

MAX_GUIDE_STATES = 65536        # the state cap of a lowered guide (the breadth-first enumeration stops there)
_CACHE_ENTRIES = 64             # lowered guides kept on the identity of their source object


class TokenFSM:
    """row_ptr [S + 1], tokens / next_states [row_ptr[S]] (int32 numpy), initial, miss, vocab.  Validated on construction:
    ValueError on unsorted or repeated tokens, a token outside [0, vocab), a next state outside [0, S), an empty state."""

    def __init__(self, row_ptr, tokens, next_states, initial: int, miss: int, vocab: int, eos_token_id: Optional[int] = None):
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        self.tokens = np.ascontiguousarray(tokens, dtype=np.int64)
        self.next_states = np.ascontiguousarray(next_states, dtype=np.int64)
        self.initial, self.miss, self.vocab = int(initial), int(miss), int(vocab)
        self.eos_token_id = None if eos_token_id is None else int(eos_token_id)
        S = self.row_ptr.shape[0] - 1
        if self.vocab < 1 or S < 1 or S > MAX_GUIDE_STATES:
            raise ValueError(f"a guide needs 1..{MAX_GUIDE_STATES} states and a vocabulary (got {S} states, vocab {self.vocab})")
        n = self.tokens.shape[0]
        if self.row_ptr[0] != 0 or self.row_ptr[-1] != n or self.next_states.shape[0] != n or n >= 2 ** 31:
            raise ValueError("row_ptr does not describe the token and next-state arrays")
        lens = np.diff(self.row_ptr)
        if (lens <= 0).any():
            raise ValueError(f"state {int(np.nonzero(lens <= 0)[0][0])} of the guide allows no token")
        if n and (self.tokens.min() < 0 or self.tokens.max() >= self.vocab):
            raise ValueError(f"a guide token lies outside the vocabulary of {self.vocab}")
        if n and (self.next_states.min() < 0 or self.next_states.max() >= S):
            raise ValueError("a next state lies outside the guide")
        rising = np.diff(self.tokens) > 0
        rising[self.row_ptr[1:-1] - 1] = True          # (the step from one state's last token to the next state's first)
        if not rising.all():
            raise ValueError("the tokens of a guide state must be sorted ascending and distinct")
        if not (0 <= self.initial < S and 0 <= self.miss < S):
            raise ValueError("initial / miss state outside the guide")
        self.row_ptr, self.tokens, self.next_states = (a.astype(np.int32) for a in (self.row_ptr, self.tokens, self.next_states))

    num_states = property(lambda self: self.row_ptr.shape[0] - 1)
    num_transitions = property(lambda self: int(self.tokens.shape[0]))

    # ------------------------------------------------------------------ host walk (admission, tests)
    def allowed(self, state: int) -> np.ndarray:
        return self.tokens[self.row_ptr[state]:self.row_ptr[state + 1]]

    def next(self, state: int, token: int) -> int:
        lo, hi = int(self.row_ptr[state]), int(self.row_ptr[state + 1])
        i = lo + int(np.searchsorted(self.tokens[lo:hi], token))
        return int(self.next_states[i]) if i < hi and int(self.tokens[i]) == int(token) else self.miss

    def advance(self, state: int, tokens: Iterable[int]) -> int:
        for t in tokens:
            state = self.next(state, int(t))
        return state

    def accepts(self, tokens: Sequence[int]) -> bool:
        """Every token of `tokens` (a request's outputs) was allowed in the state it was emitted in."""
        state = self.initial
        for t in tokens:
            if int(t) not in self.allowed(state):
                return False
            state = self.next(state, int(t))
        return True

    # ------------------------------------------------------------------ builders
    @classmethod
    def from_transitions(cls, transitions: Mapping[int, Mapping[int, Optional[int]]], initial: int, eos_token_id: int,
                         vocab: int) -> "TokenFSM":
        """{state: {token: next}} with arbitrary integer state keys, renumbered in ascending key order; the final state comes
        last and is the miss state.  A target that is None, -1 or has no entry of its own is the final state, and so is the
        target of eos_token_id wherever it is allowed (RegexGuide.get_next_state).  Allowed ids >= vocab are dropped (the
        reference's masked_select); a state left without a token is refused."""
        eos, vocab = int(eos_token_id), int(vocab)
        if not 0 <= eos < vocab:
            raise ValueError(f"eos_token_id {eos} outside the vocabulary of {vocab}: the final state would allow nothing")
        keys = sorted(int(s) for s in transitions if int(s) != -1)
        if len(keys) + 1 > MAX_GUIDE_STATES:
            raise ValueError(f"{len(keys) + 1} guide states: at most {MAX_GUIDE_STATES} are supported")
        number = {s: i for i, s in enumerate(keys)}
        final = len(keys)
        row_ptr, toks, nxt = [0], [], []
        for s in keys:
            row = {}
            for t, target in transitions[s].items():
                t = int(t)
                if t < 0:
                    raise ValueError(f"state {s}: negative token id {t}")
                if t >= vocab:
                    continue
                row[t] = final if (t == eos or target is None) else number.get(int(target), final)
            if not row:
                raise ValueError(f"state {s} of the guide allows no token below the vocabulary of {vocab}")
            for t in sorted(row):
                toks.append(t)
                nxt.append(row[t])
            row_ptr.append(len(toks))
        toks.append(eos); nxt.append(final); row_ptr.append(len(toks))
        return cls(row_ptr, toks, nxt, number.get(int(initial), final), final, vocab, eos)

    @classmethod
    def from_token_sequences(cls, choices: Sequence[Sequence[int]], eos_token_id: int, vocab: int) -> "TokenFSM":
        """The trie of `choices` (guided choice once tokenised): a choice may end -- eos_token_id -- where it is complete."""
        trans: Dict[int, Dict[int, int]] = {0: {}}
        if not choices or any(len(c) == 0 for c in choices):
            raise ValueError("guided choice needs at least one choice and no empty one")
        for c in choices:
            node = 0
            for t in c:
                t = int(t)
                if t == int(eos_token_id):
                    raise ValueError("a choice contains eos_token_id")
                if t not in trans[node]:
                    trans[node][t] = len(trans)
                    trans[len(trans)] = {}
                node = trans[node][t]
            trans[node][int(eos_token_id)] = -1
        return cls.from_transitions(trans, 0, eos_token_id, vocab)

    _cache: "OrderedDict[int, Tuple[object, int, TokenFSM]]" = OrderedDict()

    @classmethod
    def from_guide(cls, guide, vocab: int) -> "TokenFSM":
        """Lower a guide object, cached on its identity (the object is kept alive while cached).  An Outlines-shaped RegexGuide
        is read by attribute (states_to_token_maps, initial_state, eos_token_id); any other object with
        get_next_instruction(state).tokens / get_next_state(state, token) over int states is enumerated breadth-first from its
        initial_state (default 0) up to the state cap; its state -1 is the final state, a `Write` instruction contributes its
        first token only (outlines_logits_processors.py:73-75).  TypeError: not a finite automaton over int states."""
        if isinstance(guide, TokenFSM):
            return guide
        hit = cls._cache.get(id(guide))
        if hit is not None and hit[0] is guide and hit[1] == int(vocab):
            cls._cache.move_to_end(id(guide))
            return hit[2]
        maps = getattr(guide, "states_to_token_maps", None)
        if isinstance(maps, Mapping) and hasattr(guide, "eos_token_id"):
            fsm = cls.from_transitions(maps, getattr(guide, "initial_state", 0), guide.eos_token_id, vocab)
        elif callable(getattr(guide, "get_next_instruction", None)) and callable(getattr(guide, "get_next_state", None)):
            fsm = cls._enumerate(guide, vocab)
        else:
            raise TypeError(f"{type(guide).__name__} is not a finite automaton over int states")
        cls._cache[id(guide)] = (guide, int(vocab), fsm)
        while len(cls._cache) > _CACHE_ENTRIES:
            cls._cache.popitem(last=False)
        return fsm

    @classmethod
    def _enumerate(cls, guide, vocab: int) -> "TokenFSM":
        def is_state(s):
            return isinstance(s, (int, np.integer)) and not isinstance(s, bool)

        def tokens_of(state):
            ins = guide.get_next_instruction(state)
            toks = getattr(ins, "tokens", None)
            if toks is None:
                raise TypeError(f"{type(guide).__name__}: an instruction without tokens")
            toks = [int(t) for t in toks]
            return toks[:1] if type(ins).__name__ == "Write" else toks
        initial = getattr(guide, "initial_state", 0)
        if not is_state(initial):
            raise TypeError(f"{type(guide).__name__} is not a finite automaton over int states")
        last = tokens_of(-1)
        if len(last) != 1:
            raise TypeError(f"{type(guide).__name__}: the final state must write one token (eos)")
        trans: Dict[int, Dict[int, int]] = {}
        queue = deque([int(initial)])
        while queue:
            s = queue.popleft()
            if s == -1 or s in trans:
                continue
            if len(trans) + 1 >= MAX_GUIDE_STATES:
                raise ValueError(f"the guide has more than {MAX_GUIDE_STATES} states")
            row = trans[s] = {}
            for t in tokens_of(s):
                if t >= vocab:
                    continue
                n = guide.get_next_state(s, t)
                if not is_state(n):
                    raise TypeError(f"{type(guide).__name__} is not a finite automaton over int states")
                row[t] = int(n)
                queue.append(int(n))
        return cls.from_transitions(trans, int(initial), last[0], vocab)

    # ------------------------------------------------------------------ the device layout, in numpy (tests, documentation)
    def tables(self, words: Optional[int] = None):
        """(allow [S, words] uint32, rank [S, words] int32, off [S] int32, nxt int32): what qspec_guide_build writes for this
        guide at state_base = transition_base = 0."""
        S = self.num_states
        words = guide_words(self.vocab) if words is None else int(words)
        bits = np.zeros((S, words * 32), dtype=np.uint8)
        state_of = np.repeat(np.arange(S), np.diff(self.row_ptr))
        bits[state_of, self.tokens] = 1
        weights = (np.uint32(1) << np.arange(32, dtype=np.uint32))
        allow = (bits.reshape(S, words, 32).astype(np.uint32) * weights).sum(axis=2, dtype=np.uint64).astype(np.uint32)
        counts = bits.reshape(S, words, 32).sum(axis=2, dtype=np.int64)
        rank = (np.cumsum(counts, axis=1) - counts).astype(np.int32)
        return allow, rank, self.row_ptr[:-1].astype(np.int32), self.next_states.astype(np.int32)


def guide_words(vocab: int) -> int:
    """Words of an allow / rank row: ceil(vocab / 32) rounded up to a multiple of 4 (16-byte stores)."""
    return ((int(vocab) + 31) // 32 + 3) // 4 * 4


def table_next(allow, rank, off, nxt, state: int, token: int, miss: int) -> int:
    """next(state, token) from the device layout: the arithmetic of the kernels' walk, in numpy."""
    word = int(allow[state, token >> 5])
    bit = 1 << (token & 31)
    if not word & bit:
        return miss
    return int(nxt[int(off[state]) + int(rank[state, token >> 5]) + bin(word & (bit - 1)).count("1")])


class _Resident:
    __slots__ = ("fsm", "state_base", "trans_base", "refs", "tick")

    def __init__(self, fsm, state_base, trans_base, tick):
        self.fsm, self.state_base, self.trans_base, self.refs, self.tick = fsm, state_base, trans_base, 0, tick


class GuideArena:
    """Where the resident guides sit in the device arena: contiguous state rows and transitions per guide, first fit.  A guide
    is identified by object identity (a strong reference is held while it is resident), shared by the slots that use it
    (acquire / release count them) and stays resident after its last release until the space is needed or more than `keep`
    unreferenced guides are resident (least recently used first)."""

    def __init__(self, max_states: int, max_transitions: int, keep: int = 8):
        if max_states < 1 or max_transitions < 1:
            raise ValueError("the guide arena needs room for at least one state and one transition")
        self.max_states, self.max_transitions, self.keep = int(max_states), int(max_transitions), int(keep)
        self._res: Dict[int, _Resident] = {}
        self._tick = 0

    def resident(self, fsm) -> Optional[_Resident]:
        r = self._res.get(id(fsm))
        return r if r is not None and r.fsm is fsm else None

    @staticmethod
    def _fit(segments: List[Tuple[int, int]], size: int, cap: int) -> Optional[int]:
        pos = 0
        for base, n in sorted(segments):
            if base - pos >= size:
                return pos
            pos = base + n
        return pos if cap - pos >= size else None

    def plan(self, fsm: TokenFSM):
        """(guides to evict, state_base, trans_base) for a guide that is not resident; ValueError when it cannot fit even with
        every unreferenced guide gone.  No side effect."""
        S, N = fsm.num_states, fsm.num_transitions
        if S > self.max_states or N > self.max_transitions:
            raise ValueError(f"the guide has {S} states and {N} transitions: the arena holds {self.max_states} states and "
                             f"{self.max_transitions} transitions (the engine's guide_states / guide_transitions)")
        idle = sorted((r for r in self._res.values() if r.refs == 0), key=lambda r: r.tick)
        for n_out in range(len(idle) + 1):
            gone = set(id(r.fsm) for r in idle[:n_out])
            left = [r for k, r in self._res.items() if k not in gone]
            sb = self._fit([(r.state_base, r.fsm.num_states) for r in left], S, self.max_states)
            tb = self._fit([(r.trans_base, r.fsm.num_transitions) for r in left], N, self.max_transitions)
            if sb is not None and tb is not None:
                return idle[:n_out], sb, tb
        raise ValueError(f"no room for a guide of {S} states and {N} transitions beside the guides in use (the arena holds "
                         f"{self.max_states} states and {self.max_transitions} transitions)")

    def acquire(self, fsm: TokenFSM):
        """-> (resident entry, fresh): fresh = the caller must build the guide's rows at the entry's bases."""
        self._tick += 1
        r = self.resident(fsm)
        fresh = r is None
        if fresh:
            evict, sb, tb = self.plan(fsm)
            for e in evict:
                del self._res[id(e.fsm)]
            r = self._res[id(fsm)] = _Resident(fsm, sb, tb, self._tick)
        r.refs += 1
        r.tick = self._tick
        return r, fresh

    def release(self, fsm: TokenFSM) -> None:
        r = self.resident(fsm)
        if r is None or r.refs < 1:
            raise ValueError("release of a guide that is not in use")
        self._tick += 1
        r.refs -= 1
        r.tick = self._tick
        idle = sorted((x for x in self._res.values() if x.refs == 0), key=lambda x: x.tick)
        for x in idle[:max(0, len(idle) - self.keep)]:
            del self._res[id(x.fsm)]
