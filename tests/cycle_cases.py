"""Host references and case builders for the spec-decode cycle glue (include/qspec_hip.h, "spec-decode cycle glue"):
prepare_draft, advance_draft, prepare_verify, commit, snapshot / restore and collect_error_words.

Written from the header's contract, one row at a time with Python integers; numpy only carries the arrays.  No torch and
no GPU: tests/test_cycle_glue_cpu.py checks these functions against a list-and-dict model of the sequences, and
tests/test_cycle_glue_gpu.py checks the kernels against these functions."""
import numpy as np

I32_MIN = -2 ** 31
SEQ_SLOTS = 64     # slots of one sequence's block table in every case: max_blocks * block_size


# ------------------------------------------------------------------ references

def slot_of(bt_row, pos, block_size):
    """Cache slot of position `pos` of a sequence with block-table row `bt_row`; -1 beyond the row (or for pos < 0)."""
    if pos < 0:
        return -1
    blk = pos // block_size
    if blk >= len(bt_row):
        return -1
    return int(bt_row[blk]) * block_size + pos - blk * block_size


def prepare_draft(last_token, seq_lens, block_tables, block_size, step_mask=None):
    """token = last_token, position = L - 1, ctx_len = L, slot from the block table; L <= 0: token 0, position 0, ctx 1,
    slot -1.  step_mask: L = seq_lens * step_mask, returned as eff_lens."""
    B = len(seq_lens)
    tokens, positions, slots = (np.zeros(B, np.int64) for _ in range(3))
    ctx = np.zeros(B, np.int32)
    eff = None if step_mask is None else np.zeros(B, np.int32)
    for b in range(B):
        L = int(seq_lens[b])
        if step_mask is not None:
            L = L * int(step_mask[b])
            eff[b] = L
        if L <= 0:
            tokens[b], positions[b], ctx[b], slots[b] = 0, 0, 1, -1
            continue
        tokens[b] = int(last_token[b])
        positions[b] = L - 1
        ctx[b] = L
        slots[b] = slot_of(block_tables[b], L - 1, block_size)
    return dict(tokens=tokens, positions=positions, slots=slots, ctx_lens=ctx, eff_lens=eff)


def advance_draft(tokens, positions, ctx_lens, slots, sampled, block_tables, block_size):
    """Between two draft steps: the sampled token becomes the input at the next position.  A row whose slot is -1 stays as it
    is; a row whose next position lies beyond its block table freezes: slot -1, token updated, position and ctx kept."""
    tokens, positions, ctx_lens, slots = (np.array(x, copy=True) for x in (tokens, positions, ctx_lens, slots))
    for b in range(len(ctx_lens)):
        if int(slots[b]) < 0:
            continue
        tokens[b] = int(sampled[b])
        pos = int(ctx_lens[b])                 # the position after the ctx_lens known ones
        s = slot_of(block_tables[b], pos, block_size)
        if s < 0:
            slots[b] = -1
            continue
        positions[b], ctx_lens[b], slots[b] = pos, pos + 1, s
    return dict(tokens=tokens, positions=positions, slots=slots, ctx_lens=ctx_lens)


def prepare_verify(last_token, draft_ids, seq_lens, block_tables, block_size):
    """Per sequence the k + 1 queries [last_token, d_1 .. d_k] at positions L-1 .. L-1+k, ctx_len L + k; an empty slot:
    tokens 0, positions j, slots -1, ctx k + 1.  draft_ids [B, k]."""
    B, k = np.shape(draft_ids)
    n = B * (k + 1)
    tokens, positions, slots = (np.zeros(n, np.int64) for _ in range(3))
    ctx = np.zeros(B, np.int32)
    for b in range(B):
        L = int(seq_lens[b])
        for j in range(k + 1):
            r = b * (k + 1) + j
            if L <= 0:
                tokens[r], positions[r], slots[r] = 0, j, -1
            else:
                tokens[r] = int(last_token[b]) if j == 0 else int(draft_ids[b][j - 1])
                positions[r] = L - 1 + j
                slots[r] = slot_of(block_tables[b], L - 1 + j, block_size)
        ctx[b] = k + 1 if L <= 0 else L + k
    return dict(tokens=tokens, positions=positions, slots=slots, ctx_lens=ctx)


def commit(out_tokens, seq_lens, last_token, gen_tokens=None, gen_lens=None):
    """Append the emitted prefix of out_tokens[b] (everything before the first -1) to gen_tokens[b], advance seq_lens and
    gen_lens by its length n, last_token = its last element.  Capacity (gen_tokens.shape[1]): a token whose index
    gen_lens + i is at or beyond it is dropped, while gen_lens, seq_lens and last_token still advance over all n tokens --
    gen_lens counts the emitted tokens, not the stored ones."""
    seq_lens, last_token = np.array(seq_lens, copy=True), np.array(last_token, copy=True)
    gen_tokens = None if gen_tokens is None else np.array(gen_tokens, copy=True)
    gen_lens = None if gen_lens is None else np.array(gen_lens, copy=True)
    for b in range(len(seq_lens)):
        emitted = []
        for t in out_tokens[b]:
            if int(t) == -1:
                break
            emitted.append(int(t))
        if not emitted:
            continue
        if gen_tokens is not None:
            for i, t in enumerate(emitted):
                at = int(gen_lens[b]) + i
                if at < gen_tokens.shape[1]:
                    gen_tokens[b, at] = t
        if gen_lens is not None:
            gen_lens[b] += len(emitted)
        seq_lens[b] += len(emitted)
        last_token[b] = emitted[-1]
    return dict(seq_lens=seq_lens, last_token=last_token, gen_tokens=gen_tokens, gen_lens=gen_lens)


def snapshot(seq_lens, gen_lens, last_token, counters, rng_state):
    """snap_i32 [2B] = seq_lens | gen_lens; snap_i64 [B + 5] = last_token | counters [3] | rng_state [2]."""
    snap_i32 = [int(x) for x in seq_lens] + [int(x) for x in gen_lens]
    snap_i64 = [int(x) for x in last_token] + [int(x) for x in counters] + [int(x) for x in rng_state]
    assert len(counters) == 3 and len(rng_state) == 2
    return np.array(snap_i32, np.int32), np.array(snap_i64, np.int64)


def restore(snap_i32, snap_i64, B):
    """The inverse of snapshot: (seq_lens, gen_lens, last_token, counters, rng_state)."""
    return (np.array(snap_i32[:B], np.int32), np.array(snap_i32[B:2 * B], np.int32), np.array(snap_i64[:B], np.int64),
            np.array(snap_i64[B:B + 3], np.int64), np.array(snap_i64[B + 3:B + 5], np.int64))


def collect_error_words(words, clear):
    """words: up to four Python ints (int32 values) or None.  Returns (OR of |w|, the words afterwards)."""
    acc = 0
    after = []
    for w in words:
        if w is None:
            after.append(None)
            continue
        assert I32_MIN < w < 2 ** 31
        acc |= abs(int(w))
        after.append(0 if clear else int(w))
    return acc, after


# ------------------------------------------------------------------ cases

def row_pattern(block_size, k, cap=SEQ_SLOTS):
    """(L, step_mask) of the rows every batch must hold.  Position L - 1 of a live row: the first slot (L = 1), a block's
    last slot (L = bs), the next block's first (L = bs + 1), the last length whose whole cycle fits (cap - k), rows whose
    draft or verify positions run past the table (cap - 1, cap), empty rows (0 and a negative length), masked rows."""
    bs = block_size
    rows = [(1, 1), (bs, 1), (bs + 1, 1), (cap - k, 1), (cap - 1, 1), (cap, 1), (0, 1), (-3, 1), (bs + 5, 0), (cap - 1, 0),
            (0, 0), (2 * bs, 1), (cap - k + 1, 1), (cap // 2 + 3, 1)]
    return [(L, m) for L, m in rows]


def rotations(B, block_size, k):
    """The `rotate` values at which batches of B rows together hold every row of row_pattern."""
    n = len(row_pattern(block_size, k))
    return [0] if B >= n else list(range(0, n, B))


def build_batch(block_size, k, B, vocab=500, seed=0, rotate=0):
    """One batch: row b takes row_pattern[(b + rotate) % n] while b < n, then random lengths in [-1, cap] with one row in
    eight masked; block tables are a random permutation of B * max_blocks blocks, so no two rows share a block."""
    assert SEQ_SLOTS % block_size == 0
    max_blocks = SEQ_SLOTS // block_size
    rng = np.random.default_rng([seed, block_size, k, B, rotate])
    pat = row_pattern(block_size, k)
    seq_lens, mask = np.zeros(B, np.int32), np.ones(B, np.int32)
    for b in range(B):
        if b < len(pat):
            seq_lens[b], mask[b] = pat[(b + rotate) % len(pat)]
        else:
            seq_lens[b] = int(rng.integers(-1, SEQ_SLOTS + 1))
            mask[b] = int(rng.integers(0, 8) != 0)
    return dict(B=B, k=k, block_size=block_size, max_blocks=max_blocks, vocab=vocab,
                seq_lens=seq_lens, step_mask=mask,
                last_token=rng.integers(0, vocab, B).astype(np.int64),
                block_tables=rng.permutation(B * max_blocks).reshape(B, max_blocks).astype(np.int32))


def row_classes(case):
    """Which rows of a batch fall into each class the tests rely on (by (effective) length alone)."""
    bs, k, cap = case["block_size"], case["k"], case["max_blocks"] * case["block_size"]
    out = {c: [] for c in ("empty", "masked", "frozen_mid_draft", "block_last_slot", "crosses_block", "verify_past_table")}
    for b in range(case["B"]):
        L, m = int(case["seq_lens"][b]), int(case["step_mask"][b])
        if m == 0:
            out["masked"].append(b)
        if L <= 0:
            out["empty"].append(b)
        if L * m <= 0:
            continue
        pos = L - 1
        if pos % bs == bs - 1:
            out["block_last_slot"].append(b)
        if pos // bs != (pos + k) // bs and pos + k < cap:
            out["crosses_block"].append(b)          # its draft / verify positions enter the next block of the table
        if pos < cap and pos + (k - 1) >= cap:
            out["frozen_mid_draft"].append(b)       # one of the k - 1 advances leaves the table
        if pos + k >= cap:
            out["verify_past_table"].append(b)
    return out


def cycle_start_lens(block_size, k, B, seed=0, cap=SEQ_SLOTS):
    """Lengths for a multi-cycle run: most rows within a few cycles of the end of their block tables (a cycle emits 1 .. k + 1
    tokens and needs positions up to L - 1 + k < cap), some at a block edge, some empty, one already at the end."""
    rng = np.random.default_rng([seed, block_size, k, B, 99])
    lens = np.zeros(B, np.int32)
    for b in range(B):
        kind = b % 8
        if kind == 0:
            lens[b] = 0
        elif kind == 1:
            lens[b] = block_size - 1 + int(rng.integers(0, 3))
        elif kind == 2:
            lens[b] = cap - k                      # exactly one more cycle fits
        elif kind == 3:
            lens[b] = cap - k + 1                  # refused at once
        else:
            lens[b] = cap - int(rng.integers(k + 1, 5 * (k + 1)))
    return lens
