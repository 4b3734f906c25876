"""The cycle glue kernels of csrc/sampler.hip (spec_prepare_draft / spec_advance_draft / spec_prepare_verify, their `_embed`
forms, spec_commit, spec_snapshot / restore, collect_error_words) against the host references of tests/cycle_cases.py:
exact equality on every output array, output buffers pre-filled with a sentinel so that an unwritten element shows."""
import itertools

import numpy as np
import pytest
import torch

import cycle_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77            # what every output buffer holds before a launch
V, H = 500, 256
BLOCK_SIZES = (8, 16, 32)
KS = (1, 3, 7)
BATCHES = (1, 6, 64, 65, 130)      # 65 / 130: the second and third workgroup of the plain kernels, the last one partial


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from qspec_amd import ops
    return ops


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(2026)
    t = rng.standard_normal((V, H)).astype(np.float16)
    return t, dev(t)


def _bufs(n, B):
    """tokens, positions, slots [n] int64 and ctx_lens [B] int32, sentinel-filled."""
    return [torch.full((n,), SENT, dtype=torch.int64, device=DEV) for _ in range(3)] + \
           [torch.full((B,), SENT, dtype=torch.int32, device=DEV)]


def _same(got, want, what):
    got, want = host(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, f"{what}: first mismatch at {bad[0]}: got {got.ravel()[bad[0]]}, want {want.ravel()[bad[0]]}"


def _same_index_tensors(got, ref, what):
    for t, name in zip(got, ("tokens", "positions", "slots", "ctx_lens")):
        _same(t, ref[name], f"{what}.{name}")


def _hidden_of(table_np, tokens):
    """nn.Embedding with the padded-row rule: a token outside [0, V) takes row 0."""
    rows = [int(t) if 0 <= int(t) < table_np.shape[0] else 0 for t in tokens]
    return table_np[rows]


def _same_hidden(hidden, table_np, tokens, what):
    got, want = host(hidden).view(np.uint16), _hidden_of(table_np, tokens).view(np.uint16)
    assert np.array_equal(got, want), f"{what}: hidden rows {np.flatnonzero((got != want).any(1))[:8]} differ from table[token]"


def _odd_tokens(rng, n):
    """Sampled tokens with some outside [0, V): negative, V itself, just beyond, far beyond int32."""
    t = rng.integers(0, V, n).astype(np.int64)
    odd = np.array([-1, V, V + 3, -2 ** 40, 2 ** 40 + 1, -V], np.int64)
    idx = rng.permutation(n)[:max(1, n // 3)]
    t[idx] = odd[np.arange(idx.size) % odd.size]
    return t


# ------------------------------------------------------------------ prepare_draft / advance_draft / prepare_verify

@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_plain_kernels_equal_the_reference(ops, bs, k, B):
    for rotate in cc.rotations(B, bs, k):
        case = cc.build_batch(bs, k, B, vocab=V, rotate=rotate)
        rng = np.random.default_rng([21, bs, k, B, rotate])
        bt_np, lens_np, last_np = case["block_tables"], case["seq_lens"], case["last_token"]
        bt, lens, last = dev(bt_np), dev(lens_np), dev(last_np)
        t, p, s, c = _bufs(B, B)
        ops.spec_prepare_draft(last, lens, bt, bs, t, p, s, c)
        ref = cc.prepare_draft(last_np, lens_np, bt_np, bs)
        _same_index_tensors((t, p, s, c), ref, "prepare_draft")
        # more advances than a cycle makes: rows at the end of their table freeze, and stay frozen
        for step in range(k + 1):
            sampled = rng.integers(0, V, B).astype(np.int64)
            ops.spec_advance_draft(bs, t, dev(sampled), p, c, s, bt)
            ref = cc.advance_draft(ref["tokens"], ref["positions"], ref["ctx_lens"], ref["slots"], sampled, bt_np, bs)
            _same_index_tensors((t, p, s, c), ref, f"advance_draft step {step}")
        # draft ids: a contiguous [B, k] tensor, and the transposed view of a step-major [k, B] buffer (the engine's)
        ids_np = rng.integers(0, V, (B, k)).astype(np.int64)
        ref = cc.prepare_verify(last_np, ids_np, lens_np, bt_np, bs)
        for layout, ids in (("[B, k]", dev(ids_np)), ("[k, B]^T", dev(ids_np.T.copy()).transpose(0, 1))):
            assert ids.shape == (B, k)
            t, p, s, c = _bufs(B * (k + 1), B)
            ops.spec_prepare_verify(last, ids, lens, bt, bs, t, p, s, c)
            _same_index_tensors((t, p, s, c), ref, f"prepare_verify {layout}")
        _same(lens, lens_np, "seq_lens (input)")
        _same(last, last_np, "last_token (input)")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_embed_kernels_equal_the_reference(ops, table, bs, k, B):
    table_np, table_d = table
    for rotate in cc.rotations(B, bs, k):
        case = cc.build_batch(bs, k, B, vocab=V, rotate=rotate)
        rng = np.random.default_rng([22, bs, k, B, rotate])
        bt_np, lens_np, last_np, mask_np = case["block_tables"], case["seq_lens"], case["last_token"], case["step_mask"]
        bt, lens, last, mask = dev(bt_np), dev(lens_np), dev(last_np), dev(mask_np)
        t, p, s, c = _bufs(B, B)
        eff = torch.full((B,), SENT, dtype=torch.int32, device=DEV)
        hid = torch.full((B, H), 3.0, dtype=torch.float16, device=DEV)
        ops.spec_prepare_draft(last, lens, bt, bs, t, p, s, c, embed=(table_d, hid), step_mask=mask, eff_lens=eff)
        ref = cc.prepare_draft(last_np, lens_np, bt_np, bs, step_mask=mask_np)
        _same_index_tensors((t, p, s, c), ref, "prepare_draft_embed")
        _same(eff, ref["eff_lens"], "eff_lens")
        _same_hidden(hid, table_np, ref["tokens"], "prepare_draft_embed")
        eff_np = ref["eff_lens"]
        # without a step mask eff_lens is not written and seq_lens are the lengths
        t2, p2, s2, c2 = _bufs(B, B)
        hid2 = torch.full((B, H), 3.0, dtype=torch.float16, device=DEV)
        ops.spec_prepare_draft(last, lens, bt, bs, t2, p2, s2, c2, embed=(table_d, hid2))
        ref2 = cc.prepare_draft(last_np, lens_np, bt_np, bs)
        _same_index_tensors((t2, p2, s2, c2), ref2, "prepare_draft_embed without a mask")
        _same_hidden(hid2, table_np, ref2["tokens"], "prepare_draft_embed without a mask")
        for step in range(k + 1):
            sampled = _odd_tokens(rng, B)
            hid.fill_(3.0)
            ops.spec_advance_draft(bs, t, dev(sampled), p, c, s, bt, embed=(table_d, hid))
            ref = cc.advance_draft(ref["tokens"], ref["positions"], ref["ctx_lens"], ref["slots"], sampled, bt_np, bs)
            _same_index_tensors((t, p, s, c), ref, f"advance_draft_embed step {step}")
            _same_hidden(hid, table_np, ref["tokens"], f"advance_draft_embed step {step}")
        ids_np = _odd_tokens(rng, B * k).reshape(B, k)
        ref = cc.prepare_verify(last_np, ids_np, eff_np, bt_np, bs)
        for layout, ids in (("[B, k]", dev(ids_np)), ("[k, B]^T", dev(ids_np.T.copy()).transpose(0, 1))):
            n = B * (k + 1)
            t, p, s, c = _bufs(n, B)
            hid = torch.full((n, H), 3.0, dtype=torch.float16, device=DEV)
            ops.spec_prepare_verify(last, ids, eff, bt, bs, t, p, s, c, embed=(table_d, hid))
            _same_index_tensors((t, p, s, c), ref, f"prepare_verify_embed {layout}")
            _same_hidden(hid, table_np, ref["tokens"], f"prepare_verify_embed {layout}")
        _same(lens, lens_np, "seq_lens (input)")


# ------------------------------------------------------------------ commit

def _commit_case(k, B, cap, seed):
    """Rows emitting 0 .. k + 1 tokens (row b: b % (k + 2)), every third with values behind the first -1; gen_lens from an
    empty row to rows at capacity - 1, at capacity and beyond, so that part of (or all) their tokens do not fit."""
    rng = np.random.default_rng([23, k, B, seed])
    out = np.full((B, k + 1), -1, np.int64)
    for b in range(B):
        n = b % (k + 2)
        out[b, :n] = rng.integers(0, V, n)
        if b % 3 == 0 and n + 1 <= k:
            out[b, n + 1:] = rng.integers(0, V, k - n)
    gen_lens = rng.integers(0, cap - k - 1, B).astype(np.int32)
    edge = [cap - 1, cap - 2, cap, cap + 3, cap - k - 1, cap - k, 0]
    for i, b in enumerate(rng.permutation(B)[:min(B, 5 * len(edge))]):
        gen_lens[b] = edge[i % len(edge)]
    if B >= 3 * (k + 2):
        gen_lens[k + 1] = cap - 1              # emits k + 1 tokens: only the first fits
        gen_lens[k + 2 + 1] = cap - 1          # emits one token: it just fits
        gen_lens[2 * (k + 2) + k + 1] = cap    # emits k + 1 tokens: none fits
    return out, rng.integers(1, 60, B).astype(np.int32), rng.integers(0, V, B).astype(np.int64), gen_lens


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B", [1, 130])
def test_commit_equals_the_reference(ops, k, B):
    cap, pad = 24, 3
    for seed in range(k + 2 if B == 1 else 1):      # (B = 1: one row per emitted count)
        out_np, lens_np, last_np, gl_np = _commit_case(k, B, cap, seed)
        if B == 1:
            out_np[0] = -1
            out_np[0, :seed] = np.arange(seed) + 5
            gl_np[0] = cap - 1
        # gen_tokens sits in the middle of a larger buffer: the rows before and after it stay as they are
        big = torch.full((B + 2 * pad, cap), SENT, dtype=torch.int64, device=DEV)
        gen = big[pad:pad + B]
        assert gen.is_contiguous()
        lens, last, gl = dev(lens_np), dev(last_np), dev(gl_np)
        ops.spec_commit(dev(out_np), lens, last, gen, gl)
        ref = cc.commit(out_np, lens_np, last_np, np.full((B, cap), SENT, np.int64), gl_np)
        _same(gen, ref["gen_tokens"], "gen_tokens")
        _same(gl, ref["gen_lens"], "gen_lens")
        _same(lens, ref["seq_lens"], "seq_lens")
        _same(last, ref["last_token"], "last_token")
        assert (host(big[:pad]) == SENT).all() and (host(big[pad + B:]) == SENT).all()
        if B > 1:
            emitted = (ref["seq_lens"] - lens_np)
            assert set(emitted.tolist()) == set(range(k + 2))                     # 0 .. k + 1 tokens
            assert ((gl_np < cap) & (gl_np + emitted > cap)).any()                # a row only part of whose tokens fit
        # without gen_tokens: lengths and last_token alone (gen_lens still counts), and without either
        lens, last, gl = dev(lens_np), dev(last_np), dev(gl_np)
        ops.spec_commit(dev(out_np), lens, last, None, gl)
        ref = cc.commit(out_np, lens_np, last_np, None, gl_np)
        for got, name in ((lens, "seq_lens"), (last, "last_token"), (gl, "gen_lens")):
            _same(got, ref[name], name + " (gen_tokens=None)")
        lens, last = dev(lens_np), dev(last_np)
        ops.spec_commit(dev(out_np), lens, last)
        _same(lens, ref["seq_lens"], "seq_lens (no gen state)")
        _same(last, ref["last_token"], "last_token (no gen state)")


# ------------------------------------------------------------------ snapshot / restore

@pytest.mark.parametrize("B", [1, 2, 3, 65])
def test_snapshot_layout_and_restore(ops, B):
    rng = np.random.default_rng([24, B])
    state_np = [rng.integers(-5, 2 ** 31 - 1, B).astype(np.int32), rng.integers(0, 2 ** 31 - 1, B).astype(np.int32),
                rng.integers(-2 ** 62, 2 ** 62, B).astype(np.int64), rng.integers(0, 2 ** 62, 3).astype(np.int64),
                rng.integers(-2 ** 63, 2 ** 63 - 1, 2).astype(np.int64)]
    names = ("seq_lens", "gen_lens", "last_token", "counters", "rng_state")
    state = [dev(x) for x in state_np]
    extra = 4
    snap_i32 = torch.full((2 * B + extra,), SENT, dtype=torch.int32, device=DEV)
    snap_i64 = torch.full((B + 5 + extra,), SENT, dtype=torch.int64, device=DEV)
    ops.spec_snapshot(*state, snap_i32, snap_i64)
    want_i32, want_i64 = cc.snapshot(*state_np)
    _same(snap_i32, np.concatenate([want_i32, np.full(extra, SENT, np.int32)]), "snap_i32")
    _same(snap_i64, np.concatenate([want_i64, np.full(extra, SENT, np.int64)]), "snap_i64")
    for t, x, name in zip(state, state_np, names):
        _same(t, x, name + " after the snapshot")
    for t in state:                                   # a cycle went wrong: everything differs
        t.copy_(torch.full_like(t, 99))
    ops.spec_snapshot(*state, snap_i32, snap_i64, restore=True)
    for t, x, name in zip(state, cc.restore(want_i32, want_i64, B), names):
        _same(t, x, name + " restored")
    _same(snap_i32[:2 * B], want_i32, "snap_i32 after the restore")
    _same(snap_i64[:B + 5], want_i64, "snap_i64 after the restore")
    assert (host(snap_i32[2 * B:]) == SENT).all() and (host(snap_i64[B + 5:]) == SENT).all()


# ------------------------------------------------------------------ collect_error_words

WORDS = [0, 6, -9, cc.I32_MIN + 1]


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("picked", [(), (1,), (2,), (0,), (3,), (0, 1, 2, 3), (2, 1, 0, 0)])
def test_collect_error_words(ops, picked, clear):
    words = dev(np.array(WORDS + [SENT], np.int32))
    out = torch.full((2,), SENT, dtype=torch.int64, device=DEV)
    ops.collect_error_words([words[i:i + 1].data_ptr() for i in picked], out, clear=clear)
    acc, _ = cc.collect_error_words([WORDS[i] for i in picked], clear)
    after = list(WORDS)
    if clear:
        for i in picked:
            after[i] = 0
    assert host(out).tolist() == [acc, SENT]
    assert host(words).tolist() == after + [SENT]
    if clear:                                         # the clearing form the engine uses between cycles: no output word
        words = dev(np.array(WORDS + [SENT], np.int32))
        ops.collect_error_words([words[i:i + 1].data_ptr() for i in picked], None, clear=True)
        assert host(words).tolist() == after + [SENT]


# ------------------------------------------------------------------ several cycles

@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_six_cycles_follow_the_reference(ops, table, bs):
    """prepare_draft(embed, step_mask), k - 1 advance_draft, prepare_verify, commit -- six times over, sequences starting
    near the ends of their block tables; the host refuses (finishes) a sequence whose next cycle would leave its table, as
    the engine does.  Every launch is compared with the reference; over the run every slot written for a live row is one
    of the row's own and no two rows ever share one."""
    table_np, table_d = table
    B, k, cycles, cap = 40, 3, 6, cc.SEQ_SLOTS
    gcap = cycles * (k + 1) + k + 1
    case = cc.build_batch(bs, k, B, vocab=V, seed=11)
    rng = np.random.default_rng([25, bs])
    bt_np = case["block_tables"]
    own = [{int(blk) * bs + o for blk in bt_np[b] for o in range(bs)} for b in range(B)]
    st = dict(seq_lens=cc.cycle_start_lens(bs, k, B, seed=11), last_token=rng.integers(0, V, B).astype(np.int64),
              gen_tokens=np.full((B, gcap), -1, np.int64), gen_lens=np.zeros(B, np.int32))
    bt = dev(bt_np)
    d_st = {n: dev(x) for n, x in st.items()}
    ids_kb = torch.zeros((k, B), dtype=torch.int64, device=DEV)       # step-major, as the draft loop writes them
    written = [set() for _ in range(B)]
    finished = stepped = 0

    def same_state(what):
        for n in st:
            _same(d_st[n], st[n], f"{what}: {n}")

    def note(slots, live, rows_per_seq):
        for b in live:
            for s in slots[b * rows_per_seq:(b + 1) * rows_per_seq]:
                assert s >= 0                          # the host refused every step that would leave the table
                written[b].add(int(s))

    for cycle in range(cycles):
        for b in range(B):
            if st["seq_lens"][b] > 0 and st["seq_lens"][b] - 1 + k >= cap:
                st["seq_lens"][b] = 0
                finished += 1
        d_st["seq_lens"].copy_(dev(st["seq_lens"]))
        mask_np = (rng.integers(0, 5, B) != 0).astype(np.int32)
        live = [b for b in range(B) if st["seq_lens"][b] > 0 and mask_np[b]]
        draft = rng.integers(0, V, (B, k)).astype(np.int64)
        t, p, s, c = _bufs(B, B)
        eff = torch.full((B,), SENT, dtype=torch.int32, device=DEV)
        hid = torch.full((B, H), 3.0, dtype=torch.float16, device=DEV)
        ops.spec_prepare_draft(d_st["last_token"], d_st["seq_lens"], bt, bs, t, p, s, c, embed=(table_d, hid),
                               step_mask=dev(mask_np), eff_lens=eff)
        ref = cc.prepare_draft(st["last_token"], st["seq_lens"], bt_np, bs, step_mask=mask_np)
        eff_np = ref["eff_lens"]
        _same_index_tensors((t, p, s, c), ref, f"cycle {cycle} prepare_draft")
        _same(eff, eff_np, f"cycle {cycle} eff_lens")
        _same_hidden(hid, table_np, ref["tokens"], f"cycle {cycle} prepare_draft")
        same_state(f"cycle {cycle} prepare_draft")
        note(ref["slots"], live, 1)
        for i in range(k - 1):
            ids_kb[i].copy_(dev(draft[:, i]))
            embed = (table_d, hid) if (cycle + i) % 2 == 0 else None
            hid.fill_(3.0)
            ops.spec_advance_draft(bs, t, ids_kb[i], p, c, s, bt, embed=embed)
            ref = cc.advance_draft(ref["tokens"], ref["positions"], ref["ctx_lens"], ref["slots"], draft[:, i], bt_np, bs)
            _same_index_tensors((t, p, s, c), ref, f"cycle {cycle} advance_draft {i}")
            if embed:
                _same_hidden(hid, table_np, ref["tokens"], f"cycle {cycle} advance_draft {i}")
            same_state(f"cycle {cycle} advance_draft {i}")
            note(ref["slots"], live, 1)
        ids_kb[k - 1].copy_(dev(draft[:, k - 1]))
        n = B * (k + 1)
        tv, pv, sv, cv = _bufs(n, B)
        hv = torch.full((n, H), 3.0, dtype=torch.float16, device=DEV)
        ops.spec_prepare_verify(d_st["last_token"], ids_kb.transpose(0, 1), eff, bt, bs, tv, pv, sv, cv, embed=(table_d, hv))
        ref = cc.prepare_verify(st["last_token"], draft, eff_np, bt_np, bs)
        _same_index_tensors((tv, pv, sv, cv), ref, f"cycle {cycle} prepare_verify")
        _same_hidden(hv, table_np, ref["tokens"], f"cycle {cycle} prepare_verify")
        same_state(f"cycle {cycle} prepare_verify")
        note(ref["slots"], live, k + 1)
        out = np.full((B, k + 1), -1, np.int64)       # masked and empty rows emit nothing
        for b in live:
            n_acc = int(rng.integers(0, k + 1))
            out[b, :n_acc] = draft[b, :n_acc]
            out[b, n_acc] = int(rng.integers(0, V))
        ops.spec_commit(dev(out), d_st["seq_lens"], d_st["last_token"], d_st["gen_tokens"], d_st["gen_lens"])
        st = cc.commit(out, st["seq_lens"], st["last_token"], st["gen_tokens"], st["gen_lens"])
        same_state(f"cycle {cycle} commit")
        stepped += len(live)
    assert finished >= 3 and stepped >= 2 * B      # sequences did reach the end of their tables, and rows did step
    for b in range(B):
        assert written[b] <= own[b], b
    for a, b in itertools.combinations(range(B), 2):
        assert not (written[a] & written[b]), (a, b)
