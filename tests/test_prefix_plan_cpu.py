"""The launch plan of the context-split prompt attention, without a device: the library's own predicate
(qspec_paged_attention_family = attention.hip: attn_form) over a table of shapes, the split-length rule of the kernel restated,
and the engine's split rule prefill_splits."""
import pytest

from qspec_amd import ops
from qspec_amd.spec_decode import engine as E
from qspec_amd.spec_decode.engine import prefill_splits

NO_LAUNCH, GENERIC, GENERIC_VEC, PREFILL, WAVES, CHUNK, PREFILL_SPLIT = range(7)
FA_ROWS = FA_KEYS = 64


def family(q_len, S, merged, heads=(32, 8, 128), n_seqs=1, bs=16, width=64):
    nq, nkv, d = heads
    return ops.paged_attention_family(n_seqs, q_len, nq, nkv, d, bs, width, S, merged)


def test_family_numbers_are_the_header_order():
    assert (ops.ATTN_NO_LAUNCH, ops.ATTN_GENERIC, ops.ATTN_GENERIC_VEC, ops.ATTN_PREFILL, ops.ATTN_WAVES, ops.ATTN_CHUNK,
            ops.ATTN_PREFILL_SPLIT) == (NO_LAUNCH, GENERIC, GENERIC_VEC, PREFILL, WAVES, CHUNK, PREFILL_SPLIT)


@pytest.mark.parametrize("q_len", [1, 4, 6, 31])            # rows = 4 q_len < 128
@pytest.mark.parametrize("S", [1, 2, 16, 64])
def test_fewer_than_128_rows_keep_their_family(q_len, S):
    # width 64 x block 16 = 1024 keys: splits longer than one 128-key chunk below 8 splits
    long_splits = 64 * 16 > 128 * S
    assert family(q_len, S, True) == CHUNK                  # the in-kernel merge exists in the chunk kernel alone
    assert family(q_len, S, False) == (WAVES if long_splits else CHUNK)


@pytest.mark.parametrize("q_len,heads", [(32, (32, 8, 128)), (33, (32, 8, 128)), (512, (32, 8, 128)), (16, (64, 8, 128)),
                                         (128, (40, 40, 128))])
def test_128_rows_and_more(q_len, heads):
    for merged in (True, False):
        assert family(q_len, 1, merged, heads) == PREFILL
        for S in (2, 16, 64):
            assert family(q_len, S, merged, heads) == PREFILL_SPLIT
    assert family(q_len, 65, True, heads) == NO_LAUNCH      # QS_ATT_MAXSPLIT
    assert family(q_len, 0, True, heads) == NO_LAUNCH


def test_the_split_family_has_no_ticket_counters():
    # 16-row blocks x kv heads x sequences beyond the 4096 counter slots: the chunk kernel refuses a merged call (-4) ...
    assert family(6, 4, True, n_seqs=300) == NO_LAUNCH and family(6, 4, False, n_seqs=300) != NO_LAUNCH
    # ... the split prompt kernel merges in a launch of its own
    assert family(64, 4, True, n_seqs=300) == PREFILL_SPLIT


def test_other_head_sizes_and_refusals_are_unchanged():
    for S in (1, 2, 16, 64):
        for q_len in (1, 6, 128):
            assert family(q_len, S, True, (32, 4, 64)) == GENERIC_VEC and family(q_len, S, False, (32, 4, 64)) == GENERIC_VEC
    assert family(4, 1, True, (4, 2, 66)) == GENERIC and family(4, 1, False, (4, 2, 66)) == NO_LAUNCH
    assert family(4, 1, True, (4, 2, 258)) == NO_LAUNCH and family(4, 1, True, (4, 2, 65)) == NO_LAUNCH
    assert family(4, 65, True, (32, 4, 64)) == NO_LAUNCH                     # -3
    assert family(4, 1, True, (32, 5, 128)) == NO_LAUNCH                     # -1: heads % kv heads
    assert family(40, 2, True, (24, 8, 128)) == NO_LAUNCH                    # -5: group 3
    assert family(40, 2, True, bs=12) == NO_LAUNCH                           # -5: block size
    assert family(40, 2, True, n_seqs=0) == NO_LAUNCH                        # nothing to launch
    assert family(8, 1, True, (4, 2, 64), width=2048) == NO_LAUNCH           # -2: one split of 32 K keys


def split_range(ctx, S, z, n_keys):
    """attention_prefill.hip, SPLIT: the keys [k0, k1) and the 64-key chunks of split z (n_keys: the workgroup's horizon)."""
    L = -(-(-(-ctx // S)) // FA_KEYS) * FA_KEYS
    k0 = z * L
    k1 = min(k0 + L, n_keys)
    return k0, k1, max(k1 - k0 + FA_KEYS - 1, 0) // FA_KEYS


@pytest.mark.parametrize("ctx,S", [(32, 4), (70, 16), (191, 3), (193, 3), (511, 8), (513, 8), (4097, 16), (4128, 16), (1, 2)])
def test_split_ranges_tile_the_context_in_whole_chunks(ctx, S):
    covered = []
    for z in range(S):
        k0, k1, n = split_range(ctx, S, z, ctx)
        assert k0 % FA_KEYS == 0
        if k1 > k0:
            assert n == -(-(k1 - k0) // FA_KEYS)
            covered += list(range(k0, k1))
        else:
            assert n == 0                                   # wholly behind the context: the neutral partial
    assert covered == list(range(ctx))
    # a causal horizon in front of the split clips it to nothing, never to a negative chunk count
    assert all(split_range(ctx, S, z, 1)[2] == (1 if z == 0 else 0) for z in range(S))


def test_prefill_splits_is_one_without_context():
    for q in ([1], [5, 9], [32], [512, 4096], [150] * 32, [8192]):
        assert prefill_splits(q, q, 8, 4) == 1
        assert prefill_splits(q, q, 2, 4) == 1 and prefill_splits(q, q, 40, 1) == 1


def test_prefill_splits_bounds_and_monotony():
    for nkv, group in ((8, 4), (2, 4), (40, 1), (8, 8)):
        for q_lens in ([1], [32], [33], [128], [512], [32, 32, 32, 32], [1, 40, 33], [4096]):
            W = sum(-(-q * group // FA_ROWS) for q in q_lens) * nkv
            last = 1
            for prefix in (1, 63, 64, 65, 512, 1000, 2048, 4096, 8192, 100000):
                S = prefill_splits(q_lens, [q + prefix for q in q_lens], nkv, group)
                assert 1 <= S <= 16
                assert S == 1 or S * W <= 256
                assert S == 1 or (S - 1) * E.PREFILL_SPLIT_MIN_KEYS < max(q_lens) + prefix   # no split shorter than Kmin
                assert S >= last                                                              # monotone in the prefix
                last = S
    # one sequence with context is enough
    assert prefill_splits([32, 32], [32, 4128], 8, 4) > 1


def test_worked_example_32_tokens_behind_4096():
    """Llama-3-8B head layout: the unsplit kernel launches 2 row blocks x 8 kv heads = 16 workgroups on 256 CUs."""
    W = -(-32 * 4 // FA_ROWS) * 8
    assert W == 16
    S = prefill_splits([32], [4096 + 32], 8, 4)
    assert S == min(16, 256 // W, -(-(4096 + 32) // E.PREFILL_SPLIT_MIN_KEYS)) and S > 1
    assert ops.paged_attention_family(1, 32, 32, 8, 128, 16, 259, S, False) == PREFILL_SPLIT
