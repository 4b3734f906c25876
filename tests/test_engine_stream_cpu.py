"""The numpy Philox4x32-10 of tests/philox_ref.py against the published known answers, the engine stream's counter layout,
and the share of rows the GPU argmax tests skip (it depends on the numpy reference alone, so it is bounded here, for the
exact seeds and offsets tests/test_engine_stream_gpu.py uses)."""
import numpy as np
import pytest

import engine_stream_cases as esc
from philox_ref import M32, engine_r0, philox_r0, philox_words, seeded_r0

# Random123 kat_vectors, philox4x32 with 10 rounds: counter (4 words), key (2 words) -> output (4 words)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(w) for w in philox_words(*ctr, *key)) == want
    assert int(philox_r0(*ctr, *key)) == want[0]


def test_philox_broadcasts_like_its_scalar_form():
    c0 = np.arange(5).reshape(1, 5)
    c1 = np.array([7, 0x40000003]).reshape(2, 1)
    got = philox_r0(c0, c1, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert got.shape == (2, 5)
    for i in range(2):
        for j in range(5):
            assert int(got[i, j]) == int(philox_r0(int(c0[0, j]), int(c1[i, 0]), 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0))


def test_engine_counter_layout():
    """key = (seed lo, seed hi), counter = (c0, c1, offset lo, offset hi): every word is live."""
    seed, offset = esc.SEED, esc.OFFSET
    assert seed >> 32 and offset >> 32 and seed < 2 ** 63 and offset < 2 ** 63
    base = int(engine_r0(5, 9, seed, offset))
    assert base == int(philox_r0(5, 9, offset & M32, offset >> 32, seed & M32, seed >> 32))
    others = [engine_r0(6, 9, seed, offset), engine_r0(5, 10, seed, offset), engine_r0(5, 9, seed & M32, offset),
              engine_r0(5, 9, seed, offset & M32), engine_r0(5, 9, seed + 1, offset), engine_r0(5, 9, seed, offset + 1),
              engine_r0(5, 0x40000000 | 9, seed, offset)]
    assert len({base, *(int(x) for x in others)}) == 8
    # the seeded stream's c1 has its top bit set: it can never meet the engine stream's row counters
    assert int(seeded_r0(5, seed, offset & M32, 0, 9)) == int(philox_r0(5, 0x80000000 | 9, offset & M32, 0, seed & M32, seed >> 32))


@pytest.mark.parametrize("offset", [esc.OFFSET, esc.OFFSET + 1])
def test_share_of_skipped_rows_is_within_the_cap(offset):
    for case in (esc.recovered_case(offset), esc.sampled_case(offset)):
        skipped = 1.0 - case["ok"].mean()
        assert skipped <= esc.MAX_SKIPPED, skipped
        assert case["ok"].sum() >= 0.9 * case["ok"].size >= 86


def test_uniform_case_has_both_outcomes_at_every_position():
    for offset in (esc.OFFSET, esc.OFFSET + 1):
        acc = esc.uniform_case(offset)["accepted"]
        assert acc.any(0).all() and (~acc).any(0).all()
