"""The selection matrix of tests/sampling_cases.py itself, on the CPU: its float64 reference is pinned to the oracle's op-for-op
restatement of the reference project (and to logit_cases.sampler_probs for min_p), the matrix holds every boundary it
claims, the margins that make every row decidable hold, the model of the kernel passes the GPU test's checks while each
named fault fails them, and PROB_BAR is the measured oracle-to-float64 distance times a stated factor."""
import numpy as np
import pytest

import logit_cases
import sampling_cases as sc

CASES = sc.cases()
IDS = [c.name for c in CASES]


def _same_outside_boundary(case, other_keep, what):
    """`other_keep` comes from a per-token rule (a sort splits a group of equal logits arbitrarily): equal to the reference
    outside the lowest kept group, which the reference keeps whole; exactly equal when that group is one token."""
    ref = case.ref.nonzero
    if case.ref.boundary_count == 1:
        assert np.array_equal(other_keep, ref), (case.name, what, int(other_keep.sum()), int(ref.sum()))
        return True
    lg = case.logits.astype(np.float64)
    b = lg[other_keep].min()
    off = lg != b
    assert np.array_equal(other_keep[off], ref[off]), (case.name, what)
    assert ref[~off].all(), (case.name, what, "the boundary group is not whole")
    return np.array_equal(other_keep, ref)


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    """oracle.sample_top_k_top_p on every case without min_p, once: name -> (probs, token, keep)."""
    out = {}
    for c in CASES:
        if (c.min_p > 0.0 and c.temperature >= 1e-5) or np.isnan(c.logits).any():     # (the oracle's sort takes no NaN)
            continue
        tp = None if c.top_p is None else np.array([c.top_p], np.float32)
        pr, tk, keep = oracle.sample_top_k_top_p(c.logits[None], np.array([c.temperature], np.float32),
                                                 np.array([c.top_k], np.int64), tp, c.E[None])
        out[c.name] = (pr[0], int(tk[0]), keep[0])
    return out


def test_positions():
    f = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    pos = sc.positions(f)
    ok = pos >= 0
    assert (~ok).sum() == 2 * 1023 and np.isnan(f[~ok]).all()
    v, p = f[ok].astype(np.float64), pos[ok]
    order = np.argsort(p, kind="stable")
    assert (np.diff(v[order]) <= 0).all()                       # a smaller position is a larger logit ...
    same = np.diff(p[order]) == 0
    assert same.sum() == 1 and (v[order][:-1][same] == 0).all()   # ... and only the two zeros share one
    assert sc.pos_of(0.0) == sc.pos_of(-0.0) == sc.POS_ZERO and sc.pos_of(-np.inf) == sc.POS_NEG_INF
    assert sc.pos_of(65504.0) == 1024 and sc.pos_of(np.float16(-6e-8)) == sc.POS_ZERO + 2
    for q in (1024, 16383, 16384, sc.POS_ZERO, 32769, 49151, 49152, sc.POS_NEG_INF):
        assert sc.pos_of(sc.value_at(q)) == q
    assert sc.value_at(4 * 4096 - 1) == np.float16(2.0) and sc.value_at(12 * 4096) == np.float16(-2.0)   # wave edges, both signs
    row = sc.build_row([(sc.th(260, 63), 2), (sc.POS_ZERO, 3), (sc.POS_NEG_INF, 1)], 6, seed=1, neg_zeros=2)
    assert sorted(sc.positions(row)) == [sc.th(260, 63)] * 2 + [sc.POS_ZERO] * 3 + [sc.POS_NEG_INF]
    assert np.signbit(row[row == 0]).sum() == 2


def test_reference_matches_the_oracle(oracle_runs):
    exact = 0
    for c in CASES:
        if c.name not in oracle_runs:
            continue
        pr, tk, keep = oracle_runs[c.name]
        if _same_outside_boundary(c, keep, "oracle"):
            exact += 1
            assert tk == c.ref.token, (c.name, tk, c.ref.token)
            assert np.abs(pr - c.ref.probs).max() <= 1e-6, c.name
    assert exact >= len(oracle_runs) - 12     # (the rest: rows whose boundary group the oracle's sort splits)


def test_min_p_reference():
    n = 0
    for c in CASES:
        if c.min_p == 0.0:
            continue
        n += 1
        pr, keep = logit_cases.sampler_probs(c.logits, c.temperature, c.top_k, 1.0 if c.top_p is None else c.top_p, c.min_p)
        if _same_outside_boundary(c, keep, "sampler_probs"):
            assert np.abs(pr - c.ref.probs).max() <= 1e-6 and int(np.argmax(pr / c.E)) == c.ref.token, c.name
    assert n >= 12


def test_matrix_has_what_it_claims():
    have = {t for c in CASES for t in c.tags}
    assert not set(sc.TAGS) - have, sorted(set(sc.TAGS) - have)
    assert not have - set(sc.TAGS), sorted(have - set(sc.TAGS))
    thread = lambda q: q >> 6
    for c in CASES:
        r, tags = c.ref, set(c.tags)
        k = c.top_k
        ordered = np.sort(sc.positions(c.logits))
        if "tk_first_key" in tags:
            assert ordered[k - 1] % 64 == 0 and r.pos_k == ordered[k - 1]
        if "tk_last_key" in tags:
            assert ordered[k - 1] % 64 == 63 and r.boundary_count == 1
        if "tk_inside_group_last_key" in tags:
            assert r.pos_k % 64 == 63 and ordered[k - 2] == ordered[k - 1] == ordered[k] == r.pos_k
        if "tk_exact_group_end" in tags:
            assert ordered[k - 1] == r.pos_k != ordered[k] and r.boundary_count > 1
        if tags & {"tk_next_same_thread", "tk_next_thread", "tk_next_after_empty_threads", "tk_next_across_wave"}:
            assert ordered[k - 2] == r.prev_k != ordered[k - 1] == r.pos_k             # k is one past a group's end
            gap = thread(r.pos_k) - thread(r.prev_k)
            if "tk_next_same_thread" in tags:
                assert gap == 0
            if "tk_next_thread" in tags:
                assert gap == 1
            if "tk_next_after_empty_threads" in tags:
                assert gap >= 4
            if "tk_next_across_wave" in tags:
                assert r.pos_k % 4096 == 0 and r.prev_k == r.pos_k - 1
        if "k_exceeds_finite" in tags:
            assert np.isneginf(c.logits.astype(np.float32)).any() and k > np.isfinite(c.logits.astype(np.float32)).sum() and k < c.V
        if "k1_tie_at_max" in tags:
            assert k == 1 and r.kept.sum() == 3
        if any(t.startswith("tp_") for t in tags) and not tags & {"tp_one_wide", "tp_none_wide"}:
            assert r.pos_p is not None and r.tightest == "top_p", c.name
        if "tp_mid_thread" in tags:
            assert thread(r.pos_p) == thread(r.prev_p) and 0 < r.pos_p % 64 < 63
        for t, lo, hi in (("tp_later_thread_adjacent", 1, 1), ("tp_later_thread_one_empty", 2, 2), ("tp_later_thread_many_empty", 4, 999)):
            if t in tags:
                assert lo <= thread(r.pos_p) - thread(r.prev_p) <= hi
                assert (ordered >> 6 == thread(r.pos_p)).any() and ordered[ordered >> 6 == thread(r.pos_p)].min() == r.pos_p
        if "tp_across_wave" in tags:
            assert r.pos_p % 4096 == 0 and r.prev_p == r.pos_p - 1
        if "tp_pos_last_in_empty_thread" in tags:
            assert r.pos_p % 64 == 0 and thread(r.prev_p) < thread(r.pos_p) - 1 and not (ordered >> 6 == thread(r.pos_p) - 1).any()
        if "tp_first_masked_last_key" in tags:
            assert r.pos_p % 64 == 63 and thread(r.prev_p) == thread(r.pos_p)
        if tags & {"tp_max_alone_same_thread", "tp_max_alone_later_thread"}:
            assert r.prev_p == ordered[0] and (thread(r.pos_p) == thread(r.prev_p)) == ("tp_max_alone_same_thread" in tags)
        if "tp_above_top_k" in tags:
            assert r.pos_p < r.pos_k and 0 < k < c.V
        if "tk_above_top_p" in tags:
            assert r.pos_p is None and r.tightest == "top_k" and c.top_p < 1.0
        if "tp_1e-6" in tags:
            assert c.top_p == float(np.float32(1e-6)) and r.kept.sum() == 2
        if tags & {"tp_one_wide", "tp_none_wide"}:
            fin = r.d[np.isfinite(r.d)]
            assert (c.top_p is None) == ("tp_none_wide" in tags) and (c.top_p is None or c.top_p == 1.0)
            assert fin.min() <= -59.9 and r.nonzero.sum() == (min(k, c.V) if k > 0 else c.V)     # 60 nats, nothing lost
        if "mp_binding" in tags:
            assert r.tightest == "min_p"
        if "mp_not_binding" in tags:
            assert c.min_p > 0 and r.pos_mp is None
        if "mp_first_key" in tags:
            assert r.pos_mp % 64 == 0
        if "mp_last_key" in tags:
            assert r.pos_mp % 64 == 63
        if "mp_one" in tags:
            assert c.min_p == 1.0 and r.kept.sum() == 2 and r.boundary_count == 2
        for t in ("top_k", "top_p", "min_p"):
            if "tightest_" + t in tags:
                assert r.tightest == t and 0 < k < c.V and c.top_p < 1.0 and c.min_p > 0.0
        if any(t.startswith("sz_") for t in tags):
            z = c.logits[c.logits == 0]
            assert 0 < np.signbit(z).sum() < z.size
            zero_kept = r.kept[c.logits == 0]
            assert zero_kept.all() or not zero_kept.any()
        if "sz_top_k" in tags:
            assert r.pos_k == sc.POS_ZERO
        if "sz_top_p" in tags:
            assert sc.POS_ZERO in (r.pos_p, r.prev_p)
        if "sz_min_p" in tags:
            assert sc.POS_ZERO in (r.pos_mp, ordered[ordered < r.pos_mp].max())
        if "sz_max_small_p" in tags:
            assert ordered[0] == sc.POS_ZERO and c.top_p <= 0.01 and r.kept.sum() == 4
        if "subnormals" in tags:
            b = c.logits.view(np.uint16) & 0x7FFF
            assert (b < 0x0400).all() and (b > 0).sum() == c.V - 1
        if "T=0.05" in tags:
            assert (r.d < sc.UNDERFLOW).sum() > 0.9 * c.V
        if "greedy" in tags:
            assert c.temperature < 1e-5 and r.token == int(np.argmax(c.logits.astype(np.float32))) and r.kept.all()
        if "nan_takes_no_part" in tags:
            nan = np.isnan(c.logits)
            assert nan.sum() >= 10 and not r.kept[nan].any() and (r.probs[nan] == 0).all() and r.tightest == "top_p"
        if "negative_edge" in tags:
            assert r.pos_k > sc.POS_ZERO + 1 and (r.pos_p or r.pos_k) > sc.POS_ZERO + 1
        for t in tags:
            if t.startswith("V="):
                assert c.V == int(t.split("_")[0][2:])
        if "V=131080_uniform" in tags:
            assert np.unique(c.logits).size == 1 and r.kept.all() and 0 < k < c.V and c.top_p < 1.0
    # every % 64 edge and the wave edge, for top-k and for top-p, on both signs somewhere
    for what in ("pos_k", "pos_p"):
        got = [getattr(c.ref, what) for c in CASES if getattr(c.ref, what) is not None and c.ref.tightest == "top_" + what[-1]]
        assert any(q % 64 == 0 for q in got) and any(q % 64 == 63 for q in got) and any(q % 4096 == 0 for q in got), what
        assert any(q > sc.POS_ZERO for q in got) and any(q < sc.POS_ZERO for q in got), what
    assert {c.V for c in CASES} >= {1, 7, 64, 1003, 16384, 16385, 40000, 131080}
    assert all(c.V <= 1003 for c in CASES if not any(t.startswith("V=") for t in c.tags))
    assert {c.temperature for c in CASES} >= {float(np.float32(t)) for t in (0.05, 0.3, 1.0, 2.0, 0.0)}


def test_margins_hold():
    for c in CASES:
        r = c.ref
        assert r.gap_p >= sc.GAP_TOP_P and r.gap_mp >= sc.GAP_MIN_P, (c.name, r.gap_p, r.gap_mp)
        fin = r.d[np.isfinite(r.d)]
        assert not ((fin > sc.CLEAR_ZONE[0]) & (fin < sc.CLEAR_ZONE[1])).any(), c.name
        assert sc.CLEAR_ZONE[0] < sc.UNDERFLOW < sc.CLEAR_ZONE[1]
        if c.temperature >= 1e-5 and c.V > 1:
            assert r.best > 0 and r.best >= (1.0 + sc.GAP_E) * r.second, (c.name, r.best, r.second)
        assert abs(r.probs.sum() - 1.0) < 1e-12 and not r.kept[np.isneginf(c.logits.astype(np.float32))].any()
        assert c.E.dtype == np.float32 and (c.E > 0).all()


def test_batches():
    bs = sc.batches()
    assert sorted(c.name for b in bs for c in b) == sorted(IDS)
    assert all(1 <= len(b) <= 17 and len({(c.V, c.top_p is None) for c in b}) == 1 for b in bs)
    assert any(len(b) == 17 for b in bs)                         # the row index reaches past 16
    full = next(b for b in bs if len(b) == 17)
    assert len({c.top_k for c in full}) > 3 and len({c.top_p for c in full}) > 3
    lg, temp, top_k, top_p, min_p, E = sc.batch_arrays(full)
    assert lg.shape == E.shape == (17, full[0].V) and lg.dtype == np.float16 and top_k.dtype == np.int32
    assert temp.dtype == top_p.dtype == min_p.dtype == E.dtype == np.float32
    assert sc.batch_arrays([c for c in CASES if c.top_p is None])[3] is None


def _model(c, fault=None):
    return sc.model_select(c.logits, c.temperature, c.top_k, c.top_p, c.min_p, c.E, fault=fault)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_model_of_the_kernel_passes_the_gpu_checks(c):
    probs, token = _model(c)
    assert sc.check_row(c.ref, probs, token) == []


@pytest.mark.parametrize("fault", sc.FAULTS)
def test_each_fault_is_caught(fault):
    caught, worst, kept_differs = [], 0.0, False
    for c in CASES:
        if c.V > 1003:
            continue
        probs, token = _model(c, fault)
        if sc.check_row(c.ref, probs, token):
            caught.append(c.name)
            fin = np.isfinite(probs)
            kept_differs |= not fin.all() or not np.array_equal(probs > 0, c.ref.nonzero)
            if fin.all():
                worst = max(worst, float(np.abs(probs - c.ref.probs).max()))
    print(f"{fault}: caught by {len(caught)} cases {caught[:6]}, largest |dp| {worst:.3g}, kept set differs: {kept_differs}")
    assert caught, fault
    assert kept_differs or worst >= 10 * sc.PROB_BAR, (fault, worst)


def test_faults_are_caught_by_the_cases_meant_for_them():
    fails = lambda name, fault: bool(sc.check_row(BY[name].ref, *_model(BY[name], fault)))
    BY = {c.name: c for c in CASES}
    assert fails("tk_exact_group_end", "k_off_by_one") and fails("tk_last_key", "k_off_by_one")
    assert fails("sz_top_k", "split_signed_zero") and fails("sz_max_small_p", "split_signed_zero")
    assert fails("tp_max_alone_same_thread", "mask_max_group") and fails("tp_max_alone_later_thread", "mask_max_group")
    for n in ("tp_later_thread_adjacent", "tp_later_thread_one_empty", "tp_later_thread_many_empty", "tp_across_wave"):
        assert fails(n, "later_thread_not_offered"), n
    assert fails("tp_pos_last_in_empty_thread", "empty_thread_denominator")
    assert fails("tp_one_wide", "p_one_absorbs_tail") and fails("tp_none_wide", "p_one_absorbs_tail") and fails("tp_one_peaked", "p_one_absorbs_tail") \
        and fails("T=0.05", "p_one_absorbs_tail")
    assert fails("mp_one", "minp_masks_max")
    assert fails("tk_inside_group_last_key", "boundary_group_split")


def test_prob_bar_is_measured(oracle_runs):
    """PROB_BAR = 2x .. 8x the largest |oracle probs - float64 probs| over the cases whose kept sets agree."""
    worst, n = 0.0, 0
    for c in CASES:
        if c.name in oracle_runs and np.array_equal(oracle_runs[c.name][2], c.ref.nonzero):
            worst = max(worst, float(np.abs(oracle_runs[c.name][0].astype(np.float64) - c.ref.probs).max()))
            n += 1
    print(f"oracle to float64: {worst:.4g} over {n} cases; PROB_BAR = {sc.PROB_BAR:.3g} = {sc.PROB_BAR / worst:.2f}x")
    assert n >= 40
    assert 2 * worst <= sc.PROB_BAR <= 8 * worst, (worst, sc.PROB_BAR)
