"""The engine (unseeded) Philox stream of csrc/sampler.hip -- what every request without SamplingParams.seed draws from:
key = seed, counter = (c0, c1, offset lo, offset hi), c1 = b * k + i for the rejection sampler and 0x40000000 | row for
the sampler (include/qspec_hip.h).  The layout is pinned against a numpy Philox (tests/philox_ref.py), rng_state's
advance is checked eagerly and under graph replay, and the draws of the rows of ONE call must follow the distributions."""
import numpy as np
import pytest
import torch

import engine_stream_cases as esc
from test_seeded_sampling_gpu import _tv_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, OFFSET = esc.SEED, esc.OFFSET
MAX_ROWS = 4096       # batch * k of one qspec_rejection_sample call (csrc/capi.hip)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from qspec_amd import ops
    return ops


def _rng_args(mode, seed, offset):
    """The two ways a call names its place in the stream: the scalars, or a device rng_state = [seed, offset]."""
    if mode == "scalars":
        return dict(seed=seed, offset=offset), None
    rs = torch.tensor([seed, offset], dtype=torch.int64, device=DEV)
    return dict(seed=1, offset=2, rng_state=rs), rs          # (the scalars are overridden by rng_state)


def _reject(ops, case, rng_kw):
    B, k, V = case["dp"].shape
    out = torch.full((B, k + 1), -5, dtype=torch.int64, device=DEV)
    acc = torch.full((B, k), 9, dtype=torch.uint8, device=DEV)
    rec = torch.full((B, k), -5, dtype=torch.int64, device=DEV)
    ops.rejection_sample(dev(case["tq"]), dev(case["bonus"].astype(np.int64)), dev(case["dp"]), dev(case["ids"].astype(np.int64)),
                         out, acc, rec, None, **rng_kw)
    torch.cuda.synchronize()
    return host(out), host(acc), host(rec)


class _Sampler:
    """One sampler call's buffers (temperature 1, no top-k / top-p unless given), reusable under graph capture."""

    def __init__(self, ops, logits, temp=1.0, top_k=-1, top_p=1.0):
        T, V = logits.shape
        self.ops, self.logits = ops, dev(logits)
        self.probs = torch.empty(T, V, dtype=torch.float32, device=DEV)
        self.tok = torch.full((T,), -5, dtype=torch.int64, device=DEV)
        self.temp = torch.full((T,), temp, dtype=torch.float32, device=DEV)
        self.top_k = torch.full((T,), top_k, dtype=torch.int32, device=DEV)
        self.top_p = torch.full((T,), top_p, dtype=torch.float32, device=DEV)
        self.ws = ops.new_sample_workspace(T, DEV)

    def __call__(self, **rng_kw):
        self.ops.sample_top_k_top_p(self.logits, self.probs, self.tok, self.temp, self.top_k, self.top_p, workspace=self.ws,
                                    **rng_kw)


def _check_argmax(got, case, what):
    ok = case["ok"]
    assert 1.0 - ok.mean() <= esc.MAX_SKIPPED
    bad = np.flatnonzero((got != case[what])[ok].ravel())
    assert bad.size == 0, f"{bad.size} of {ok.sum()} checked rows differ from the numpy stream, first {bad[:5]}"


# ------------------------------------------------------------------ 1. counter and key layout

@pytest.mark.parametrize("mode", ["scalars", "rng_state"])
def test_accept_uniform_layout(ops, mode):
    case = esc.uniform_case()
    kw, rs = _rng_args(mode, SEED, OFFSET)
    _, acc, _ = _reject(ops, case, kw)
    assert np.array_equal(acc.astype(bool), case["accepted"])
    if rs is not None:
        assert host(rs).tolist() == [SEED, OFFSET + 1]


@pytest.mark.parametrize("mode", ["scalars", "rng_state"])
def test_recovered_token_layout(ops, mode):
    case = esc.recovered_case()
    kw, _ = _rng_args(mode, SEED, OFFSET)
    out, acc, rec = _reject(ops, case, kw)
    assert not acc.any()                                   # q[x] = 0: every draft token is rejected
    _check_argmax(rec, case, "recovered")
    assert np.array_equal(out[:, 0], rec[:, 0]) and (out[:, 1:] == -1).all()


@pytest.mark.parametrize("mode", ["scalars", "rng_state"])
def test_sampled_token_layout(ops, mode):
    case = esc.sampled_case()
    kw, _ = _rng_args(mode, SEED, OFFSET)
    s = _Sampler(ops, case["logits"])
    s(**kw)
    torch.cuda.synchronize()
    _check_argmax(host(s.tok), case, "token")


# ------------------------------------------------------------------ 2. rng_state

def test_rng_state_advances_by_one_and_matches_numpy_at_both_offsets(ops):
    """Two back-to-back calls on one rng_state draw at offset and offset + 1, the seed word is left alone; and a call with
    rng_state gives what the same scalars give."""
    rs = torch.tensor([SEED, OFFSET], dtype=torch.int64, device=DEV)
    for n in range(2):
        case = esc.uniform_case(OFFSET + n)
        out, acc, rec = _reject(ops, case, dict(rng_state=rs))
        assert host(rs).tolist() == [SEED, OFFSET + n + 1]
        assert np.array_equal(acc.astype(bool), case["accepted"])
        same = _reject(ops, case, dict(seed=SEED, offset=OFFSET + n))
        assert all(np.array_equal(a, b) for a, b in zip((out, acc, rec), same))
    rs = torch.tensor([SEED, OFFSET], dtype=torch.int64, device=DEV)
    for n in range(2):
        case = esc.recovered_case(OFFSET + n)
        out, acc, rec = _reject(ops, case, dict(rng_state=rs))
        assert host(rs).tolist() == [SEED, OFFSET + n + 1]
        _check_argmax(rec, case, "recovered")
    rs = torch.tensor([SEED, OFFSET], dtype=torch.int64, device=DEV)
    s = _Sampler(ops, esc.sampled_case()["logits"])
    for n in range(2):
        case = esc.sampled_case(OFFSET + n)
        s(rng_state=rs)
        torch.cuda.synchronize()
        assert host(rs).tolist() == [SEED, OFFSET + n + 1]
        tok, probs = host(s.tok).copy(), host(s.probs).copy()
        _check_argmax(tok, case, "token")
        s(seed=SEED, offset=OFFSET + n)
        torch.cuda.synchronize()
        assert np.array_equal(host(s.tok), tok) and np.array_equal(host(s.probs), probs)
        assert host(rs).tolist() == [SEED, OFFSET + n + 1]      # a call with scalars leaves it alone


def test_graph_replays_draw_at_consecutive_offsets(ops):
    """One captured sampler call (a single kernel chain), replayed twice: the draws of offset and offset + 1."""
    s = _Sampler(ops, esc.sampled_case()["logits"])
    rs = torch.tensor([SEED, 5], dtype=torch.int64, device=DEV)
    s(rng_state=rs)                                         # (first use outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s(rng_state=rs)
    rs.copy_(torch.tensor([SEED, OFFSET], dtype=torch.int64))
    for n in range(2):
        s.tok.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        assert host(rs).tolist() == [SEED, OFFSET + n + 1]
        _check_argmax(host(s.tok), esc.sampled_case(OFFSET + n), "token")


# ------------------------------------------------------------------ 3. distributions over the rows of one call

def _tv(counts, p):
    n = counts.sum()
    return 0.5 * np.abs(counts / n - p).sum(), _tv_bound(p, n)


def test_sampler_rows_of_one_call_follow_the_distribution(ops):
    rng = np.random.default_rng(44)
    V, T = 64, 4096
    logits = np.tile(rng.normal(0, 1.5, V).astype(np.float16), (T, 1))
    s = _Sampler(ops, logits, temp=0.9, top_k=20, top_p=0.95)
    s(seed=SEED, offset=OFFSET)
    torch.cuda.synchronize()
    p, tok = host(s.probs), host(s.tok)
    assert np.array_equal(p, np.tile(p[0], (T, 1)))
    probs = p[0].astype(np.float64)
    counts = np.bincount(tok, minlength=V).astype(np.float64)
    assert (counts[probs == 0] == 0).all() and 1 < (probs > 0).sum() <= 20
    tv, bound = _tv(counts, probs)
    assert tv < bound, (tv, bound)


def _dist_case(rng, form, N, k, V):
    q = esc.softmax32(rng.normal(0, 1, (k + 1, V)))
    tq = np.tile(q, (N, 1, 1))
    if form == "one_hot":
        p = None
        ids = rng.integers(0, V, (N, k))
        dp = np.zeros((N, k, V), np.float32)
        np.put_along_axis(dp, ids[..., None], 1.0, -1)
    else:
        p = esc.softmax32(rng.normal(0, 1, (k, V)))
        dp = np.tile(p, (N, 1, 1))
        ids = np.stack([rng.choice(V, N, p=p[i].astype(np.float64) / p[i].astype(np.float64).sum()) for i in range(k)], 1)
    return dict(tq=tq, dp=dp, ids=ids, bonus=rng.integers(0, V, N)), q.astype(np.float64), p


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("form", ["one_hot", "dense"])
def test_rejection_rows_of_one_call_follow_the_target(ops, form, k):
    """The emitted token at position 0 follows q_0 whatever the draft; with k = 2, among the rows that accepted position 0,
    the token at position 1 follows q_1 (accepted or recovered) -- which draws shared between the positions of a row, or
    an accept uniform tied to the recovery noise, would break.  Dense drafts: the acceptance rate at position 0 is
    sum_v min(p_v, q_v)."""
    rng = np.random.default_rng([45, k, form == "dense"])
    N, V = 4096, 16
    case, q, p = _dist_case(rng, form, N, k, V)
    # one call takes at most MAX_ROWS (b, i) rows (qspec_rejection_sample refuses more): k = 1 is one call of all N rows, k = 2
    # two calls of N / 2 rows at consecutive offsets -- within a call only the row index separates the draws
    per_call = MAX_ROWS // k
    assert N % per_call == 0
    parts = [_reject(ops, {name: x[r:r + per_call] for name, x in case.items()}, dict(seed=SEED, offset=OFFSET + c))
             for c, r in enumerate(range(0, N, per_call))]
    out, acc = np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts])
    assert out.shape == (N, k + 1)
    assert (out[:, 0] >= 0).all()
    tv, bound = _tv(np.bincount(out[:, 0], minlength=V).astype(np.float64), q[0])
    assert tv < bound, ("position 0", tv, bound)
    if k == 2:
        rows = acc[:, 0] == 1
        assert rows.sum() >= 100 and (out[rows, 1] >= 0).all()
        tv, bound = _tv(np.bincount(out[rows, 1], minlength=V).astype(np.float64), q[1])
        assert tv < bound, ("position 1 of the rows that accepted position 0", rows.sum(), tv, bound)
    if form == "dense":
        a = np.minimum(p[0].astype(np.float64), q[0]).sum()
        rate = acc[:, 0].mean()
        assert abs(rate - a) <= 3.0 * np.sqrt(a * (1.0 - a) / N), (rate, a)
