"""Per-request seeded sampling (SamplingParams.seed) inside the captured speculative cycle.

A seeded sampled request draws every random number from Philox4x32-10 keyed by (seed, base position, stream, j, v) alone
(include/qspec_hip.h, "seeded draws"), so its tokens do not depend on its slot, on the other requests of the batch or on
the engine's Philox stream.  The device analogue of the reference's tests/samplers/test_rejection_sampler.py
test_deterministic_when_seeded / test_mixed_seeded_batch, plus the key layout pinned against a numpy Philox."""
import numpy as np
import pytest
import torch

from philox_ref import philox_r0, seeded_r0  # noqa: F401  (numpy Philox4x32-10, shared with the engine-stream tests)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M32 = 0xFFFFFFFF


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from qspec_amd import ops
    return ops


def _sample(ops, logits, temp, top_k, top_p, rng_state, seeds=None, seeded=None, base=None, rows_per_seq=1, j_base=0,
            draw_stream=2):
    T, V = logits.shape
    probs = torch.empty(T, V, dtype=torch.float32, device=DEV)
    tok = torch.empty(T, dtype=torch.int64, device=DEV)
    rs = torch.tensor(rng_state, dtype=torch.int64, device=DEV)
    kw = {}
    if seeds is not None:
        kw = dict(seq_seeds=dev(np.asarray(seeds, np.int64)), seq_seeded=dev(np.asarray(seeded, np.int32)),
                  base_pos=dev(np.asarray(base, np.int32)), rows_per_seq=rows_per_seq, j_base=j_base, draw_stream=draw_stream)
    ops.sample_top_k_top_p(dev(logits), probs, tok, dev(np.asarray(temp, np.float32)), dev(np.asarray(top_k, np.int32)),
                           dev(np.asarray(top_p, np.float32)), rng_state=rs, workspace=ops.new_sample_workspace(T, DEV), **kw)
    torch.cuda.synchronize()
    return host(probs), host(tok), host(rs)


def _reject(ops, tq, dp, ids, bonus, rng_state, seeds=None, seeded=None, base=None):
    B, k, V = dp.shape
    out = torch.empty(B, k + 1, dtype=torch.int64, device=DEV)
    acc = torch.empty(B, k, dtype=torch.uint8, device=DEV)
    rec = torch.empty(B, k, dtype=torch.int64, device=DEV)
    rs = torch.tensor(rng_state, dtype=torch.int64, device=DEV)
    kw = {}
    if seeds is not None:
        kw = dict(seq_seeds=dev(np.asarray(seeds, np.int64)), seq_seeded=dev(np.asarray(seeded, np.int32)),
                  base_pos=dev(np.asarray(base, np.int32)))
    ops.rejection_sample(dev(tq), dev(bonus.astype(np.int64)), dev(dp), dev(ids.astype(np.int64)), out, acc, rec, None,
                         rng_state=rs, **kw)
    torch.cuda.synchronize()
    return host(out), host(acc), host(rec), host(rs)


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _f64(p):
    p = np.asarray(p, np.float64)
    return p / p.sum()


def _rej_inputs(rng, B, k, V):
    tq = _softmax(rng.normal(0, 2, (B, k + 1, V)))
    dp = _softmax(rng.normal(0, 2, (B, k, V)))
    ids = np.stack([[rng.choice(V, p=_f64(dp[b, i])) for i in range(k)] for b in range(B)])
    bonus = rng.integers(0, V, B)
    return tq, dp, ids, bonus


# ------------------------------------------------------------------ 1. kernel invariance

def test_seeded_sample_row_independent_of_slot_batch_and_rng_state(ops):
    rng = np.random.default_rng(0)
    V = 4096
    L = (rng.normal(0, 3, V)).astype(np.float16)
    p1, t1, _ = _sample(ops, L[None], [0.8], [50], [0.9], [5, 3], seeds=[1234], seeded=[1], base=[77])
    lg = (rng.normal(0, 3, (8, V))).astype(np.float16)
    lg[5] = L
    temp = [0.0, 1.0, 1.0, 0.7, 1.1, 0.8, 0.9, 1.3]
    topk = [-1, -1, 20, 40, -1, 50, 10, -1]
    topp = [1.0, 0.95, 1.0, 0.9, 0.8, 0.9, 1.0, 0.7]
    seeds = [1234, 7, 8, 99, 2 ** 40 + 5, 1234, 1235, -3]
    seeded = [0, 0, 0, 1, 1, 1, 1, 1]
    base = [77, 77, 3, 77, 12, 77, 77, 78]
    p8, t8, _ = _sample(ops, lg, temp, topk, topp, [9, 11], seeds=seeds, seeded=seeded, base=base)
    assert np.array_equal(p1[0], p8[5]) and t1[0] == t8[5]
    # rows_per_seq: row 3 of a [4 sequences x 2 rows] call is sequence 1 at j = j_base + 1
    lg2 = (rng.normal(0, 3, (8, V))).astype(np.float16)
    lg2[3] = L
    p2, t2, _ = _sample(ops, lg2, [0.8] * 8, [50] * 8, [0.9] * 8, [1, 2], seeds=[5, 1234, 6, 7], seeded=[1, 1, 0, 1],
                        base=[1, 77, 2, 3], rows_per_seq=2, j_base=4, draw_stream=1)
    p1b, t1b, _ = _sample(ops, L[None], [0.8], [50], [0.9], [4, 4], seeds=[1234], seeded=[1], base=[77], j_base=5,
                          draw_stream=1)
    assert np.array_equal(p2[3], p1b[0]) and t2[3] == t1b[0]


def test_seeded_rejection_row_independent_of_slot_batch_and_rng_state(ops):
    rng = np.random.default_rng(1)
    k, V = 3, 2048
    tq, dp, ids, bonus = _rej_inputs(rng, 8, k, V)
    o1, a1, r1, _ = _reject(ops, tq[5:6], dp[5:6], ids[5:6], bonus[5:6], [3, 0], seeds=[42], seeded=[1], base=[100])
    o8, a8, r8, _ = _reject(ops, tq, dp, ids, bonus, [8, 21], seeds=[1, 2, 3, 4, 5, 42, 43, 44],
                            seeded=[0, 1, 0, 1, 1, 1, 0, 1], base=[100, 100, 5, 6, 101, 100, 100, 99])
    assert np.array_equal(o1[0], o8[5]) and np.array_equal(a1[0], a8[5]) and np.array_equal(r1[0], r8[5])


def test_seeds_and_base_positions_change_the_draws(ops):
    """Over many rows (not asserted for any single one): another seed or another base position, other tokens."""
    rng = np.random.default_rng(2)
    T, V = 256, 4096
    lg = np.tile(rng.normal(0, 1, V).astype(np.float16), (T, 1))
    ones = [1] * T
    _, ta, _ = _sample(ops, lg, [1.0] * T, [-1] * T, [1.0] * T, [0, 0], seeds=range(T), seeded=ones, base=[10] * T)
    _, tb, _ = _sample(ops, lg, [1.0] * T, [-1] * T, [1.0] * T, [0, 0], seeds=range(T, 2 * T), seeded=ones, base=[10] * T)
    _, tc, _ = _sample(ops, lg, [1.0] * T, [-1] * T, [1.0] * T, [0, 0], seeds=range(T), seeded=ones, base=[11] * T)
    _, ta2, _ = _sample(ops, lg, [1.0] * T, [-1] * T, [1.0] * T, [7, 7], seeds=range(T), seeded=ones, base=[10] * T)
    assert np.array_equal(ta, ta2)
    assert (ta != tb).mean() > 0.9 and (ta != tc).mean() > 0.9
    assert len(set(ta.tolist())) > T // 2          # distinct seeds of one distribution: spread out
    k = 2
    tq, dp, ids, bonus = _rej_inputs(rng, 128, k, 256)
    ra = _reject(ops, tq, dp, ids, bonus, [0, 0], seeds=range(128), seeded=[1] * 128, base=[10] * 128)
    rb = _reject(ops, tq, dp, ids, bonus, [0, 0], seeds=range(128, 256), seeded=[1] * 128, base=[10] * 128)
    rc = _reject(ops, tq, dp, ids, bonus, [0, 0], seeds=range(128), seeded=[1] * 128, base=[11] * 128)
    assert (ra[2] != rb[2]).mean() > 0.5 and (ra[2] != rc[2]).mean() > 0.5      # recovered tokens
    assert (ra[1] != rb[1]).any() and (ra[1] != rc[1]).any()                      # accept decisions


# ------------------------------------------------------------------ 2. unseeded rows unchanged

def test_unseeded_rows_are_bit_identical_to_the_existing_entries(ops):
    rng = np.random.default_rng(3)
    T, V = 8, 4096
    lg = (rng.normal(0, 3, (T, V))).astype(np.float16)
    temp = [0.0, 1.0, 0.8, 0.7, 1.1, 0.8, 0.9, 1.3]
    topk, topp = [-1, -1, 20, 40, -1, 50, 10, -1], [1.0, 0.95, 1.0, 0.9, 0.8, 0.9, 1.0, 0.7]
    p_old, t_old, s_old = _sample(ops, lg, temp, topk, topp, [17, 4])
    p_off, t_off, s_off = _sample(ops, lg, temp, topk, topp, [17, 4], seeds=range(T), seeded=[0] * T, base=[9] * T)
    assert np.array_equal(p_old, p_off) and np.array_equal(t_old, t_off) and np.array_equal(s_old, s_off)
    assert s_old.tolist() == [17, 5]
    mixed = [0, 0, 1, 0, 1, 0, 0, 1]
    p_mix, t_mix, s_mix = _sample(ops, lg, temp, topk, topp, [17, 4], seeds=range(T), seeded=mixed, base=[9] * T)
    assert np.array_equal(p_old, p_mix) and np.array_equal(s_old, s_mix)
    off = np.array(mixed) == 0
    assert np.array_equal(t_old[off], t_mix[off])

    B, k = 8, 3
    tq, dp, ids, bonus = _rej_inputs(rng, B, k, 1024)
    old = _reject(ops, tq, dp, ids, bonus, [23, 6])
    allz = _reject(ops, tq, dp, ids, bonus, [23, 6], seeds=range(B), seeded=[0] * B, base=[50] * B)
    for a, b in zip(old, allz):
        assert np.array_equal(a, b)
    assert old[3].tolist() == [23, 7]
    mix = _reject(ops, tq, dp, ids, bonus, [23, 6], seeds=range(B), seeded=mixed, base=[50] * B)
    for a, b in zip(old[:3], mix[:3]):
        assert np.array_equal(a[off], b[off])
    assert np.array_equal(old[3], mix[3])


# ------------------------------------------------------------------ 3. key layout pinned against numpy Philox

def test_rejection_uniform_key_layout(ops):
    """accepted = u < q[x] / p[x] with a one-hot draft (p[x] = 1): a threshold of exactly u rejects, the next float
    above u accepts -- which pins u = (r0 >> 8) / 2^24 of stream 4, c0 = 0xFFFFFFFF, bit for bit."""
    B, k, V = 64, 3, 64
    rng = np.random.default_rng(4)
    seeds = rng.integers(-2 ** 63, 2 ** 63 - 1, B, dtype=np.int64)
    base = rng.integers(1, 2 ** 31 - 1, B).astype(np.int32)
    ids = rng.integers(0, V, (B, k))
    i = np.arange(k)[None, :]
    r0 = seeded_r0(0xFFFFFFFF, seeds.view(np.uint64)[:, None], base[:, None].astype(np.uint64), 4, i)
    u = (r0 >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    acc_want = rng.integers(0, 2, (B, k)).astype(bool) & (u > 0)
    thr = np.where(acc_want, np.nextafter(u, np.float32(2)), u).astype(np.float32)
    dp = np.zeros((B, k, V), np.float32)
    np.put_along_axis(dp, ids[..., None], 1.0, -1)
    tq = np.full((B, k + 1, V), 0.01, np.float32)
    np.put_along_axis(tq[:, :k], ids[..., None], thr[..., None], -1)
    _, acc, _, _ = _reject(ops, tq, dp, ids, rng.integers(0, V, B), [0, 0], seeds=seeds, seeded=[1] * B, base=base)
    assert np.array_equal(acc.astype(bool), acc_want)


def test_sampled_token_key_layout(ops):
    """token = argmax_v p_v / -log(u_v), u_v = ((r0 >> 8) + 0.5) / 2^24 of stream 1 / 2, c0 = v, j = j_base + t % rows_per_seq
    (rows whose top-2 relative gap is < 1e-3 are skipped: the kernel's log is __logf)."""
    rng = np.random.default_rng(5)
    nseq, rps, V = 64, 2, 512
    T = nseq * rps
    lg = rng.normal(0, 1, (T, V)).astype(np.float16)
    seeds = rng.integers(0, 2 ** 63 - 1, nseq, dtype=np.int64)
    base = rng.integers(1, 100000, nseq).astype(np.int32)
    checked = 0
    for stream, j_base in ((1, 3), (2, 0)):
        probs, tok, _ = _sample(ops, lg, [1.0] * T, [-1] * T, [1.0] * T, [0, 0], seeds=seeds, seeded=[1] * nseq, base=base,
                                rows_per_seq=rps, j_base=j_base, draw_stream=stream)
        t = np.arange(T)
        r0 = seeded_r0(np.arange(V)[None, :], seeds.view(np.uint64)[t // rps, None], base[t // rps, None].astype(np.uint64),
                       stream, (j_base + t % rps)[:, None])
        uo = ((r0 >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
        val = probs.astype(np.float64) / -np.log(uo)
        top2 = np.sort(val, -1)[:, -2:]
        ok = (top2[:, 1] - top2[:, 0]) / top2[:, 1] >= 1e-3
        assert ok.mean() > 0.9
        assert np.array_equal(tok[ok], val.argmax(-1)[ok])
        checked += ok.sum()
    assert checked > T


# ------------------------------------------------------------------ 4. distributions over thousands of seeds

def _tv_bound(p, n):
    return 3.0 * 0.5 * np.sqrt(p / n).sum() + 1e-3


def test_seeded_sampler_distribution(ops):
    """One processed distribution (temperature, top-k, top-p), 4096 distinct seeds: the token histogram matches probs."""
    rng = np.random.default_rng(6)
    V, R, calls = 64, 512, 8
    L = rng.normal(0, 1.5, V).astype(np.float16)
    lg = np.tile(L, (R, 1))
    counts, probs = np.zeros(V), None
    for c in range(calls):
        p, tok, _ = _sample(ops, lg, [0.9] * R, [20] * R, [0.95] * R, [c, 0], seeds=np.arange(R) + c * R + 1000,
                            seeded=[1] * R, base=[33] * R)
        probs = p[0].astype(np.float64)
        assert np.array_equal(p, np.tile(p[0], (R, 1)))
        counts += np.bincount(tok, minlength=V)
    n = R * calls
    assert (counts[probs == 0] == 0).all()
    assert (probs > 0).sum() <= 20
    tv = 0.5 * np.abs(counts / n - probs).sum()
    assert tv < _tv_bound(probs, n), tv


@pytest.mark.parametrize("form", ["one_hot", "dense"])
def test_seeded_rejection_sampler_distribution(ops, form):
    """The emitted token at position 0 follows the target distribution whatever the draft (one-hot or dense draft
    distribution with the draft token drawn from it): the reference's approximation test, one seed per sequence."""
    rng = np.random.default_rng(7)
    N, k, V = 4096, 1, 16
    q = _softmax(rng.normal(0, 1, V))
    tq = np.tile(q, (N, k + 1, 1))
    if form == "one_hot":
        ids = rng.integers(0, V, (N, k))
        dp = np.zeros((N, k, V), np.float32)
        np.put_along_axis(dp, ids[..., None], 1.0, -1)
    else:
        p = _softmax(rng.normal(0, 1, V))
        dp = np.tile(p, (N, k, 1))
        ids = rng.choice(V, (N, k), p=_f64(p))
    out, _, _, _ = _reject(ops, tq, dp, ids, rng.integers(0, V, N), [0, 0], seeds=np.arange(N) * 7919 + 11,
                           seeded=[1] * N, base=[64] * N)
    counts = np.bincount(out[:, 0], minlength=V)
    tv = 0.5 * np.abs(counts / N - q.astype(np.float64)).sum()
    assert tv < _tv_bound(q.astype(np.float64), N), tv


# ------------------------------------------------------------------ 5. engine

def _tiny():
    from qspec_amd.model import QuarotLlamaConfig, QuarotLlamaForCausalLM
    cfg = QuarotLlamaConfig(1024, 3584, 8, 2, 2, 2048, 1e-5, 10000.0, 512, "tiny")
    return QuarotLlamaForCausalLM(cfg, DEV).init_synthetic(seed=1, lm_head_std=0.05)


@pytest.fixture(scope="module")
def tiny():
    assert torch.cuda.is_available()
    return _tiny()


SEEDED = dict(temperature=0.8, top_k=50, top_p=0.9, seed=20261016)


def _layouts(tiny, use_graph, prompts, seeded=SEEDED):
    """The seeded request alone in slot 0 (engine seed 0), and in slot 2 beside a greedy, an unseeded sampled and an
    otherwise-seeded request (engine seed 7, admitted in between)."""
    from qspec_amd.spec_decode import QSpecEngine
    a = QSpecEngine(tiny, 3, 4, max_model_len=256, block_size=16, max_new_tokens=64, use_graph=use_graph, seed=0)
    a.set_sampling_params(0, **seeded)
    a.add_sequence(0, prompts[0])
    b = QSpecEngine(tiny, 3, 4, max_model_len=256, block_size=16, max_new_tokens=64, use_graph=use_graph, seed=7)
    b.set_sampling_params(1, temperature=1.0)
    b.add_sequence(1, prompts[1])
    b.add_sequence(0, prompts[2])                         # greedy
    b.set_sampling_params(2, **seeded)
    b.add_sequence(2, prompts[0])
    b.set_sampling_params(3, temperature=0.7, top_k=20, seed=99)
    b.add_sequence(3, prompts[3])
    return (a, 0), (b, 2)


def _prompts(tiny):
    rng = np.random.default_rng(31)
    return [rng.integers(0, tiny.config.vocab_size, n).tolist() for n in (21, 30, 9, 44)]


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_seeded_request_independent_of_slot_and_neighbours(tiny, use_graph):
    prompts = _prompts(tiny)
    (a, sa), (b, sb) = _layouts(tiny, use_graph, prompts)
    for _ in range(4):
        a.step(); b.step()
    ga, gb = a.generated()[sa], b.generated()[sb]
    assert len(ga) >= 5 and ga == gb
    assert b._mode_sampling and (not use_graph or (b._graph_s is not None and b._graph is None))
    # a new seed between replays: no re-capture, and the other layout follows it
    graph = b._graph_s
    b.set_sampling_params(sb, **{**SEEDED, "seed": 5}); a.set_sampling_params(sa, **{**SEEDED, "seed": 5})
    a.step(); b.step()
    assert b._graph_s is graph
    assert a.generated()[sa] == b.generated()[sb]
    # recover(): the last cycle re-run from its snapshot repeats the same draws
    before = b.generated()[sb]
    b.recover()
    assert b.generated()[sb] == before


def test_engine_seeded_graph_equals_eager(tiny):
    prompts = _prompts(tiny)
    gens = []
    for use_graph in (False, True):
        (a, sa), _ = _layouts(tiny, use_graph, prompts)
        for _ in range(4):
            a.step()
        gens.append(a.generated()[sa])
    assert gens[0] == gens[1]


def test_step_no_spec_samples_with_the_seed(tiny):
    prompts = _prompts(tiny)
    (a, sa), (b, sb) = _layouts(tiny, False, prompts)
    for _ in range(3):
        a.step_no_spec(); b.step_no_spec()
    assert a.generated()[sa] == b.generated()[sb] and len(a.generated()[sa]) == 4
    assert len(b.generated()[0]) == 4                                           # the greedy neighbour stepped too
    # the step samples: some seed takes a non-argmax token (temperature 1, no top-k / top-p)
    from qspec_amd.spec_decode import QSpecEngine
    eng = QSpecEngine(tiny, 3, 4, max_model_len=256, block_size=16, max_new_tokens=64, use_graph=False, seed=0)
    non_argmax = 0
    for seed in range(6):
        eng.set_sampling_params(1, temperature=1.0, seed=seed)
        eng.add_sequence(1, prompts[1])
        for _ in range(2):
            eng.step_no_spec()
            torch.cuda.synchronize()
            non_argmax += int(eng.draft_ids_kb[0, 1]) != int(eng.draft_probs_kbv[0, 1].argmax())
        eng.free_slot(1)
        assert int(eng.seq_seeded[1]) == 0
    assert non_argmax > 0


# ------------------------------------------------------------------ 6. worker

def test_worker_seeded_request_same_tokens_in_another_batch(tiny):
    from qspec_amd.spec_decode import ExecuteModelRequest, SequenceGroupMetadata, create_spec_worker
    from qspec_amd.spec_decode.worker import SamplingParams, SequenceData, SpeculativeConfig
    prompts = _prompts(tiny)
    target = SamplingParams(seed=777, temperature=0.8, top_k=50, top_p=0.9)
    layouts = [
        [("s", prompts[0], target)],
        [("g", prompts[2], SamplingParams()), ("u", prompts[1], SamplingParams(temperature=1.0)),
         ("s", prompts[0], target), ("o", prompts[3], SamplingParams(seed=3, temperature=0.7))],
    ]
    results = []
    for li, layout in enumerate(layouts):
        w = create_spec_worker(model_config=tiny.config, model=tiny, speculative_config=SpeculativeConfig(3),
                               max_num_seqs=4, max_model_len=256, block_size=16, device=DEV, seed=li * 13)
        w.init_device()
        w.initialize_cache(64, 0)
        sgs, toks = [], []
        for rid, prompt, sp in layout:              # one prompt pass per request
            sg = SequenceGroupMetadata(rid, True, {len(sgs): SequenceData(list(prompt))}, sampling_params=sp)
            out = w.execute_model(ExecuteModelRequest([sg], num_lookahead_slots=0))
            if rid == "s":
                toks.append(out[0].token_ids()[0])
            sg.is_prompt = False
            sgs.append(sg)
        pos = [s.request_id for s in sgs].index("s")
        for _ in range(3):
            outs = w.execute_model(ExecuteModelRequest(sgs, num_lookahead_slots=3))
            toks += [t for t in (o.token_ids()[pos] for o in outs) if t != -1]
        results.append(toks)
    assert len(results[0]) >= 4 and results[0] == results[1]
