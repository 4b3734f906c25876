"""Prompt passes behind a context that is already in the paged cache, through the engine and the worker on the tiny model:
chunked prefill, prefix-cache hits (shared blocks stay byte-identical), the full hit, a prefilling slot that is inert in the
captured cycle, prompt logprobs gathered over chunks, the fp8 cache, and scheduler-shaped requests with a prompt chunk inside
a speculative step.  Block tables are brought by the tests (the cache has fewer blocks than slots x max_model_len)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import logprob_cases as lc
from test_model_gpu import _rel3, _w4a16_noise_floor, tiny  # noqa: F401  (tiny: the module-scoped model fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BS, NB = 16, 60
RNG = np.random.default_rng(2024)
A = RNG.integers(0, 2048, 100).tolist()                 # the running request
B = A[:64] + RNG.integers(0, 2048, 41).tolist()          # shares 64 tokens = 4 blocks with it
LONG = RNG.integers(0, 2048, 150).tolist()
T_A, T_B, T_LONG = list(range(0, 8)), list(range(0, 4)) + list(range(20, 27)), list(range(30, 42))


def make_engine(model, use_graph=False, **kw):
    from qspec_amd.spec_decode.engine import QSpecEngine
    return QSpecEngine(model, 3, 4, max_model_len=256, block_size=BS, max_new_tokens=64, use_graph=use_graph, seed=3,
                       num_blocks=NB, **kw)


def spy_first(eng):
    """The hidden rows the engine samples first tokens from, in call order."""
    seen, inner = [], eng._first_token

    def spy(hs, *a, **kw):
        seen.append(hs.clone())
        return inner(hs, *a, **kw)
    eng._first_token = spy
    return seen


class ForwardRows:
    """Rows per model.forward call while active (wrapped on the instance, removed again)."""

    def __init__(self, model):
        self.model, self.rows, self.splits = model, [], []      # splits: the context splits of each call's attention

    def __enter__(self):
        inner = self.model.forward

        def spy(ids, pos, kv, md, *a, **kw):
            self.rows.append(ids.numel())
            self.splits.append(md.n_splits)
            return inner(ids, pos, kv, md, *a, **kw)
        self.model.forward = spy
        return self.rows

    def __exit__(self, *exc):
        del self.model.forward


@pytest.fixture(scope="module")
def refs(tiny):
    """OracleModel.forward over the whole prompts (computed once, read only): prompt -> (hidden [T, H], kv per layer, inp)."""
    from oracle.model import OracleModel
    om = OracleModel.from_torch_model(tiny, BS)
    cfg, out = tiny.config, {}
    for name, toks, table in (("long", LONG, T_LONG), ("b", B, T_B)):
        T = len(toks)
        bt = np.zeros((1, 16), np.int32)
        bt[0, :len(table)] = table
        pos = np.arange(T, dtype=np.int64)
        kv = [(np.zeros((NB, BS, cfg.num_key_value_heads, cfg.head_dim), np.float16),) * 2 for _ in range(cfg.num_hidden_layers)]
        inp = dict(ids=np.asarray(toks, np.int64), pos=pos, slots=bt[0, pos // BS].astype(np.int64) * BS + pos % BS, bt=bt,
                   ctx=np.array([T], np.int32), q_start=np.array([0, T], np.int32), kv_np=kv)
        kv_ref = [(k.copy(), v.copy()) for k, v in kv]
        ref = om.forward(inp["ids"], inp["pos"], kv_ref, inp["slots"], inp["bt"], inp["ctx"], inp["q_start"], False)
        floor = _w4a16_noise_floor(om, inp, ref)
        om.w4a16_f32acc = True
        try:                                             # the same floor for the K/V the forward writes
            kv2 = [(k.copy(), v.copy()) for k, v in kv]
            om.forward(inp["ids"], inp["pos"], kv2, inp["slots"], inp["bt"], inp["ctx"], inp["q_start"], False)
        finally:
            om.w4a16_f32acc = False
        out[name] = SimpleNamespace(hidden=ref, floor=floor, kv=kv_ref, kv2=kv2, logits=om.logits(ref[-1:]), inp=inp)
    return out


def within_floor(got, ref, floor, what):
    """The bars of test_model_gpu.test_forward_matches_oracle_model: against the noise floor of the comparison.  The floor is
    taken over ALL rows of the prompt, as there: over the 1024 values of one row its quantiles move by a factor of two from
    prompt to prompt (1.95 at the last row of B, 3.61 at that of LONG) while the whole-prompt HIP pass sits at 3.5 on either."""
    rel = _rel3(got, ref)
    print(f"{what}, err / 1e-3: max {rel.max():.2f} q99 {np.quantile(rel, 0.99):.2f}; floor max {floor.max():.2f} "
          f"q99 {np.quantile(floor, 0.99):.2f}")
    assert np.quantile(rel, 0.99) < max(1.5 * np.quantile(floor, 0.99), 2.0) and rel.max() < max(2.0 * floor.max(), 4.0), \
        (what, np.quantile(rel, 0.99), np.quantile(floor, 0.99), rel.max(), floor.max())
    return rel


def kv_rows(eng, table, T):
    """K and V of positions 0 .. T-1 of a request, per layer, as float64 [T, nkv, d]."""
    pos = np.arange(T)
    blk, off = torch.tensor(np.asarray(table)[pos // BS]), torch.tensor(pos % BS)
    return [(k[blk, off].cpu().numpy().astype(np.float64), v[blk, off].cpu().numpy().astype(np.float64)) for k, v in eng.kv_caches]


def ref_kv_rows(kv, table, T):
    pos = np.arange(T)
    blk, off = np.asarray(table)[pos // BS], pos % BS
    return [(k[blk, off].astype(np.float64), v[blk, off].astype(np.float64)) for k, v in kv]


def run_cycles(eng, n, slots):
    emitted = np.zeros(eng.B, np.int64)
    for _ in range(n):
        eng.step()
        out, err = eng.read_outputs()
        assert err == 0
        count = (out != -1).sum(1)
        eng.note_emitted(count.tolist())
        emitted += count.numpy()
    assert all(emitted[b] >= n for b in slots) and all(emitted[b] == 0 for b in range(eng.B) if b not in slots), emitted
    return emitted


def chunked(eng, slot, toks, table, sizes, **kw):
    c = 0
    for q in sizes:
        eng.add_sequence(slot, toks, table, num_computed_tokens=c, token_chunk_size=q, **kw)
        c += q
        assert eng.is_prefilling(slot) == (c < len(toks)) and int(eng.seq_lens[slot]) == (0 if c < len(toks) else len(toks) + 1)


@pytest.mark.parametrize("kmin,splits", [(None, [1, 1, 1]), (64, [1, 2, 3])], ids=["unsplit", "context-splits"])
def test_chunked_prefill_matches_the_oracle_over_the_whole_prompt(tiny, refs, monkeypatch, kmin, splits):
    """kmin 64: the contexts of the tiny model (max_position_embeddings 512) never reach the measured Kmin, so the split rule is
    given a short one: the second chunk (64 tokens x group 4 = 256 rows behind 64 keys, S = 2) then runs the context-split
    prompt kernel and its merge launch, the third (88 rows behind 128 keys, S = 3) the 16-row kernels over three splits."""
    from qspec_amd.spec_decode import engine as E
    if kmin is not None:
        monkeypatch.setattr(E, "PREFILL_SPLIT_MIN_KEYS", kmin)
    r = refs["long"]
    whole = make_engine(tiny)
    seen_w = spy_first(whole)
    whole.add_sequence(0, LONG, T_LONG)
    eng = make_engine(tiny)
    seen = spy_first(eng)
    fr = ForwardRows(tiny)
    with fr as rows:
        chunked(eng, 0, LONG, T_LONG, (64, 64, 22))
    assert rows == [64, 64, 22] and fr.splits == splits and len(seen) == 1 and seen[0].shape[0] == 1
    rel_w = _rel3(seen_w[0].cpu().numpy(), r.hidden[-1:])
    print(f"whole-prompt HIP pass, err / 1e-3: max {rel_w.max():.2f} q99 {np.quantile(rel_w, 0.99):.2f}")
    within_floor(seen[0].cpu().numpy(), r.hidden[-1:], r.floor, "chunked 64/64/22, last hidden row")
    holder = SimpleNamespace(logits=torch.empty(1, tiny.config.vocab_size, dtype=torch.float16, device=DEV))
    logits = tiny.compute_logits(seen[0], holder).cpu().numpy().astype(np.float64)
    assert np.quantile(np.abs(logits - r.logits.astype(np.float64)), 0.99) < 3e-2
    assert int(eng.gen_tokens[0, 0]) == int(whole.gen_tokens[0, 0]) or np.sort(logits[0])[-1] - np.sort(logits[0])[-2] < 6e-2
    for li, ((k, v), (rk, rv), (fk, fv)) in enumerate(zip(kv_rows(eng, T_LONG, 150), ref_kv_rows(r.kv, T_LONG, 150),
                                                          ref_kv_rows(r.kv2, T_LONG, 150))):
        within_floor(k, rk, _rel3(fk, rk), f"layer {li} K of the 150 tokens")
        within_floor(v, rv, _rel3(fv, rv), f"layer {li} V of the 150 tokens")
    assert eng.active_slots() == [0] and eng.n_active == 1
    run_cycles(eng, 2, [0])


def prefix_hit(tiny, refs, **kw):
    eng = make_engine(tiny, **kw)
    eng.add_sequence(0, A, T_A)
    shared = [(k[:4].clone(), v[:4].clone()) for k, v in eng.kv_caches]
    seen = spy_first(eng)
    with ForwardRows(tiny) as rows:
        eng.add_sequence(1, B, T_B, num_computed_tokens=64)
    assert rows == [len(B) - 64]
    for (k, v), (k0, v0) in zip(eng.kv_caches, shared):
        assert torch.equal(k[:4], k0) and torch.equal(v[:4], v0)          # byte-identical in every layer
    assert int(eng.seq_lens[1]) == len(B) + 1 and 0 <= int(eng.gen_tokens[1, 0]) < 2048
    hidden = seen[0].cpu().numpy()
    assert np.isfinite(hidden).all()
    run_cycles(eng, 3, [0, 1])
    return hidden


def test_prefix_hit_computes_the_rest_and_leaves_the_shared_blocks(tiny, refs):
    whole = make_engine(tiny)
    seen_w = spy_first(whole)
    whole.add_sequence(1, B, T_B)
    rel_w = _rel3(seen_w[0].cpu().numpy(), refs["b"].hidden[-1:])
    print(f"whole-prompt HIP pass, err / 1e-3: max {rel_w.max():.2f} q99 {np.quantile(rel_w, 0.99):.2f}")
    hidden = prefix_hit(tiny, refs)
    within_floor(hidden, refs["b"].hidden[-1:], refs["b"].floor, "64-token hit, last hidden row")


def test_full_hit_computes_one_row(tiny):
    eng = make_engine(tiny)
    eng.add_sequence(0, A, T_A)
    with ForwardRows(tiny) as rows:
        eng.add_sequence(2, A[:64], T_A[:4] + [50], num_computed_tokens=64)
    assert rows == [1]
    assert int(eng.seq_lens[2]) == 65 and int(eng.gen_lens[2]) == 1 and 0 <= int(eng.gen_tokens[2, 0]) < 2048
    run_cycles(eng, 1, [0, 2])


def test_a_prefilling_slot_is_inert_in_the_captured_cycle(tiny):
    alone = make_engine(tiny, use_graph=True)
    alone.add_sequence(0, A, T_A)
    for _ in range(3):
        alone.step()
    want = alone.generated()[0]
    eng = make_engine(tiny, use_graph=True)
    eng.add_sequence(0, A, T_A)
    eng.add_sequence(1, LONG, T_LONG, token_chunk_size=64)
    graphs = None
    for i in range(3):
        eng.step()
        graphs = dict(eng._graphs) if graphs is None else graphs
        if i == 1:
            eng.add_sequence(1, LONG, T_LONG, num_computed_tokens=64, token_chunk_size=64)   # between replays
            eng.sync_lens()
            assert eng.is_prefilling(1)
    assert eng.generated()[0] == want and eng.generated()[1] == [] and int(eng.seq_lens[1]) == 0
    with pytest.raises(ValueError):
        eng.step(participants=[0, 1])
    eng.add_sequence(1, LONG, T_LONG, num_computed_tokens=128)
    eng.sync_lens()
    before = [len(g) for g in eng.generated()]
    eng.step()
    after = [len(g) for g in eng.generated()]
    assert after[0] > before[0] and before[1] == 1 and after[1] > 1
    assert eng._graphs == graphs                                           # nothing was captured again


def check_prompt_logprobs(tiny, eng, slot, toks, seen, n):
    lp, rank, top, tlp = eng.take_prompt_logprobs(slot)
    assert eng.take_prompt_logprobs(slot) is None
    T, V = len(toks), tiny.config.vocab_size
    assert lp.shape == (T - 1,) and rank.shape == (T - 1,) and top.shape == (T - 1, n) and tlp.shape == (T - 1, n)
    holder = SimpleNamespace(logits=torch.empty(256, V, dtype=torch.float16, device=DEV))
    logits = torch.cat([tiny.compute_logits(h, holder)[:h.shape[0]].clone() for h in seen])
    assert logits.shape[0] == T - 1
    ref = lc.ref_token_logprobs(logits.cpu().numpy(), np.asarray(toks[1:]), n, "logits")
    assert lc.compare(lc.Result(lp.numpy(), rank.numpy(), top.numpy(), tlp.numpy()), ref, "logits") == []
    want = torch.log_softmax(logits.double(), dim=-1).cpu()
    assert torch.allclose(lp.double(), want.gather(-1, torch.tensor(toks[1:]).unsqueeze(-1)).squeeze(-1), rtol=0, atol=1e-4)


def spy_prompt_logits(eng):
    seen, inner = [], eng._prompt_logits

    def spy(hs):
        seen.append(hs.clone())
        return inner(hs)
    eng._prompt_logits = spy
    return seen


def test_prompt_logprobs_over_three_chunks_and_behind_a_hit(tiny):
    eng = make_engine(tiny)
    seen = spy_prompt_logits(eng)
    with ForwardRows(tiny) as rows:
        c = 0
        for q in (64, 64, 22):
            assert eng.take_prompt_logprobs(0) is None                  # handed over once, after the last chunk
            eng.add_sequence(0, LONG, T_LONG, num_computed_tokens=c, token_chunk_size=q, prompt_logprobs=3)
            c += q
    assert rows == [64, 64, 22] and [h.shape[0] for h in seen] == [64, 64, 21]
    check_prompt_logprobs(tiny, eng, 0, LONG, seen, 3)
    # behind a hit: no saving -- the cached rows are computed again, and nothing is written into the shared blocks
    eng3 = make_engine(tiny)
    eng3.add_sequence(0, A, T_A)
    shared = [(k[:4].clone(), v[:4].clone()) for k, v in eng3.kv_caches]
    seen3 = spy_prompt_logits(eng3)
    with ForwardRows(tiny) as rows:
        eng3.add_sequence(1, B, T_B, num_computed_tokens=64, prompt_logprobs=3)
    assert rows == [len(B)] and [h.shape[0] for h in seen3] == [len(B) - 1]
    for (k, v), (k0, v0) in zip(eng3.kv_caches, shared):
        assert torch.equal(k[:4], k0) and torch.equal(v[:4], v0)
    check_prompt_logprobs(tiny, eng3, 1, B, seen3, 3)


def test_fp8_cache_chunked_prefill_and_prefix_hit(tiny, refs):
    """The fp8 engine path is held to discrete bars in this suite (tests/test_kv_fp8_gpu.py: layout, state, finite values):
    the same here; the distance to the whole-prompt pass over the same cache type is printed."""
    kw = dict(kv_cache_dtype="fp8", kv_scales=[(0.75, 1.5), (1.0, 2.0)])
    whole = make_engine(tiny, **kw)
    seen_w = spy_first(whole)
    whole.add_sequence(0, LONG, T_LONG)
    eng = make_engine(tiny, **kw)
    seen = spy_first(eng)
    with ForwardRows(tiny) as rows:
        chunked(eng, 0, LONG, T_LONG, (64, 64, 22))
    assert rows == [64, 64, 22] and torch.isfinite(seen[0].float()).all()
    assert all(k.dtype == torch.uint8 for k, _ in eng.kv_caches) and any(int(k[30:42].max()) > 0 for k, _ in eng.kv_caches)
    rel = _rel3(seen[0].cpu().numpy(), seen_w[0].cpu().numpy())
    print(f"fp8 chunked vs fp8 whole-prompt HIP pass, err / 1e-3: max {rel.max():.2f} q99 {np.quantile(rel, 0.99):.2f}")
    assert 0 <= int(eng.gen_tokens[0, 0]) < 2048
    run_cycles(eng, 2, [0])
    prefix_hit(tiny, refs, **kw)


def test_worker_chunked_prefill_with_a_prompt_chunk_in_a_speculative_step(tiny):
    from qspec_amd.spec_decode import ExecuteModelRequest, SequenceGroupMetadata, create_spec_worker
    from qspec_amd.spec_decode.worker import SequenceData
    from test_kv_fp8_gpu import _vllm_config
    w = create_spec_worker(vllm_config=_vllm_config("auto"), local_rank=0, rank=0, is_driver_worker=True, device=DEV, model=tiny)
    w.init_device()
    w.initialize_cache(64, 0)
    k = 3
    d0, d1 = SequenceData(A[:20]), SequenceData(LONG)
    r0 = SequenceGroupMetadata("r0", True, {0: d0}, token_chunk_size=20)

    def r1(size, ends):
        return SequenceGroupMetadata("r1", True, {1: d1}, do_sample=ends, token_chunk_size=size)
    out = w.execute_model(ExecuteModelRequest([r1(64, False), r0], num_lookahead_slots=0))
    assert len(out) == 1 and out[0].outputs[0].samples == [] and 0 <= out[0].outputs[1].samples[0].output_token < 2048
    d1.update_num_computed_tokens(64)
    d0.output_token_ids.append(out[0].outputs[1].samples[0].output_token)
    r0.is_prompt = False

    def spec_step(groups):
        outs = w.execute_model(ExecuteModelRequest(groups, num_lookahead_slots=k))
        assert 1 <= len(outs) <= k + 1 and all(len(o.outputs) == len(groups) for o in outs)
        return np.array([o.token_ids() for o in outs]).T               # [groups, steps]
    toks = spec_step([r1(64, False), r0])                              # a prompt chunk inside the speculative step
    assert (toks[0] == -1).all() and toks[1, 0] >= 0 and w.engine.is_prefilling(w._slots["r1"])
    d1.update_num_computed_tokens(64)
    d0.output_token_ids.extend(int(t) for t in toks[1] if t >= 0)
    toks = spec_step([r1(22, True), r0])                               # the chunk that ends the prompt
    assert 0 <= toks[0, 0] < 2048 and (toks[0, 1:] == -1).all() and toks[1, 0] >= 0
    d1.update_num_computed_tokens(22)
    d1.output_token_ids.append(int(toks[0, 0]))
    d0.output_token_ids.extend(int(t) for t in toks[1] if t >= 0)
    toks = spec_step([SequenceGroupMetadata("r1", False, {1: d1}), r0])   # the request decodes on the following step
    assert toks[0, 0] >= 0 and toks[1, 0] >= 0 and (toks < 2048).all()
    assert int(w.engine.seq_lens[w._slots["r1"]]) == 151 + int((toks[0] >= 0).sum())
