"""KV block operations on the GPU: the copy / gather / scatter kernels bit for bit against torch indexing over WHOLE caches of
random bytes (a stray write shows), the engine's swap and fork against undisturbed twins, and a group of n = 3 sampled
sequences through the worker against three single-sequence requests with the derived seeds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYERS, BLOCKS = 2, 24

PAIR_SETS = {
    "one": [(3, 17)],
    # one src feeds three dst; block ids 0 and 23 take part
    "seven": [(0, 10), (0, 11), (0, 23), (1, 12), (2, 13), (22, 14), (4, 15)],
    "nineteen": [(i % 5, 5 + i) for i in range(19)],
}


@pytest.fixture(scope="module")
def ops():
    from qspec_amd import ops as O
    return O


def _caches(block_size, nkv, d, dtype, seed):
    """LAYERS x (K, V) of [BLOCKS, block_size, nkv, d], every byte random."""
    g = torch.Generator().manual_seed(seed)
    elem = torch.empty(0, dtype=dtype).element_size()
    out = []
    for _ in range(2 * LAYERS):
        raw = torch.randint(0, 256, (BLOCKS, block_size, nkv, d * elem), dtype=torch.uint8, generator=g)
        out.append(raw.view(dtype).to(DEV))
    return out[0::2], out[1::2]


def _bytes(caches):
    return [t.contiguous().view(torch.uint8).cpu() for t in caches]


@pytest.mark.parametrize("pairs", list(PAIR_SETS))
@pytest.mark.parametrize("dtype", [torch.float16, torch.uint8])
@pytest.mark.parametrize("nkv,d", [(1, 64), (8, 128)])
@pytest.mark.parametrize("block_size", [8, 16, 32])
def test_copy_blocks_equals_torch_indexing_over_the_whole_cache(ops, block_size, nkv, d, dtype, pairs):
    kc, vc = _caches(block_size, nkv, d, dtype, seed=block_size + nkv)
    want = [t.clone() for t in kc + vc]
    src = torch.tensor([s for s, _ in PAIR_SETS[pairs]], device=DEV)
    dst = torch.tensor([t for _, t in PAIR_SETS[pairs]], device=DEV)
    for t in want:
        t.view(torch.uint8)[dst] = t.view(torch.uint8)[src]
    blocks = ops.KVBlocks(kc, vc)
    assert blocks.block_bytes == block_size * nkv * d * kc[0].element_size() and blocks.num_blocks == BLOCKS
    ops.copy_blocks(blocks, PAIR_SETS[pairs])
    torch.cuda.synchronize()
    for got, ref in zip(_bytes(kc + vc), _bytes(want)):
        assert torch.equal(got, ref)


@pytest.mark.parametrize("dtype", [torch.float16, torch.uint8])
@pytest.mark.parametrize("block_size,nkv,d", [(8, 1, 64), (16, 8, 128), (32, 8, 128)])
def test_gather_gives_contiguous_records_and_scatter_round_trips(ops, block_size, nkv, d, dtype):
    kc, vc = _caches(block_size, nkv, d, dtype, seed=5)
    blocks = ops.KVBlocks(kc, vc)
    ids, onto = [23, 0, 7, 7, 12], [1, 22, 0, 9, 5]                      # (a block may be gathered twice)
    before = _bytes(kc + vc)
    staging = torch.full((len(ids) + 1, blocks.record_bytes), 0xA5, dtype=torch.uint8, device=DEV)
    ops.gather_blocks(blocks, ids, staging)
    torch.cuda.synchronize()
    planes = [t.view(torch.uint8).reshape(BLOCKS, -1) for kv in zip(kc, vc) for t in kv]      # K0, V0, K1, V1
    want = torch.stack([torch.cat([p[b] for p in planes]) for b in ids])                      # [n, layers, 2, block_bytes]
    assert torch.equal(staging[:len(ids)].cpu(), want.cpu())
    assert bool((staging[len(ids)] == 0xA5).all())                        # nothing behind the last record
    for got, ref in zip(_bytes(kc + vc), before):                         # a gather writes no cache byte
        assert torch.equal(got, ref)
    kc2, vc2 = _caches(block_size, nkv, d, dtype, seed=6)
    want2 = [t.clone() for t in kc2 + vc2]
    for t2, t in zip(want2, kc + vc):
        t2.view(torch.uint8)[torch.tensor(onto, device=DEV)] = t.view(torch.uint8)[torch.tensor(ids, device=DEV)]
    ops.scatter_blocks(ops.KVBlocks(kc2, vc2), onto, staging)
    torch.cuda.synchronize()
    for got, ref in zip(_bytes(kc2 + vc2), _bytes(want2)):
        assert torch.equal(got, ref)


def test_no_pairs_enqueue_nothing_bad_pairs_raise_and_the_dispatcher_op_is_the_same(ops):
    import qspec_amd.torch_ops  # noqa: F401
    from qspec_amd import _lib
    kc, vc = _caches(16, 2, 64, torch.float16, seed=9)
    before = _bytes(kc + vc)
    blocks = ops.KVBlocks(kc, vc)
    ops.copy_blocks(blocks, [])
    ops.gather_blocks(blocks, [], None)
    ops.scatter_blocks(blocks, [], None)
    lib = _lib.load()
    for name, extra in (("qspec_copy_blocks", ()), ("qspec_gather_blocks", (None,)), ("qspec_scatter_blocks", (None,))):
        assert getattr(lib, name)(None, LAYERS, None, 0, blocks.block_bytes, *extra, None) == 0   # returns before any launch
    assert lib.qspec_copy_blocks(blocks.layer_ptrs.data_ptr(), LAYERS, None, 0, 24, None) != 0    # block_bytes % 16
    for bad in ([(0, 24)], [(24, 0)], [(0, 1), (2, 1)], [(0, 1), (1, 2)], [(5, 5)]):
        with pytest.raises(ValueError):
            ops.copy_blocks(blocks, bad)
    with pytest.raises(ValueError):
        ops.scatter_blocks(blocks, [3, 3], torch.empty(2, blocks.record_bytes, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.gather_blocks(blocks, [1, 2], torch.empty(1, blocks.record_bytes, dtype=torch.uint8, device=DEV))   # too small
    torch.cuda.synchronize()
    for got, ref in zip(_bytes(kc + vc), before):
        assert torch.equal(got, ref)
    want = [t.clone() for t in kc + vc]
    for t in want:
        t[torch.tensor([20, 21], device=DEV)] = t[torch.tensor([2, 2], device=DEV)]
    torch.ops.qspec.copy_blocks(kc, vc, torch.tensor([[2, 20], [2, 21]]))
    torch.cuda.synchronize()
    for got, ref in zip(_bytes(kc + vc), _bytes(want)):
        assert torch.equal(got, ref)


# ---------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def tiny():
    from qspec_amd.model import QuarotLlamaConfig, QuarotLlamaForCausalLM
    cfg = QuarotLlamaConfig(1024, 3584, 8, 2, 2, 2048, 1e-5, 10000.0, 512, "tiny")
    return QuarotLlamaForCausalLM(cfg, DEV).init_synthetic(seed=1, lm_head_std=0.05)


def _engine(tiny, **kw):
    from qspec_amd.spec_decode import QSpecEngine
    return QSpecEngine(tiny, 3, 4, max_model_len=256, block_size=16, max_new_tokens=64, use_graph=True, seed=0, **kw)


def _prompt(n, seed=31):
    return np.random.default_rng(seed).integers(0, 60, n).tolist()


@pytest.mark.parametrize("kv_cache_dtype", ["auto", "fp8"])
def test_engine_swap_out_and_in_to_other_blocks_changes_no_token(tiny, kv_cache_dtype):
    prompt = _prompt(21)
    twin = _engine(tiny, kv_cache_dtype=kv_cache_dtype)
    twin.add_sequence(0, prompt)
    for _ in range(6):
        twin.step()
    want = twin.generated()[0]

    plain = _engine(tiny, kv_cache_dtype=kv_cache_dtype)
    assert plain.cpu_cache is None and plain._kv_blocks is None and plain._swap_staging is None   # never asked: nothing made
    with pytest.raises(ValueError):
        plain.swap_out([(0, 0)])
    del plain

    eng = _engine(tiny, kv_cache_dtype=kv_cache_dtype, num_cpu_blocks=5)
    record = 2 * 2 * 16 * 2 * 128 * (1 if kv_cache_dtype == "fp8" else 2)
    assert eng.cpu_cache.shape == (5, record) and eng.cpu_cache.dtype == torch.uint8 and eng.cpu_cache.is_pinned()
    eng.add_sequence(0, prompt)
    for _ in range(3):
        eng.step()
    eng.sync_lens()
    used = (eng._len_ub[0] + 15) // 16                                    # blocks 0 .. used-1 of the slot's default range hold KV
    assert 2 <= used <= 3
    for bad in ([(0, 5)], [(eng.num_blocks, 0)], [(0, 1), (1, 1)]):
        with pytest.raises(ValueError):
            eng.swap_out(bad)
    eng.swap_out([(b, 4 - b) for b in range(used)])
    for k, v in eng.kv_caches:                                            # the next tenant scribbles over the blocks
        for t in (k, v):
            raw = t.view(torch.uint8)
            raw[:used] = torch.randint(0, 256, raw[:used].shape, dtype=torch.uint8, device=DEV)
    eng.swap_in([(4 - b, 20 + b) for b in range(used)])
    eng.set_block_table(0, [20, 21, 22, 23])
    for _ in range(3):
        eng.step()
    assert eng.generated()[0] == want
    assert eng._swap_staging.shape[0] == used


def test_engine_fork_after_copy_on_write_emits_the_parents_tokens(tiny):
    """Levels 2 and 3: repetition + frequency penalties and a multi-token bad word cut from the sequence's own plain output.
    The fork's table differs from the parent's in the copied, partially filled block -- and in the still unwritten blocks behind
    it, which a scheduler hands each sequence fresh.  The request is sampled and SEEDED: its draws then depend on (seed, base
    position, stream, j, v) alone, so the fork in another slot repeats them; an unseeded or greedy row takes its rejection
    draws from the engine stream, which is keyed by the row index, and may accept differently in another slot."""
    prompt = _prompt(21)
    plain = _engine(tiny)
    plain.add_sequence(0, prompt)
    for _ in range(5):
        plain.step()
    g = plain.generated()[0]
    kw = dict(temperature=0.8, seed=11, repetition_penalty=1.3, frequency_penalty=0.4, bad_words_token_ids=[g[2:4], g[5:8]])

    twin = _engine(tiny)
    twin.set_sampling_params(0, **kw)
    twin.add_sequence(0, prompt)
    for _ in range(5):
        twin.step()
    want = twin.generated()[0]
    assert want != g                                                      # the processors did something

    eng = _engine(tiny)
    eng.set_sampling_params(0, **kw)
    eng.add_sequence(0, prompt)
    for _ in range(2):
        eng.step()
    eng.sync_lens()
    j = (eng._len_ub[0] - 1) // 16                                        # the block the next cycle writes into
    table = list(range(j)) + [40 + i for i in range(4 - j)]
    eng.copy_blocks([(j, 40)])
    eng.fork_slot(0, 2, table)
    with pytest.raises(ValueError):
        eng.fork_slot(0, 2)                                               # occupied now
    with pytest.raises(ValueError):
        eng.fork_slot(1, 3)                                               # nothing to fork
    for _ in range(3):
        eng.step()
    out = eng.generated()
    assert out[0] == out[2] == want


# ---------------------------------------------------------------------- worker, end to end
def _worker(tiny):
    from qspec_amd.spec_decode import create_spec_worker
    from qspec_amd.spec_decode.worker import SpeculativeConfig
    w = create_spec_worker(model_config=tiny.config, model=tiny, speculative_config=SpeculativeConfig(3), max_num_seqs=4,
                           max_model_len=256, block_size=16, device=DEV, seed=0)
    w.init_device()
    w.initialize_cache(64, 0)
    return w


def _decode_steps(w, sg, toks, steps, **first_step):
    """`steps` speculative steps of the decode group(s) `sg`; toks: seq id -> its tokens so far (extended in place)."""
    from qspec_amd.spec_decode import ExecuteModelRequest
    for i in range(steps):
        outs = w.execute_model(ExecuteModelRequest(sg, num_lookahead_slots=3, **(first_step if i == 0 else {})))
        for pos, s in enumerate(sg):
            for o in outs:
                for sample in o.outputs[pos].samples:
                    if sample.output_token != -1:
                        toks[sample.parent_seq_id].append(sample.output_token)
                        s.seq_data[sample.parent_seq_id].output_token_ids.append(sample.output_token)


def test_group_of_three_samples_equals_three_requests_with_the_derived_seeds(tiny):
    """block_size 16, a 20-token prompt: the samples share block 0 for good and block 1 until their second step, which brings
    each child its own copy of it through blocks_to_copy and its own table -- what vLLM's block manager sends.  Seeded draws
    depend on (seed, base position, stream, j, v) alone, so sample i IS the single request with seed derive(s, i)."""
    from qspec_amd.spec_decode import ExecuteModelRequest, QSpecEngine, SequenceGroupMetadata
    from qspec_amd.spec_decode.worker import SamplingParams, SequenceData
    prompt, s = _prompt(20, seed=4), 1234567
    derive = lambda i: (s + i * QSpecEngine.SAMPLE_SEED_STRIDE) % (1 << 64)   # noqa: E731
    assert QSpecEngine.SAMPLE_SEED_STRIDE == 0x9E3779B97F4A7C15

    # three single-sequence requests: a prompt pass each, then stepped together as one batch of three
    w1 = _worker(tiny)
    want, singles = {}, []
    for i in range(3):
        sg = SequenceGroupMetadata(f"r{i}", True, {i: SequenceData(list(prompt))}, block_tables={i: [3 * i, 3 * i + 1, 3 * i + 2]},
                                   sampling_params=SamplingParams(temperature=1.0, seed=derive(i)))
        out = w1.execute_model(ExecuteModelRequest([sg]))
        want[i] = [out[0].outputs[0].samples[0].output_token]
        sg.seq_data[i].output_token_ids.append(want[i][0])
        sg.is_prompt = False
        singles.append(sg)
    _decode_steps(w1, singles, want, 4)

    # the group: ONE prompt pass, three samples
    w2 = _worker(tiny)
    sp = SamplingParams(temperature=1.0, seed=s, n=3)
    group = SequenceGroupMetadata("g", True, {10: SequenceData(list(prompt))}, block_tables={10: [0, 1]}, sampling_params=sp)
    calls = w2.scorer_calls
    out = w2.execute_model(ExecuteModelRequest([group]))
    assert w2.scorer_calls == calls + 1
    samples = out[0].outputs[0].samples
    assert [x.parent_seq_id for x in samples] == [10, 10, 10]
    first = [x.output_token for x in samples]
    assert first == [want[i][0] for i in range(3)]
    # the scheduler forks: children 11 and 12 in sample order, each with its copy of block 1 and fresh blocks behind it
    got = {10 + i: [first[i]] for i in range(3)}
    tables = {10: [0, 1, 2], 11: [0, 3, 4], 12: [0, 5, 6]}
    step = SequenceGroupMetadata("g", False, {q: SequenceData(list(prompt), [got[q][0]]) for q in (10, 11, 12)},
                                 block_tables=tables, sampling_params=sp)
    _decode_steps(w2, [step], got, 4, blocks_to_copy=[(1, 3), (1, 5)])
    # (samples with equal first tokens are bound in ascending order: the comparison is by sample index either way)
    slots = w2._groups["g"].bound
    for i in range(3):
        seq = next(q for q, b in slots.items() if b == w2._groups["g"].slots[i])
        assert got[seq] == want[i], (i, got[seq], want[i])
    assert len(set(map(tuple, want.values()))) > 1                        # the seeds matter: the samples differ
    w2.execute_model(ExecuteModelRequest([], finished_requests_ids=["g"]))
    assert w2.engine.active_slots() == [] and w2._slots == {}
