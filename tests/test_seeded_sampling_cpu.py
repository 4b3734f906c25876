"""Seeded sampling on the host side (no GPU): the worker forwards SamplingParams.seed to the engine, the C ABI declares,
binds and exports the seeded entries, and the engine keeps its seed arrays in step with the slots."""
import ctypes

import pytest
import torch

from qspec_amd import _lib
from qspec_amd.model import QuarotLlamaConfig
from host_engine import HostEngine
from test_worker_cpu import FakeEngine, fake_memory_probe

from qspec_amd.spec_decode.worker import (ExecuteModelRequest, SamplingParams, SequenceData, SequenceGroupMetadata,
                                          SpeculativeConfig, create_spec_worker)

CFG = QuarotLlamaConfig(1024, 3584, 8, 2, 2, 2048, 1e-5, 10000.0, 512, "tiny")
SEEDED = ("qspec_sample_top_k_top_p_seeded", "qspec_rejection_sample_seeded")


class SeedEngine(FakeEngine):
    """The scripted engine of test_worker_cpu, with a set_sampling_params that knows the `seed` keyword."""

    def set_sampling_params(self, slot, *args, **kwargs):
        self.calls.append(("params", slot, args, kwargs))


def _worker():
    w = create_spec_worker(model_config=CFG, model=object(), speculative_config=SpeculativeConfig(3), max_num_seqs=4,
                           max_model_len=256, block_size=16, device="cpu", engine_factory=SeedEngine,
                           disable_log_stats=True, memory_probe=fake_memory_probe)
    w.init_device()
    nb, _ = w.determine_num_available_blocks()
    w.initialize_cache(nb, 0)
    return w


def _admit(w, sp, rid="r0"):
    sg = SequenceGroupMetadata(rid, True, {0: SequenceData([1, 2, 3])}, sampling_params=sp)
    w.execute_model(ExecuteModelRequest([sg], num_lookahead_slots=0))
    return [c for c in w.engine.calls if c[0] == "params"]


def test_admit_forwards_the_seed():
    w = _worker()
    calls = _admit(w, SamplingParams(seed=1234, temperature=0.8, top_k=50, top_p=0.9))
    assert calls[0] == ("params", 0, (0.8, 50, 0.9), {"seed": 1234})


def test_admit_without_seed_calls_as_before():
    w = _worker()
    calls = _admit(w, SamplingParams(temperature=0.8, top_k=50, top_p=0.9))
    assert calls[0] == ("params", 0, (0.8, 50, 0.9), {})
    calls = _admit(_worker(), None)
    assert calls[0] == ("params", 0, (0.0, -1, 1.0), {})


def test_unseeded_admission_works_with_an_engine_that_has_no_seed_keyword():
    w = create_spec_worker(model_config=CFG, model=object(), speculative_config=SpeculativeConfig(3), max_num_seqs=4,
                           max_model_len=256, block_size=16, device="cpu", engine_factory=FakeEngine,
                           disable_log_stats=True, memory_probe=fake_memory_probe)
    w.init_device()
    w.initialize_cache(w.determine_num_available_blocks()[0], 0)
    _admit(w, SamplingParams(temperature=0.8))
    assert w.engine.sampling[0] == (0.8, -1, 1.0)


def test_engine_seed_arrays_follow_set_sampling_params_and_free_slot():
    eng = HostEngine()
    s = eng.sampling
    eng.set_sampling_params(2, 0.8, 50, 0.9, seed=1234)
    assert s.seq_seed.tolist() == [0, 0, 1234, 0] and s.seq_seeded.tolist() == [0, 0, 1, 0]
    eng.set_sampling_params(1, 1.0, seed=2 ** 64 - 1)          # mod 2^64, stored as the int64 with the same bits
    assert int(s.seq_seed[1]) == -1 and int(s.seq_seeded[1]) == 1
    eng.set_sampling_params(3, 0.0, seed=5)                     # greedy: no draws, no seed
    assert int(s.seq_seeded[3]) == 0
    eng.set_sampling_params(2, 0.8, 50, 0.9)                    # the seed goes, the parameters stay
    assert int(s.seq_seeded[2]) == 0 and s._samp_host[2] == (0.8, 50, 0.9)
    eng.free_slot(1)
    assert s.seq_seeded.tolist() == [0, 0, 0, 0] and s._seed_host == [None] * 4


def test_seeded_symbols_declared_bound_and_exported():
    declared = _lib.header_symbols()
    for name in SEEDED:
        assert name in declared and name in _lib.SIGNATURES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SEEDED:
        assert hasattr(lib, name)
    lib = _lib.load()
    assert lib.qspec_abi_version() == 6
    # argument validation happens before any HIP call
    rc = lib.qspec_sample_top_k_top_p_seeded(1, None, None, None, None, 0, 0, None, 1, 1, 1, 4, 16, None, 1, 1, 4, 1, 0, 2,
                                             1, None)
    assert rc != 0 and b"seq_seeds" in lib.qspec_last_error()
    rc = lib.qspec_sample_top_k_top_p_seeded(1, None, None, None, None, 0, 0, None, 1, 1, 1, 8, 16, 1, 1, 1, 4, 1, 0, 2,
                                             1, None)
    assert rc != 0 and b"does not cover" in lib.qspec_last_error()
    rc = lib.qspec_sample_top_k_top_p_seeded(1, None, None, None, None, 0, 0, None, 1, 1, 1, 4, 16, 1, 1, 1, 4, 1, 0, 3,
                                             1, None)
    assert rc != 0 and b"draw_stream" in lib.qspec_last_error()
    rc = lib.qspec_rejection_sample_seeded(1, 1, 1, 1, None, None, 0, 0, None, 4, 3, 16, 48, 16, 3, 1, 1, 1, 1, 1, None,
                                           None, None, 1, 1, 1, None)
    assert rc != 0 and b"seq_seeds" in lib.qspec_last_error()


def test_ops_pick_the_entry_by_the_seed_arguments(monkeypatch):
    from qspec_amd import ops
    seen = []
    monkeypatch.setattr(ops, "_call", lambda name, *args: seen.append(name))
    monkeypatch.setattr(ops, "_chk", lambda t, name, dtype=None: 1)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "sample_workspace", lambda rows, device: torch.zeros(1))
    logits = torch.zeros(4, 16, dtype=torch.float16)
    probs, tok = torch.zeros(4, 16), torch.zeros(4, dtype=torch.int64)
    ops.sample_top_k_top_p(logits, probs, tok)
    s = torch.zeros(4, dtype=torch.int64)
    f = torch.zeros(4, dtype=torch.int32)
    ops.sample_top_k_top_p(logits, probs, tok, seq_seeds=s, seq_seeded=f, base_pos=f)
    assert seen == ["qspec_sample_top_k_top_p", "qspec_sample_top_k_top_p_seeded"]
    with pytest.raises(RuntimeError, match="go together"):
        ops.sample_top_k_top_p(logits, probs, tok, seq_seeds=s)
