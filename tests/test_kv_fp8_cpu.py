"""FP8 (e4m3) KV cache, the parts that need no GPU: the `_kv8` C entries exist and validate their arguments, the worker reads
cache_config.cache_dtype (block size in bytes, block count, engine keywords, refusals), the checkpoint carries the scales."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from qspec_amd import _lib, checkpoint
from qspec_amd.model import QuarotLlamaConfig, QuarotLlamaForCausalLM
from qspec_amd.spec_decode.worker import create_spec_worker

GiB = 1 << 30
KV8_ENTRIES = ("qspec_rope_kv_write_kv8", "qspec_reshape_and_cache_flash_kv8", "qspec_paged_attention_kv8",
               "qspec_qkv_rope_linear_s4s4_kv8", "qspec_qkv_rope_linear_w4a16_kv8", "qspec_qkv_rope_linear_w4a16_xp_kv8",
               "qspec_qkv_rope_linear_w4a16_xp32_kv8", "qspec_ln_qkv_rope_linear_s4s4_kv8")


# ------------------------------------------------------------------ C ABI

def test_kv8_entries_in_header_binding_and_library():
    header = _lib.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in KV8_ENTRIES:
        assert name in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        base = name[:-len("_kv8")]
        # uint8_t caches + two float scales in place of the two qspec_half pointers: two more arguments, floats behind value_cache
        args, base_args = _lib.SIGNATURES[name][1], _lib.SIGNATURES[base][1]
        assert len(args) == len(base_args) + 2
        fl = [i for i in range(len(args) - 1) if args[i] is ctypes.c_float and args[i + 1] is ctypes.c_float
              and args[i - 1] is ctypes.c_void_p and args[i - 2] is ctypes.c_void_p]
        assert fl, name
        assert args[:fl[0]] + args[fl[0] + 2:] == base_args
    assert _lib.load().qspec_abi_version() == 6   # additive change


def test_kv8_argument_validation_without_gpu():
    lib = _lib.load()
    # NULL pointers: refused before any HIP call, the error names the _kv8 entry
    rc = lib.qspec_rope_kv_write_kv8(None, None, None, None, None, 1.0, 1.0, None, 4, 8, 2, 128, 128, None)
    assert rc != 0 and b"NULL" in lib.qspec_last_error() and b"qspec_rope_kv_write_kv8" in lib.qspec_last_error()
    rc = lib.qspec_reshape_and_cache_flash_kv8(None, None, None, None, 1.0, 1.0, None, 4, 2, 128, 256, 256, None)
    assert rc != 0 and b"NULL" in lib.qspec_last_error()
    rc = lib.qspec_paged_attention_kv8(None, 0, None, None, 1.0, 1.0, None, 4, None, None, 1, 1, 1, 8, 2, 128, 16, 0.1, 1,
                                       None, None, None)
    assert rc != 0 and b"NULL" in lib.qspec_last_error() and b"qspec_paged_attention_kv8" in lib.qspec_last_error()
    rc = lib.qspec_qkv_rope_linear_s4s4_kv8(None, None, None, None, None, 4, 1536, 1024, None, None, None, None, 1.0, 1.0,
                                            None, 8, 2, 128, 128, None)
    assert rc != 0 and b"NULL" in lib.qspec_last_error()
    rc = lib.qspec_ln_qkv_rope_linear_s4s4_kv8(None, None, None, 1e-5, None, None, None, 4, 1536, 1024, None, None, None, None,
                                               1.0, 1.0, None, 8, 2, 128, 128, None, None)
    assert rc != 0 and b"NULL" in lib.qspec_last_error()
    # every entry reports under its own name, the _xp / _xp32 forms included
    for name in ("qspec_qkv_rope_linear_w4a16_kv8", "qspec_qkv_rope_linear_w4a16_xp_kv8", "qspec_qkv_rope_linear_w4a16_xp32_kv8"):
        n_args = len(_lib.SIGNATURES[name][1])
        fl = [i for i, t in enumerate(_lib.SIGNATURES[name][1]) if t is ctypes.c_float]
        args = [None if t is ctypes.c_void_p else 4 for t in _lib.SIGNATURES[name][1]]
        for i in fl:
            args[i] = 1.0
        assert len(args) == n_args
        rc = getattr(lib, name)(*args)
        assert rc != 0 and (name + ":").encode() in lib.qspec_last_error(), lib.qspec_last_error()
    # scales must be positive and finite
    for ks, vs in ((0.0, 1.0), (1.0, -2.0), (float("inf"), 1.0), (float("nan"), 1.0)):
        rc = lib.qspec_rope_kv_write_kv8(None, None, None, None, None, ks, vs, None, 4, 8, 2, 128, 128, None)
        assert rc != 0 and b"k_scale" in lib.qspec_last_error()
    # a head size that only the scalar generic kernel serves: refused with the reason, before any HIP call
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.qspec_paged_attention_kv8(p, 0, p, p, 1.0, 1.0, p, 4, p, p, 1, 1, 1, 8, 2, 66, 16, 0.1, 1, p, p, None)
    assert rc != 0 and b"no fp8 form" in lib.qspec_last_error()
    # the base entry still reports under its own name afterwards (the fp8 scope ends with the call)
    rc = lib.qspec_rope_kv_write(None, None, None, None, None, None, 4, 8, 2, 128, 128, None)
    assert rc != 0 and b"qspec_rope_kv_write:" in lib.qspec_last_error()


def test_ops_dispatch_on_cache_dtype_refuses_scale_with_fp16_cache():
    from qspec_amd import ops
    kc = torch.zeros(2, 16, 2, 128, dtype=torch.float16)
    with pytest.raises(ValueError, match="fp8 KV cache"):
        ops._kv(kc, kc, 0.5, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # the dtype is accepted, the device is not
        ops._kv(kc.to(torch.uint8), kc.to(torch.uint8), 0.5, 1.0)
    with pytest.raises(ValueError, match="positive"):
        ops._kv(kc.to(torch.uint8), kc.to(torch.uint8), 0.0, 1.0)


# ------------------------------------------------------------------ worker

class StrictEngine:
    """An engine double with the constructor of an engine that predates the fp8 cache: unknown keywords raise TypeError."""

    def __init__(self, model, k, max_batch, max_model_len, block_size, seed=0, num_blocks=None, acceptance_sampler=None):
        self.k, self.num_blocks = k, num_blocks
        self.sampler = SimpleNamespace(num_accepted_tokens=None, num_emitted_tokens=None, num_draft_tokens=0)
        self.kw = {}


class Fp8Engine(StrictEngine):
    def __init__(self, *a, kv_cache_dtype="auto", kv_scales=None, **kw):
        super().__init__(*a, **kw)
        self.kw = {"kv_cache_dtype": kv_cache_dtype, "kv_scales": kv_scales}


def probe():
    return 200 * GiB, 256 * GiB, 1 * GiB    # free, total, torch peak increase


def vllm_config(cache_dtype=None, tp=1):
    hf = SimpleNamespace(model_type="llama_quarot", hidden_size=1024, intermediate_size=3584, num_attention_heads=8,
                         num_key_value_heads=2, num_hidden_layers=2, vocab_size=2048, rms_norm_eps=1e-5,
                         rope_theta=10000.0, max_position_embeddings=512)
    cc = SimpleNamespace(block_size=16, gpu_memory_utilization=0.9, swap_space_bytes=4 * GiB)
    if cache_dtype is not None:
        cc.cache_dtype = cache_dtype
    return SimpleNamespace(
        model_config=SimpleNamespace(hf_config=hf, max_model_len=256, model="/nonexistent", seed=0, max_logprobs=5),
        cache_config=cc,
        scheduler_config=SimpleNamespace(max_num_seqs=4, max_num_batched_tokens=2048),
        parallel_config=SimpleNamespace(tensor_parallel_size=tp, pipeline_parallel_size=1),
        load_config=SimpleNamespace(load_format="dummy"),
        speculative_config=SimpleNamespace(num_speculative_tokens=3, speculative_disable_by_batch_size=None,
                                           disable_log_stats=True, disable_logprobs=True,
                                           draft_token_acceptance_method="rejection_sampler",
                                           speculative_disable_mqa_scorer=False))


def make_worker(factory, **kw):
    w = create_spec_worker(vllm_config=vllm_config(**kw), local_rank=0, rank=0, distributed_init_method="tcp://127.0.0.1:29556",
                           is_driver_worker=True, device="cpu", model=object(), engine_factory=factory)
    w._memory_probe = probe
    w.init_device()
    return w


def available_bytes(w):
    free, total, peak = probe()
    return total * w.gpu_memory_utilization - ((total - free) + peak) - 2 * peak


@pytest.mark.parametrize("dtype", ["fp8", "fp8_e4m3"])
def test_worker_fp8_halves_the_block_and_tells_the_engine(dtype):
    auto = make_worker(StrictEngine, cache_dtype="auto")
    w = make_worker(Fp8Engine, cache_dtype=dtype)
    assert auto.cache_block_size_bytes() == 2 * 2 * 16 * 2 * 128 * 2
    assert w.cache_block_size_bytes() * 2 == auto.cache_block_size_bytes()
    nb, ncpu = w.determine_num_available_blocks()
    assert nb == int(available_bytes(w) // w.cache_block_size_bytes())
    assert ncpu == (4 * GiB) // w.cache_block_size_bytes()
    nb_auto, ncpu_auto = auto.determine_num_available_blocks()
    assert nb in (2 * nb_auto, 2 * nb_auto + 1) and ncpu == 2 * ncpu_auto
    assert w.memory_profile["cache_block_size"] == w.cache_block_size_bytes()
    w.initialize_cache(nb, ncpu)
    assert w.engine.kw["kv_cache_dtype"] == "fp8" and w.engine.num_blocks == nb


@pytest.mark.parametrize("cache_dtype", [None, "auto"])
def test_worker_auto_passes_no_new_keyword(cache_dtype):
    w = make_worker(StrictEngine, cache_dtype=cache_dtype)   # StrictEngine raises TypeError on any unknown keyword
    nb, ncpu = w.determine_num_available_blocks()
    w.initialize_cache(nb, ncpu)
    assert w.engine.num_blocks == nb and w.kv_cache_dtype == "auto"


@pytest.mark.parametrize("bad", ["fp8_e5m2", "int8"])
def test_worker_refuses_other_cache_dtypes(bad):
    with pytest.raises(ValueError, match=bad):
        make_worker(Fp8Engine, cache_dtype=bad)


def test_worker_refuses_fp8_with_tensor_parallelism():
    with pytest.raises(NotImplementedError, match="fp8 KV cache with tensor parallelism"):
        make_worker(Fp8Engine, cache_dtype="fp8", tp=2)


# ------------------------------------------------------------------ checkpoint

def tiny_model(seed=0):
    m = QuarotLlamaForCausalLM(QuarotLlamaConfig(1024, 3584, 8, 2, 2, 512, 1e-5, 10000.0, 256, "tiny"), "cpu")
    g = torch.Generator().manual_seed(seed)
    for layer in m.layers:
        for lin in layer.linears():
            n, kb = lin.weight.shape
            lin.weight.copy_(torch.randint(0, 256, (n, kb), generator=g, dtype=torch.int16).to(torch.uint8).view(torch.int8))
            lin.weight_scales.copy_((torch.rand(n, 1, generator=g) * 0.01 + 1e-3).to(torch.float16))
    m.embed_tokens.copy_((torch.randn(m.embed_tokens.shape, generator=g) * 0.02).to(torch.float16))
    m.lm_head.copy_((torch.randn(m.lm_head.shape, generator=g) * 0.02).to(torch.float16))
    return m


def test_checkpoint_scales_round_trip(tmp_path):
    src = tiny_model()
    assert not any(k.endswith("_scale") for k in checkpoint.reference_state_dict(src))   # all 1.0: nothing written
    src.kv_scales = [(0.75, 1.5), (0.5, 2.0)]
    sd = checkpoint.reference_state_dict(src)
    assert sd["model.layers.0.self_attn.k_scale"].dtype == torch.float32 and sd["model.layers.0.self_attn.k_scale"].dim() == 0
    checkpoint.save_qspec_checkpoint(src, str(tmp_path))
    dst = tiny_model(1)
    checkpoint.load_qspec_checkpoint(dst, str(tmp_path))
    assert dst.kv_scales == [(0.75, 1.5), (0.5, 2.0)]


def test_checkpoint_scales_default_to_one():
    src = tiny_model()
    sd = {checkpoint._rename(k): v for k, v in checkpoint.reference_state_dict(src).items()}
    dst = tiny_model(1)
    dst.kv_scales = [(3.0, 3.0)] * 2
    checkpoint.load_state_dict(dst, dict(sd))
    assert dst.kv_scales is None                       # absent: 1.0 everywhere
    sd["model.layers.0.self_attn.k_scale"] = torch.tensor(0.0)     # non-positive -> 1.0
    sd["model.layers.0.self_attn.v_scale"] = torch.tensor(-1.0)
    sd["model.layers.1.self_attn.v_scale"] = torch.tensor(2.0)     # k_scale of layer 1 absent -> 1.0
    checkpoint.load_state_dict(dst, dict(sd))
    assert dst.kv_scales == [(1.0, 1.0), (1.0, 2.0)]
