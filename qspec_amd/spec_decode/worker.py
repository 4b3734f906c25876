"""Worker boundary: what vLLM's executor calls.

`create_spec_worker(*args, **kwargs) -> SpecDecodeWorker` and the methods vLLM's WorkerBase contract needs
(`init_device`, `load_model`, `determine_num_available_blocks`, `initialize_cache`, `execute_model`,
`get_cache_block_size_bytes`, `start_worker_execution_loop`, `rank`, `device`), mirroring
vllm/spec_decode/spec_decode_worker.py:53-113,118-470,461-560,582-664,722-755,972-1110,1178-1210.

The factory binds the way the reference's does: `kwargs["vllm_config"]` (duck-typed: `model_config.{hf_config,
max_model_len, model, seed, max_logprobs}`, `cache_config.{block_size, gpu_memory_utilization, swap_space_bytes, cache_dtype}`,
`scheduler_config.{max_num_seqs, max_num_batched_tokens}`, `speculative_config.{num_speculative_tokens,
speculative_disable_by_batch_size, disable_log_stats, disable_logprobs, draft_token_acceptance_method}`,
`parallel_config.{tensor_parallel_size, pipeline_parallel_size}`, `load_config.load_format`) plus `local_rank`, `rank`,
`distributed_init_method`, `is_driver_worker` (:53-113; vllm/worker/worker.py:46-60).  A second, explicit-keyword path
(`model_config=`, `max_num_seqs=`, ...) is kept for tests and benchmarks.

vLLM itself is not importable here, so the request / output records are small dataclasses with the reference's
field names (vllm/sequence.py:37-48,1017-1078; vllm/model_executor/layers/sampler.py SamplerOutput): what
`MultiStepOutputProcessor` reads -- `output.samples[0].output_token`, `.parent_seq_id`, `.logprobs`
(vllm/engine/output_processor/multi_step.py:100-176) -- is there under those names.

QSpec specifics preserved:
  * proposer and scorer are the SAME model object and the SAME KV cache (:339-345, :421-444); the block count is the
    scorer's, not split between the two (:421-423);
  * `execute_model_req.w4a4 = True` only around the proposer (:797-812); `ExecuteModelRequest.clone()` does not
    carry `w4a4`, so the scorer always runs W4A16 (vllm/sequence.py:1301,1331-1348);
  * prefill never runs the proposer (:699);
  * one `SamplerOutput` per emitted position, `-1` = no token for that sequence, the list stops at the first position
    where no sequence emitted anything (:1023-1026);
  * bonus-token bookkeeping is kept (:1178-1210) although `llama_quarot` skips the batch expansion it feeds
    (multi_step_worker.py:74-80): the verify pass has already written the KV of every accepted position.
The decisions the reference inherits from `attn_backend.get_name() == "FLASH_ATTN"` (MQA scorer, on-GPU draft
loop; :214-235, draft_model_runner.py:154) are owned here: both are always on.

Batch membership follows `seq_group_metadata_list` on EVERY call: requests are identified by `request_id`, keep their
engine slot -- one per sequence id: a group sampling n / best_of > 1 sequences holds that many -- until
`finished_requests_ids` names them, may be scheduled in any order and in any subset (sequences that
sit out a step do not advance), and new prompts are admitted whenever a slot is free.  The scheduler's block tables
(`SequenceGroupMetadata.block_tables`) are honoured when given.

Tensor parallelism (the verify pass shards, qspec_amd/parallel.py): the driver rank broadcasts the step's control
record and the request, non-driver ranks sit in `start_worker_execution_loop()` and mirror the call
(:524-538, :722-755; vllm/worker/worker_base.py:340-344).
"""
from __future__ import annotations

import functools
import os
from collections import defaultdict
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Set, Tuple

import torch

from ..model import CONFIGS, QuarotLlamaConfig, QuarotLlamaForCausalLM
from .engine import QSpecEngine
from .guides import TokenFSM
from .metrics import AsyncMetricsCollector, SpecDecodeWorkerMetrics

VLLM_INVALID_TOKEN_ID = -1       # vllm/sequence.py:29
MAX_LOGPROBS = 32                # QS_MAX_LOGPROBS (include/qspec_hip.h): the cap of max_logprobs with disable_logprobs=False


# ---------------------------------------------------------------------- records (vllm/sequence.py field names)

@dataclass
class SamplingParams:
    """The fields of vllm/sampling_params.py the worker and the output processor read."""
    logprobs: Optional[int] = None
    prompt_logprobs: Optional[int] = None
    max_tokens: int = 16
    ignore_eos: bool = False
    seed: Optional[int] = None
    # Sampler.forward's inputs (sampler.py:216-316).  temperature 0 = greedy -- the reference's demo and BASELINE.json's configs;
    # vLLM's own default is 1.0, a caller coming from vLLM passes its SamplingParams object and with it the real value
    temperature: float = 0.0
    top_k: int = -1
    top_p: float = 1.0
    # the logit processors of Sampler.forward (sampler.py:258-278), applied inside the captured cycle
    min_p: float = 0.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    repetition_penalty: float = 1.0
    min_tokens: int = 0
    stop_token_ids: Optional[List[int]] = None   # (a vLLM object also carries all_stop_token_ids: these + the EOS id)
    # token constraints, applied in front of the processors above (vllm/entrypoints/openai/logits_processors.py:10-86,
    # vllm/logits_process.py:48-119).  A vLLM object arrives with the first two already lowered into logits_processors and its
    # bad words as strings; the worker has no tokenizer, so its own field takes token ids.
    logit_bias: Optional[Dict[Any, float]] = None
    allowed_token_ids: Optional[List[int]] = None
    bad_words_token_ids: Optional[List[List[int]]] = None
    logits_processors: Optional[List[Any]] = None
    # guided decoding: a guides.TokenFSM (vLLM's guided_decoding arrives lowered to an Outlines processor in logits_processors,
    # which the worker recognises; the worker has no tokenizer, so its own field takes the finished automaton)
    guided_fsm: Optional[Any] = None
    # parallel sampling: best_of (default: n) sequences are sampled from one prompt pass; beam search is refused
    n: int = 1
    best_of: Optional[int] = None
    use_beam_search: bool = False


@dataclass
class SequenceData:
    prompt_token_ids: List[int]
    output_token_ids: List[int] = field(default_factory=list)
    _num_computed_tokens: int = 0        # tokens whose K/V an earlier chunk of the prompt has written (vllm/sequence.py)

    def get_num_computed_tokens(self) -> int:
        return self._num_computed_tokens

    def update_num_computed_tokens(self, num_new_computed_tokens: int) -> None:
        self._num_computed_tokens += num_new_computed_tokens

    def get_len(self):
        return len(self.prompt_token_ids) + len(self.output_token_ids)

    def get_output_len(self):
        return len(self.output_token_ids)

    def get_prompt_token_ids(self):
        return list(self.prompt_token_ids)

    def get_token_ids(self):
        return list(self.prompt_token_ids) + list(self.output_token_ids)


@dataclass
class SequenceGroupMetadata:
    request_id: str
    is_prompt: bool
    seq_data: Dict[int, SequenceData]
    num_speculative_tokens: Optional[int] = None
    block_tables: Optional[Dict[int, List[int]]] = None   # seq_id -> physical block ids (vllm/sequence.py)
    sampling_params: Optional[SamplingParams] = None
    do_sample: bool = True
    token_chunk_size: Optional[int] = None
    computed_block_nums: Optional[List[int]] = None       # prefix caching: leading blocks whose K/V is already valid


@dataclass
class ExecuteModelRequest:
    seq_group_metadata_list: List[SequenceGroupMetadata]
    num_lookahead_slots: int = 0
    running_queue_size: int = 0
    finished_requests_ids: List[str] = field(default_factory=list)   # vllm/sequence.py:1295
    w4a4: bool = False                                   # vllm/sequence.py:1301
    # block moves in front of the step (vllm/sequence.py; vllm/worker/worker.py, execute_worker): (cpu, gpu), (gpu, cpu), (src, dst)
    blocks_to_swap_in: List[Tuple[int, int]] = field(default_factory=list)
    blocks_to_swap_out: List[Tuple[int, int]] = field(default_factory=list)
    blocks_to_copy: List[Tuple[int, int]] = field(default_factory=list)

    def clone(self, seq_group_metadata_list):
        """vllm/sequence.py:1331-1348: every field except `w4a4` is carried over."""
        return ExecuteModelRequest(seq_group_metadata_list=seq_group_metadata_list,
                                   num_lookahead_slots=self.num_lookahead_slots,
                                   running_queue_size=self.running_queue_size,
                                   finished_requests_ids=self.finished_requests_ids,
                                   blocks_to_swap_in=list(self.blocks_to_swap_in),
                                   blocks_to_swap_out=list(self.blocks_to_swap_out),
                                   blocks_to_copy=list(self.blocks_to_copy))


@dataclass
class Logprob:
    """vllm/sequence.py:37-48."""
    logprob: float
    rank: Optional[int] = None
    decoded_token: Optional[str] = None


@dataclass
class SequenceOutput:
    """vllm/sequence.py:1017-1045."""
    parent_seq_id: int
    output_token: int
    logprobs: Dict[int, Logprob]


@dataclass
class CompletionSequenceGroupOutput:
    """vllm/sequence.py:1060-1078."""
    samples: List[SequenceOutput]
    prompt_logprobs: Optional[List[Optional[Dict[int, Logprob]]]] = None


@dataclass
class SamplerOutput:
    """One decode position for the whole batch (vllm/model_executor/layers/sampler.py SamplerOutput): `outputs[i]` is
    the i-th sequence group of the request, in request order.  The device-side fields are cleared before the list
    leaves the worker, as the reference does (:715-719)."""
    outputs: List[CompletionSequenceGroupOutput]
    sampled_token_probs: Optional[torch.Tensor] = None
    sampled_token_ids: Optional[torch.Tensor] = None
    logprobs: Optional[torch.Tensor] = None
    spec_decode_worker_metrics: Optional[SpecDecodeWorkerMetrics] = None
    hidden_states: Optional[torch.Tensor] = None

    def __getitem__(self, idx: int) -> CompletionSequenceGroupOutput:
        return self.outputs[idx]

    def __len__(self):
        return len(self.outputs)

    def token_ids(self) -> List[int]:
        """Convenience (tests, benchmarks): the output token per sequence group, -1 where a group has none."""
        return [o.samples[0].output_token if o.samples else VLLM_INVALID_TOKEN_ID for o in self.outputs]


@dataclass
class SpeculativeConfig:
    num_speculative_tokens: int = 3
    speculative_disable_mqa_scorer: bool = False
    speculative_disable_by_batch_size: Optional[int] = None
    draft_token_acceptance_method: str = "rejection_sampler"       # or "typical_acceptance_sampler"
    typical_acceptance_sampler_posterior_threshold: float = 0.09    # vllm/config.py defaults
    typical_acceptance_sampler_posterior_alpha: float = 0.3
    disable_logprobs: bool = True        # vllm/config.py:1788-1789: logprobs are off during speculation by default
    disable_log_stats: bool = False


@dataclass
class _SampleGroup:
    """A request sampling several sequences from one prompt: its engine slots (the parent's first, then the samples' in
    sample order), the first token of each, and which sequence id sits in which slot.  The samples' sequence ids are the
    scheduler's to choose: they are bound when the group first comes back with them."""
    slots: List[int]
    first: List[int] = field(default_factory=list)
    bound: Dict[int, int] = field(default_factory=dict)


class DeviceHandoffTimeout(RuntimeError):
    """A device-side hand-off (spread Hadamard exchange, norm hand-off, one-shot all-reduce) timed out and the recovery
    replay without hand-offs failed as well: the cycle's results are invalid on every rank."""


def create_logprobs_output(token_id: int, token_id_logprob_rank: int, token_id_logprob: float,
                           topk_token_ids: List[Optional[int]], topk_logprobs: List[Optional[float]]) -> Dict[int, Logprob]:
    """vllm/spec_decode/util.py:54-88."""
    logprobs = {token_id: Logprob(logprob=token_id_logprob, rank=token_id_logprob_rank)}
    logprobs.update({tid: Logprob(logprob=lp if lp is not None else 0.0, rank=i + 1)
                     for i, (tid, lp) in enumerate(zip(topk_token_ids, topk_logprobs)) if tid is not None})
    return logprobs


def create_sequence_group_output(token_id: int, token_id_logprob_rank: int, token_id_logprob: float, seq_id: int,
                                 topk_token_ids: List[Optional[int]], topk_logprobs: List[Optional[float]],
                                 prompt_logprobs=None) -> CompletionSequenceGroupOutput:
    """vllm/spec_decode/util.py:91-126."""
    logprobs = create_logprobs_output(token_id, token_id_logprob_rank, token_id_logprob, topk_token_ids, topk_logprobs)
    return CompletionSequenceGroupOutput(
        samples=[SequenceOutput(parent_seq_id=seq_id, output_token=token_id, logprobs=logprobs)],
        prompt_logprobs=prompt_logprobs)


# ---------------------------------------------------------------------- factory (:53-113)

def model_config_from_hf(hf_config, name: str = "hf") -> QuarotLlamaConfig:
    """HF LlamaConfig-shaped object -> the fields this path needs (quarot_llama.py:319-360,436-470)."""
    g = lambda k, d=None: getattr(hf_config, k, d)  # noqa: E731
    return QuarotLlamaConfig(g("hidden_size"), g("intermediate_size"), g("num_attention_heads"),
                             g("num_key_value_heads", g("num_attention_heads")), g("num_hidden_layers"),
                             g("vocab_size"), g("rms_norm_eps", 1e-5), float(g("rope_theta", 10000.0)),
                             g("max_position_embeddings", 8192), g("_name_or_path", name) or name)


def create_spec_worker(*args, **kwargs) -> "SpecDecodeWorker":
    """Entry point resolved from `parallel_config.worker_cls` (vllm/platforms/rocm.py:130-131); reference :53-113.

    Path 1 (what vLLM's WorkerWrapper passes): kwargs = {vllm_config, local_rank, rank, distributed_init_method,
    is_driver_worker}.  Path 2 (tests, benchmarks): model_config (QuarotLlamaConfig or a CONFIGS name),
    speculative_config, max_num_seqs, max_model_len, block_size, device, model (a pre-built
    QuarotLlamaForCausalLM), seed, pipeline_parallel_size, rank, engine_factory."""
    vllm_config = kwargs.get("vllm_config")
    if vllm_config is not None:
        spec = vllm_config.speculative_config
        assert spec is not None                                                     # :59
        par = vllm_config.parallel_config
        if getattr(par, "pipeline_parallel_size", 1) > 1:                           # :61-63
            raise NotImplementedError("Speculative decoding is currently incompatible with pipeline parallelism")
        method = getattr(spec, "draft_token_acceptance_method", "rejection_sampler")
        if method not in ("rejection_sampler", "typical_acceptance_sampler"):       # :95-110
            raise ValueError(f"draft_token_acceptance_method {method!r}: expected rejection_sampler or typical_acceptance_sampler")
        mc, cc, sc = vllm_config.model_config, vllm_config.cache_config, vllm_config.scheduler_config
        model_type = getattr(mc.hf_config, "model_type", "llama_quarot")
        if model_type not in ("llama_quarot", "llama"):
            raise NotImplementedError(f"model_type {model_type!r}: this worker runs the llama_quarot QSpec model only "
                                      "(vllm/worker/model_runner.py:1104-1148)")
        local_rank = kwargs.get("local_rank", 0)
        load_format = getattr(getattr(vllm_config, "load_config", None), "load_format", "auto")
        return SpecDecodeWorker(
            model_config_from_hf(mc.hf_config, str(getattr(mc, "model", "hf"))), spec,
            max_num_seqs=sc.max_num_seqs, max_model_len=mc.max_model_len, block_size=cc.block_size,
            device=kwargs.get("device", f"cuda:{local_rank}"), model=kwargs.get("model"),
            seed=getattr(mc, "seed", 0) or 0, rank=kwargs.get("rank", 0),
            disable_log_stats=getattr(spec, "disable_log_stats", False), engine_factory=kwargs.get("engine_factory"),
            model_path=getattr(mc, "model", None), load_format=str(load_format),
            tensor_parallel_size=getattr(par, "tensor_parallel_size", 1),
            distributed_init_method=kwargs.get("distributed_init_method"),
            is_driver_worker=kwargs.get("is_driver_worker", kwargs.get("rank", 0) == 0),
            gpu_memory_utilization=getattr(cc, "gpu_memory_utilization", 0.9),
            swap_space_bytes=getattr(cc, "swap_space_bytes", 0),
            cache_dtype=getattr(cc, "cache_dtype", "auto"),
            max_num_batched_tokens=getattr(sc, "max_num_batched_tokens", None),
            max_logprobs=getattr(mc, "max_logprobs", 20),
            disable_logprobs=getattr(spec, "disable_logprobs", True))
    if kwargs.get("pipeline_parallel_size", 1) > 1:
        raise NotImplementedError("Speculative decoding is currently incompatible with pipeline parallelism")
    spec = kwargs.get("speculative_config") or SpeculativeConfig()
    if spec.draft_token_acceptance_method not in ("rejection_sampler", "typical_acceptance_sampler"):
        raise ValueError(f"draft_token_acceptance_method {spec.draft_token_acceptance_method!r}: expected rejection_sampler or "
                         "typical_acceptance_sampler")
    cfg = kwargs.get("model_config", "llama-3-8b")
    if isinstance(cfg, str):
        cfg = CONFIGS[cfg]
    return SpecDecodeWorker(cfg, spec, max_num_seqs=kwargs.get("max_num_seqs", 4),
                            max_model_len=kwargs.get("max_model_len", 1024), block_size=kwargs.get("block_size", 16),
                            device=kwargs.get("device", "cuda:0"), model=kwargs.get("model"),
                            seed=kwargs.get("seed", 0), rank=kwargs.get("rank", 0),
                            disable_log_stats=kwargs.get("disable_log_stats", getattr(spec, "disable_log_stats", False)),
                            engine_factory=kwargs.get("engine_factory"), model_path=kwargs.get("model_path"),
                            load_format=kwargs.get("load_format", "dummy" if kwargs.get("model_path") is None else "auto"),
                            gpu_memory_utilization=kwargs.get("gpu_memory_utilization", 0.9),
                            max_num_batched_tokens=kwargs.get("max_num_batched_tokens"),
                            max_logprobs=kwargs.get("max_logprobs", 20),
                            disable_logprobs=getattr(spec, "disable_logprobs", True),
                            memory_probe=kwargs.get("memory_probe"), cache_dtype=kwargs.get("cache_dtype", "auto"))


class SpecDecodeWorker:
    def __init__(self, model_config: QuarotLlamaConfig, speculative_config, max_num_seqs: int,
                 max_model_len: int, block_size: int, device: str, model: Optional[QuarotLlamaForCausalLM] = None,
                 seed: int = 0, rank: int = 0, disable_log_stats: bool = False, engine_factory=None,
                 model_path: Optional[str] = None, load_format: str = "auto", tensor_parallel_size: int = 1,
                 distributed_init_method: Optional[str] = None, is_driver_worker: bool = True,
                 gpu_memory_utilization: float = 0.9, swap_space_bytes: int = 0,
                 max_num_batched_tokens: Optional[int] = None, max_logprobs: int = 20, disable_logprobs: bool = True,
                 memory_probe: Optional[Callable[[], Tuple[int, int, int]]] = None, cache_dtype: str = "auto"):
        # cache_config.cache_dtype (vllm/config.py CacheConfig): "auto" = the model's fp16; "fp8" / "fp8_e4m3" = OCP e4m3
        # bytes (include/qspec_hip.h, "FP8 KV cache").  Anything else is refused here, not served from an fp16 cache.
        if cache_dtype not in ("auto", "fp8", "fp8_e4m3"):
            raise ValueError(f"cache_config.cache_dtype = {cache_dtype!r}: this worker serves 'auto', 'fp8' and 'fp8_e4m3'")
        self.kv_cache_dtype = "auto" if cache_dtype == "auto" else "fp8"
        if self.kv_cache_dtype == "fp8" and tensor_parallel_size > 1:
            raise NotImplementedError("fp8 KV cache with tensor parallelism")
        self.model_config = model_config
        self.speculative_config = speculative_config
        self.max_num_seqs = max_num_seqs
        self.max_model_len = max_model_len
        self.block_size = block_size
        self._device = torch.device(device)
        self._model = model
        self._model_path, self._load_format = model_path, load_format
        self._seed = seed
        self._rank = rank
        self._driver_rank = 0
        self._is_driver_worker = is_driver_worker
        self._tp_size, self._dist_init = tensor_parallel_size, distributed_init_method
        self.gpu_memory_utilization, self.swap_space_bytes = gpu_memory_utilization, swap_space_bytes
        self.max_num_batched_tokens = max_num_batched_tokens
        if not disable_logprobs and max_logprobs > MAX_LOGPROBS:
            raise ValueError(f"max_logprobs = {max_logprobs} with disable_logprobs=False: the logprob kernel returns at most "
                             f"{MAX_LOGPROBS} per position")
        self.max_logprobs = max_logprobs
        self._disable_logprobs = disable_logprobs
        self._memory_probe = memory_probe
        self.disable_by_batch_size = getattr(speculative_config, "speculative_disable_by_batch_size", None)
        self._disable_log_stats = disable_log_stats
        self._engine_factory = engine_factory or QSpecEngine
        self.engine: Optional[QSpecEngine] = None
        self._metrics: Optional[AsyncMetricsCollector] = None
        self._slots: Dict[str, int] = {}                 # request_id -> engine slot
        # :1178-1210 -- sequences that received a bonus token in their last step / request -> its sequence ids
        self._seq_with_bonus_token_in_last_step: Set[int] = set()
        self._request_id_seq_id_mapping: Dict[str, Set[int]] = defaultdict(set)
        self.proposer_calls = 0     # forwards run with w4a4=True (for tests of the toggle)
        self.scorer_calls = 0
        self.memory_profile: Dict[str, Any] = {}

    # ------------------------------------------------------------------ WorkerBase contract
    @property
    def rank(self):
        return self._rank

    @property
    def device(self):
        return self._device

    @property
    def _tp(self):
        tp = getattr(self._model, "tp", None)
        return tp if tp is not None and tp.world > 1 else None

    def init_device(self) -> None:
        """:326-369: the scorer initialises the device and loads the model, the proposer receives the very same
        object (`proposer_worker.load_model(self.scorer_worker.model_runner.model)`, :342)."""
        if self._device.type == "cuda":
            torch.cuda.set_device(self._device)
        if self._tp_size > 1 and self._model is None:
            import torch.distributed as dist
            if not dist.is_initialized():     # vllm/worker/worker.py:init_worker_distributed_environment
                dist.init_process_group("nccl", init_method=self._dist_init, world_size=self._tp_size, rank=self._rank,
                                        device_id=self._device)
        if self._model is None:
            self._model = self._load_model()
        self.scorer_model = self._model
        self.proposer_model = self._model

    def _load_model(self) -> QuarotLlamaForCausalLM:
        """vllm/worker/model_runner.py:1096-1148: `model_config.model` is a directory holding the two safetensors
        shards of a QSpec checkpoint (loaded through qspec_amd/checkpoint.py: key renames, fuse_qkv / fuse_gate_up);
        `load_format == "dummy"` (vLLM's random-weights format) gives the SURVEY 8d synthetic weights.  Anything else
        raises: a worker must never run on silently invented weights."""
        model = QuarotLlamaForCausalLM(self.model_config, self._device)
        if self._load_format == "dummy":
            model.init_synthetic(self._seed)
        elif self._model_path is not None and os.path.isdir(str(self._model_path)):
            from ..checkpoint import load_qspec_checkpoint
            load_qspec_checkpoint(model, str(self._model_path))
        else:
            raise FileNotFoundError(f"model_config.model = {self._model_path!r} is not a local QSpec checkpoint directory "
                                    "(no hub access here); pass load_format='dummy' for synthetic weights")
        if self._tp_size > 1:
            from ..parallel import attach_tp
            k = self.speculative_config.num_speculative_tokens
            attach_tp(model, self._rank, self._tp_size, tokens=self.max_num_seqs * (k + 1))
        return model

    def load_model(self, *args, **kwargs):
        pass                                   # :371 (the model is loaded in init_device, as in the reference)

    def get_model(self):
        return self._model

    def cache_block_size_bytes(self) -> int:
        """vllm/worker/cache_engine.py:101-119: K and V of one block over all layers, 2 bytes per element (fp16) or 1
        (cache_dtype fp8).  The KV cache is NOT sharded under this worker's tensor parallelism (replicated draft pass), so
        kv heads are not divided."""
        c = self.model_config
        elem = 1 if self.kv_cache_dtype == "fp8" else 2
        return 2 * c.num_hidden_layers * self.block_size * c.num_key_value_heads * c.head_dim * elem

    def _profile_memory(self) -> Tuple[int, int, int]:
        """(free bytes now, total bytes, peak increase of one profiled prompt pass + cycle).  vllm/worker/worker.py:176-205:
        `profile_run()` under `memory_profiling`: here a throw-away engine with a KV cache just large enough for the
        profiled batch runs the worst-case prompt pass (max_num_batched_tokens over max_num_seqs prompts) and one
        captured cycle; torch's peak allocation above the weights is what the cycle needs besides the KV cache."""
        if self._memory_probe is not None:
            return self._memory_probe()
        if self._device.type != "cuda":
            raise RuntimeError("memory profiling needs the GPU (pass memory_probe= for host-side tests)")
        import gc
        dev = self._device
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        k = self.speculative_config.num_speculative_tokens
        budget = self.max_num_batched_tokens or self.max_model_len
        per_seq = max(1, min(self.max_model_len - (k + 2), budget // self.max_num_seqs))
        blocks_per_seq = (per_seq + k + 2 + self.block_size - 1) // self.block_size
        n_blocks = self.max_num_seqs * blocks_per_seq
        eng = self._engine_factory(self._model, k, self.max_num_seqs, self.max_model_len, self.block_size,
                                   seed=self._seed, num_blocks=n_blocks, **self._sampler_kwargs(), **self._kv_kwargs())
        kv_bytes = n_blocks * self.cache_block_size_bytes()
        tables = [list(range(b * blocks_per_seq, (b + 1) * blocks_per_seq)) for b in range(self.max_num_seqs)]
        eng.add_sequences_to(list(range(self.max_num_seqs)), [[0] * per_seq] * self.max_num_seqs, tables)
        eng.step()
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev) - base - kv_bytes
        del eng
        gc.collect()
        torch.cuda.empty_cache()
        free, total = torch.cuda.mem_get_info(dev)
        return int(free), int(total), int(max(peak, 0))

    def determine_num_available_blocks(self) -> Tuple[int, int]:
        """:400-426 over vllm/worker/worker.py:176-265: profile the scorer, then
            available = total x gpu_memory_utilization - non_kv_cache_memory - avoid_oom_memory,
        with non_kv_cache_memory = weights + non-torch + torch peak increase (vllm/utils.py:2053-2056) and the fork's
        head-room for speculative decoding avoid_oom_memory = 2 x torch peak increase (worker.py:227-231); the count is
        NOT split between proposer and scorer (shared cache, :421-423)."""
        free, total, peak = self._profile_memory()
        used_without_kv = total - free                    # weights + non-torch + whatever else lives on the card
        avoid_oom = 2 * peak                              # worker.py:227-231 (speculative_config is not None here)
        available = total * self.gpu_memory_utilization - (used_without_kv + peak) - avoid_oom
        block = self.cache_block_size_bytes()
        num_gpu_blocks = max(int(available // block), 0)
        num_cpu_blocks = max(int(self.swap_space_bytes // block), 0)
        self.memory_profile = dict(free=free, total=total, torch_peak_increase=peak, avoid_oom_memory=avoid_oom,
                                   available_kv_cache_memory=int(available), cache_block_size=block)
        return num_gpu_blocks, num_cpu_blocks

    def initialize_cache(self, num_gpu_blocks: int, num_cpu_blocks: int) -> None:
        """:428-444 + vllm/worker/worker.py:290-327 (raise_if_cache_size_invalid, ref_initilize_cache): one cache
        engine of `num_gpu_blocks` blocks for both passes, and -- only when num_cpu_blocks > 0, through a call of its own behind
        the constructor, so that an engine (or a test double) that predates swapping is built and used exactly as before -- its
        swap space of `num_cpu_blocks` pinned blocks (QSpecEngine.allocate_cpu_cache)."""
        if num_gpu_blocks <= 0:
            raise ValueError("No available memory for the cache blocks. Try increasing `gpu_memory_utilization` when "
                             "initializing the engine.")
        if self.max_model_len > self.block_size * num_gpu_blocks:
            raise ValueError(f"The model's max seq len ({self.max_model_len}) is larger than the maximum number of "
                             f"tokens that can be stored in KV cache ({self.block_size * num_gpu_blocks}). Try "
                             "increasing `gpu_memory_utilization` or decreasing `max_model_len` when initializing the engine.")
        self.engine = self._engine_factory(self._model, self.speculative_config.num_speculative_tokens,
                                           self.max_num_seqs, self.max_model_len, self.block_size, seed=self._seed,
                                           num_blocks=num_gpu_blocks, **self._sampler_kwargs(), **self._kv_kwargs())
        if num_cpu_blocks and num_cpu_blocks > 0 and hasattr(self.engine, "allocate_cpu_cache"):
            self.engine.allocate_cpu_cache(int(num_cpu_blocks))
        self._metrics = AsyncMetricsCollector(self.engine.sampler)
        self._metrics.init_gpu_tensors(self._rank)

    def _kv_kwargs(self) -> dict:
        """Engine keywords of the fp8 KV cache; none for "auto", so an engine (or a test double) that predates them is
        called exactly as before."""
        return {"kv_cache_dtype": "fp8"} if self.kv_cache_dtype == "fp8" else {}

    def _sampler_kwargs(self) -> dict:
        """spec_decode_worker.py:95-110: the acceptance sampler named by `draft_token_acceptance_method`."""
        spec = self.speculative_config
        if getattr(spec, "draft_token_acceptance_method", "rejection_sampler") != "typical_acceptance_sampler":
            return {}
        from .typical_acceptance_sampler import TypicalAcceptanceSampler
        return {"acceptance_sampler": TypicalAcceptanceSampler(
            posterior_threshold=getattr(spec, "typical_acceptance_sampler_posterior_threshold", 0.09),
            posterior_alpha=getattr(spec, "typical_acceptance_sampler_posterior_alpha", 0.3), seed=self._seed)}

    def get_cache_block_size_bytes(self):
        raise NotImplementedError  # as the reference (:1259-1268)

    def start_profile(self):
        torch.cuda.profiler.start()

    def stop_profile(self):
        torch.cuda.profiler.stop()

    # ------------------------------------------------------------------ TP control plane (:524-538, :722-755)
    def start_worker_execution_loop(self) -> None:
        """Non-driver ranks: mirror the driver's calls until it sends the empty record (execute_model(None))."""
        assert self._rank != self._driver_rank, "the driver rank calls execute_model, not the loop"
        while self._run_non_driver_rank():
            pass

    def _run_non_driver_rank(self) -> bool:
        """One mirrored step; False when the driver signalled the end of the loop (:722-755)."""
        assert self._rank != self._driver_rank
        data = self._tp.broadcast_object(None, src=self._driver_rank) if self._tp is not None else {}
        if not data:
            return False
        self._execute(data["request"], data["no_spec"], data["disable_all_speculation"], data["num_lookahead_slots"])
        return True

    # ------------------------------------------------------------------ execute_model (:461-560)
    @torch.no_grad()   # (the reference uses inference_mode; tensors made under it could not be updated by a later
    # hipGraph capture outside it -- the CUDA generator's graph-safe state among them -- and nothing here needs it)
    def execute_model(self, execute_model_req: Optional[ExecuteModelRequest] = None) -> List[SamplerOutput]:
        if self._rank != self._driver_rank:
            self._run_non_driver_rank()
            return []
        if execute_model_req is None:
            # the signal that ends start_worker_execution_loop() on the other ranks (:470-478)
            if self._tp is not None:
                self._tp.broadcast_object({}, src=self._driver_rank)
            return []
        sgml = execute_model_req.seq_group_metadata_list
        assert sgml is not None, "speculative decoding requires non-None seq_group_metadata_list"
        num_lookahead_slots = execute_model_req.num_lookahead_slots
        all_prompt = all(s.is_prompt for s in sgml)
        all_zero_spec = all(s.num_speculative_tokens == 0 for s in sgml)
        if all_prompt and sgml:
            assert num_lookahead_slots == 0, "Prompt only runs should have num_lookahead_slots equal to 0."
        disable_all_speculation = self._should_disable_all_speculation(execute_model_req)
        no_spec = num_lookahead_slots == 0 or disable_all_speculation or all_zero_spec
        if self._tp is not None:   # broadcast_tensor_dict of the control scalars (+ the inputs, worker_base.py:340-344)
            self._tp.broadcast_object(dict(num_lookahead_slots=num_lookahead_slots, no_spec=no_spec,
                                           disable_all_speculation=disable_all_speculation,
                                           run_spec_proposer_for_prefill=any(s.is_prompt for s in sgml),
                                           request=execute_model_req), src=self._driver_rank)
        return self._execute(execute_model_req, no_spec, disable_all_speculation, num_lookahead_slots)

    def _execute(self, req: ExecuteModelRequest, no_spec: bool, disable_all_speculation: bool,
                 num_lookahead_slots: int) -> List[SamplerOutput]:
        self._check_requested_logprobs(req.seq_group_metadata_list or ())
        self._apply_block_operations(req)
        self._track_finished_requests(req)
        if not req.seq_group_metadata_list:
            return []
        if no_spec:
            return self._run_no_spec(req, skip_proposer=True)      # skip_proposer forced (:699)
        return self._run_speculative_decoding_step(req, num_lookahead_slots)

    def _apply_block_operations(self, req) -> None:
        """vllm/worker/worker.py, execute_worker: swap in, swap out, copy -- in that order, in front of everything else of the
        step, on every rank (the lists arrive with the broadcast request).  The engine is called only for a non-empty list."""
        for name, method in (("blocks_to_swap_in", "swap_in"), ("blocks_to_swap_out", "swap_out"), ("blocks_to_copy", "copy_blocks")):
            pairs = getattr(req, name, None)
            if pairs:
                getattr(self.engine, method)([(int(a), int(b)) for a, b in pairs])

    @property
    def _real_logprobs(self) -> bool:
        """Real logprobs are computed by the rank that returns the outputs (logits and probabilities are full-width on every
        rank); with disable_logprobs=True -- the default -- nobody computes any and the outputs carry the dummy entries."""
        return not self._disable_logprobs and self._rank == self._driver_rank

    def _check_requested_logprobs(self, sgml) -> None:
        """disable_logprobs=False: a request asking for more than max_logprobs is refused before anything is enqueued (the
        dummy lists of the default never looked at the numbers)."""
        if self._disable_logprobs:
            return
        for s in sgml:
            sp = s.sampling_params
            for name in ("logprobs", "prompt_logprobs"):
                n = getattr(sp, name, None) if sp is not None else None
                if n is not None and not 0 <= n <= self.max_logprobs:
                    raise ValueError(f"request {s.request_id}: {name} = {n} outside 0..max_logprobs = {self.max_logprobs}")

    @staticmethod
    def _num_logprobs(s) -> int:
        return (getattr(s.sampling_params, "logprobs", None) or 0) if s.sampling_params is not None else 0

    def _should_disable_all_speculation(self, req: ExecuteModelRequest) -> bool:
        return self.disable_by_batch_size is not None and req.running_queue_size >= self.disable_by_batch_size

    def _track_finished_requests(self, req: ExecuteModelRequest) -> None:
        """:1178-1188 plus the slot bookkeeping: a finished request gives its engine slot back."""
        for rid in req.finished_requests_ids:
            for seq_id in self._request_id_seq_id_mapping.get(rid, ()):
                self._seq_with_bonus_token_in_last_step.discard(seq_id)
            self._request_id_seq_id_mapping.pop(rid, None)
            self._release(rid)

    # ---- slots: one per sequence id.  self._slots: request id -> the slot of its first (for most requests: only) sequence;
    # self._groups: request id -> _SampleGroup, for the requests that hold more than one slot
    _groups: Optional[Dict[str, _SampleGroup]] = None

    def _group(self, rid: str) -> Optional[_SampleGroup]:
        return self._groups.get(rid) if self._groups else None

    def _release(self, rid: str) -> None:
        """The request leaves (finished, aborted, or about to be recomputed): ALL of its slots go back to the engine."""
        slot = self._slots.pop(rid, None)
        group = self._groups.pop(rid, None) if self._groups else None
        for b in (group.slots if group is not None else [] if slot is None else [slot]):
            self.engine.free_slot(b)

    def _taken_slots(self) -> Set[int]:
        return set(self._slots.values()).union(*(g.slots for g in (self._groups or {}).values()))

    @staticmethod
    def _only_seq(s: SequenceGroupMetadata) -> Tuple[int, SequenceData]:
        if len(s.seq_data) != 1:
            raise NotImplementedError("a prompt or a batch row carries exactly one sequence (beam search is not on the QSpec path)")
        return next(iter(s.seq_data.items()))

    @staticmethod
    def _num_samples(s: SequenceGroupMetadata) -> int:
        """Sequences a PROMPT starts: SamplingParams.best_of (default: n).  A request that comes back for recomputation with
        outputs already has its sequences: one.  Beam search is refused."""
        sp = s.sampling_params
        if sp is not None and getattr(sp, "use_beam_search", False):
            raise NotImplementedError("beam search (use_beam_search) is not on the QSpec path")
        _, data = SpecDecodeWorker._only_seq(s)
        if sp is None or data.get_output_len():
            return 1
        return max(1, int(getattr(sp, "best_of", None) or getattr(sp, "n", 1) or 1))

    def _sequence_rows(self, sgml) -> Tuple[list, Optional[List[int]]]:
        """One batch row per SEQUENCE: (rows, owner).  A group that arrives with several sequence ids (the samples of an
        n / best_of > 1 request, from their second step on) becomes one single-sequence row each, in its seq_data order;
        owner[r] = the index of row r's group in sgml.  Every group single-sequence: (sgml itself, None)."""
        if all(len(s.seq_data) == 1 for s in sgml):
            return sgml, None
        rows, owner = [], []
        for i, s in enumerate(sgml):
            if len(s.seq_data) == 1:
                rows.append(s)
                owner.append(i)
                continue
            if s.is_prompt:
                self._only_seq(s)   # raises
            sp = s.sampling_params
            if sp is not None and getattr(sp, "use_beam_search", False):
                raise NotImplementedError("beam search (use_beam_search) is not on the QSpec path")
            self._bind_samples(s)
            for seq_id, data in s.seq_data.items():
                tables = getattr(s, "block_tables", None)
                rows.append(SequenceGroupMetadata(
                    s.request_id, False, {seq_id: data}, getattr(s, "num_speculative_tokens", None),
                    {seq_id: tables[seq_id]} if tables and tables.get(seq_id) is not None else None, sp,
                    getattr(s, "do_sample", True), getattr(s, "token_chunk_size", None)))
                owner.append(i)
        return rows, owner

    def _bind_samples(self, s) -> None:
        """The scheduler names the samples of a group on their second step.  Each unknown sequence id (ascending) takes the
        reserved sample slot (ascending sample index) whose first token is that sequence's last output token; samples with
        equal first tokens are interchangeable up to their seed."""
        group = self._group(s.request_id)
        if group is None:
            if s.request_id not in self._slots:
                raise KeyError(f"request {s.request_id} was never prefilled on this worker (or has finished)")
            raise ValueError(f"request {s.request_id} arrives with {len(s.seq_data)} sequences but was admitted with one")
        for seq_id in sorted(q for q in s.seq_data if q not in group.bound):
            toks = s.seq_data[seq_id].get_token_ids()
            taken = set(group.bound.values())
            slot = next((b for b, t in zip(group.slots, group.first) if b not in taken and toks and t == toks[-1]), None)
            if slot is None:
                raise ValueError(f"request {s.request_id}: sequence {seq_id} ends in a token none of the group's unbound samples "
                                 "produced")
            group.bound[seq_id] = slot

    def _slot_of(self, rid: str, seq_id: int) -> int:
        group = self._group(rid)
        if group is not None:
            if seq_id not in group.bound:
                raise KeyError(f"request {rid}: sequence {seq_id} is not one of the group's sequences")
            return group.bound[seq_id]
        return self._slots[rid]

    def _prompt_window(self, s) -> Tuple[int, int, bool]:
        """(context, q, terminal) of a prompt group, as the reference's model runner computes them (model_runner.py:488-590):
        context tokens have valid K/V -- earlier chunks (SequenceData.get_num_computed_tokens) or a prefix-cache hit
        (computed_block_nums) --, the pass computes the q tokens behind them, terminal: it reaches the end of the token list.
        A hit that covers the whole chunk leaves its last token to compute."""
        _, data = self._only_seq(s)
        total = data.get_len()
        get = getattr(data, "get_num_computed_tokens", None)
        context = int(get()) if get is not None else 0
        seq_len = min(total, context + (getattr(s, "token_chunk_size", None) or total))
        blocks = getattr(s, "computed_block_nums", None) or ()
        hit = len(blocks) * self.engine.block_size if blocks else 0
        if context < hit < seq_len:
            context = hit
        elif hit >= seq_len:
            context = seq_len - 1
        return context, seq_len - context, seq_len == total

    def _admit(self, prompts: List[SequenceGroupMetadata], prompt_logprobs: bool = False) -> List[int]:
        """Prompts (or preempted requests coming back for recomputation) take the first free slots; their prompt pass
        is ONE varlen forward (engine.add_sequences_to); prompt_logprobs: hand the requests' SamplingParams.prompt_logprobs
        to it (disable_logprobs=False, on the rank that returns the outputs).  The engine validates every slot, prompt and block table
        before its first forward; should the admission still fail half-way (several prompt passes, one raising), the
        slots it had occupied are given back, so that worker and engine never disagree about which slots are free.
        Prefix hits and chunked prefill: every prompt is translated by _prompt_window; a request whose slot holds a partly
        computed prompt with exactly the tokens the scheduler counts continues in it, any other known request starts over.
        The new engine keywords are used only when some request needs them."""
        windows = [self._prompt_window(s) for s in prompts]
        for s, (_, _, terminal) in zip(prompts, windows):
            if getattr(s, "do_sample", True) and not terminal:
                raise ValueError(f"request {s.request_id}: do_sample on a prompt chunk that does not end the prompt")
        prefilling = getattr(self.engine, "is_prefilling", None)
        resumed = []
        for s in prompts:
            slot = self._slots.get(s.request_id)
            get = getattr(self._only_seq(s)[1], "get_num_computed_tokens", None)
            resumed.append(slot is not None and prefilling is not None and prefilling(slot) and get is not None
                           and int(get()) == self.engine.num_computed_tokens(slot))
        counts = [0 if r else self._num_samples(s) for s, r in zip(prompts, resumed)]   # (a request sampling m sequences takes m slots)
        for s, r in zip(prompts, resumed):
            if s.request_id in self._slots and not r:          # recomputation: start over
                self._release(s.request_id)
        taken = self._taken_slots()
        free = [b for b in range(self.max_num_seqs) if b not in taken]
        if len(free) < sum(counts):
            short = next(i for i in range(len(prompts)) if sum(counts[:i + 1]) > len(free))
            raise RuntimeError(f"no free sequence slot for request {prompts[short].request_id}: "
                               f"max_num_seqs={self.max_num_seqs} are running")
        it = iter(free)
        slots, samples = [], []
        for s, m in zip(prompts, counts):            # the request's own slot, then those of its additional samples
            if m == 0:                               # (a resumed request keeps what it holds)
                group = self._group(s.request_id)
                slots.append(self._slots[s.request_id])
                samples.append(list(group.slots[1:]) if group is not None else [])
                continue
            slots.append(next(it))
            samples.append([next(it) for _ in range(m - 1)])
        fresh = [b for b, extra, r in zip(slots, samples, resumed) if not r for b in [b, *extra]]
        toks, tables, npts, plps = [], [], [], []
        try:
            for s, b, r, (_, _, terminal) in zip(prompts, slots, resumed, windows):
                seq_id, data = self._only_seq(s)
                toks.append(data.get_token_ids())
                tables.append(s.block_tables.get(seq_id) if s.block_tables else None)
                sp = s.sampling_params   # before the prompt pass: the first token is sampled with them too
                seed = getattr(sp, "seed", None)   # (forwarded only when set: an engine double need not know the keyword)
                extra = {} if seed is None else {"seed": seed}
                lp = self._logit_processor_args(sp)
                lp.update(self._token_constraint_args(sp))
                lp.update(self._guide_args(sp, getattr(getattr(self, "model_config", None), "vocab_size", None)))
                extra.update(lp)
                if not r:   # (they belong to the request: a resumed one has them since its first chunk)
                    self.engine.set_sampling_params(b, getattr(sp, "temperature", 0.0) or 0.0, getattr(sp, "top_k", -1) or -1,
                                                    getattr(sp, "top_p", 1.0) if sp is not None else 1.0, **extra)
                # recomputation: prompt + outputs come back as one token list; penalties and min_tokens tell them apart
                # (nothing else does: a request without them is admitted exactly as before)
                npts.append(len(data.get_prompt_token_ids()) if lp and data.get_output_len() else None)
                # (a chunk that does not end the prompt never samples; its rows still belong to the prompt's logprobs)
                plps.append(getattr(sp, "prompt_logprobs", None) if prompt_logprobs and (s.do_sample or not terminal) else None)
            kw = {}   # (each only when needed: an engine double need not know the keywords)
            if any(n is not None for n in npts):
                kw["num_prompt_tokens"] = npts
            if any(n is not None for n in plps):
                kw["prompt_logprobs"] = plps
            if any(e for e, r in zip(samples, resumed) if not r):
                kw["sample_slots"] = [[] if r else e for e, r in zip(samples, resumed)]
            if any(c > 0 or not terminal for c, _, terminal in windows):
                kw["num_computed_tokens"] = [c for c, _, _ in windows]
                kw["token_chunk_sizes"] = [q for _, q, _ in windows]
            self.engine.add_sequences_to(slots, toks, tables, **kw)
        except Exception:
            for b in fresh:
                self.engine.free_slot(b)
            raise
        for s, slot, extra, r in zip(prompts, slots, samples, resumed):
            if r:
                continue
            self._slots[s.request_id] = slot
            seq_id = self._only_seq(s)[0]
            self._request_id_seq_id_mapping[s.request_id].add(seq_id)
            if extra:
                if self._groups is None:
                    self._groups = {}
                self._groups[s.request_id] = _SampleGroup(slots=[slot] + extra, bound={seq_id: slot})
        return slots

    @staticmethod
    def _logit_processor_args(sp) -> Dict[str, Any]:
        """The min_p / penalty / min_tokens keywords of engine.set_sampling_params for a request, EMPTY when every field has
        its default (as `seed`: such a request makes exactly the calls it always made).  The stop ids of min_tokens are
        `all_stop_token_ids` where the object has it (a vLLM SamplingParams: stop_token_ids + the EOS id), else
        `stop_token_ids`; they are forwarded only with a min_tokens > 0, the one thing that reads them."""
        if sp is None:
            return {}
        out: Dict[str, Any] = {}
        for name, default in (("min_p", 0.0), ("presence_penalty", 0.0), ("frequency_penalty", 0.0),
                              ("repetition_penalty", 1.0), ("min_tokens", 0)):
            v = getattr(sp, name, None)
            if v is not None and v != default:
                out[name] = v
        if out.get("min_tokens", 0) > 0:
            stop = getattr(sp, "all_stop_token_ids", None)
            if stop is None:
                stop = getattr(sp, "stop_token_ids", None)
            stop = sorted(set(int(t) for t in (stop or ())))
            if len(stop) > 16:
                raise ValueError(f"min_tokens with {len(stop)} stop token ids: at most 16 are supported")
            out["stop_token_ids"] = tuple(stop)
        return out

    @staticmethod
    def _token_constraint_args(sp) -> Dict[str, Any]:
        """The logit_bias / allowed_token_ids / bad_words_token_ids keywords of engine.set_sampling_params for a request, EMPTY
        when it has none.  Sources: the plain fields (logit_bias keys may be strings; the biases are clamped to [-100, 100]
        as the reference's lowering does, logits_processors.py:62-66) and the three processors that lowering leaves in
        `logits_processors` (llm_engine.py:1950-2009), recognised by name and attributes -- nothing is imported:
          functools.partial(logit_bias_logits_processor, {id: bias}); AllowedTokenIdsLogitsProcessor with `allowed_ids`, or,
          once it has been called (the objects are cached and shared between requests), with `mask` alone (True = forbidden);
          NoBadWordsLogitsProcessor with `bad_words_ids`.
        A field and a processor that say the same thing are one constraint: biases are merged by id (the processor's value is
        the one the reference would apply), allowed sets intersect, bad words are deduplicated.  Any other callable in
        logits_processors is ignored, as before."""
        if sp is None:
            return {}
        bias: Dict[int, float] = {}
        allowed = None
        words: List[Tuple[int, ...]] = []
        try:
            for t, b in (getattr(sp, "logit_bias", None) or {}).items():
                bias[int(t)] = min(100.0, max(-100.0, float(b)))
        except (TypeError, ValueError) as exc:
            raise ValueError("Found token_id in logit_bias that is not an integer or string representing an integer") from exc
        ids = getattr(sp, "allowed_token_ids", None)
        if ids is not None:
            allowed = set(int(t) for t in ids)
            if not allowed:
                raise ValueError("Empty allowed_token_ids provided")
        for w in (getattr(sp, "bad_words_token_ids", None) or ()):
            words.append(tuple(int(t) for t in w))
        for proc in (getattr(sp, "logits_processors", None) or ()):
            name = type(proc).__name__
            if isinstance(proc, functools.partial) and getattr(proc.func, "__name__", "") == "logit_bias_logits_processor" \
                    and proc.args and isinstance(proc.args[0], dict):
                for t, b in proc.args[0].items():
                    bias[int(t)] = float(b)
            elif name == "AllowedTokenIdsLogitsProcessor" and (getattr(proc, "allowed_ids", None) is not None
                                                              or getattr(proc, "mask", None) is not None):
                if getattr(proc, "allowed_ids", None) is not None:
                    got = set(int(t) for t in proc.allowed_ids)
                else:
                    mask = proc.mask.tolist() if hasattr(proc.mask, "tolist") else list(proc.mask)
                    got = set(i for i, forbidden in enumerate(mask) if not forbidden)
                allowed = got if allowed is None else allowed & got
                if not allowed:
                    raise ValueError("Empty allowed_token_ids provided")
            elif name == "NoBadWordsLogitsProcessor" and getattr(proc, "bad_words_ids", None) is not None:
                words.extend(tuple(int(t) for t in w) for w in proc.bad_words_ids)
        out: Dict[str, Any] = {}
        if bias:
            out["logit_bias"] = bias
        if allowed is not None:
            out["allowed_token_ids"] = sorted(allowed)
        if words:
            out["bad_words_token_ids"] = [list(w) for w in dict.fromkeys(words)]
        return out

    @staticmethod
    def _guide_args(sp, vocab: Optional[int]) -> Dict[str, Any]:
        """The `guide` keyword of engine.set_sampling_params for a request, EMPTY when it has none.  Sources: the worker's own
        `guided_fsm` field (a TokenFSM) and the processor the reference's engine lowers guided_decoding to, at index 0 of
        logits_processors (llm_engine.py:1950-2009; outlines_logits_processors.py:34-93), recognised by name and attributes --
        nothing is imported: an object whose class is named RegexLogitsProcessor or JSONLogitsProcessor, or any processor with
        a `_guide` that TokenFSM.from_guide accepts (its `_fsm_state`, the reference's hash chain, is ignored: the state is
        rebuilt from the request's outputs).  NotImplementedError naming the class, never silence: a guided processor whose
        guide is not a finite automaton over int states (CFGLogitsProcessor, CFGState), more than one guide on a request, and
        a `guided_decoding` that arrives un-lowered (there is no tokenizer here to lower it with)."""
        if sp is None:
            return {}
        if getattr(sp, "guided_decoding", None) is not None:
            raise NotImplementedError(f"SamplingParams.guided_decoding = {type(sp.guided_decoding).__name__} arrived un-lowered: "
                                      "this worker has no tokenizer; hand it the lowered processor (the engine's "
                                      "_build_logits_processors) or a TokenFSM in guided_fsm")
        found = []
        own = getattr(sp, "guided_fsm", None)
        if own is not None:
            if not isinstance(own, TokenFSM):
                raise ValueError("guided_fsm must be a TokenFSM")
            found.append(own)
        for proc in (getattr(sp, "logits_processors", None) or ()):
            name, guide = type(proc).__name__, getattr(proc, "_guide", None)
            if name == "CFGLogitsProcessor" or type(guide).__name__ == "CFGGuide":
                raise NotImplementedError(f"{name}: a context-free-grammar guide is not a finite automaton over int states")
            if name not in ("RegexLogitsProcessor", "JSONLogitsProcessor") and guide is None:
                continue
            if guide is None or vocab is None:
                raise NotImplementedError(f"{name}: no `_guide` to lower" if guide is None else f"{name}: the vocabulary is unknown")
            try:
                found.append(TokenFSM.from_guide(guide, int(vocab)))
            except TypeError as exc:
                raise NotImplementedError(f"{name}: {exc}") from exc
        if len(set(id(f) for f in found)) > 1:
            raise NotImplementedError("more than one guide on one request")
        return {"guide": found[0]} if found else {}

    def _decode_slots(self, sgml) -> List[int]:
        """Engine slots of a decode batch in request order; refreshes block tables (the engine uploads a table only when
        it changed); cross-checks the lengths."""
        slots = []
        for s in sgml:
            if s.request_id not in self._slots:
                raise KeyError(f"request {s.request_id} was never prefilled on this worker (or has finished)")
            seq_id, data = self._only_seq(s)
            slot = self._slot_of(s.request_id, seq_id)
            if s.block_tables and s.block_tables.get(seq_id) is not None:
                self.engine.set_block_table(slot, s.block_tables[seq_id])
            if data.output_token_ids and data.get_len() != self.engine._len_ub[slot]:
                raise ValueError(f"request {s.request_id}: the scheduler holds {data.get_len()} tokens, the worker "
                                 f"{self.engine._len_ub[slot]}: outputs were dropped or re-ordered between steps")
            slots.append(slot)
        if len(set(slots)) != len(slots):
            raise ValueError("a request (or a sequence of it) appears twice in seq_group_metadata_list")
        return slots

    def _read_cycle(self):
        """The one host read of a cycle: output tokens + the cycle's error word.  On a timed-out device-side hand-off the
        cycle is re-run once without hand-offs (engine.recover(), bit-identical results); every rank reads the same
        all-reduced word, so all ranks re-run -- or raise -- together."""
        out, err = self.engine.read_outputs()
        if err:
            self.engine.recover()
            out, err = self.engine.read_outputs()
            if err:
                raise DeviceHandoffTimeout("a device-side hand-off timed out during this cycle and again in the replay "
                                           "without hand-offs (results invalid)")
        return out

    def _prefill_rows(self, sgml, prompts: List[int], tokens: List[int], more: Dict[int, list], real: Dict[int, tuple],
                      prompt_real: Dict[int, list]) -> None:
        """The prompt rows `prompts` of a batch: one prompt pass (_admit), then per row whose pass ended its prompt the first
        token (tokens[i]), the additional samples (more[i]) and, with real logprobs, their entries (real[i], prompt_real[i]: the
        WHOLE prompt's, gathered over its chunks).  A chunk that does not end its prompt leaves its row as it is."""
        ended = [i for i in prompts if self._prompt_window(sgml[i])[2]]   # (read before the pass)
        slots = dict(zip(prompts, self._admit([sgml[i] for i in prompts], prompt_logprobs=self._real_logprobs)))
        first = self.engine.gen_tokens[:, 0].cpu()
        self._check_out_of_cycle_errors("the prompt pass")
        for i in ended:
            tokens[i] = int(first[slots[i]])
            group = self._group(sgml[i].request_id)
            if group is not None:       # the samples' first tokens: what binds their sequence ids on the next step
                group.first = [int(first[b]) for b in group.slots]
                more[i] = [[t, None] for t in group.first[1:]]
        self.scorer_calls += 1          # one scorer call for the prompt batch, as in the reference
        if self._real_logprobs and ended:
            real.update(self._token_logprobs("first", [sgml[i] for i in ended], ended, [slots[i] for i in ended], tokens))
            for i in more:              # (per sample, as for a single sequence)
                sample_slots = self._group(sgml[i].request_id).slots[1:]
                n_top = self._num_logprobs(sgml[i])
                lp, rank, top, tlp = (t.tolist() for t in self.engine.token_logprobs(
                    "first", sample_slots, [t for t, _ in more[i]], n_top))
                for j, entry in enumerate(more[i]):
                    entry[1] = (rank[j], lp[j], top[j][:n_top], tlp[j][:n_top])
            for i in ended:
                got = self.engine.take_prompt_logprobs(slots[i])
                if got is not None:
                    prompt_real[i] = self._prompt_logprob_dicts(sgml[i], got)

    def _run_no_spec(self, req: ExecuteModelRequest, skip_proposer: bool) -> List[SamplerOutput]:
        """:666-720.  Prompts: W4A16 prefill, first token sampled by the target.  Decode sequences with speculation off
        for this step: the scorer alone, one token each.  A batch may hold both (prompts first, as vLLM orders them).
        Output: `_serialize_sampler_output_no_logprobs` (:582-664)."""
        groups = req.seq_group_metadata_list
        sgml, owner = self._sequence_rows(groups)    # one row per sequence
        assert req.w4a4 is False
        tokens = [VLLM_INVALID_TOKEN_ID] * len(sgml)
        more: Dict[int, list] = {}             # batch index of a prompt -> [token, logprob entry or None] per additional sample
        real: Dict[int, tuple] = {}            # batch index -> (rank, logprob, top ids, top logprobs) of its token
        prompt_real: Dict[int, list] = {}      # batch index -> its prompt_logprobs list
        prompts = [i for i, s in enumerate(sgml) if s.is_prompt]
        decodes = [i for i, s in enumerate(sgml) if not s.is_prompt]
        dslots = self._decode_slots([sgml[i] for i in decodes])     # before admissions: validates the running ones
        if prompts:
            self._prefill_rows(sgml, prompts, tokens, more, real, prompt_real)
        if decodes:
            tok = self._no_spec_step(dslots)
            for i, slot in zip(decodes, dslots):
                tokens[i] = tok[slot]
            if self._real_logprobs:
                real.update(self._token_logprobs("no_spec", [sgml[i] for i in decodes], decodes, dslots, tokens))
        return self._regroup([self._serialize_sampler_output_no_logprobs(sgml, tokens, real, prompt_real, more)], owner, len(groups))

    @staticmethod
    def _regroup(outs: List[SamplerOutput], owner: Optional[List[int]], num_groups: int) -> List[SamplerOutput]:
        """Per-sequence rows back to `outputs[i]` = the i-th sequence group: the samples of a group's rows in one output."""
        if owner is None:
            return outs
        for out in outs:
            merged: List[Optional[CompletionSequenceGroupOutput]] = [None] * num_groups
            for row, i in zip(out.outputs, owner):
                if merged[i] is None:
                    merged[i] = row
                else:
                    merged[i].samples.extend(row.samples)
            out.outputs = merged
        return outs

    def _token_logprobs(self, kind: str, sgs, idx: List[int], slots: List[int], tokens: List[int]) -> Dict[int, tuple]:
        """disable_logprobs=False on the paths outside the cycle (`_run_no_spec` returns the scorer's own SamplerOutput there,
        :710-713): batch index -> (rank, logprob, top ids, top logprobs) of the token each of `sgs` has just received, from
        the distribution it was sampled from (engine.token_logprobs)."""
        num_top = max([self._num_logprobs(s) for s in sgs], default=0)
        lp, rank, top, tlp = (t.tolist() for t in self.engine.token_logprobs(kind, slots, [tokens[i] for i in idx], num_top))
        return {i: (rank[j], lp[j], top[j][:self._num_logprobs(s)], tlp[j][:self._num_logprobs(s)])
                for j, (i, s) in enumerate(zip(idx, sgs))}

    def _prompt_logprob_dicts(self, s, got) -> List[Dict[int, Logprob]]:
        """SamplingParams.prompt_logprobs = n: for every prompt token but the first its logprob and rank + the n best, from the
        target's RAW logits ("Logprobs").  A recomputed request's token list also holds its outputs: the prompt's
        rows come first."""
        ids = self._only_seq(s)[1].get_prompt_token_ids()[1:]
        lp, rank, top, tlp = (t[:len(ids)].tolist() for t in got)
        return [create_logprobs_output(t, rank[j], lp[j], [v if v >= 0 else None for v in top[j]], tlp[j])
                for j, t in enumerate(ids)]

    def _check_out_of_cycle_errors(self, what: str) -> None:
        """Prompt passes and non-speculative steps run outside the captured cycle (other stream, no error-word collection
        at their end): their launches are followed by a host read anyway, so the sticky words of EVERY hand-off workspace
        of the device and of the one-shot all-reduce are checked from the host there.  No replay for these: the call fails."""
        if self.engine.error_flag():
            raise DeviceHandoffTimeout(f"a device-side hand-off timed out during {what} (results invalid)")

    def _no_spec_step(self, dslots: List[int]) -> Dict[int, int]:
        self.engine.step_no_spec(participants=dslots)
        self.scorer_calls += 1
        out = self.engine.out_tokens[:, 0].cpu()
        self._check_out_of_cycle_errors("a non-speculative decode step")
        self.engine.note_emitted([1 if b in dslots else 0 for b in range(self.max_num_seqs)])
        return {b: int(out[b]) for b in dslots}

    def _serialize_sampler_output_no_logprobs(self, sgml, tokens: List[int], real: Optional[Dict[int, tuple]] = None,
                                              prompt_real: Optional[Dict[int, list]] = None,
                                              more: Optional[Dict[int, list]] = None) -> SamplerOutput:
        """:582-664: only the token ids are populated; a sequence group without a sample (`do_sample` False: a
        non-terminal prompt chunk) still gets its own, empty, output.  real / prompt_real (disable_logprobs=False): the
        entries that replace the dummies, by batch index.  more: the additional samples of a prompt that starts several sequences,
        [token, logprob entry or None] each -- all of a group's samples name the prompt's sequence as their parent, as the
        reference's sampler does."""
        outs = []
        for i, (s, tok) in enumerate(zip(sgml, tokens)):
            if not s.do_sample:
                outs.append(CompletionSequenceGroupOutput(samples=[], prompt_logprobs=None))
                continue
            seq_id, data = self._only_seq(s)
            sp = s.sampling_params
            prompt_logprobs = None
            if s.is_prompt and sp is not None and sp.prompt_logprobs is not None and sp.prompt_logprobs > 0:
                prompt_logprobs = [create_logprobs_output(t, -1, 0.0, [], []) for t in data.get_prompt_token_ids()[1:]]
            if prompt_real and i in prompt_real:
                prompt_logprobs = prompt_real[i]
            rank, lp, top, tlp = real[i] if real and i in real else (-1, 0.0, [], [])
            outs.append(create_sequence_group_output(tok, rank, lp, seq_id, [v if v >= 0 else None for v in top], tlp,
                                                     prompt_logprobs))
            for t, entry in (more or {}).get(i, ()):
                rank, lp, top, tlp = entry if entry is not None else (-1, 0.0, [], [])
                outs[-1].samples.append(SequenceOutput(parent_seq_id=seq_id, output_token=t, logprobs=create_logprobs_output(
                    t, rank, lp, [v if v >= 0 else None for v in top], tlp)))
        return SamplerOutput(outputs=outs)

    def _run_speculative_decoding_step(self, req: ExecuteModelRequest, num_lookahead_slots: int) -> List[SamplerOutput]:
        """:758-858 as one graph replay: proposals (w4a4=True) -> scoring (w4a4=False) -> verification.  Requests with
        `num_speculative_tokens == 0` in an otherwise speculative batch get the target's one token (the reference scores
        them with proposal length 0, top1_proposer.py:103-135): they sit out the cycle and take the scorer-only step."""
        k = self.engine.k
        if num_lookahead_slots != k:
            raise ValueError(f"num_lookahead_slots = {num_lookahead_slots}, but the cycle was captured for "
                             f"num_speculative_tokens = {k} (SpeculativeConfig.num_speculative_tokens)")
        groups = req.seq_group_metadata_list
        sgml, owner = self._sequence_rows(groups)    # one row per sequence
        # Prompt chunks scheduled into a speculative step (chunked prefill; spec_decode_worker.py:484-537, 818-825): their own
        # W4A16 forward in front of the cycle, which the proposer never sees (:827).  A prompt's row is [first token, -1 x k]
        # when the chunk ends the prompt and all -1 otherwise; the request joins the cycle with the next step.
        prompts = [i for i, s in enumerate(sgml) if s.is_prompt]
        decodes = [i for i, s in enumerate(sgml) if not s.is_prompt]
        slots: List[Optional[int]] = [None] * len(sgml)
        for i, b in zip(decodes, self._decode_slots([sgml[i] for i in decodes])):   # before admissions: validates the running ones
            slots[i] = b
        rows = [[VLLM_INVALID_TOKEN_ID] * (k + 1) for _ in sgml]
        more: Dict[int, list] = {}
        first_real: Dict[int, tuple] = {}
        prompt_real: Dict[int, list] = {}
        if prompts:
            first_tokens = [VLLM_INVALID_TOKEN_ID] * len(sgml)
            self._prefill_rows(sgml, prompts, first_tokens, more, first_real, prompt_real)
            for i in prompts:
                rows[i][0] = first_tokens[i]
        spec = [i for i in decodes if sgml[i].num_speculative_tokens != 0]
        nospec = [i for i in decodes if sgml[i].num_speculative_tokens == 0]
        req.w4a4 = True                                   # :799
        self.proposer_calls += k
        scorer_req = req.clone(groups)                    # mqa_scorer.py:65: clone drops w4a4 -> W4A16
        assert scorer_req.w4a4 is False
        req.w4a4 = False                                  # :812
        self.scorer_calls += 1
        spec_slots = [slots[i] for i in spec]
        self.engine.step(participants=spec_slots)
        out = self._read_cycle()
        self.engine.note_emitted([int((out[b] != -1).sum()) if b in spec_slots else 0 for b in range(out.shape[0])])
        for i in spec:
            rows[i] = out[slots[i]].tolist()
        cycle_real = None
        if self._real_logprobs and spec:
            cycle_real = self.engine.token_logprobs("cycle", spec_slots, [[max(t, 0) for t in rows[i]] for i in spec],
                                                    max(self._num_logprobs(sgml[i]) for i in spec))
        riders = dict(first_real) or None
        if nospec:
            tok = self._no_spec_step([slots[i] for i in nospec])
            for i in nospec:
                rows[i][0] = tok[slots[i]]
            if self._real_logprobs:
                riders = {**first_real, **self._token_logprobs("no_spec", [sgml[i] for i in nospec], nospec,
                                                               [slots[i] for i in nospec], [r[0] for r in rows])}
        outs = self._create_output_sampler_list(sgml, rows, k, slots, spec, cycle_real, riders)
        if outs:   # step 0 carries what only a prompt row has: the additional samples and the prompt's logprobs
            for i, extra in more.items():
                seq_id = self._only_seq(sgml[i])[0]
                for t, entry in extra:
                    rank, lp, top, tlp = entry if entry is not None else (-1, 0.0, [], [])
                    logprobs = create_logprobs_output(t, rank, lp, [v if v >= 0 else None for v in top], tlp)
                    outs[0].outputs[i].samples.append(SequenceOutput(parent_seq_id=seq_id, output_token=t, logprobs=logprobs))
            for i, lps in prompt_real.items():
                outs[0].outputs[i].prompt_logprobs = lps
        return self._regroup(outs, owner, len(groups))

    def _create_output_sampler_list(self, sgml, rows: List[List[int]], k: int, slots: List[int],
                                    spec: Optional[List[int]] = None, cycle_real=None,
                                    riders: Optional[Dict[int, tuple]] = None) -> List[SamplerOutput]:
        """:972-1063: [batch, k+1] accepted token ids -> one SamplerOutput per step, padded with -1 so that every
        sequence has the same number of outputs; the list stops at the first step in which no sequence emitted a token
        (:1023-1026); metrics ride on the first one.  disable_logprobs=False: cycle_real = engine.token_logprobs("cycle", ...)
        of the batch indices `spec`, riders = the step-0 entries of the requests that took the scorer-only step."""
        batch_size, num_steps = len(sgml), k + 1
        by_step = [[rows[b][j] for b in range(batch_size)] for j in range(num_steps)]
        ranks, lps, topk_lps, topk_ids = self._create_dummy_logprob_lists(batch_size, num_steps, self.max_logprobs)
        if cycle_real is not None:
            self._fill_logprob_lists(ranks, lps, topk_lps, topk_ids, spec, cycle_real)
        for b, (rank, lp, top, tlp) in (riders or {}).items():
            ranks[0][b], lps[0][b], topk_ids[0][b], topk_lps[0][b] = rank, lp, [v if v >= 0 else None for v in top], tlp
        seq_ids = [self._only_seq(s)[0] for s in sgml]                                   # get_all_seq_ids_and_request_ids
        num_logprobs_per_seq = [(s.sampling_params.logprobs or 0) if s.sampling_params is not None else 0
                                for s in sgml]                                           # get_all_num_logprobs
        outs: List[SamplerOutput] = []
        for step in range(num_steps):
            if all(t == VLLM_INVALID_TOKEN_ID for t in by_step[step]):
                break
            outs.append(SamplerOutput(outputs=[
                create_sequence_group_output(
                    token_id=by_step[step][b], token_id_logprob_rank=ranks[step][b], token_id_logprob=lps[step][b],
                    seq_id=seq_ids[b], topk_token_ids=topk_ids[step][b][:num_logprobs_per_seq[b]],
                    topk_logprobs=topk_lps[step][b][:num_logprobs_per_seq[b]])
                for b in range(batch_size)]))
        self._track_sequences_with_bonus_tokens(sgml, by_step)
        if outs and not self._disable_log_stats:
            m = self._metrics.maybe_collect_rejsample_metrics(k)
            if m is not None:
                outs[0].spec_decode_worker_metrics = m
        return outs

    @staticmethod
    def _create_dummy_logprob_lists(batch_size: int, num_steps: int, num_top_k: int):
        """:1083-1127: ranks -1, logprobs 0.0, top-k entries None (dropped by create_logprobs_output)."""
        ranks = [[-1] * batch_size for _ in range(num_steps)]
        lps = [[0.0] * batch_size for _ in range(num_steps)]
        topk_lps = [[[None] * num_top_k for _ in range(batch_size)] for _ in range(num_steps)]
        topk_ids = [[[None] * num_top_k for _ in range(batch_size)] for _ in range(num_steps)]
        return ranks, lps, topk_lps, topk_ids

    @staticmethod
    def _fill_logprob_lists(ranks, lps, topk_lps, topk_ids, spec: List[int], cycle_real) -> None:
        """:1129-1176 (`disable_logprobs=False`): log of the target's probabilities of the cycle, the accepted token's
        logprob and rank (vllm/spec_decode/util.py:34-52) and the best per position -- one kernel launch on the engine's
        [B, k+1, V] target distribution (engine.token_logprobs; a position without a token was asked about token 0, as the
        reference's clamp does) instead of torch passes over it; here only the lists are filled, [step][batch index]."""
        lp, rank, top, tlp = (t.tolist() for t in cycle_real)
        for j, b in enumerate(spec):
            for step in range(len(ranks)):
                ranks[step][b], lps[step][b] = rank[j][step], lp[j][step]
                topk_ids[step][b] = [v if v >= 0 else None for v in top[j][step]]
                topk_lps[step][b] = tlp[j][step]

    def _track_sequences_with_bonus_tokens(self, sgml, accepted_token_ids_by_step: List[List[int]]) -> None:
        """:1190-1210: a sequence whose last step position holds a token (!= -1) received the bonus token."""
        for idx, s in enumerate(sgml):
            seq_id, _ = self._only_seq(s)
            if accepted_token_ids_by_step[-1][idx] == VLLM_INVALID_TOKEN_ID:
                self._seq_with_bonus_token_in_last_step.discard(seq_id)
            else:
                self._seq_with_bonus_token_in_last_step.add(seq_id)
            self._request_id_seq_id_mapping[s.request_id].add(seq_id)
