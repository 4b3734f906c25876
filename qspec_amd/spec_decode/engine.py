"""QSpecEngine: the draft -> verify -> accept cycle with all state resident on the GPU.

What the reference does per step on the host (vllm/spec_decode/spec_decode_worker.py:758-1063) --
toggle `w4a4`, run the k-step draft loop (draft_model_runner.py:169-376), build the MQA scoring batch
(mqa_scorer.py:12-114), run the target, rejection-sample, `.tolist()` three times -- becomes here ONE
captured hipGraph per cycle:

    prepare_draft -> k x [ forward(W4A4) -> lm_head -> softmax/argmax -> advance_step ]
                  -> prepare_verify -> forward(W4A16) -> lm_head -> softmax/argmax
                  -> rejection sample -> commit

The draft and the verify pass share one packed-int4 weight buffer per layer and one paged KV cache
(spec_decode_worker.py:339-345,421-444; vllm/worker/worker.py:309-327); the verify pass rewrites the
k+1 KV slots the draft pass wrote (mqa_scorer.py:42-60), which is also why no bonus-token batch
expansion is needed (multi_step_worker.py:74-80).

Batch membership: the graph is captured for `max_batch` SLOTS; a slot is empty while seq_lens[slot] == 0 and then
runs through the cycle as a dummy that writes nothing and emits nothing (include/qspec_hip.h, spec-decode glue), so
requests join (`add_sequence`) and leave (`free_slot`) between replays without re-capturing.  Block tables are per
slot and may be set from the scheduler's tables (`set_block_table`); by default slot b owns a contiguous range.

Capacity is part of the contract: `step()` refuses (ValueError, nothing enqueued) a cycle that could write beyond a
sequence's block table / max_model_len / output buffer, from a host-side upper bound of every sequence length that is
exact after `sync_lens()` (the worker syncs once per cycle anyway) and grows by k+1 per unsynced step otherwise.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional, Sequence

import os

import torch

from .. import ops
from ..model import AttentionMetadata, QuarotLlamaForCausalLM, Scratch
from .metrics import SpecDecodeWorkerMetrics, metrics_from_counters
from .rejection_sampler import RejectionSampler
from .slot_sampling import SlotSampling

ATTN_CHUNK = 128  # keys per context split of the attention kernel (QS_ATT_CHUNK)


def n_splits_for(ctx: int, n_groups: int = 0) -> int:
    """Context splits of the attention kernel.  Decode (n_groups = sequences x kv heads x row blocks > 0): enough
    workgroups to occupy the 256 CUs (8 at batch 4 -- measured best: 6 and 12+ are slower), independent of the context
    length: a split longer than 128 keys is walked in 128-key chunks inside the kernel, so the partials the next launch
    merges do not grow with the context.  Prefill-sized queries (n_groups = 0) fill the chip with row blocks: 1."""
    if n_groups > 0:
        forced = int(os.environ.get("QSPEC_ATTN_SPLITS", "0"))   # dev knob for sweeps
        if forced > 0:
            return forced
        n = max(1, min(16, (256 + n_groups - 1) // n_groups))
        if n_groups > 64 and 256 % n_groups:
            # group counts that do not divide the chip (Llama-2-13B at batch 4: 4 x 40 kv heads = 160): two workgroups are
            # resident per CU, so fill the 512 slots -- 160 x 3 = 480 workgroups of 171 keys instead of 320 of 256, of which
            # 64 CUs carried two (cycle 13.49 -> 12.99 ms; 4 splits = 640 workgroups: 13.28)
            n = max(n, min(16, 512 // n_groups))
        return n
    return 1


PREFILL_SPLIT_ROWS = 64        # rows of a workgroup of the prompt attention kernels (QS_FA_ROWS)
# Kmin, the shortest context split worth a workgroup of its own: measured (profiles/prefix_attention.txt)
PREFILL_SPLIT_MIN_KEYS = 512


def prefill_splits(q_lens: Sequence[int], ctx_lens: Sequence[int], num_kv_heads: int, group: int) -> int:
    """Context splits of the attention of a PROMPT pass (q_lens[i] query tokens at the end of ctx_lens[i] keys; group = query
    heads per kv head).  No sequence with keys in front of its queries -- every pass before prefix hits and chunked prefill
    existed --: 1, the unsplit prompt kernel.  Otherwise the row blocks W = sum ceil(q group / 64) x kv heads that the unsplit
    kernel would launch are multiplied until they fill the 256 CUs, S = 256 // W in 1 .. 16, but no split shorter than
    PREFILL_SPLIT_MIN_KEYS keys: S <= ceil(longest context / Kmin)."""
    if all(int(c) == int(q) for q, c in zip(q_lens, ctx_lens)):
        return 1
    W = sum(-(-int(q) * group // PREFILL_SPLIT_ROWS) for q in q_lens) * num_kv_heads
    S = max(1, min(16, 256 // max(W, 1)))
    return max(1, min(S, -(-max(int(c) for c in ctx_lens) // PREFILL_SPLIT_MIN_KEYS)))


class QSpecEngine:
    def __init__(self, model: QuarotLlamaForCausalLM, num_speculative_tokens: int = 3, max_batch: int = 4,
                 max_model_len: int = 1024, block_size: int = 16, max_new_tokens: int = 1024, use_graph: bool = True,
                 seed: int = 0, num_blocks: Optional[int] = None, acceptance_sampler=None, kv_cache_dtype: str = "auto",
                 kv_scales=None, num_cpu_blocks: int = 0, guide_states: int = 1024, guide_transitions: int = 1 << 24):
        """kv_cache_dtype: "auto" (fp16 cache) or "fp8" / "fp8_e4m3" (one e4m3 byte per element, half the cache bytes;
        include/qspec_hip.h, "FP8 KV cache").  kv_scales: per layer (k_scale, v_scale) for the fp8 cache, kept on THIS engine
        and handed to every forward (the model, which other engines may share, is not touched); None keeps the model's
        (read from the checkpoint) or 1.0.  num_cpu_blocks: blocks of the pinned host cache swap_out / swap_in move KV blocks to
        and from (initialize_cache's second number); 0 allocates nothing.  guide_states / guide_transitions: the capacity of
        the guide arena (guided decoding: resident automaton states and transitions over all resident guides; at Llama-3's
        vocabulary a state costs 32 KB and a transition 4 B); allocated with the first guided request, never before."""
        if kv_cache_dtype not in ("auto", "fp8", "fp8_e4m3"):
            raise ValueError(f"kv_cache_dtype {kv_cache_dtype!r}: 'auto', 'fp8' or 'fp8_e4m3'")
        self.kv_cache_dtype = "auto" if kv_cache_dtype == "auto" else "fp8"
        if kv_scales is not None and self.kv_cache_dtype != "fp8":
            raise ValueError("kv_scales belong to kv_cache_dtype='fp8'")
        if self.kv_cache_dtype == "fp8" and getattr(model, "tp", None) is not None and getattr(model.tp, "world", 1) > 1:
            raise NotImplementedError("fp8 KV cache with tensor parallelism")
        self.model = model
        self.cfg = cfg = model.config
        if max_model_len > cfg.max_position_embeddings:
            # the RoPE table has max_position_embeddings rows (quarot_llama.py:112-120); vLLM refuses such a
            # max_model_len at config time -- a position beyond it would read past the table
            raise ValueError(f"max_model_len {max_model_len} > max_position_embeddings {cfg.max_position_embeddings}")
        self.k = k = num_speculative_tokens
        self.B = B = max_batch
        self.block_size = block_size
        self.max_model_len = max_model_len
        self.use_graph = use_graph
        dev = self.device = model.device
        i64, i32 = torch.int64, torch.int32
        # ---- one KV cache for both passes: [num_blocks, block_size, n_kv, d] per layer
        # num_blocks: what the worker's initialize_cache(num_gpu_blocks) hands over (the scheduler allocates block ids
        # below it and sends block tables); default: every slot owns a contiguous range of max_model_len tokens
        self.blocks_per_seq = (max_model_len + block_size - 1) // block_size
        self.num_blocks = B * self.blocks_per_seq if num_blocks is None else int(num_blocks)
        if self.num_blocks < 1:
            raise ValueError("the KV cache needs at least one block")
        shape = (self.num_blocks, block_size, cfg.num_key_value_heads, cfg.head_dim)
        kv_dtype = torch.uint8 if self.kv_cache_dtype == "fp8" else torch.float16   # byte 0 = e4m3 +0.0
        if kv_scales is not None:
            kv_scales = [(float(a), float(b)) for a, b in kv_scales]
            if len(kv_scales) != cfg.num_hidden_layers or any(not (a > 0 and b > 0) for a, b in kv_scales):
                raise ValueError("kv_scales: one positive (k_scale, v_scale) pair per layer")
        self.kv_scales = kv_scales
        self._kv_fw = {} if kv_scales is None else {"kv_scales": kv_scales}   # forward() keywords; empty unless fp8 + own scales
        self.kv_caches = [(torch.zeros(shape, dtype=kv_dtype, device=dev),
                           torch.zeros(shape, dtype=kv_dtype, device=dev)) for _ in range(cfg.num_hidden_layers)]
        # ---- the swap space: one pinned record (K and V of every layer) per CPU block, made only when asked for
        if int(num_cpu_blocks) < 0:
            raise ValueError("num_cpu_blocks < 0")
        if int(num_cpu_blocks):
            self.allocate_cpu_cache(int(num_cpu_blocks))
        if self.num_blocks >= B * self.blocks_per_seq:
            self.block_tables = torch.arange(B * self.blocks_per_seq, dtype=i32, device=dev).view(B, self.blocks_per_seq).contiguous()
            self._capacity = [self.blocks_per_seq * block_size] * B    # tokens the slot's block table covers (host)
        else:   # fewer blocks than max_num_seqs x max_model_len (vLLM's normal case): every request brings its table
            self.block_tables = torch.zeros(B, self.blocks_per_seq, dtype=i32, device=dev)
            self._capacity = [0] * B
        self._bt_host: List[Optional[List[int]]] = [None] * B      # the table last uploaded per slot (None: the default)
        self._len_ub = [0] * B                                     # host upper bound of seq_lens (0 = empty slot)
        self._gen_ub = [0] * B                                     # host upper bound of gen_lens
        # ---- sequence state (seq_lens[b] == 0: empty slot)
        self.seq_lens = torch.zeros(B, dtype=i32, device=dev)      # L: tokens known (KV valid below L-1)
        self.last_token = torch.zeros(B, dtype=i64, device=dev)
        self.gen_tokens = torch.full((B, max_new_tokens + k + 1), -1, dtype=i64, device=dev)
        self.gen_lens = torch.zeros(B, dtype=i32, device=dev)
        self.n_active = 0
        # sequences taking part in the next step (the scheduler may leave a running request out of a step): the cycle
        # works on eff_lens = seq_lens * step_mask, so a request that sits out looks like an empty slot and keeps its state
        self.step_mask = torch.ones(B, dtype=i32, device=dev)
        self.eff_lens = torch.zeros(B, dtype=i32, device=dev)
        self._mask_host = [1] * B
        self._len_before, self._gen_before = [0] * B, [0] * B
        # ---- per-cycle buffers
        V = cfg.vocab_size
        n_splits = n_splits_for(max_model_len, B * cfg.num_key_value_heads)
        self.d_tokens = torch.zeros(B, dtype=i64, device=dev)
        self.d_pos = torch.zeros(B, dtype=i64, device=dev)
        self.d_slots = torch.zeros(B, dtype=i64, device=dev)
        self.d_ctx = torch.zeros(B, dtype=i32, device=dev)
        self.d_qstart = torch.arange(B + 1, dtype=i32, device=dev)
        self.draft_probs_kbv = torch.zeros(k, B, V, dtype=torch.float32, device=dev)   # step-major
        self.draft_ids_kb = torch.zeros(k, B, dtype=i64, device=dev)
        T = B * (k + 1)
        self.v_tokens = torch.zeros(T, dtype=i64, device=dev)
        self.v_pos = torch.zeros(T, dtype=i64, device=dev)
        self.v_slots = torch.zeros(T, dtype=i64, device=dev)
        self.v_ctx = torch.zeros(B, dtype=i32, device=dev)
        self.v_qstart = (torch.arange(B + 1, dtype=i32, device=dev) * (k + 1)).contiguous()
        self.target_probs = torch.zeros(B, k + 1, V, dtype=torch.float32, device=dev)
        self.target_tokens = torch.zeros(B, k + 1, dtype=i64, device=dev)
        # the cycle's output and its error word in ONE buffer: the worker's single host read per cycle
        self._out_err = torch.full((B * (k + 1) + 1,), -1, dtype=i64, device=dev)
        self._out_err[-1] = 0
        self.out_tokens = self._out_err[:B * (k + 1)].view(B, k + 1)
        self.err_word = self._out_err[B * (k + 1):]               # OR of the sticky device-side error words (0 = fine)
        self._out_err_host = torch.empty(B * (k + 1) + 1, dtype=i64, pin_memory=(dev.type == "cuda"))
        self._snap_i32 = torch.zeros(2 * B, dtype=i32, device=dev)  # sequence state at the start of the last cycle
        self._snap_i64 = torch.zeros(B + 5, dtype=i64, device=dev)
        self.recoveries = 0                                         # cycles re-run without device-side hand-offs
        self.accepted = torch.zeros(B, k, dtype=torch.uint8, device=dev)
        self.recovered = torch.zeros(B, k, dtype=i64, device=dev)
        # the acceptance sampler (spec_decode_worker.py:95-110): RejectionSampler by default, or the instance handed in
        # (TypicalAcceptanceSampler) -- same call surface, same counters
        self.sampler = acceptance_sampler if acceptance_sampler is not None else RejectionSampler(seed=seed)
        self.sampler.init_gpu_tensors(str(dev))
        self.scratch_draft = Scratch(cfg, B, B, 1, n_splits, dev)
        self.scratch_verify = Scratch(cfg, T, B, k + 1, n_splits, dev)
        self.md_draft = AttentionMetadata(self.d_slots, self.block_tables, self.d_ctx, self.d_qstart, 1, n_splits)
        self.md_verify = AttentionMetadata(self.v_slots, self.block_tables, self.v_ctx, self.v_qstart, k + 1, n_splits)
        # ---- what the requests' SamplingParams become on the device (slot_sampling.py) and the mode level the occupied slots ask
        # for: 0 greedy -- the cycle above (fused lm_head + softmax); 1 sampling -- EVERY row goes through ops.sample_top_k_top_p;
        # 2 logit processors -- + the token-table catch-up and the logits pre-pass; 3 token constraints -- the pre-pass's constrained
        # entry (same launches); 4 token guides -- its guided entry plus the guide catch-up at the head of the cycle.  One captured
        # cycle per level a batch has asked for, keyed (level, "full"), or (level, "draft"): the fallback, the proposer alone with
        # the verify pass eager.  Every other batch replays what it always did.
        self.sampling = SlotSampling(B, k, V, dev, guide_states, guide_transitions)
        self._level = 0
        self._graphs: dict = {}
        # the sampling front end's histogram workspaces (draft / non-speculative rows, verify rows), zero-filled here --
        # outside any capture -- and left zeroed by every call
        self._sample_ws_d = ops.new_sample_workspace(B, dev)
        self._sample_ws_v = ops.new_sample_workspace(T, dev)
        # test hooks: injected random draws for the rejection sampler (eager mode only)
        self.inject_uniform: Optional[torch.Tensor] = None
        self.inject_exponential: Optional[torch.Tensor] = None
        self._prefill_scratch: Optional[Scratch] = None

    # names the benchmark, scripts and tests read: whole-cycle graph per level, draft-only fallback, modes, state of self.sampling
    _graph, _graph_s, _graph_p, _graph_c, _graph_g = (property(lambda self, lv=lv: self._graphs.get((lv, "full"))) for lv in range(5))
    _graph_draft = property(lambda self: self._graphs.get((0, "draft")))
    _mode_sampling, _mode_processing, _mode_constrained, _mode_guided = (
        property(lambda self, lv=lv: self._level >= lv) for lv in (1, 2, 3, 4))
    seq_seeded, lp_gen_base, tok_table, counted_len, proc_logits_d, proc_logits_v, tc, _lp_host, _tc_host, tg, guide_arena = (
        property(lambda self, n=n: getattr(self.sampling, n)) for n in
        "seq_seeded lp_gen_base tok_table counted_len proc_logits_d proc_logits_v tc _lp_host _tc_host tg guide_arena".split())

    # the embedding lookups of the cycle's four forwards ride in the bookkeeping launches in front of them (5 launches less)
    EMBED_IN_BOOKKEEPING = os.environ.get("QSPEC_EMBED_IN_BOOKKEEPING", "1") != "0"
    PREFILL_TOKEN_BUDGET = 4096   # tokens per prompt-pass forward when several requests are admitted together
    PROMPT_LOGPROB_ROWS = 256     # prompt rows per lm_head launch of the prompt logprobs (ONE fp16 [rows, V] buffer, made at first use)
    # logprobs (token_logprobs / take_prompt_logprobs): everything below stays None until a request asks for them
    # chunked prefill (add_sequence: num_computed_tokens / token_chunk_size): both stay None until a prompt arrives in chunks
    _prefilling: Optional[dict] = None        # slot -> its request while the prompt is only partly computed (_normalise_admission)
    _reserved: Optional[dict] = None          # sample slot -> the prefilling slot that holds it for its additional samples
    _prefix_scratch = None                    # (splits, Scratch) of the single-request prompt passes with context splits
    _first_probs: Optional[dict] = None       # slot -> (the processed distribution its first token was sampled from, row)
    _prompt_results: Optional[dict] = None    # slot -> host tensors waiting for take_prompt_logprobs()
    _plp_logits: Optional[torch.Tensor] = None
    _lp_dev: Optional[torch.Tensor] = None    # one int32 device buffer for a call's four outputs, and its pinned host twin
    _lp_host: Optional[torch.Tensor] = None
    # block operations (copy_blocks / swap_out / swap_in): everything below stays None until one is asked for
    num_cpu_blocks = 0
    cpu_cache: Optional[torch.Tensor] = None       # pinned uint8 [num_cpu_blocks, record_bytes]
    _kv_blocks = None                              # ops.KVBlocks: the device array of the 2 x layers cache base pointers
    _swap_staging: Optional[torch.Tensor] = None   # device uint8 [largest call so far, record_bytes]
    SAMPLE_SEED_STRIDE = 0x9E3779B97F4A7C15        # sample i of a seeded group draws with (seed + i * this) mod 2^64

    # ------------------------------------------------------------------ prefill (_run_no_spec, :666-720)
    @torch.no_grad()
    def add_sequences(self, prompts: Sequence[Sequence[int]]):
        """Prompt pass for slots 0 .. len(prompts)-1 (a full batch in the benchmarks and most tests): ONE varlen
        forward over all prompts (vLLM batches prompts the same way), the target's greedy token per prompt."""
        assert len(prompts) <= self.B
        self.add_sequences_to(list(range(len(prompts))), prompts)

    @torch.no_grad()
    def add_sequences_to(self, slots: Sequence[int], prompts: Sequence[Sequence[int]],
                         block_tables: Optional[Sequence[Optional[Sequence[int]]]] = None,
                         num_prompt_tokens: Optional[Sequence[Optional[int]]] = None,
                         prompt_logprobs: Optional[Sequence[Optional[int]]] = None,
                         sample_slots: Optional[Sequence[Optional[Sequence[int]]]] = None,
                         num_computed_tokens: Optional[Sequence[Optional[int]]] = None,
                         token_chunk_sizes: Optional[Sequence[Optional[int]]] = None) -> None:
        """Admit several requests at once: one W4A16 forward over the concatenated prompts (flash-attn varlen form).
        num_prompt_tokens[i] (None: all of it): how many tokens of prompts[i] are the request's PROMPT -- a preempted
        request comes back with prompt + outputs as one token list, and the penalties / min_tokens tell the two apart.
        prompt_logprobs[i] (None: not asked for): SamplingParams.prompt_logprobs of request i -- the logprob and rank of every
        token of prompts[i] but the first plus that many best, from the RAW target logits; take_prompt_logprobs(slot) hands
        them over.  sample_slots[i] (None: none): further EMPTY slots that receive additional first-token samples of prompts[i]
        (SamplingParams.n / best_of > 1) -- see add_sequence.  num_computed_tokens[i] (None: 0) / token_chunk_sizes[i] (None:
        the rest of the prompt): a prefix hit and / or one chunk of a chunked prefill -- see add_sequence; requests with
        different (computed, chunk) share the forward."""
        n = len(slots)
        if n == 0:
            return
        if len(set(slots)) != len(slots):
            raise ValueError("a slot appears twice in one admission")
        opt = lambda v: [None] * n if v is None else list(v)   # noqa: E731
        tables, npts, plps = opt(block_tables), opt(num_prompt_tokens), opt(prompt_logprobs)
        cs, qs = opt(num_computed_tokens), opt(token_chunk_sizes)
        extra = [()] * n if sample_slots is None else [tuple(int(c) for c in (e or ())) for e in sample_slots]
        # Validate EVERY slot, prompt and block table before the first forward: a later request that does not fit must
        # not leave earlier ones of the same call admitted (their slots would be occupied here and free in the worker).
        reqs = [self._normalise_admission(slots[i], prompts[i], tables[i], npts[i], plps[i], extra[i], cs[i], qs[i])
                for i in range(n)]
        self._check_sample_slots([c for r in reqs for c in r.fresh_slots])
        if n == 1:
            self._prompt_pass_one(reqs[0])
            self._sync()
            return
        if sum(r.rows for r in reqs) > self.PREFILL_TOKEN_BUDGET:
            # several passes of at most PREFILL_TOKEN_BUDGET tokens (measured: 4 x 512 tokens in one pass 37 ms vs 49 ms
            # one by one, but 32 x 512 in one pass 335 ms vs 283 ms)
            group, tokens = [], 0
            for i in range(n + 1):
                if i == n or (group and tokens + reqs[i].rows > self.PREFILL_TOKEN_BUDGET):
                    if len(group) == 1:
                        self._prompt_pass_one(group[0])
                    else:
                        self._prompt_pass_many(group)
                    group, tokens = [], 0
                if i < n:
                    group.append(reqs[i])
                    tokens += reqs[i].rows
        else:
            self._prompt_pass_many(reqs)
        self._sync()

    def _prompt_pass_many(self, reqs) -> None:
        """One varlen forward over the rows of several requests (each: positions first .. c + q - 1 behind c valid keys)."""
        cfg, dev = self.cfg, self.device
        n = len(reqs)
        for r in reqs:
            if r.table is not None:
                self.set_block_table(r.slot, r.table)
        lens = [r.rows for r in reqs]
        Ttot, Tmax = sum(lens), max(lens)
        ctx = [r.c + r.q for r in reqs]
        S = prefill_splits(lens, ctx, cfg.num_key_value_heads, cfg.num_attention_heads // cfg.num_key_value_heads)
        s = Scratch(cfg, Ttot, n, Tmax, S, dev, logits_rows=n)
        ids = torch.tensor([t for r in reqs for t in r.tokens[r.first:r.c + r.q]], dtype=torch.int64, device=dev)
        pos = torch.cat([torch.arange(r.first, r.c + r.q, dtype=torch.int64, device=dev) for r in reqs])
        slot_map = torch.cat([self._write_slots(r, torch.arange(r.first, r.c + r.q, dtype=torch.int64, device=dev)) for r in reqs])
        q_start = torch.tensor([0] + list(torch.tensor(lens).cumsum(0).tolist()), dtype=torch.int32, device=dev)
        md = AttentionMetadata(slot_map, self.block_tables[[r.slot for r in reqs]].contiguous(),
                               torch.tensor(ctx, dtype=torch.int32, device=dev), q_start, Tmax, S)
        hs = self.model.forward(ids, pos, self.kv_caches, md, s, w4a4=False, **self._kv_fw)
        self._finish_prompt_pass(reqs, hs, q_start.tolist(), s)

    @torch.no_grad()
    def add_sequence(self, slot: int, prompt: Sequence[int], block_table: Optional[Sequence[int]] = None,
                     sync: bool = True, num_prompt_tokens: Optional[int] = None, prompt_logprobs: Optional[int] = None,
                     sample_slots: Sequence[int] = (), num_computed_tokens: int = 0,
                     token_chunk_size: Optional[int] = None) -> None:
        """Admit a request into an empty slot: scorer-only W4A16 prompt pass (the proposer never runs on prefill,
        spec_decode_worker.py:699); the first generated token is the target's greedy token.  prompt_logprobs: see
        add_sequences_to.
        sample_slots (SamplingParams.n / best_of > 1): further EMPTY slots that each receive one more first-token sample of the
        same prompt.  The prompt pass runs ONCE; the first token is sampled over the prompt's last hidden row repeated once per
        sample.  Every sample slot gets the parent's block table (the prompt's blocks are shared until the scheduler hands a
        sample its own copy: copy_blocks + set_block_table), the prompt in its token table, the parent's sampling parameters and
        its own first token; sample i (the parent is 0) of a seeded request draws with seed (seed + i * SAMPLE_SEED_STRIDE)
        mod 2^64, unseeded samples with the engine stream (row-indexed: the rows differ).

        Prefix hits and chunked prefill (model_runner.py:482-590): `prompt` is always the request's FULL token list;
        num_computed_tokens = c tokens of it already have valid K/V in the slot's block table (blocks another request filled, or
        earlier chunks of this one), token_chunk_size = q tokens are computed now (None: the rest).  The pass computes rows
        c .. c + q - 1 at positions c .. behind c keys read from the cache.  c >= len(prompt) (everything hit): the last token
        alone is computed, c = len - 1.  c + q < len: the slot is PREFILLING afterwards -- occupied on the host (no admission,
        fork or step may name it), still the empty slot seq_lens == 0 on the device, so every captured cycle runs on untouched;
        the next call for it brings the same token list and c >= the count reached (larger: the caller vouches for the tokens
        in between).  c + q == len: the first token is sampled and the slot is in the state a whole-prompt admission leaves.
        The sampling state takes the prompt at the first chunk; sample_slots are held from the first chunk and admitted with the
        last.  Prompt logprobs are gathered over the chunks and handed over after the last; a request that asks for them gets
        no saving from a hit: its cached rows are computed again (their K/V is NOT written: slot_mapping -1).  c > 0 for a
        slot that is not prefilling needs a block table brought by the request.  ValueError, nothing enqueued, on any breach."""
        r = self._normalise_admission(slot, prompt, block_table, num_prompt_tokens, prompt_logprobs,
                                      [int(c) for c in sample_slots], num_computed_tokens, token_chunk_size)
        self._check_sample_slots(r.fresh_slots)
        self._prompt_pass_one(r)
        if sync:
            self._sync()

    def _sync(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize()

    def _prompt_pass_one(self, r) -> None:
        cfg, dev, b = self.cfg, self.device, r.slot
        if r.table is not None:
            self.set_block_table(b, r.table)
        T, ctx = r.rows, r.c + r.q
        S = prefill_splits([T], [ctx], cfg.num_key_value_heads, cfg.num_attention_heads // cfg.num_key_value_heads)
        if S == 1:
            if self._prefill_scratch is None or self._prefill_scratch.T < T:
                self._prefill_scratch = Scratch(cfg, T, 1, T, n_splits_for(T), dev, logits_rows=1)
            s = self._prefill_scratch
        else:   # the Scratch of a pass is sized with the splits of that pass
            if self._prefix_scratch is None or self._prefix_scratch[0] != S or self._prefix_scratch[1].T < T:
                self._prefix_scratch = (S, Scratch(cfg, T, 1, T, S, dev, logits_rows=1))
            s = self._prefix_scratch[1]
        ids = torch.tensor(r.tokens[r.first:ctx], dtype=torch.int64, device=dev)
        pos = torch.arange(r.first, ctx, dtype=torch.int64, device=dev)
        md = AttentionMetadata(self._write_slots(r, pos), self.block_tables[b:b + 1].contiguous(),
                               torch.tensor([ctx], dtype=torch.int32, device=dev),
                               torch.tensor([0, T], dtype=torch.int32, device=dev), T, S)
        hs = self.model.forward(ids, pos, self.kv_caches, md, s, w4a4=False, **self._kv_fw)
        self._finish_prompt_pass([r], hs, [0, T], s)

    def _write_slots(self, r, pos: torch.Tensor) -> torch.Tensor:
        """slot_mapping of a request's rows: rows in front of its computed count (re-computed for the prompt logprobs only) write
        nothing -- their blocks may be shared with running sequences."""
        slots = self._slots_for(r.slot, pos)
        return slots if r.first == r.c else torch.where(pos < r.c, torch.full_like(slots, -1), slots)

    def _normalise_admission(self, b: int, prompt: Sequence[int], table, npt, plp, extra, c, q):
        """One request of an admission call, checked against the slot's state (nothing enqueued, ValueError on a breach):
        slot, tokens, T; c valid tokens, q tokens computed now, first: the first row of the pass (< c only for prompt logprobs);
        rows = c + q - first; rec: the slot's record when this call continues a chunked prefill; terminal: the first token
        follows; fresh_slots: the slots that must be empty."""
        if not 0 <= b < self.B:
            raise ValueError(f"slot {b} outside the captured batch of {self.B}")
        rec = (self._prefilling or {}).get(b)
        tokens, T = [int(t) for t in prompt], len(prompt)
        if rec is None and not self._is_empty(b):
            raise ValueError(f"slot {b} is occupied; free_slot() it first")
        if table is not None:
            table = [int(x) for x in table]
            self._validate_block_table(table)
        c = 0 if c is None else int(c)
        if c < 0 or (q is not None and int(q) < 1):
            raise ValueError(f"slot {b}: num_computed_tokens {c} / token_chunk_size {q}")
        if rec is not None:
            if tokens != rec.tokens:
                raise ValueError(f"slot {b} is prefilling another token list: free_slot() it first")
            if c < rec.computed:
                raise ValueError(f"slot {b}: num_computed_tokens {c} < the {rec.computed} tokens already computed")
            npt, plp, extra = rec.npt, rec.plp, rec.extra
        else:
            if npt is not None and not 1 <= npt <= T:
                raise ValueError(f"num_prompt_tokens {npt} outside 1..{T}")
            self._check_num_top(plp)
            if c > 0 and table is None and self._bt_host[b] is None:
                raise ValueError(f"slot {b}: num_computed_tokens {c} without a block table that holds them")
        cap = self._capacity[b] if table is None else len(table) * self.block_size
        if T < 1 or T + 1 > min(cap, self.max_model_len):
            raise ValueError(f"prompt of {T} tokens does not fit slot {b} (capacity {cap} tokens, max_model_len "
                             f"{self.max_model_len})" + ("" if cap else ": the request brought no block table"))
        c = min(c, T - 1)                      # everything hit: the last token is computed again (model_runner.py:525-531)
        q = T - c if q is None else min(int(q), T - c)
        first = c if plp is None else (rec.computed if rec is not None else 0)
        return SimpleNamespace(slot=b, tokens=tokens, T=T, table=table, npt=npt, plp=plp, extra=list(extra), c=c, q=q,
                               first=first, rows=c + q - first, rec=rec, terminal=c + q == T,
                               fresh_slots=([] if rec is not None else [b]) + ([] if rec is not None else list(extra)))

    def _finish_prompt_pass(self, reqs, hs, starts: List[int], scratch) -> None:
        """Behind the forward: the sampling state takes the prompt (first chunk); a request whose prompt is not through leaves
        its record and holds its sample slots, the others get their additional samples and the first token; then the prompt
        logprobs of the rows computed (row at position p predicts token p + 1), gathered per slot until the last chunk."""
        dev = self.device
        done = []
        for i, r in enumerate(reqs):
            b = r.slot
            if r.rec is None:
                self.sampling.admit_tokens(b, r.tokens, r.npt)
            r.parts = r.rec.parts if r.rec is not None else []
            if not r.terminal:
                if self._prefilling is None:
                    self._prefilling, self._reserved = {}, {}
                self._prefilling[b] = SimpleNamespace(tokens=r.tokens, computed=r.c + r.q, npt=r.npt, plp=r.plp, extra=r.extra,
                                                      parts=r.parts)
                for c in r.extra:
                    self._reserved[c] = b
                continue
            if r.rec is not None:
                del self._prefilling[b]
                for c in r.extra:
                    self._reserved.pop(c, None)
            self._admit_samples(b, r.extra, r.tokens, r.npt)
            done.append((i, r))
        if done:
            rows, row_slots, row_lens = [], [], []      # one first-token row per request and per additional sample of it
            for i, r in done:
                rows += [starts[i + 1] - 1] * (1 + len(r.extra))
                row_slots += [r.slot, *r.extra]
                row_lens += [r.T] * (1 + len(r.extra))
            if len(done) == 1:
                first_hs = hs[rows[0]:rows[0] + 1]
                first_hs = first_hs if len(rows) == 1 else first_hs.expand(len(rows), -1).contiguous()
            else:
                first_hs = hs[torch.tensor(rows, dtype=torch.int64, device=dev)].contiguous()
            self._first_token(first_hs, scratch, row_slots, row_lens)
        self.n_active = len(self.active_slots())
        for i, r in enumerate(reqs):
            if r.plp is None:
                continue
            n_lp = min(r.c + r.q, r.T - 1) - r.first
            if r.terminal and r.rec is None:   # the whole prompt in one pass
                self._prompt_logprobs(r.slot, hs[starts[i]:starts[i] + n_lp], r.tokens, r.plp)
                continue
            if n_lp > 0:
                r.parts.append(self._prompt_logprobs(None, hs[starts[i]:starts[i] + n_lp], r.tokens[r.first:], r.plp))
            if r.terminal:
                if self._prompt_results is None:
                    self._prompt_results = {}
                self._prompt_results[r.slot] = tuple(torch.cat([p[j] for p in r.parts]) for j in range(4))

    def _is_empty(self, b: int) -> bool:
        """Nothing holds the slot: no sequence, no partly computed prompt, no reservation for a prefilling request's samples."""
        return self._len_ub[b] == 0 and not (self._prefilling and b in self._prefilling) and not (self._reserved and b in self._reserved)

    def is_prefilling(self, slot: int) -> bool:
        return bool(self._prefilling) and slot in self._prefilling

    def num_computed_tokens(self, slot: int) -> int:
        """Tokens of the partly computed prompt in `slot` whose K/V is valid (0: the slot is not prefilling)."""
        return self._prefilling[slot].computed if self.is_prefilling(slot) else 0

    def _check_sample_slots(self, slots: List[int]) -> None:
        """Every slot of one admission, sample slots included: distinct, inside the batch, empty."""
        if len(set(slots)) != len(slots):
            raise ValueError("a slot appears twice in one admission")
        for c in slots:
            if not 0 <= c < self.B or not self._is_empty(c):
                raise ValueError(f"slot {c} is not an empty slot of this engine")

    def _admit_samples(self, parent: int, sample_slots: Sequence[int], prompt: Sequence[int], num_prompt_tokens: Optional[int]) -> None:
        """What a sample slot shares with its parent, in front of the first token: block table, sampling parameters (seed
        derived), token-table row of the prompt."""
        for i, c in enumerate(sample_slots, 1):
            if self._bt_host[parent] is not None:
                self.set_block_table(c, self._bt_host[parent])
            elif self._bt_host[c] is not None or self.num_blocks >= self.B * self.blocks_per_seq:
                # contiguous mode: the parent's default range (recorded as a brought table: free_slot restores the slot's own)
                lo = parent * self.blocks_per_seq
                self.set_block_table(c, list(range(lo, lo + self.blocks_per_seq)))
            self.sampling.clone_params(parent, c, seed_add=i * self.SAMPLE_SEED_STRIDE)
            self.sampling.admit_tokens(c, prompt, num_prompt_tokens)

    def _first_token(self, hs, scratch, slots: List[int], prompt_lens: List[int]) -> None:
        """The target's first token of freshly admitted prompts (hs: their last hidden rows): greedy, or sampled with the
        slots' parameters (a seeded request: target stream, j = 0, base position = its prompt length).  The mode comes from the
        admitted slots alone; position 0 of a request has no in-flight tokens (gen_lens of a fresh slot is 0)."""
        n, level, greedy = len(slots), self.sampling.level(slots), not self.sampling.sampling_on(slots)
        if scratch.logits.shape[0] < n:   # additional samples of a prompt: more rows than the prompt pass's scratch has
            scratch = SimpleNamespace(logits=torch.empty(n, self.cfg.vocab_size, dtype=torch.float16, device=self.device))
        probs = torch.empty(n, self.cfg.vocab_size, dtype=torch.float32, device=self.device)
        tok = torch.empty(n, dtype=torch.int64, device=self.device)
        rows = self.sampling.gathered_rows(slots, level, not greedy, scratch.logits[:n])
        base_pos = None if greedy else torch.tensor(prompt_lens, dtype=torch.int32, device=self.device)
        self._sample(level, rows, hs, scratch, probs, tok, base_pos=base_pos, argmax=greedy)
        if self._first_probs is None:
            self._first_probs = {}
        for i, (b, T) in enumerate(zip(slots, prompt_lens)):   # the slots are occupied from here on
            self._first_probs[b] = (probs, i)   # kept for token_logprobs("first"); free_slot / the next admission drops it
            self.seq_lens[b] = T + 1
            self.last_token[b] = tok[i]
            self.gen_tokens[b].fill_(-1)
            self.gen_tokens[b, 0] = tok[i]
            self.gen_lens[b] = 1
            self._len_ub[b] = T + 1
            self._gen_ub[b] = 1
        self.n_active = len(self.active_slots())

    def _sample(self, level: int, rows, hs, scratch, probs, token, base_pos, rows_per_seq: int = 1, j_base: int = 0,
                draw_stream: int = 2, active_lens=None, draft_ids=None, workspace=None, shard_vocab: bool = False, hook=None,
                fused_greedy: bool = False, argmax: bool = False) -> None:
        """THE sampling front end -- the first token, the non-speculative step, every draft step and the verify pass come through
        here: lm_head -> the bench-only hook -> from level 2 on the logits pre-pass (self._process, out of place: the raw logits
        stay in scratch.logits; level 3: its constrained entry, level 4: its guided entry) -> ops.sample_top_k_top_p over EVERY row (greedy rows take the
        argmax there; min_p from level 2 on), or with `argmax` ops.softmax_argmax.  probs [T, V] fp32 is the
        PROCESSED distribution: what the rejection sampler must see.  rows: the per-row arrays (SlotSampling.draft_rows /
        verify_rows / gathered_rows); row t belongs to sequence t // rows_per_seq and is position j_base + t % rows_per_seq of
        its cycle; draw_stream: 1 draft, 2 target; base_pos: the seeded draws' base position per sequence.  fused_greedy: level 0
        may take the fused lm_head + softmax launch (model.sample_greedy decides; same bits)."""
        if level == 0 and fused_greedy:
            self.model.sample_greedy(hs, scratch, probs, token, shard_vocab=shard_vocab, logits_hook=hook)
            return
        logits = self.model.compute_logits(hs, scratch, shard_vocab=shard_vocab)
        if hook is not None:
            hook(logits)
        if level >= 2:
            logits = self._process(logits, rows.proc_out, rows_per_seq, j_base, draft_ids, active_lens, slot_ids=rows.slot_ids,
                                   constrained=level >= 3, **({"guided": True} if level == 4 else {}))
        if argmax:
            ops.softmax_argmax(logits, probs, token)
        else:
            ops.sample_top_k_top_p(logits, probs, token, rows.temp, rows.topk, rows.topp, rng_state=self.sampler.rng_state,
                                   workspace=workspace, min_p=rows.minp if level >= 2 else None, seq_seeds=rows.seeds,
                                   seq_seeded=rows.seeded, base_pos=base_pos, rows_per_seq=rows_per_seq, j_base=j_base,
                                   draw_stream=draw_stream)

    def free_slot(self, slot: int) -> None:
        """The request in `slot` has finished (EOS / max_tokens / aborted): the slot goes back to empty."""
        self.seq_lens[slot] = 0
        self.gen_lens[slot] = 0
        self._len_ub[slot] = 0
        self._gen_ub[slot] = 0
        if self._prefilling:                    # a partly computed prompt: its record and the slots held for its samples
            self._prefilling.pop(slot, None)
            for c in [c for c, parent in self._reserved.items() if parent == slot or c == slot]:
                del self._reserved[c]
        for kept in (self._first_probs, self._prompt_results):
            if kept:
                kept.pop(slot, None)
        self.set_sampling_params(slot)          # back to greedy, no seed
        if self._bt_host[slot] is not None:
            # the request's blocks go back to the scheduler: the slot must not keep a table (and a capacity) that the
            # next admission could pass validation against.  Contiguous mode: the slot's own default range again;
            # brought-table mode (fewer blocks than slots x max_model_len): no table, capacity 0 until one arrives.
            if self.num_blocks >= self.B * self.blocks_per_seq:
                lo = slot * self.blocks_per_seq
                self.block_tables[slot].copy_(torch.arange(lo, lo + self.blocks_per_seq, dtype=torch.int32, device=self.device))
                self._capacity[slot] = self.blocks_per_seq * self.block_size
            else:
                self.block_tables[slot].zero_()
                self._capacity[slot] = 0
            self._bt_host[slot] = None
        self.n_active = len(self.active_slots())

    # ------------------------------------------------------------------ block operations and forks (vllm/worker/worker.py, execute_worker)
    def _blocks(self):
        if self._kv_blocks is None:   # the pointer array is built once, at the first block operation
            self._kv_blocks = ops.KVBlocks([k for k, _ in self.kv_caches], [v for _, v in self.kv_caches])
        return self._kv_blocks

    def allocate_cpu_cache(self, num_cpu_blocks: int) -> None:
        """The swap space (the constructor's num_cpu_blocks; the worker's initialize_cache calls this): ONE pinned uint8
        [num_cpu_blocks, record_bytes] tensor, a record = K and V of one block over all layers."""
        if num_cpu_blocks < 1:
            raise ValueError("the CPU cache needs at least one block")
        k0 = self.kv_caches[0][0]
        record = 2 * len(self.kv_caches) * k0[0].numel() * k0.element_size()
        self.cpu_cache = torch.empty(num_cpu_blocks, record, dtype=torch.uint8, pin_memory=(self.device.type == "cuda"))
        self.num_cpu_blocks = num_cpu_blocks

    def _staging(self, n: int) -> torch.Tensor:
        blocks = self._blocks()
        if self._swap_staging is None or self._swap_staging.shape[0] < n:   # sized to the largest call so far
            self._swap_staging = torch.empty(n, blocks.record_bytes, dtype=torch.uint8, device=self.device)
        return self._swap_staging

    def _swap_pairs(self, pairs, gpu_first: bool):
        if self.cpu_cache is None:
            if not list(pairs):
                return []
            raise ValueError("this engine has no CPU cache (num_cpu_blocks = 0)")
        n_src, n_dst = (self.num_blocks, self.num_cpu_blocks) if gpu_first else (self.num_cpu_blocks, self.num_blocks)
        return ops.validate_block_pairs(pairs, n_src, n_dst, same_space=False)

    @torch.no_grad()
    def copy_blocks(self, pairs) -> None:
        """blocks_to_copy: cache[dst] = cache[src] for the (src, dst) block pairs in every layer's K and V -- one launch on the
        current stream, outside every captured graph (copy-on-write, forks).  One src may feed several dst; ValueError, nothing
        enqueued: an id outside the cache, a dst twice, a dst that is also a src of the call."""
        pairs = ops.validate_block_pairs(pairs, self.num_blocks, self.num_blocks)
        if pairs:
            ops.copy_blocks(self._blocks(), pairs)

    @torch.no_grad()
    def swap_out(self, pairs) -> None:
        """blocks_to_swap_out: (gpu block, cpu block) pairs.  ONE gather launch packs the blocks into contiguous records (K and V
        of every layer), then one asynchronous record-sized copy per block lands them in the pinned CPU cache; all on the
        current stream, so a later swap_in or cycle is ordered behind it.  ValueError with nothing enqueued on a bad pair."""
        pairs = self._swap_pairs(pairs, gpu_first=True)
        if not pairs:
            return
        stage = self._staging(len(pairs))
        ops.gather_blocks(self._blocks(), [g for g, _ in pairs], stage)
        for i, (_, c) in enumerate(pairs):
            self.cpu_cache[c].copy_(stage[i], non_blocking=True)

    @torch.no_grad()
    def swap_in(self, pairs) -> None:
        """blocks_to_swap_in: (cpu block, gpu block) pairs: the record copies first, then ONE scatter launch."""
        pairs = self._swap_pairs(pairs, gpu_first=False)
        if not pairs:
            return
        stage = self._staging(len(pairs))
        for i, (c, _) in enumerate(pairs):
            stage[i].copy_(self.cpu_cache[c], non_blocking=True)
        ops.scatter_blocks(self._blocks(), [g for _, g in pairs], stage)

    @torch.no_grad()
    def fork_slot(self, src: int, dst: int, block_table: Optional[Sequence[int]] = None) -> None:
        """The sequence in the occupied slot `src` continues in the empty slot `dst` as well (a scheduler forking mid-generation):
        every per-slot piece of state is copied -- lengths, last token, generated tokens, host bounds, the SlotSampling state
        (parameters, seed, token-table row, constraint rows and tail).  block_table: the fork's own table (shared blocks plus
        its copy of the last, partially filled one: copy_blocks first); None: the parent's."""
        for b, want in ((src, True), (dst, False)):
            if not 0 <= b < self.B or (self._len_ub[b] > 0 if want else not self._is_empty(b)) != want:
                raise ValueError(f"slot {b} is not {'an occupied' if want else 'an empty'} slot of this engine")
        if block_table is None:
            block_table = self._bt_host[src]
            if block_table is None:
                lo = src * self.blocks_per_seq
                block_table = list(range(lo, lo + self.blocks_per_seq))
        self._validate_block_table([int(b) for b in block_table])
        self.sync_lens()   # exact bounds: the fork starts from what the parent really holds
        self.set_block_table(dst, block_table)
        self.sampling.fork(src, dst)
        for t in (self.seq_lens, self.gen_lens, self.last_token, self.gen_tokens):
            t[dst].copy_(t[src])
        self._len_ub[dst], self._gen_ub[dst] = self._len_ub[src], self._gen_ub[src]
        if self._first_probs and src in self._first_probs:
            self._first_probs[dst] = self._first_probs[src]
        self.n_active = len(self.active_slots())

    # ------------------------------------------------------------------ logprobs (sampler.py:284, :861-879, :882 ff.)
    @staticmethod
    def _check_num_top(num_top: Optional[int]) -> None:
        if num_top is not None and not 0 <= int(num_top) <= ops.MAX_LOGPROBS:
            raise ValueError(f"{num_top} logprobs asked for: 0..{ops.MAX_LOGPROBS} are supported")

    def _logprob_buffers(self, rows: int, num_top: int):
        """(logprob [rows] f32, rank [rows] i32, top ids [rows * num_top] i32, top logprobs [rows * num_top] f32) as views of
        ONE device buffer, and the matching pinned host views: a call's results come back in one copy.  Made at first use."""
        need = rows * (2 + 2 * num_top)
        if self._lp_dev is None or self._lp_dev.numel() < need:
            self._lp_dev = torch.empty(need, dtype=torch.int32, device=self.device)
            self._lp_host = torch.empty(need, dtype=torch.int32, pin_memory=(self.device.type == "cuda"))

        def views(buf):
            n = rows * num_top
            return (buf[:rows].view(torch.float32), buf[rows:2 * rows], buf[2 * rows:2 * rows + n],
                    buf[2 * rows + n:2 * rows + 2 * n].view(torch.float32))
        return views(self._lp_dev), views(self._lp_host), need

    def _read_logprobs(self, host, need: int, shape, num_top: int):
        self._lp_host[:need].copy_(self._lp_dev[:need], non_blocking=True)
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        lp, rank, ids, tlp = host
        return lp.clone().view(*shape), rank.clone().view(*shape), ids.clone().view(*shape, num_top), tlp.clone().view(*shape, num_top)

    @torch.no_grad()
    def token_logprobs(self, kind: str, slots: Sequence[int], token_ids, num_top: int = 0):
        """Logprob, rank and the num_top best of the tokens a step has just produced, from the PROCESSED distribution the
        sampler drew them from (what the reference's `logprobs` tensor is the log of): eager, after the step, one launch
        per run of consecutive rows, one host read.
        kind "cycle": target_probs[slot], token_ids [len(slots), k + 1] (a position without a token: any id outside the
        vocabulary gives the dummy 0.0 / -1); "no_spec": the distribution of the last step_no_spec(); "first": that of the
        slot's admission.  token_ids [len(slots)] for the latter two.  Returns host tensors (logprob f32, rank i32 of shape
        [len(slots)] or [len(slots), k + 1]; top ids i32 and top logprobs f32 with a trailing [num_top])."""
        self._check_num_top(num_top)
        slots, V = list(slots), self.cfg.vocab_size
        n, rps = len(slots), (self.k + 1 if kind == "cycle" else 1)
        shape = (n, rps) if kind == "cycle" else (n,)
        ids = torch.as_tensor(token_ids, dtype=torch.int64).reshape(n * rps).to(self.device)
        (lp, rank, top, tlp), host, need = self._logprob_buffers(n * rps, num_top)
        if kind == "cycle":
            src = {b: (self.target_probs.view(-1, V), b * rps) for b in slots}
        elif kind == "no_spec":
            src = {b: (self.draft_probs_kbv[0], b) for b in slots}
        elif kind == "first":
            src = {b: (self._first_probs or {})[b] for b in slots}
        else:
            raise ValueError(f"kind {kind!r}: 'cycle', 'no_spec' or 'first'")
        i = 0
        while i < n:   # slots i .. j-1: consecutive rows of one tensor
            t, r0 = src[slots[i]]
            j = i + 1
            while j < n and src[slots[j]][0].data_ptr() == t.data_ptr() and src[slots[j]][1] == r0 + (j - i) * rps:
                j += 1
            a, e = i * rps, j * rps
            ops.token_logprobs_from_probs(t[r0:r0 + e - a], ids[a:e], num_top, lp[a:e], rank[a:e],
                                          top[a * num_top:e * num_top] if num_top else None,
                                          tlp[a * num_top:e * num_top] if num_top else None)
            i = j
        return self._read_logprobs(host, need, shape, num_top)

    def _prompt_logits(self, hs):
        """Raw target logits of up to PROMPT_LOGPROB_ROWS prompt rows in the ONE buffer all prompt forms share (tests wrap this
        on the instance)."""
        R = self.PROMPT_LOGPROB_ROWS
        if self._plp_logits is None or self._plp_logits.shape[0] != R:
            self._plp_logits = torch.empty(R, self.cfg.vocab_size, dtype=torch.float16, device=self.device)
        return self.model.compute_logits(hs, SimpleNamespace(logits=self._plp_logits))

    def _prompt_logprobs(self, slot: Optional[int], hs, prompt: Sequence[int], num_top: int):
        """hs: the hidden rows 0 .. T-2 of the prompt in `slot` (row t predicts prompt[t + 1]): lm_head in chunks, logprobs
        from the raw logits -- no temperature, penalties or constraints --, results kept for take_prompt_logprobs(slot).
        slot None (one chunk of a prompt, `prompt` starting at the chunk's first row): the results are returned instead."""
        rows, R = hs.shape[0], self.PROMPT_LOGPROB_ROWS
        ids = torch.tensor(list(prompt[1:]), dtype=torch.int64, device=self.device)
        (lp, rank, top, tlp), host, need = self._logprob_buffers(rows, num_top)
        for a in range(0, rows, R):
            e = min(a + R, rows)
            ops.token_logprobs_from_logits(self._prompt_logits(hs[a:e]), ids[a:e], num_top, lp[a:e], rank[a:e],
                                           top[a * num_top:e * num_top] if num_top else None,
                                           tlp[a * num_top:e * num_top] if num_top else None)
        got = self._read_logprobs(host, need, (rows,), num_top)
        if slot is None:
            return got
        if self._prompt_results is None:
            self._prompt_results = {}
        self._prompt_results[slot] = got

    def take_prompt_logprobs(self, slot: int):
        """The prompt logprobs of the request admitted into `slot` with prompt_logprobs set -- host tensors (logprob [T-1],
        rank [T-1], top ids [T-1, n], top logprobs [T-1, n]) for prompt tokens 1 .. T-1 -- or None; handed over once."""
        return self._prompt_results.pop(slot, None) if self._prompt_results else None

    def set_sampling_params(self, slot: int, temperature: float = 0.0, top_k: int = -1, top_p: float = 1.0,
                            seed: Optional[int] = None, min_p: float = 0.0, presence_penalty: float = 0.0,
                            frequency_penalty: float = 0.0, repetition_penalty: float = 1.0, min_tokens: int = 0,
                            stop_token_ids: Sequence[int] = (), logit_bias=None, allowed_token_ids=None,
                            bad_words_token_ids=None, guide=None) -> None:
        """The request in `slot` samples with these parameters (vllm/sampling_params.py; temperature < 1e-5 = greedy, for
        which vLLM itself resets top_k / top_p).  seed (SamplingParams.seed, taken mod 2^64): the request's draws depend
        on it and its own positions only; a greedy request makes no draws and ignores it.  Uploaded only when they
        change; a change never re-captures the graph (the kernels read the seed arrays at replay).
        min_p / presence_penalty / frequency_penalty / repetition_penalty / min_tokens (+ stop_token_ids: every id that may
        not be emitted before min_tokens tokens were generated, the EOS id included): vllm/sampling_params.py; applied per row
        of the cycle as the non-speculative sampler would apply them at that position.  They belong to the request: set them
        BEFORE its admission (the admission builds the slot's token table).  Refused with ValueError, nothing enqueued: more
        than 16 stop ids, min_p outside [0, 1], repetition_penalty <= 0, min_tokens < 0, non-finite penalties.
        logit_bias ({id: bias}, taken as given: the reference clamps to [-100, 100] where it lowers the request, not here),
        allowed_token_ids, bad_words_token_ids (lists of token ids; single-token words are unlimited, at most 32 longer ones
        of at most 8 tokens, at most 512 biases): hard constraints applied in front of everything above, per row, the bad
        words matched against the request's OUTPUTS (in flight included), never its prompt.  Like the penalties they are set
        BEFORE admission.  Refused with ValueError, nothing enqueued: an id outside the vocabulary, an empty allowed set or
        bad word, a cap exceeded, a non-finite bias, an occupied slot, and a request that can never emit anything (every
        allowed token is a single-token bad word -- or, with min_tokens, a stop id).
        guide (guided decoding: a guides.TokenFSM, e.g. TokenFSM.from_guide(processor._guide, vocab)): in front of everything
        above, every token the guide's state does not allow is set to -inf and every element of the row gets the fp32 zero of the
        reference's mask (outlines_logits_processors.py:34-93); the state is the guide's initial state advanced over the
        request's OUTPUTS, in flight included, never its prompt.  Set BEFORE admission.  Guides are shared by object identity:
        requests that bring the same TokenFSM use one resident copy.  Refused with ValueError, nothing enqueued: not a TokenFSM,
        another vocabulary, an occupied slot, no room in the guide arena (guide_states / guide_transitions) beside the guides in
        use.  A row a guide leaves without a finite logit follows the rule of the constraints: token 0 is emitted."""
        self.sampling.set(slot, temperature, top_k, top_p, seed, min_p, presence_penalty, frequency_penalty, repetition_penalty,
                          min_tokens, stop_token_ids, logit_bias, allowed_token_ids, bad_words_token_ids,
                          occupied=not self._is_empty(slot), guide=guide)

    def _process(self, logits, out, rows_per_seq: int, j_base: int, draft_ids, active_lens, slot_ids=None,
                 constrained: Optional[bool] = None, guided: Optional[bool] = None):
        """The logits pre-pass of the front end (tests wrap it on the instance: it is looked up at call time)."""
        return self.sampling.process(logits, out, rows_per_seq, j_base, draft_ids, active_lens, self.gen_tokens, self.gen_lens,
                                     slot_ids=slot_ids, constrained=self._level >= 3 if constrained is None else constrained,
                                     guided=self._level == 4 if guided is None else guided)

    def set_block_table(self, slot: int, blocks: Sequence[int]) -> None:
        """The scheduler's block table of the request in `slot` (vLLM SequenceGroupMetadata.block_tables); it must
        cover every position a cycle can touch (vLLM allocates them as num_lookahead_slots).  The scheduler resends
        the table on every step: it is uploaded only when it differs from the one the slot already has."""
        blocks = [int(b) for b in blocks]
        if self._bt_host[slot] == blocks:
            return
        self._validate_block_table(blocks)
        n = len(blocks)
        row = torch.zeros(self.blocks_per_seq, dtype=torch.int32)
        row[:n] = torch.tensor(blocks, dtype=torch.int32)
        self.block_tables[slot].copy_(row.to(self.device))
        self._capacity[slot] = n * self.block_size
        self._bt_host[slot] = blocks

    def _validate_block_table(self, blocks: Sequence[int]) -> None:
        n = len(blocks)
        if n > self.blocks_per_seq:
            raise ValueError(f"{n} blocks > {self.blocks_per_seq} per sequence (max_model_len {self.max_model_len})")
        if n and (min(blocks) < 0 or max(blocks) >= self.num_blocks):
            raise ValueError("block id outside the KV cache")

    def active_slots(self) -> List[int]:
        """Slots that hold a request: running sequences and partly computed prompts."""
        return [b for b in range(self.B) if self._len_ub[b] > 0 or (self._prefilling and b in self._prefilling)]

    def sync_lens(self) -> None:
        """Make the host-side length bounds exact (one small device read)."""
        both = torch.stack((self.seq_lens, self.gen_lens)).tolist()
        lens, gens = both[0], both[1]
        for b in range(self.B):
            if self._len_ub[b] > 0:
                self._len_ub[b], self._gen_ub[b] = int(lens[b]), int(gens[b])

    def note_emitted(self, emitted: Sequence[int]) -> None:
        """Exact bookkeeping from a cycle's output the caller has already read (the worker's one host read)."""
        for b in range(self.B):
            if self._len_before[b] > 0 and self._len_ub[b] > 0:
                self._len_ub[b] = self._len_before[b] + int(emitted[b])
                self._gen_ub[b] = self._gen_before[b] + int(emitted[b])

    def _check_capacity(self, per_step: int, slots: Optional[Sequence[int]] = None) -> None:
        cap_out = self.gen_tokens.shape[1]
        for b in (range(self.B) if slots is None else slots):
            L = self._len_ub[b]
            if L <= 0:
                continue
            # the cycle writes KV at positions L-1 .. L-1+k and then knows up to L+k+1 tokens
            if L - 1 + per_step > min(self._capacity[b], self.max_model_len):
                raise ValueError(f"slot {b}: a cycle from length {L} (upper bound) needs positions up to {L - 1 + per_step - 1} "
                                 f"but the sequence holds {min(self._capacity[b], self.max_model_len)} "
                                 "(block table / max_model_len): finish the request or extend its block table")
            if self._gen_ub[b] + per_step > cap_out:
                raise ValueError(f"slot {b}: output buffer of {cap_out} tokens is full (max_new_tokens)")

    def _slots_for(self, b: int, pos: torch.Tensor) -> torch.Tensor:
        bt = self.block_tables[b].to(torch.int64)
        return (bt[pos // self.block_size] * self.block_size + pos % self.block_size).contiguous()

    # ------------------------------------------------------------------ one speculative cycle (:758-858)
    def _snapshot(self):
        # the small sequence state aside: what recover() restarts the cycle from if a device-side hand-off timed out
        ops.spec_snapshot(self.seq_lens, self.gen_lens, self.last_token, self.sampler.counters, self.sampler.rng_state,
                          self._snap_i32, self._snap_i64)

    def _cycle_head(self):
        self._snapshot()
        if self._level >= 2:   # the tokens committed since the last catch-up enter the table (idempotent: slot_sampling.py)
            self.sampling.catch_up(self.gen_tokens, self.gen_lens)
        if self._level == 4:   # ... and the guided slots' states advance over them (idempotent in the same way)
            self.sampling.guide_catch_up(self.gen_tokens, self.gen_lens)

    def _cycle_body(self):
        self._cycle_head()
        self._draft_body()
        self._verify_body()
        self._collect_errors()

    def _comm(self):
        tp = getattr(self.model, "tp", None)
        return tp if tp is not None and tp.world > 1 else None

    def _collect_errors(self):
        """Last launches of a cycle: err_word = OR of the sticky error words of this stream's hand-off workspaces and of
        the one-shot all-reduce, summed over the ranks under tensor parallelism -- every rank reads the SAME word with
        its output tokens, so the decision to re-run (or to give up) is collective by construction."""
        tp = self._comm()
        extra = []
        if tp is not None and hasattr(tp.comm, "error_word_address"):
            extra.append(tp.comm.error_word_address())
        ops.collect_error_words(ops.stream_error_words(self.device, extra), out=self.err_word)
        if tp is not None:
            tp.all_reduce(self.err_word)

    def _draft_body(self):
        m, k, B, bs = self.model, self.k, self.B, self.block_size
        # proposer: k draft steps, W4A4  (execute_model_req.w4a4 = True, :799)
        # (the lengths of the slots taking part, the first draft step's inputs and its embedding rows: one launch)
        emb_d = (m.embed_tokens, self.scratch_draft.hidden[:B]) if self.EMBED_IN_BOOKKEEPING else None
        if emb_d is not None:
            ops.spec_prepare_draft(self.last_token, self.seq_lens, self.block_tables, bs, self.d_tokens, self.d_pos,
                                   self.d_slots, self.d_ctx, embed=emb_d, step_mask=self.step_mask, eff_lens=self.eff_lens)
        else:
            torch.mul(self.seq_lens, self.step_mask, out=self.eff_lens)
            ops.spec_prepare_draft(self.last_token, self.eff_lens, self.block_tables, bs, self.d_tokens, self.d_pos,
                                   self.d_slots, self.d_ctx)
        tp = self._comm()
        draft_sv = tp is not None and getattr(tp, "shard_draft_vocab", False)   # vocab-parallel lm_head on the draft pass too
        for i in range(k):
            hs = m.forward(self.d_tokens, self.d_pos, self.kv_caches, self.md_draft, self.scratch_draft, w4a4=True,
                           embedded=emb_d is not None, **self._kv_fw)
            # (from level 1 on SAMPLED from the processed draft distribution, sampler.py:216-316; step i sees d_1 .. d_i in flight)
            self._sample(self._level, self.sampling.draft_rows(), hs, self.scratch_draft, self.draft_probs_kbv[i],
                         self.draft_ids_kb[i], base_pos=self.seq_lens, j_base=i, draw_stream=1, active_lens=self.eff_lens,
                         draft_ids=self.draft_ids_kb, workspace=self._sample_ws_d, shard_vocab=draft_sv, fused_greedy=True)
            if i != k - 1:  # _gpu_advance_step (draft_model_runner.py:78-135)
                ops.spec_advance_draft(bs, self.d_tokens, self.draft_ids_kb[i], self.d_pos, self.d_ctx, self.d_slots,
                                       self.block_tables, embed=emb_d)

    def _verify_body(self):
        m, k, B, bs = self.model, self.k, self.B, self.block_size
        # scorer: one W4A16 pass over [last, d_1..d_k] per sequence  (w4a4 = False, :812; mqa_scorer.py)
        draft_ids = self.draft_ids_kb.transpose(0, 1)            # [B,k] view
        draft_probs = self.draft_probs_kbv.transpose(0, 1)       # [B,k,V] view
        emb_v = (m.embed_tokens, self.scratch_verify.hidden[:B * (k + 1)]) if self.EMBED_IN_BOOKKEEPING else None
        ops.spec_prepare_verify(self.last_token, draft_ids, self.eff_lens, self.block_tables, bs, self.v_tokens,
                                self.v_pos, self.v_slots, self.v_ctx, embed=emb_v)
        hs = m.forward(self.v_tokens, self.v_pos, self.kv_caches, self.md_verify, self.scratch_verify, w4a4=False,
                       embedded=emb_v is not None, **self._kv_fw)
        # verify row j = 0..k sees d_1 .. d_j in flight
        self._sample(self._level, self.sampling.verify_rows(), hs, self.scratch_verify, self.target_probs.view(B * (k + 1), -1),
                     self.target_tokens.view(-1), base_pos=self.seq_lens, rows_per_seq=k + 1, active_lens=self.eff_lens,
                     draft_ids=self.draft_ids_kb, workspace=self._sample_ws_v, shard_vocab=True,
                     hook=self._verify_logits_hook(draft_ids), fused_greedy=True)
        # the rejection sampler's own draws are seeded per sequence in the sampling modes only; base position = seq_lens at the
        # start of the cycle (read on the device at replay, restored by recover(), so a replayed cycle repeats its draws)
        seeded = dict(seq_seeds=self.sampling.seq_seed, seq_seeded=self.sampling.seq_seeded, base_pos=self.seq_lens) \
            if self._level >= 1 else {}
        # _verify_tokens (:861-970): bonus = the target's own token at the last position
        self.sampler.forward(self.target_probs, self.target_tokens[:, k], draft_probs, draft_ids, out=self.out_tokens,
                             accepted=self.accepted, recovered=self.recovered, uniform=self.inject_uniform,
                             exponential=self.inject_exponential, active_lens=self.eff_lens, **seeded)
        # _create_output_sampler_list bookkeeping (:972-1063)
        ops.spec_commit(self.out_tokens, self.seq_lens, self.last_token, self.gen_tokens, self.gen_lens)

    @torch.no_grad()
    def _verify_logits_hook(self, draft_ids):
        """A callable(logits) applied to the verify logits inside the cycle, or None.  The product has none; bench.py's
        BenchEngine overrides this (synthetic draft/target agreement).  A method, not a stored closure: an engine must
        not sit in a reference cycle -- its hipGraphs would then be destroyed by the cyclic collector at an arbitrary
        moment, and destroying a graph while another capture is under way aborts the process."""
        return None

    def _set_participants(self, participants: Optional[Sequence[int]]) -> List[int]:
        if participants is not None and self._prefilling and any(b in self._prefilling for b in participants):
            raise ValueError(f"slot {[b for b in participants if b in self._prefilling]}: the prompt is only partly computed")
        want = [1] * self.B if participants is None else [1 if b in participants else 0 for b in range(self.B)]
        if want != self._mask_host:
            self.step_mask.copy_(torch.tensor(want, dtype=torch.int32), non_blocking=False)
            self._mask_host = want
        return [b for b in range(self.B) if want[b] and self._len_ub[b] > 0]

    def step_no_spec(self, participants: Optional[Sequence[int]] = None):
        """One NON-speculative decode step (spec_decode_worker.py:666-720 on a decode batch: the scorer alone, W4A16,
        one token per sequence): taken when speculation is disabled for a step (`num_lookahead_slots == 0`,
        `speculative_disable_by_batch_size`).  Eager: it is the rare path, the captured graph is the cycle's."""
        m, bs = self.model, self.block_size
        on = self._set_participants(participants)
        self._check_capacity(1, on)
        self._len_before, self._gen_before = list(self._len_ub), list(self._gen_ub)
        torch.mul(self.seq_lens, self.step_mask, out=self.eff_lens)
        ops.spec_prepare_draft(self.last_token, self.eff_lens, self.block_tables, bs, self.d_tokens, self.d_pos,
                               self.d_slots, self.d_ctx)                   # [last token] at position seq_len - 1
        hs = m.forward(self.d_tokens, self.d_pos, self.kv_caches, self.md_draft, self.scratch_draft, w4a4=False, **self._kv_fw)
        # the mode of ALL occupied slots; position j = 0, nothing in flight: catch up with the committed tokens, then the pre-pass
        level = self.sampling.level(self.active_slots())
        if level >= 2:
            self.sampling.catch_up(self.gen_tokens, self.gen_lens)
        if level == 4:
            self.sampling.guide_catch_up(self.gen_tokens, self.gen_lens)
        self._sample(level, self.sampling.draft_rows(), hs, self.scratch_draft, self.draft_probs_kbv[0], self.draft_ids_kb[0],
                     base_pos=self.seq_lens, active_lens=self.eff_lens, workspace=self._sample_ws_d, argmax=level == 0)
        self.out_tokens.fill_(-1)
        self.out_tokens[:, 0] = torch.where(self.eff_lens > 0, self.draft_ids_kb[0], torch.full_like(self.draft_ids_kb[0], -1))
        ops.spec_commit(self.out_tokens, self.seq_lens, self.last_token, self.gen_tokens, self.gen_lens)
        for b in on:
            self._len_ub[b] += 1
            self._gen_ub[b] += 1

    @torch.no_grad()
    def step(self, participants: Optional[Sequence[int]] = None):
        """Enqueue one cycle on the current stream (graph replay after the first call).  Raises ValueError -- before
        anything is enqueued -- if a sequence could outgrow its block table, max_model_len or the output buffer.
        participants: the slots taking part (default: every occupied slot); the others keep their state."""
        on = self._set_participants(participants)
        self._check_capacity(self.k + 1, on)
        self._len_before, self._gen_before = list(self._len_ub), list(self._gen_ub)
        for b in on:                       # until the caller reports / syncs the real numbers: the worst case
            self._len_ub[b] += self.k + 1
            self._gen_ub[b] += self.k + 1
        # (every rank sees the same requests: the same decisions)
        level = self._level = self.sampling.level(self.active_slots())
        if not self.use_graph:
            self._cycle_body()
            return
        full, draft = self._graphs.get((level, "full")), self._graphs.get((level, "draft"))
        if full is None and draft is None:
            self._capture()
            if not self.use_graph:
                self._cycle_body()
                return
            full, draft = self._graphs.get((level, "full")), self._graphs.get((level, "draft"))
        if full is not None:
            full.replay()
        else:   # the verify pass could not be captured (its collectives): proposer from its graph, scorer eagerly.
            # The same bracket as _cycle_body: the state snapshot sits at the head of the draft graph (_capture), the
            # error words are collected behind the eager verify pass -- read_outputs() / recover() work in this mode too
            draft.replay()
            self._verify_body()
            self._collect_errors()

    def _capture(self):
        """Capture the cycle of the current level: the whole cycle, else the draft pass alone (verify eager), else eager."""
        import gc
        import warnings
        # warm up outside capture (lazy module loads, LDS attribute), on a side stream as torch requires.
        # The warm-up cycle advances the sequence state; restore it so capture does not consume tokens.
        live = (self.seq_lens, self.last_token, self.gen_tokens, self.gen_lens, self.sampler.counters, self.sampler.rng_state)
        state = [t.clone() for t in live]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._cycle_body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gc.collect()   # no stale CUDAGraph may be finalised while this capture is under way
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._cycle_body()
            self._graphs[(self._level, "full")] = g
        except Exception as exc:  # e.g. a collective backend that cannot be captured: loudly, not silently
            torch.cuda.synchronize()
            try:   # the proposer has no collectives (replicated under TP): keep its k forwards in a graph
                gd = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gd):
                    self._cycle_head()
                    self._draft_body()
                self._graphs[(self._level, "draft")] = gd
                warnings.warn(f"hipGraph capture of the whole cycle failed ({exc!r}); "
                              "the draft pass replays from a graph, the verify pass runs eagerly")
            except Exception as exc2:
                warnings.warn(f"hipGraph capture failed ({exc!r}; draft only: {exc2!r}); running the cycle eagerly")
                self.use_graph = False
        torch.cuda.synchronize()
        for t, s in zip(live, state):   # every exit path: the sequence state of before the warm-up
            t.copy_(s)

    # ------------------------------------------------------------------ results
    def generated(self) -> List[List[int]]:
        torch.cuda.synchronize()
        lens = self.gen_lens.tolist()
        toks = self.gen_tokens.cpu()
        return [toks[b, :lens[b]].tolist() for b in range(self.B)]

    def metrics(self) -> SpecDecodeWorkerMetrics:
        a, e, d = (int(v) for v in self.sampler.counters.tolist())
        return metrics_from_counters(a, e, d, self.k)

    def max_cycles_left(self) -> int:
        """Cycles that can still run before step() would refuse (exact lengths: syncs)."""
        self.sync_lens()
        room = []
        for b in self.active_slots():
            cap = min(self._capacity[b], self.max_model_len)
            room.append((cap - self._len_ub[b] + 1) // (self.k + 1))
            room.append((self.gen_tokens.shape[1] - self._gen_ub[b]) // (self.k + 1))
        return max(0, min(room)) if room else 0

    def read_outputs(self):
        """The worker's ONE host read per cycle: (out_tokens [B, k+1] on the host, error word).  A non-zero error word
        means a device-side hand-off (spread Hadamard, norm hand-off, one-shot all-reduce) timed out somewhere in the
        cycle on some rank: the tokens are invalid; see recover()."""
        self._out_err_host.copy_(self._out_err, non_blocking=True)
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        host = self._out_err_host
        return host[:-1].view(self.B, self.k + 1), int(host[-1])

    @torch.no_grad()
    def recover(self) -> None:
        """Re-run the cycle that has just failed (read_outputs() returned a non-zero error word) from the state
        snapshot taken at its start, eagerly and WITHOUT the kernels that wait for partner workgroups: the spread MLP
        Hadamard and the norm hand-off fall back to their one-workgroup / recompute forms, which are bit-identical
        (tests/test_kernels_gpu.py), so the replayed cycle emits exactly what the failed one should have.  The KV slots
        the failed cycle wrote are the ones the replay rewrites.  The caller reads the outputs again; a second failure
        (e.g. a lost tensor-parallel peer) is final."""
        ops.spec_snapshot(self.seq_lens, self.gen_lens, self.last_token, self.sampler.counters, self.sampler.rng_state,
                          self._snap_i32, self._snap_i64, restore=True)
        self.clear_error_words()
        with ops.no_handoffs():   # this thread only: other engines of the process keep their launch forms
            self._cycle_body()
        self.recoveries += 1

    def clear_error_words(self) -> None:
        ops.clear_error_words(self.device)
        tp = self._comm()
        if tp is not None and hasattr(tp.comm, "error_word_address"):
            ops.collect_error_words([tp.comm.error_word_address()], clear=True)
        self.err_word.zero_()

    def error_flag(self) -> int:
        """Sticky device-side error words of EVERY hand-off workspace of the device and of the one-shot all-reduce, read
        from the host (0 = fine).  The cycle itself reports through read_outputs(); this is the out-of-band check."""
        words = ops.error_words(self.device)
        flag = int(torch.cat(words).abs().max().item()) if words else 0
        tp = self._comm()
        if tp is not None and hasattr(tp.comm, "error"):
            flag |= int(tp.comm.error())
        return flag
