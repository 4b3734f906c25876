"""QuarotLlamaForCausalLM on MI355X: the model shared by the draft (W4A4) and verify (W4A16) passes.

Mirror of vllm/model_executor/models/quarot_llama.py (QuarotLlamaAttention :62, QuarotLlamaMLP :247,
QuarotDecoderLayer :319, LlamaModel :436, QuarotLlamaForCausalLM :597): same weights, same op order, same
`forward(input_ids, positions, kv_caches, attn_metadata, **kwargs)` with the `w4a4` kwarg selecting the pass.
One set of packed int4 weights and one paged KV cache serve both passes.

Two implementations of the layer body:
  * `forward`            -- the product path: 7 (draft) / 9 (verify) fused HIP launches per layer, no transposes / copies;
  * `forward_modulewise` -- module by module through qspec_amd.quarot_nn exactly in the reference's order
                            (one reference op per call); kept for parity tests of the fusion.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import List, NamedTuple, Optional

import torch

from . import hadamard_tables, ops, quarot_nn


@dataclass
class QuarotLlamaConfig:
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_attention_heads: int = 32
    num_key_value_heads: int = 8
    num_hidden_layers: int = 32
    vocab_size: int = 128256
    rms_norm_eps: float = 1e-5
    rope_theta: float = 500000.0
    max_position_embeddings: int = 8192
    name: str = "llama-3-8b"

    @property
    def head_dim(self):
        return self.hidden_size // self.num_attention_heads

    @property
    def q_size(self):
        return self.num_attention_heads * self.head_dim

    @property
    def kv_size(self):
        return self.num_key_value_heads * self.head_dim

    def packed_weight_bytes_per_layer(self):
        H, I = self.hidden_size, self.intermediate_size
        return ((self.q_size + 2 * self.kv_size) * H + H * H + 2 * I * H + H * I) // 2

    def algorithmic_bytes_per_forward(self):
        """packed weights + channel scales + fp16 lm_head (KV reads and activations excluded)."""
        H, I, L = self.hidden_size, self.intermediate_size, self.num_hidden_layers
        scales = 2 * (self.q_size + 2 * self.kv_size + H + 2 * I + H) * L
        return self.packed_weight_bytes_per_layer() * L + scales + 2 * self.vocab_size * H


CONFIGS = {
    "llama-3-8b": QuarotLlamaConfig(),
    "tinyllama-1.1b": QuarotLlamaConfig(2048, 5632, 32, 4, 22, 32000, 1e-5, 10000.0, 2048, "tinyllama-1.1b"),
    "llama-2-13b": QuarotLlamaConfig(5120, 13824, 40, 40, 40, 32000, 1e-5, 10000.0, 4096, "llama-2-13b"),
    "llama-3-70b": QuarotLlamaConfig(8192, 28672, 64, 8, 80, 128256, 1e-5, 500000.0, 8192, "llama-3-70b"),
}


@dataclass
class AttentionMetadata:
    """What vllm's FlashAttentionMetadata carries for this path (vllm/attention/backends/flash_attn.py:96-180)."""
    slot_mapping: torch.Tensor          # [T] i64
    block_tables: torch.Tensor          # [B, max_blocks] i32
    ctx_lens: torch.Tensor              # [B] i32: keys visible to the LAST query token of each sequence
    q_start: torch.Tensor               # [B+1] i32: query_start_loc
    max_q_len: int
    n_splits: int                       # context splits for the attention kernel (fixed per captured graph)


class Scratch:
    """Per-shape activation buffers, allocated once (the reference re-allocates ten of them every draft step,
    vllm/spec_decode/draft_model_runner.py:279-320; names kept)."""

    def __init__(self, cfg: QuarotLlamaConfig, T: int, n_seqs: int, max_q_len: int, n_splits: int, device,
                 logits_rows: Optional[int] = None):
        H, I = cfg.hidden_size, cfg.intermediate_size
        f16, i8 = torch.float16, torch.int8
        e = lambda *s, dtype=f16: torch.empty(*s, dtype=dtype, device=device)  # noqa: E731
        self.T = T
        self.hidden = e(T, H)
        self.normed = e(T, H)                                  # verify: fp16 LN output
        self.quantized_buffer_qkv = e(T, H // 2, dtype=i8)     # draft: int4 activations of width H
        self.quantized_buffer_mlp = e(T, I // 2, dtype=i8)
        self.scale_buffer = e(T)
        self.input_sum_buffer = e(T)
        self.act_buffer_qkv = e(T, cfg.q_size + 2 * cfg.kv_size)
        self.act_buffer_attn = e(T, cfg.q_size)
        self.act_buffer_had = e(T, cfg.q_size)
        self.act_buffer_output = e(T, H)
        self.act_buffer_gate_up = e(T, 2 * I)
        self.act_buffer_had_mlp = e(T, I)
        self.logits = e(T if logits_rows is None else logits_rows, cfg.vocab_size)
        # verify pass: raw fp32 K-slice sums of down_proj, finished inside the next norm (ops.w4a16_linear_partial)
        # (17..256 tokens: the M-tiled kernel's plan slices narrow layers up to eight ways)
        self.down_part = e(4 if T <= 16 else 8, T, H, dtype=torch.float32) if T <= 256 else None
        # verify pass: fragment-major 16-row activation tiles between the producers and the W4A16 GEMMs -- one up to 16 tokens
        # (ops.w4a16_act_layout_supported), two up to 32 (..._layout32_supported); rows past T are never read back into a result
        z = lambda k: torch.zeros(16 if T <= 16 else 32, k, dtype=f16, device=device) if T <= 32 else None  # noqa: E731
        self.xp_normed, self.xp_had, self.xp_had_mlp = z(H), z(cfg.q_size), z(I)
        self.tp_part = e(1, min(T, 32), H, dtype=torch.float32)   # TP verify pass (T <= 32): fp32 row-parallel partials
        self.had_part_amax = e(min(T, 16), 8, dtype=torch.float32)  # draft pass (T <= 4): partial row maxima of the spread head Hadamard
        # draft pass at 17..32 tokens: int32 K-slice sums of down_proj + the activation scales they were computed with
        self.down_ipart = e(2, T, H, dtype=torch.int32) if 16 < T <= 32 else None
        self.down_xs = e(T) if 16 < T <= 32 else None
        ws = ops.paged_attention_workspace_bytes(n_seqs * max_q_len, cfg.num_attention_heads, cfg.head_dim, n_splits)
        self.attn_ws = torch.zeros(ws, dtype=torch.uint8, device=device)   # ticket counters start at zero

    def k_slices(self, S: int, T: int, int32: bool = False):
        """[S, T, H] at the head of down_part (raw fp32 K-slice sums of a W4A16 GEMM) or down_ipart (int32, of an s4s4 GEMM)."""
        buf = self.down_ipart if int32 else self.down_part
        H = buf.shape[-1]
        return buf.view(-1)[:S * T * H].view(S, T, H)

    def mlp_rows(self, T: int):
        """[T, I] at the head of act_buffer_gate_up: where the fp16 MLP transform goes once gate_up's output is consumed."""
        I = self.act_buffer_gate_up.shape[1] // 2
        return self.act_buffer_gate_up.view(-1)[:T * I].view(T, I)


@dataclass(frozen=True)
class ForwardPlan:
    """The launch form of one forward() call (QuarotLlamaForCausalLM._plan); the layer stages branch on nothing else."""
    form: str        # last_forward_form: "two-tile" | "fragment-major" | "fused" | "unfused"
    w4a4: bool       # draft pass
    fuse: bool       # fused GEMM epilogues (qkv + RoPE + KV write, gate_up + SiLU)
    ln_fused: bool   # draft: residual add + LN + int4 quant in the qkv / gate_up prologues (gemm_stream_w4a4.hip), no hand-over
    hq: bool         # ... and the head transform's quantiser in o_proj's prologue
    xp: bool         # verify, <= 16 tokens: fragment-major activation tiles
    xp32: bool       # verify, 17..32 tokens: two tiles, the two-token-tile streaming kernel
    tp_on: bool      # verify: o_proj / gate_up / down_proj sharded over self.tp
    heads: str       # head transform: "merged" | "mix_merged" (it merges the attention's context splits) | "generic"
    S_down: int      # K slices whose raw sums the next norm finishes (0: the plain launch) of the draft down_proj (int32 sums),
    S_mlp: int       # ... the verify down_proj,
    S_o: int         # ... the verify o_proj,
    S32: int         # ... the down_proj of the two-tile form


class Delta(NamedTuple):
    """What a projection hands to the next norm, which adds it to the residual stream: its fp16 output (f16), its raw K-slice
    sums -- fp32 of a W4A16 GEMM (part), int32 of an s4s4 GEMM with its activation scales (ipart, x_scale) -- or nothing."""
    f16: Optional[torch.Tensor] = None
    part: Optional[torch.Tensor] = None
    ipart: Optional[torch.Tensor] = None
    x_scale: Optional[torch.Tensor] = None
    w_scale: Optional[torch.Tensor] = None
    slices: int = 0


def _knob(name: str, default):
    """The environment's QSPEC_<name>: an int where the default is one, else a switch that only "0" turns off."""
    v = os.environ.get("QSPEC_" + name)
    return default if v is None else (v != "0" if isinstance(default, bool) else int(v))


class DecoderLayerWeights:
    def __init__(self, cfg: QuarotLlamaConfig, device):
        H, I = cfg.hidden_size, cfg.intermediate_size
        mk = lambda i, o: quarot_nn.Linear4bit(i, o, bias=False, device=device)  # noqa: E731
        self.qkv_proj = mk(H, cfg.q_size + 2 * cfg.kv_size)   # rows [q; k; v]   (fuse_qkv, quarot_llama.py:152-173)
        self.o_proj = mk(H, H)
        self.gate_up = mk(H, 2 * I)                            # rows [up; gate]  (fuse_gate_up, :301-314)
        self.down_proj = mk(I, H)

    def linears(self):
        return (self.qkv_proj, self.o_proj, self.gate_up, self.down_proj)


class QuarotLlamaForCausalLM:
    def __init__(self, cfg: QuarotLlamaConfig, device="cuda:0"):
        self.config = cfg
        self.device = torch.device(device)
        self.layers: List[DecoderLayerWeights] = [DecoderLayerWeights(cfg, device) for _ in range(cfg.num_hidden_layers)]
        self.embed_tokens = torch.zeros(cfg.vocab_size, cfg.hidden_size, dtype=torch.float16, device=device)
        self.lm_head = torch.zeros(cfg.vocab_size, cfg.hidden_size, dtype=torch.float16, device=device)
        had, self.had_K = hadamard_tables.get_hadK(cfg.intermediate_size)
        self.had_rem_dim = had.to(torch.float16).to(device) if had is not None else None
        hh, self.head_had_K = hadamard_tables.get_hadK(cfg.num_attention_heads)   # table factor for 12/20/28/40.. heads
        self.head_had = hh.to(torch.float16).to(device) if hh is not None else None
        self.head_had_scale = float(1.0 / torch.tensor(cfg.num_attention_heads).sqrt())      # hadamard.py:12
        self.mlp_had_scale = float(1.0 / torch.tensor(cfg.intermediate_size).sqrt())         # hadamard.py:13
        self.sm_scale = cfg.head_dim ** -0.5
        self.cos_sin_cache = make_cos_sin_cache(cfg.head_dim, cfg.max_position_embeddings, cfg.rope_theta).to(device)
        # module-wise mirrors share the same buffers
        self.norm = quarot_nn.RMSNorm(cfg.hidden_size, cfg.rms_norm_eps)
        self.quantizer = quarot_nn.Quantizer()
        self.tp = None   # qspec_amd.parallel.TensorParallel for the verify pass (None = single GPU)

    # ------------------------------------------------------------------ weights
    @torch.no_grad()
    def init_synthetic(self, seed: int = 0, lm_head_std: float = 0.02):
        """SURVEY.md 8d synthetic model: int4 weights U{-8..7}, scales |N(0,1)|*0.01+1e-3, embed/lm_head N(0,0.02)."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        for layer in self.layers:
            for lin in layer.linears():
                n, kb = lin.weight.shape
                lin.weight.copy_(torch.randint(0, 256, (n, kb), generator=g, device=self.device, dtype=torch.int16)
                                 .to(torch.uint8).view(torch.int8))
                lin.weight_scales.copy_((torch.randn(n, 1, generator=g, device=self.device).abs() * 0.01 + 1e-3)
                                        .to(torch.float16))
        self.embed_tokens.copy_((torch.randn(self.embed_tokens.shape, generator=g, device=self.device) * 0.02)
                                .to(torch.float16))
        self.lm_head.copy_((torch.randn(self.lm_head.shape, generator=g, device=self.device) * lm_head_std)
                           .to(torch.float16))
        return self

    # M above which the fused GEMM epilogues (QKV+RoPE+KV write, gate_up+SiLU) give way to plain GEMM + separate kernels
    BIG_M = 64
    # verify pass: the fused-epilogue W4A16 forms are the 16-row streaming kernels; from 17 rows on the M-tiled kernel
    # (gemm_tiled.hip) + separate RoPE / SiLU launches is faster than the first-generation 2-D kernel that used to take
    # 17..64 rows (Llama-3-70B, bs = 8, T = 32: 51.2 -> 47.9 ms per cycle; Llama-3-8B bs = 8: 9.81 -> 9.56).  The
    # tensor-parallel shard views (K-sliced / channel-sharded streaming forms, T <= 32) keep the fused path.
    VERIFY_FUSE_MAX_M = _knob("VERIFY_FUSE_MAX_M", 16)
    # draft pass: LN in the GEMM prologue up to this many tokens (0 = always a separate LN launch; bit-identical).
    # Measured in the engine (round 2): bs = 4 fused 8.39 vs separate 8.43 ms per cycle; bs = 16 fused (hand-off form)
    # 14.30 vs separate 13.38 ms -- the standalone norm launch (3.4 us) beats the hand-off from 8 tokens on.
    FUSE_LN_MAX_M = _knob("FUSE_LN_MAX_M", 4)
    # dev knob (2 / 4): the verify o_proj at <= 16 tokens as K slices whose raw sums the norm finishes, as down_proj's are --
    # measured, not the default: the slice order of the sum also breaks the bit identity with the
    # module-wise path
    VERIFY_O_SLICES = _knob("VERIFY_O_SLICES", 0)
    FUSE_LN = True
    # draft pass, T <= 4, 32 heads of 128: merge + head Hadamard spread over 8 workgroups per token (fp16 + partial row maxima),
    # the Quantizer of :235-238 in the o_proj launch's prologue: same bits as the quantising head transform + plain o_proj
    HADAMARD_QUANT_IN_OPROJ = _knob("HQ_OPROJ", True)
    # verify pass at <= 16 tokens (one GPU): the norm / head transform / MLP transform store their fp16 rows as the
    # FRAGMENT-MAJOR tile the W4A16 GEMMs' MFMA operands are loaded from (include/qspec_hip.h "activation layout"), which
    # removes the LDS regrouping pass from the head of four launches per layer.  Same bits either way.
    ACT_FRAGMENT_MAJOR = _knob("ACT_FRAGMENT_MAJOR", True)
    XP32_DOWN_SLICES = _knob("XP32_DOWN_SLICES", True)
    TILED_PARTIAL_IN_NORM = _knob("TILED_PARTIAL_IN_NORM", True)
    MERGE_IN_HADAMARD = True   # False: the attention kernel merges its context splits itself (ticket + fences)
    DOWN_K_SLICES = _knob("DOWN_K_SLICES", True)   # draft down_proj at 17..32 tokens as K slices

    # FP8 KV cache: per-layer (k_scale, v_scale) read from the checkpoint (model.layers.{i}.self_attn.k_scale / .v_scale);
    # None = 1.0 everywhere.  Only consulted when the cache tensors are bytes.  A caller with scales of its own (the engine's
    # `kv_scales`) passes them to forward(): several engines share one model, so nobody writes them here.
    kv_scales = None

    def _kv_kw(self, li, kc, kv_scales=None):
        """Keywords of the ops that touch the cache of layer li: nothing for an fp16 cache (the calls are exactly those of a
        model that knows no fp8), the layer's scales for an fp8 cache -- the caller's, else the checkpoint's, else 1.0.  No
        launch-form decision depends on it."""
        if kc.dtype == torch.float16:
            return {}
        if kv_scales is None:
            kv_scales = self.kv_scales
        ks, vs = kv_scales[li] if kv_scales is not None else (1.0, 1.0)
        return {"k_scale": float(ks), "v_scale": float(vs)}

    def weight_bytes(self):
        n = sum(lin.weight.numel() + lin.weight_scales.numel() * 2 for l in self.layers for lin in l.linears())
        return n + self.embed_tokens.numel() * 2 + self.lm_head.numel() * 2

    # ------------------------------------------------------------------ fused product path
    def _plan(self, T: int, w4a4: bool, n_splits: int, s: Scratch) -> ForwardPlan:
        """Every launch-form decision of one forward() call, from host values only: the config, the knobs above, self.tp,
        which optional buffers `s` has, and the library's shape queries.  Not memoised: the knobs may change between calls."""
        cfg, K = self.config, self.head_had_K
        H, I, Q, nh, hd = cfg.hidden_size, cfg.intermediate_size, cfg.q_size, cfg.num_attention_heads, cfg.head_dim
        row = Q + 2 * cfg.kv_size
        tp_sharded = self.tp is not None and self.tp.world > 1 and getattr(self.tp, "shard_layers", True) and not w4a4
        # (head size 64 -- TinyLlama -- has the fused qkv + RoPE + KV-write epilogue on the streaming kernels only)
        fuse_hd = hd == 128 or (hd == 64 and T <= 32 and ops.qkv_rope_linear_supported(w4a4, T, row, H, 64))
        fuse = fuse_hd and (w4a4 or T <= (min(self.BIG_M, 32) if tp_sharded else self.VERIFY_FUSE_MAX_M))
        # tensor parallelism only on the verify pass at decode-sized M; the draft pass and prefill run replicated
        tp_on = tp_sharded and fuse and T <= 32
        # head transform: for 32 / 64 heads of 128 the split merge of the attention kernel runs at the head of the Hadamard
        # launch (other head sizes -- TinyLlama's 64 -- leave their split partials to the same launch when there are 32 heads);
        # a head count with a table factor (40 heads = had40) spreads merge + transform over 8 workgroups per token
        splits_ok = self.MERGE_IN_HADAMARD and n_splits <= 64
        mix_spread = splits_ok and K > 1 and ops.heads_hadamard_mix_merged_spread_supported(T, nh, hd, K)
        merged = splits_ok and K == 1 and ((hd == 128 and nh in (32, 64)) or (hd != 128 and hd % 8 == 0 and nh == 32))
        ln_fused = bool(w4a4 and fuse and self.FUSE_LN and T <= self.FUSE_LN_MAX_M
                        and ops.ln_linear_s4s4_supported(T, row, H) and ops.ln_linear_s4s4_supported(T, 2 * I, H)
                        and ops.rowwise_scaled_linear_s4s4_residual_supported(T, H, H)
                        and ops.rowwise_scaled_linear_s4s4_residual_supported(T, H, I))
        hq = bool(ln_fused and self.HADAMARD_QUANT_IN_OPROJ and splits_ok
                  and (ops.heads_hadamard_merged_spread_supported(T, nh, hd) if K == 1 else mix_spread)
                  and ops.rowwise_scaled_linear_s4s4_residual_hq_supported(T, H, Q))
        S_down = (ops.rowwise_scaled_linear_s4s4_partial_slices(T, H, I)
                  if (w4a4 and fuse and not ln_fused and s.down_ipart is not None and self.DOWN_K_SLICES) else 0)
        # verify down_proj as K slices: long K at <= 16 tokens (streaming kernel), narrow layers above (M-tiled kernel's plan)
        S = (ops.w4a16_linear_partial_slices(T, H, I) if (not w4a4 and not tp_on and s.down_part is not None
                                                          and (fuse or (T > 16 and self.TILED_PARTIAL_IN_NORM))) else 0)
        tiles = not w4a4 and not tp_sharded and self.ACT_FRAGMENT_MAJOR and splits_ok and hd == 128 and s.xp_normed is not None
        # verify pass at <= 16 tokens: every producer and consumer has its fragment-major form at this shape
        down_k = I // S if 0 < S <= 4 else (I if S == 0 else 0)
        xp = bool(tiles and fuse and T <= 16 and self.VERIFY_O_SLICES <= 1 and down_k and (nh == 32 if K == 1 else mix_spread)
                  and ops.w4a16_act_layout_supported(T, H) and ops.w4a16_act_layout_supported(T, Q)
                  and ops.w4a16_act_layout_supported(T, down_k) and ops.mlp_hadamard_act_layout_supported(T, I, self.had_K))
        # verify pass at 17..32 tokens: qkv / o_proj / gate_up on the two-token-tile W4A16 streaming kernel over two
        # fragment-major tiles (fused epilogues as at <= 16 tokens); down_proj stays on the M-tiled kernel (its K passes lose) ...
        xp32 = bool(tiles and not fuse and 16 < T <= 32 and s.xp_normed.shape[0] == 32
                    and ops.w4a16_act_layout32_supported(T, row, H) and ops.w4a16_act_layout32_supported(T, H, Q)
                    and ops.w4a16_act_layout32_supported(T, 2 * I, H) and (nh in (32, 64) if K == 1 else mix_spread))
        # ... or runs as one-pass K slices of the same kernel across the workgroups, finished inside the next norm
        S32 = (ops.w4a16_linear_partial_slices_xp32(T, H, I) if (xp32 and s.down_part is not None and self.XP32_DOWN_SLICES
                                                                 and ops.mlp_hadamard_act_layout_supported(T, I, self.had_K)) else 0)
        # verify o_proj at 17+ tokens: where the M-tiled kernel's plan slices K, the norm finishes the raw sums (same bits)
        sliced_o = not (w4a4 or tp_on or xp or xp32) and s.down_part is not None
        S_o = ops.w4a16_linear_partial_slices(T, H, Q) if (sliced_o and T > 16 and self.TILED_PARTIAL_IN_NORM) else 0
        S_o = S_o if 1 < S_o <= 8 else 0
        if sliced_o and fuse and T <= 16 and self.VERIFY_O_SLICES > 1:
            S_o = self.VERIFY_O_SLICES
        return ForwardPlan(form="two-tile" if xp32 else ("fragment-major" if xp else ("fused" if fuse else "unfused")),
                           w4a4=w4a4, fuse=bool(fuse), ln_fused=ln_fused, hq=hq, xp=xp, xp32=xp32, tp_on=bool(tp_on),
                           heads="mix_merged" if mix_spread else ("merged" if merged else "generic"),
                           S_down=S_down if S_down > 1 else 0, S_mlp=S if 0 < S <= (4 if T <= 16 else 8) else 0,
                           S_o=S_o, S32=S32 if 1 < S32 <= 8 else 0)

    def forward(self, input_ids, positions, kv_caches, attn_metadata: AttentionMetadata, scratch: Scratch,
                w4a4: bool = False, embedded: bool = False, kv_scales=None, **kwargs):
        """LlamaModel.forward (quarot_llama.py:484-535) + final norm; returns the normed hidden states [T,H].
        embedded: scratch.hidden[:T] already holds embed_tokens[input_ids] (the engine's bookkeeping launches write it:
        ops.spec_prepare_draft / spec_advance_draft / spec_prepare_verify with embed=...)."""
        s, T = scratch, input_ids.numel()
        p = self._plan(T, w4a4, attn_metadata.n_splits, s)
        self.last_forward_form = p.form   # (tests)
        tiles = p.xp or p.xp32
        # what the stages share: the plan, the inputs and the [:T] views of the buffers.  (x, xs): what the norms and the draft
        # head transform write and the GEMMs read -- int4 rows + scales in the draft pass, fp16 rows in the verify pass; they
        # and had, the fp16 head transform, are fragment-major tiles in the two tile forms.  act: silu(gate)*up, [T, I]
        c = SimpleNamespace(p=p, s=s, md=attn_metadata, T=T, positions=positions, eps=self.config.rms_norm_eps, tiles=tiles,
                            hidden=s.hidden[:T], qkv=s.act_buffer_qkv[:T], attn=s.act_buffer_attn[:T], o=s.act_buffer_output[:T],
                            gu=s.act_buffer_gate_up[:T], act=s.act_buffer_had_mlp[:T], q3=s.quantized_buffer_mlp[:T],
                            normed=s.normed[:T], had=s.xp_had if tiles else s.act_buffer_had[:T],
                            x=s.quantized_buffer_qkv[:T] if w4a4 else (s.xp_normed if tiles else s.normed[:T]),
                            xs=s.scale_buffer[:T] if w4a4 else None)
        if not embedded:
            ops.embedding(input_ids, self.embed_tokens, c.hidden)
        delta = Delta()
        for li, layer in enumerate(self.layers):
            kc, vc = kv_caches[li]
            kvs = self._kv_kw(li, kc, kv_scales)
            if p.ln_fused:
                self._ln_fused_layer(c, layer, kc, vc, kvs)
            else:
                self._norm_qkv(c, layer, kc, vc, kvs, delta)
                self._attention_o_proj(c, layer, kc, vc, kvs)
                delta = self._mlp(c, layer)
        self._add_norm(c, delta, final=True)
        return c.normed

    def _add_norm(self, c, delta: Delta, final: bool = False):
        """hidden += delta; then the norm of hidden into (c.x, c.xs) -- the final norm is always fp16 and row-major, in both
        passes (self.norm(hidden_states) without kwargs, :533)."""
        hidden, eps = c.hidden, c.eps
        i4 = c.p.w4a4 and not final
        out, xp = (c.normed, False) if final else (c.x, c.tiles)
        if delta.ipart is not None:
            ops.add_rms_norm_ipartial(hidden, hidden, delta.ipart, delta.x_scale, delta.w_scale, delta.slices, eps,
                                      q=out if i4 else None, scale=c.xs if i4 else None, out_f16=None if i4 else out)
        elif delta.part is not None:
            ops.add_rms_norm_fp16_partial(out, hidden, hidden, delta.part, delta.w_scale, delta.slices, eps, xp=xp)
        elif i4:
            ops.add_rms_norm_i4(out, c.xs, hidden, hidden, delta.f16, eps)
        else:
            ops.add_rms_norm_fp16(out, hidden, hidden, delta.f16, eps, xp=xp)

    def _attention_hadamard(self, c, kc, vc, kvs, part_amax=None):
        """Attention + head Hadamard (quarot_llama.py:213-238): + quant into (c.x, c.xs) in the draft pass, fp16 into c.had in the
        verify pass -- and in the draft pass with part_amax [T, 8], which takes the spread kernels' partial row maxima."""
        p, md, s, T, cfg = c.p, c.md, c.s, c.T, self.config
        nh, hd, n_tok = cfg.num_attention_heads, cfg.head_dim, md.ctx_lens.numel() * md.max_q_len
        spread = part_amax is not None
        q1, sc = (c.x, c.xs) if p.w4a4 and not spread else (None, None)
        had = c.had if q1 is None else None
        # attn None: the head transform merges the context splits; the spread kernels (part_amax) always do, whatever p.heads says
        attn = c.attn if p.heads == "generic" and not spread else None
        ops.paged_attention(c.qkv, c.qkv.shape[1], kc, vc, md.block_tables, md.ctx_lens, md.q_start, T, md.max_q_len, nh,
                            self.sm_scale, md.n_splits, s.attn_ws, attn, **kvs)
        if self.head_had_K > 1:   # table-factor head count (Llama-2-13B: had40)
            if attn is None:
                ops.heads_hadamard_mix_merged_spread(s.attn_ws, n_tok, md.n_splits, T, nh, hd, self.head_had, self.head_had_K,
                                                     self.head_had_scale, c.had, part_amax, xp=c.tiles)
            else:   # generic kernels: one workgroup per token
                ops.heads_hadamard_mix(attn.view(T, nh, hd), self.head_had, self.head_had_K, self.head_had_scale, c.had)
            if q1 is not None:
                ops.fuse_sym_quant(c.had, sc, q1)
        elif spread:
            ops.heads_hadamard_merged_spread(s.attn_ws, n_tok, md.n_splits, T, nh, hd, self.head_had_scale, had, part_amax)
        elif attn is None:
            ops.heads_hadamard_merged(s.attn_ws, n_tok, md.n_splits, T, nh, hd, self.head_had_scale, out_f16=had, q=q1,
                                      scale=sc, xp=c.tiles)
        else:
            ops.heads_hadamard(attn, self.head_had_scale, out_f16=had, q=q1, scale=sc, heads=nh)

    def _ln_fused_layer(self, c, layer, kc, vc, kvs):
        """The draft layer at <= FUSE_LN_MAX_M tokens, 7 launches: the norms run in the qkv / gate_up prologues, the residual
        stream is updated in the o_proj / down_proj epilogues (hidden = residual + proj_out, :380,390) -- nothing is handed over."""
        cfg, md, hidden = self.config, c.md, c.hidden
        o_w, o_s = layer.o_proj.weight, layer.o_proj._scales()
        ops.ln_qkv_rope_linear(hidden, None, None, c.eps, layer.qkv_proj.weight, layer.qkv_proj._scales(), c.qkv, c.positions,
                               self.cos_sin_cache, kc, vc, md.slot_mapping, cfg.num_attention_heads, cfg.num_key_value_heads,
                               cfg.head_dim, **kvs)                                                 # :373-374,183-226
        if c.p.hq:
            amax = c.s.had_part_amax[:c.T]
            self._attention_hadamard(c, kc, vc, kvs, part_amax=amax)
            ops.rowwise_scaled_linear_s4s4_residual_hq(c.had, amax, 1.0, o_w, o_s, hidden, hidden)
        else:
            self._attention_hadamard(c, kc, vc, kvs)                                                # :213-238
            ops.rowwise_scaled_linear_s4s4_residual(c.x, c.xs, o_w, o_s, hidden, hidden)
        ops.ln_gate_up_silu_linear(hidden, None, None, c.eps, layer.gate_up.weight, layer.gate_up._scales(), c.act)   # :380-388,266-284
        ops.mlp_hadamard(c.act, self.had_rem_dim, self.had_K, self.mlp_had_scale, q=c.q3, scale=c.xs)
        ops.rowwise_scaled_linear_s4s4_residual(c.q3, c.xs, layer.down_proj.weight, layer.down_proj._scales(), hidden, hidden)

    def _norm_qkv(self, c, layer, kc, vc, kvs, delta: Delta):
        """input_layernorm (+ residual add of the previous MLP) -> qkv_proj -> rope -> kv write    :373-374,183-226"""
        p, cfg, md = c.p, self.config, c.md
        nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        w, w_s = layer.qkv_proj.weight, layer.qkv_proj._scales()
        self._add_norm(c, delta)
        if p.xp32:
            ops.qkv_rope_linear_xp32(c.x, w, w_s, c.qkv, c.positions, self.cos_sin_cache, kc, vc, md.slot_mapping, nh, nkv, hd,
                                     c.T, **kvs)
        elif p.fuse:
            ops.qkv_rope_linear(c.x, c.xs, w, w_s, c.qkv, c.positions, self.cos_sin_cache, kc, vc, md.slot_mapping, nh, nkv, hd,
                                xp=p.xp, tokens=c.T, **kvs)
        else:
            if p.w4a4:
                ops.rowwise_scaled_linear_cutlass_s4s4_unified(c.x, c.xs, w, w_s, None, c.qkv)
            else:
                ops.w4a16_linear(c.x, w, w_s, c.qkv)   # (every M reads the packed int4 buffer: streaming / M-tiled kernel)
            ops.rope_kv_write(c.positions, c.qkv, self.cos_sin_cache, kc, vc, md.slot_mapping, nh, nkv, hd, **kvs)

    def _attention_o_proj(self, c, layer, kc, vc, kvs):
        """attention -> heads hadamard (+ quant) -> o_proj -> residual + post_attention_layernorm     :231-243,380-387"""
        w, w_s = layer.o_proj.weight, layer.o_proj._scales()
        self._attention_hadamard(c, kc, vc, kvs)
        delta = Delta(f16=c.o)
        if c.p.w4a4:
            ops.rowwise_scaled_linear_cutlass_s4s4_unified(c.x, c.xs, w, w_s, None, c.o)
        elif c.p.xp32:
            ops.w4a16_linear_xp32(c.had, w, w_s, c.o, c.T)
        else:
            delta = self._w4a16_delta(c, c.had, layer.o_proj, c.p.S_o)
        self._add_norm(c, delta)

    def _w4a16_delta(self, c, x, lin, S: int) -> Delta:
        """A verify-pass projection whose output the next norm adds: row-parallel under tensor parallelism, as S K slices
        whose raw sums the norm finishes, or plain."""
        w, w_s, T = lin.weight, lin._scales(), c.T
        if c.p.tp_on:   # this rank's K range: raw fp32 sums, all-reduce in fp32; scale + ONE fp16 rounding + add inside the norm
            k0, k1 = self.tp.k_range(2 * w.shape[1])   # K: two int4 weights per packed byte
            part = c.s.tp_part[:, :T]
            ops.w4a16_linear_ksliced_raw(x, w, part[0], k0, k1)
            self.tp.all_reduce(part)
            return Delta(part=part, w_scale=w_s, slices=1)
        if S:
            part = c.s.k_slices(S, T)
            ops.w4a16_linear_partial(x, w, part, S, xp=c.p.xp, tokens=T)
            return Delta(part=part, w_scale=w_s, slices=S)
        ops.w4a16_linear(x, w, w_s, c.o, xp=c.p.xp, tokens=T)
        return Delta(f16=c.o)

    def _mlp(self, c, layer) -> Delta:
        """gate_up -> silu*up -> online hadamard (+ quant) -> down_proj; returns what the next norm adds     :266-299"""
        p, s, T, I = c.p, c.s, c.T, self.config.intermediate_size
        g_w, g_s = layer.gate_up.weight, layer.gate_up._scales()
        w, w_s = layer.down_proj.weight, layer.down_proj._scales()
        had = (self.had_rem_dim, self.had_K, self.mlp_had_scale)
        if p.xp32:
            ops.gate_up_silu_linear_xp32(c.x, g_w, g_s, c.act, T)
        elif p.tp_on:   # column-parallel gate_up: own channels of [T, I], then all-gather of the channel ranges
            c0, c1 = self.tp.channel_range(I)
            ops.gate_up_silu_linear_shard(c.x, g_w, g_s, c.act, c0, c1 - c0)
            self.tp.all_gather_channels(c.act, I)
        elif p.fuse:
            ops.gate_up_silu_linear(c.x, c.xs, g_w, g_s, c.act, xp=p.xp, tokens=T)
        elif p.w4a4:
            ops.rowwise_scaled_linear_cutlass_s4s4_unified(c.x, c.xs, g_w, g_s, None, c.gu)
        else:
            ops.w4a16_linear(c.x, g_w, g_s, c.gu)
        if p.w4a4:   # (K-sliced down_proj: its activation scales outlive the next norm's, so they get their own buffer)
            xs = s.down_xs[:T] if p.S_down else c.xs
            if p.fuse:
                ops.mlp_hadamard(c.act, *had, q=c.q3, scale=xs)
            else:
                ops.silu_mul_hadamard(c.gu, *had, q=c.q3, scale=xs)
            if p.S_down:   # 17..32 tokens: K slices, int32 sums finished inside the next norm (ops.add_rms_norm_ipartial)
                ipart = s.k_slices(p.S_down, T, int32=True)
                ops.rowwise_scaled_linear_s4s4_partial(c.q3, w, ipart, p.S_down)
                return Delta(ipart=ipart, x_scale=xs, w_scale=w_s, slices=p.S_down)
            ops.rowwise_scaled_linear_cutlass_s4s4_unified(c.q3, xs, w, w_s, None, c.o)
            return Delta(f16=c.o)
        if p.xp or p.S32:
            y = s.xp_had_mlp
            ops.mlp_hadamard(c.act, *had, out_f16=y, xp=True)
        elif p.fuse or p.xp32:
            y = s.mlp_rows(T)
            ops.mlp_hadamard(c.act, *had, out_f16=y)
        else:
            y = c.act
            ops.silu_mul_hadamard(c.gu, *had, out_f16=y)
        if p.S32:
            part = s.k_slices(p.S32, T)
            ops.w4a16_linear_partial_xp32(y, w, part, p.S32, T)
            return Delta(part=part, w_scale=w_s, slices=p.S32)
        return self._w4a16_delta(c, y, layer.down_proj, p.S_mlp)

    def compute_logits(self, hidden_states, scratch: Scratch, shard_vocab: bool = False):
        """LogitsProcessor with a plain nn.Linear lm_head (vllm/model_executor/layers/logits_processor.py:92-97).
        shard_vocab (verify pass under TP): this rank's vocab range + all-gather (logits_processor.py:104-107)."""
        T = hidden_states.shape[0]
        logits = scratch.logits[:T]
        if shard_vocab and self.tp is not None and self.tp.world > 1:
            v0, v1 = self.tp.vocab_range(self.config.vocab_size)
            local = self.tp._buf("vocab.local", (T, v1 - v0), torch.float16, self.device)
            ops.linear_f16(hidden_states, self.lm_head[v0:v1], local)
            return self.tp.all_gather_vocab(local, logits, self.config.vocab_size)
        ops.linear_f16(hidden_states, self.lm_head, logits)
        return logits

    def sample_greedy(self, hidden_states, scratch: Scratch, probs, token, shard_vocab: bool = False, logits_hook=None):
        """compute_logits + Sampler.forward (greedy, modify_greedy_probs = False: sampler.py:216-316): probs [T, V] fp32,
        token [T] (batches with non-greedy rows: QSpecEngine._sample).  At decode-sized T on one GPU the lm_head launch and the softmax are fused (ops.lm_head_softmax_argmax);
        a vocab-parallel lm_head, a large T or a logits hook (bench only) take the two-step path.  Same bits."""
        T = hidden_states.shape[0]
        V, K = self.lm_head.shape
        sharded = shard_vocab and self.tp is not None and self.tp.world > 1
        if not sharded and logits_hook is None and ops.lm_head_softmax_argmax_supported(T, V, K):
            ops.lm_head_softmax_argmax(hidden_states, self.lm_head, scratch.logits[:T], probs, token)
            return
        logits = self.compute_logits(hidden_states, scratch, shard_vocab=shard_vocab)
        if logits_hook is not None:
            logits_hook(logits)
        ops.softmax_argmax(logits, probs, token)

    # ------------------------------------------------------------------ module-wise path (reference op order)
    def forward_modulewise(self, input_ids, positions, kv_caches, attn_metadata: AttentionMetadata, w4a4=False,
                           attn_override=None, kv_scales=None):
        """attn_override (tests): per layer an fp16 [T, q_size] tensor that REPLACES the attention output of that layer
        (teacher forcing of the one stage whose fp32 summation order the hardware fixes)."""
        cfg, md = self.config, attn_metadata
        kw = {"w4a4": w4a4}
        T = input_ids.numel()
        hidden = torch.empty(T, cfg.hidden_size, dtype=torch.float16, device=self.device)
        ops.embedding(input_ids, self.embed_tokens, hidden)
        head_had = quarot_nn.OnlineHadamard(cfg.num_attention_heads, device=self.device)
        mlp_had = quarot_nn.OnlineHadamard(cfg.intermediate_size, device=self.device)
        if self.had_rem_dim is not None:
            mlp_had.had_rem_dim = self.had_rem_dim
        ws = torch.zeros(ops.paged_attention_workspace_bytes(md.q_start.numel() * md.max_q_len, cfg.num_attention_heads,
                                                             cfg.head_dim, md.n_splits), dtype=torch.uint8, device=self.device)
        for li, layer in enumerate(self.layers):
            kc, vc = kv_caches[li]
            kvs = self._kv_kw(li, kc, kv_scales)
            residual = hidden
            x = self.norm(hidden, **kw)
            qkv = layer.qkv_proj(x, **kw)
            q, k, v = qkv.split([cfg.q_size, cfg.kv_size, cfg.kv_size], dim=-1)
            ops.rotary_embedding(positions, q, k, cfg.head_dim, self.cos_sin_cache)
            ops.reshape_and_cache_flash(k.view(T, cfg.num_key_value_heads, cfg.head_dim),
                                        v.view(T, cfg.num_key_value_heads, cfg.head_dim), kc, vc, md.slot_mapping, **kvs)
            attn = torch.empty(T, cfg.q_size, dtype=torch.float16, device=self.device)
            ops.paged_attention(qkv, qkv.shape[1], kc, vc, md.block_tables, md.ctx_lens, md.q_start, T, md.max_q_len,
                                cfg.num_attention_heads, self.sm_scale, md.n_splits, ws, attn, **kvs)
            if attn_override is not None:
                attn.copy_(attn_override[li])
            a = attn.view(-1, cfg.num_attention_heads, cfg.head_dim)
            a = head_had(a.transpose(-1, -2).reshape(-1, cfg.num_attention_heads), **kw)          # :231
            a = a.view(-1, cfg.head_dim, cfg.num_attention_heads).transpose(-1, -2).reshape(T, cfg.hidden_size).contiguous()
            a = self.quantizer(a, **kw)
            hidden = ops_add(residual, layer.o_proj(a, **kw))                                      # :380
            residual = hidden
            x = self.norm(hidden, **kw)
            gu = layer.gate_up(x, **kw)
            g = ops.silu_mul(gu, torch.empty(T, cfg.intermediate_size, dtype=torch.float16, device=self.device))  # :279-284
            g = mlp_had(g, **kw).view(-1, cfg.intermediate_size)
            g = self.quantizer(g, **kw)
            hidden = ops_add(residual, layer.down_proj(g, **kw))                                   # :390
        return self.norm(hidden)


def ops_add(a, b):
    return a + b  # fp16 tensor add: one rounding per element, as in the reference


def make_cos_sin_cache(head_size: int, max_pos: int, base: float) -> torch.Tensor:
    """RotaryEmbedding._compute_cos_sin_cache (vllm/model_executor/layers/rotary_embedding.py), cast to fp16
    as quarot_llama.py:120 does; rope_scaling is ignored there and here."""
    inv_freq = 1.0 / (base ** (torch.arange(0, head_size, 2, dtype=torch.float32) / head_size))
    t = torch.arange(max_pos, dtype=torch.float32)
    freqs = torch.einsum("i,j->ij", t, inv_freq)
    return torch.cat((freqs.cos(), freqs.sin()), dim=-1).to(torch.float16)
