"""Hadamard / quantiser cases for the parity tests: the host-side dispatch of every entry of hadamard.hip (and of the row-absmax
quantiser) restated in Python, float64 references with the kernels' documented rounding points, rows BUILT to put the row
maximum where a kernel could lose it, and a case list that reaches every reachable row -- the Hadamard counterpart of
gemm_cases.py and sampling_cases.py.

Rows (what `route` returns; the names carry the template arguments.  -1 / -2: the entry refuses the shape, -2 is an LDS cap;
"noop": zero tokens, nothing is launched):
  fwht                              fast_hadamard_transform
    fwht.scale_round                   scale_round_kernel                     N = 1
    fwht.lds(TH64|TH128|TH256)         fwht_kernel, min(max(N/2, 64), 256) threads       N = 2^p <= 32768
  hadk_mix                          hadamard_mix
    mix.gen                            hadk_mix_kernel                        1 <= K <= 172
  heads_hadamard                    heads_hadamard(out_f16 | q, scale)
    hh.wide(NH32|NH64,f16|quant)       heads_hadamard_wide_kernel             d = 128
    hh.gen(NH8|16|32|64,f16|quant,TH64|TH128)   heads_hadamard_kernel         even d <= 256; TH128 (d > 128): two waves, the
                                                                              row maximum crosses LDS
  heads_hadamard_mix                heads_hadamard_mix
    hhx.gen                            heads_hadamard_mix_kernel              heads = K 2^p, 2 <= K <= 172, LDS <= 64 KB (-2)
  heads_hadamard_merge              heads_hadamard_merged[_xp]
    hhm.spread32(f16[,xp])             heads_hadamard_merge_spread32_kernel<false>   32 x 128, no quantiser, T <= 128
    hhm.merge(NH32|NH64,f16|quant)     heads_hadamard_merge_kernel            32 | 64 x 128 (NH32,f16 only at T > 128)
    hhm.merge(NH64,f16,xp)             the same kernel, fragment-major tile   T <= 32
    hhm.cols(NH32,f16|quant,TH64|TH128)  heads_hadamard_merge_cols_kernel     32 heads, d % 8 == 0, 8 <= d <= 256, d != 128;
                                                                              min(max(n_splits, 1), 4) splits
  heads_hadamard_merge_spread       heads_hadamard_merged_spread
    hhm.spread32(amax)                 heads_hadamard_merge_spread32_kernel<true>    32 x 128, T <= 128
  heads_hadamard_mix_merge_spread   heads_hadamard_mix_merged_spread[_xp]
    hhx.spread(f16[,xp]|amax)          heads_hadamard_mix_merge_spread_kernel heads = K 2^p <= 64, d = 128, T <= 128; xp T <= 32
  silu_mul_hadamard / mlp_hadamard  silu_mul_hadamard(gate_up) ["gate"], mlp_hadamard[_xp](act, workspace | None) ["preact"]
    smh.spread28(P512,NB8)             silu_mul_hadamard_kernel<8, 28, true, 8>        workspace, T <= 32
    smh.spread28(P1024,NB16)           <16, 28, true, 16>                               workspace, T <= 16
    smh.spread108(P128,NB16|NB8)       <8, 108, true, NB, 128>                          workspace, T <= 16 | 17 <= T <= 32
    smh.one(EPL2|4|8|16|32,KH28|44|12|0,gate|preact)   one workgroup per token; P = 64 EPL; KH0: any other K (K = 1: no mix)
      each smh row runs in the modes q (int4 + scale), f16 and -- preact, T <= 32 -- xp (fragment-major tile)
  rowabsmax_quant                   fuse_sym_quant (norm_quant.hip; the quantiser every form above repeats)
    rq.row(vec8|scalar)                rowabsmax_quant_kernel, K % 8 == 0 | any other even K

Rows no shape reaches (UNREACHABLE): smh.one(EPL32,KH28,*) needs 64 + 4 I + 4 K^2 = 227 KB of LDS (KB = 1024 bytes) for I = 28 x 2048, over
the 160 KB - 64 cap (-2); smh.one(EPL16,KH44,*) 183 KB and smh.one(EPL32,KH44,*) 359 KB likewise; hhm.merge(NH32,f16,xp): the
fragment-major tile stops at 32 tokens, where 32 heads without a quantiser always take hhm.spread32.
`T > QS_XWG_MAX_TOKENS` (256) in smh_spread never decides: T * nb <= 256 with nb >= 8 already stops the spread forms at 32
tokens; T = 256 / 257 are held as cases all the same.

Two data tiers:
  exact      inputs are small integers times a power of two and had_scale is a power of two, so every fp32 partial sum is exact
             in any order, y lands on a grid the table mix sums exactly, and each rounding point rounds an exactly known
             value once.  Bar: fp16 rows, int4 bytes, scales, partial maxima and tiles equal the float64 reference BIT FOR BIT.
             Merge forms: splits with equal maxima (every weight 2^0), sum l a power of two, empty splits (-inf, 0, 0).
  realistic  rand_hidden rows (Gaussian + outlier channels) and had_scale = fp32(1 / sqrt(n)).  Bar: the oracle's bits (this
             family's bar since the first parity tests).  Merge forms with unequal maxima: |out - ref| <= 2e-3 max(1, |ref|max)
             (MERGE_BAR, the bar test_spread_table_factor_head_transform_bit_exact_on_given_partials holds; the hardware 2^x
             is in it).  How far the oracle is from the float64 reference on this tier is MEASURED, not chosen: ORACLE_DIST.

Built rows (exact tier).  The transform is orthogonal with +-1 entries: the preimage of a one-hot output row is a +-1 input
row, its image one spike of A K P had_scale with every other output exactly 0.  Bounded integer noise ({-1, 0, 1} units) on top
leaves the row maximum at the chosen output with a margin of 2 that `build` asserts on the reference.  Token t of a case puts
its maximum into block (t + shift) % nblocks of the row's owners (`owners`: the column blocks of the spread forms' workgroups
and of part_amax, else the waves of the workgroup), alternately on the block's first (low nibble) and last (high nibble)
element, and cycles through pos / neg / ties; a case of six or more tokens ends with tiny / sub / zero rows, one of ten or
more with both / over / tiny / sub / zero
  pos / neg / both     one spike, a negative one, two of opposite sign in different blocks
  ties                 spikes a c with a = 14 (the maximum) and every odd |a| < 14: z / scale = a / 2 = k + 1/2 exactly (clip 1)
  sub                  integer noise scaled down until y = h(wht had_scale) loses bits below 2^-24 and the outputs are fp16 subnormals
  tiny                 nonzero outputs of 2^-24: amax / 7 rounds to a scale of 0, and x / 0 = +-inf clamps to +7 / -8 (the reference
                       kernel's __hdiv and the oracle; only 0 / 0 -> NaN -> 0)
  zero                 an all-zero row: 0 / 0 -> NaN -> 0
  over                 a spike that overflows fp16: reference and kernel must agree on +-inf (fp16 rows, tiles, partial maxima).
                       Such tokens are EXCLUDED from the quantiser's comparison: there the scale is inf and inf / inf = NaN
                       meets the reference kernel's unspecified float -> int conversion.
Quantising modes run at two clip ratios per case, 1.0 and one of 0.9 / 0.5 (a `both` row reaches +7 and -8 below 1).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from gemm_cases import pack_i4, unpack_i4  # noqa: F401  (the oracle-independent int4 packing)

F16, F32, F64 = np.float16, np.float32, np.float64

# ------------------------------------------------------------------ constants of the product build (hadamard.hip)

SMH_LDS_CAP = 160 * 1024 - 64     # silu_mul_hadamard(): -2 above
HHX_LDS_CAP = 64 * 1024           # heads_hadamard_mix(): -2 above
XWG_MAX_TOKENS = 256              # QS_XWG_MAX_TOKENS
MERGE_BAR = 2e-3                  # x max(1, |ref|max): merge forms with unequal maxima

# max |oracle - float64 reference| / max |oracle| per row, realistic tier, largest over the cases of the family; the fraction
# of fp16 values that differ is printed next to it.  Measured (not chosen) by
#   python -m pytest tests/test_hadamard_cases.py -k oracle_distance -s
# The distance is the fp32 rounding of the butterflies (the reference sums in float64) moving an fp16 rounding: <= 1 ulp16 of
# a value at most as large as the row maximum, 2^-10 relative to it, and 2 ulp where the table mix sums such values.
# Measured: fwht 2.085e-04 (0.07 % of the values differ, worst fwht-N32768), hadk_mix 0 (the k-ordered fp32 chain of +-1 x fp16
# is exact here), heads 9.667e-05 (< 0.01 %), mlp 6.317e-04 (0.08 %, worst mlp-had28xH256), rq 0.
# silu: the same distance for g = h(h(silu(gate)) up) (the oracle's fp32 exp against float64): 1.465e-04 of the VALUES differ.
SILU_DIFF = 1.5e-4
ORACLE_DIST = {"fwht": 2.1e-4, "hadk_mix": 0.0, "heads": 9.7e-5, "mlp": 6.4e-4, "rq": 0.0}


def is_pow2(n: int) -> bool:
    return n >= 1 and (n & (n - 1)) == 0


# ------------------------------------------------------------------ route: the host dispatch, restated

def smh_spread(T, P, K, preact, ws) -> int:
    """hadamard.hip smh_spread(): workgroups per token."""
    if not ws or not preact or T > XWG_MAX_TOKENS:
        return 1
    nb = 1
    if K == 28:
        nb = 8 if P == 512 else (16 if P == 1024 else 1)
    if K == 108 and P == 128:
        nb = 8 if T * 16 > 256 else 16
    return nb if T * nb <= 256 else 1


def smh_lds(I, K) -> int:
    return 64 + I * 2 * (2 if K > 1 else 1) + (K * K * 4 if K > 1 else 0)


def mlp_xp_supported(T, I, K) -> bool:
    """hadamard.hip mlp_hadamard_xperm_supported() (qspec_mlp_hadamard_act_layout_supported)."""
    if T < 1 or T > 32 or K < 1 or K > 172 or I % K:
        return False
    P = I // K
    if not is_pow2(P) or smh_lds(I, K) > SMH_LDS_CAP:
        return False
    if smh_spread(T, P, K, True, True) > 1:
        return True
    return T > 16 and P in (128, 256, 512, 1024, 2048) and I % 128 == 0


def heads_merge_spread_supported(T, heads, d) -> bool:
    return T >= 0 and T * 8 <= 1024 and heads == 32 and d == 128


def heads_mix_merge_spread_supported(T, heads, d, K) -> bool:
    if d != 128 or K < 2 or K > 172 or heads % K or heads * 16 > 1024 or T < 0 or T * 8 > 1024:
        return False
    return is_pow2(heads // K)


def generic_splits(n_splits) -> int:
    return 1 if n_splits < 1 else min(n_splits, 4)


def _smh(T, I, K, preact, ws, quant, xp):
    if K < 1 or K > 172 or I % K or I % 8:
        return -1
    P = I // K
    if not is_pow2(P):
        return -1
    if smh_lds(I, K) > SMH_LDS_CAP:
        return -2
    if xp and (quant or T > 32 or not preact):
        return -1
    nb = smh_spread(T, P, K, preact, ws)
    if nb > 1:
        return f"smh.spread{K}(P{P},NB{nb})"
    if P not in (128, 256, 512, 1024, 2048):
        return -1
    return f"smh.one(EPL{P // 64},KH{K if K in (28, 44, 12) else 0},{'preact' if preact else 'gate'})"


def route(entry: str, **a):
    """The row an entry takes at a shape, or its error code.  Keyword arguments per entry:
    fwht(rows, N)   hadk_mix(T, K, M)   heads_hadamard(T, heads, d, quant)   heads_hadamard_mix(T, heads, d, K)
    heads_hadamard_merge(T, heads, d, S, quant, xp=False, max_tokens=T)   heads_hadamard_merge_spread(T, heads, d, S, max_tokens=T)
    heads_hadamard_mix_merge_spread(T, heads, d, K, S, amax, xp=False, max_tokens=T)
    silu_mul_hadamard(T, I, K, quant)   mlp_hadamard(T, I, K, ws, quant, xp=False)   rowabsmax_quant(T, K)"""
    T = a.get("T", a.get("rows"))
    if T < 0:
        return -1
    if T == 0:
        return "noop"
    if entry == "fwht":
        N = a["N"]
        if N == 1:
            return "fwht.scale_round"
        if N < 2 or N > 32768 or not is_pow2(N):
            return -1
        return f"fwht.lds(TH{min(max(N // 2, 64), 256)})"
    if entry == "hadk_mix":
        return "mix.gen" if 1 <= a["K"] <= 172 else -1
    if entry == "heads_hadamard":
        heads, d, qn = a["heads"], a["d"], "quant" if a["quant"] else "f16"
        if d % 2 or d // 2 > 128 or d < 2:
            return -1
        if d == 128 and heads in (32, 64):
            return f"hh.wide(NH{heads},{qn})"
        if heads in (8, 16, 32, 64):
            return f"hh.gen(NH{heads},{qn},TH{64 if d <= 128 else 128})"
        return -1
    if entry == "heads_hadamard_mix":
        heads, d, K = a["heads"], a["d"], a["K"]
        if K < 2 or K > 172 or heads % K or not is_pow2(heads // K):
            return -1
        return "hhx.gen" if (heads * d + K * K) * 4 <= HHX_LDS_CAP else -2
    if entry == "heads_hadamard_merge":
        heads, d, S, quant, xp = a["heads"], a["d"], a["S"], a["quant"], a.get("xp", False)
        qn = "quant" if quant else "f16"
        if not ((d == 128 and heads in (32, 64)) or (heads == 32 and d % 8 == 0 and 8 <= d <= 256)):
            return -1
        if xp and (quant or heads not in (32, 64) or T > 32 or d != 128):
            return -1
        if S < 1 or T > a.get("max_tokens", T):
            return -1
        if d != 128:
            return f"hhm.cols(NH32,{qn},TH{64 if d <= 128 else 128})"
        if not quant and heads == 32 and T * 8 <= 1024:
            return "hhm.spread32(f16,xp)" if xp else "hhm.spread32(f16)"
        if xp and heads != 64:
            return -1
        return f"hhm.merge(NH{heads},{qn}{',xp' if xp else ''})"
    if entry == "heads_hadamard_merge_spread":
        if not heads_merge_spread_supported(T, a["heads"], a["d"]) or a["S"] < 1 or T > a.get("max_tokens", T):
            return -1
        return "hhm.spread32(amax)"
    if entry == "heads_hadamard_mix_merge_spread":
        xp, amax = a.get("xp", False), a["amax"]
        if not heads_mix_merge_spread_supported(T, a["heads"], a["d"], a["K"]) or (xp and (amax or T > 32)):
            return -1
        if a["S"] < 1 or T > a.get("max_tokens", T):
            return -1
        return "hhx.spread(amax)" if amax else ("hhx.spread(f16,xp)" if xp else "hhx.spread(f16)")
    if entry == "silu_mul_hadamard":
        return _smh(T, a["I"], a["K"], False, False, a["quant"], False)
    if entry == "mlp_hadamard":
        return _smh(T, a["I"], a["K"], True, a["ws"], a["quant"], a.get("xp", False))
    if entry == "rowabsmax_quant":
        K = a["K"]
        if K <= 0 or K % 2:
            return -1
        return "rq.row(vec8)" if K % 8 == 0 else "rq.row(scalar)"
    raise KeyError(entry)


def _all_rows():
    rows = ["fwht.scale_round", "fwht.lds(TH64)", "fwht.lds(TH128)", "fwht.lds(TH256)", "mix.gen", "hhx.gen"]
    for qn in ("f16", "quant"):
        rows += [f"hh.wide(NH{n},{qn})" for n in (32, 64)]
        rows += [f"hh.gen(NH{n},{qn},TH{th})" for n in (8, 16, 32, 64) for th in (64, 128)]
        rows += [f"hhm.merge(NH{n},{qn})" for n in (32, 64)]
        rows += [f"hhm.cols(NH32,{qn},TH{th})" for th in (64, 128)]
    rows += ["hhm.merge(NH32,f16,xp)", "hhm.merge(NH64,f16,xp)", "hhm.spread32(f16)", "hhm.spread32(f16,xp)", "hhm.spread32(amax)",
             "hhx.spread(f16)", "hhx.spread(f16,xp)", "hhx.spread(amax)",
             "smh.spread28(P512,NB8)", "smh.spread28(P1024,NB16)", "smh.spread108(P128,NB16)", "smh.spread108(P128,NB8)"]
    rows += [f"smh.one(EPL{e},KH{k},{p})" for e in (2, 4, 8, 16, 32) for k in (28, 44, 12, 0) for p in ("gate", "preact")]
    rows += ["rq.row(vec8)", "rq.row(scalar)"]
    return rows


ALL_ROWS = _all_rows()
UNREACHABLE = {f"smh.one(EPL{e},KH{k},{p})": f"had{k} x H{64 * e} needs {smh_lds(64 * e * k, k) // 1024} KB of LDS, over the 160 KB cap (-2)"
               for e, k in ((32, 28), (16, 44), (32, 44)) for p in ("gate", "preact")}
UNREACHABLE["hhm.merge(NH32,f16,xp)"] = "the tile stops at 32 tokens, where 32 heads without a quantiser take hhm.spread32"


# ------------------------------------------------------------------ float64 references

def h(x):
    """The kernels' f2h of an fp32 value: float64 -> fp32 -> fp16, both round-to-nearest-even."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, F64).astype(F32).astype(F16)


def sylvester_row(j: int, P: int) -> np.ndarray:
    p = np.arange(P)
    v = j & p
    par = np.zeros(P, np.int64)
    while v.any():
        par ^= v & 1
        v = v >> 1
    return 1 - 2 * par


def wht(x):
    """Unnormalised Sylvester-order Walsh-Hadamard transform of the last axis, float64."""
    x = np.array(x, F64)
    shp, n = x.shape, x.shape[-1]
    s = 1
    with np.errstate(invalid="ignore"):
        while s < n:
            y = x.reshape(shp[:-1] + (n // (2 * s), 2, s))
            x = np.stack([y[..., 0, :] + y[..., 1, :], y[..., 0, :] - y[..., 1, :]], axis=-2).reshape(shp)
            s *= 2
    return x


def _sequency_perm(n: int) -> np.ndarray:
    """Sylvester index of the row with i sign changes (bit-reversed Gray code)."""
    bits = n.bit_length() - 1
    out = np.empty(n, np.int64)
    for i in range(n):
        g = i ^ (i >> 1)
        out[i] = int(format(g, f"0{bits}b")[::-1], 2) if bits else 0
    return out


def table(K: int) -> Optional[np.ndarray]:
    """The +-1 table get_hadK uses for a factor K (None for K = 1)."""
    if K == 1:
        return None
    from qspec_amd import hadamard_tables
    H = np.array(hadamard_tables.hadamard_matrix(K), F64)
    return np.roll(H, 1, axis=0) if is_pow2(K) else H     # (a Sylvester table is symmetric: its rows rotated, it no longer is)


def pow2_scale(n: int) -> float:
    """The power of two next to 1 / sqrt(n): the exact tier's had_scale."""
    return 2.0 ** -math.ceil(math.log2(n) / 2)


def rsqrt_scale(n: int) -> float:
    return float(F32(1.0) / np.sqrt(F32(n)))


def ref_silu_mul(gate_up, I):
    """g = h(h(silu(gate)) up); gate_up [T, 2I], up first."""
    up, gate = gate_up[:, :I].astype(F64), gate_up[:, I:].astype(F64)
    with np.errstate(over="ignore"):
        a = h(gate / (1.0 + np.exp(-gate))).astype(F64)
    return h(a * up)


def ref_transform(g, had, K, scale, fault=None):
    """g [.., K P] fp16 -> z = h(sum_k hadK[i, k] y[k, j]), y = h(f32(WHT_P(g)) had_scale); z = y for K = 1."""
    g = np.asarray(g)
    lead, n = g.shape[:-1], g.shape[-1]
    P = n // K
    w = wht(g.astype(F64).reshape(lead + (K, P)))
    if fault == "sequency_order":
        w = w[..., _sequency_perm(P)]
    s32 = F32(1.0) if fault == "scale_after_mix" and K > 1 else F32(scale)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (w.astype(F32) * s32).astype(F16)
        if K == 1:
            return y.reshape(lead + (n,))
        hk = had.T if fault == "table_transposed" else had
        z = np.einsum("ik,...kj->...ij", hk, y.astype(F64))
        if fault == "scale_after_mix":
            z = (z.astype(F32) * F32(scale)).astype(F64)
        return h(z).reshape(lead + (n,))


def ref_heads(attn, heads, had, K, scale, fault=None):
    """attn [T, heads d] -> the same transform over the head axis of every column."""
    T = attn.shape[0]
    d = attn.shape[1] // heads
    xt = np.ascontiguousarray(attn.reshape(T, heads, d).transpose(0, 2, 1))
    yt = ref_transform(xt, had, K, scale, fault)
    return np.ascontiguousarray(yt.transpose(0, 2, 1)).reshape(T, heads * d)


def ref_merge(o, m, l, fault=None):
    """out = h(sum_s 2^((m_s - M) log2 e) o_s / sum_s 2^(..) l_s); o [T, H, S, d], m, l [T, H, S]; empty splits weigh 0."""
    o, m, l = np.asarray(o, F64), np.asarray(m, F64), np.asarray(l, F64)
    T, H, S, d = o.shape
    if fault == "wrong_split_stride":       # the partials read as [T, S, H, d]
        o = o.reshape(T, S, H, d).transpose(0, 2, 1, 3)
    M = m.max(axis=2, keepdims=True)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isneginf(m), 0.0, np.exp2((m - M) * math.log2(math.e)))
    num, den = (w[..., None] * o).sum(axis=2), (w * l).sum(axis=2)
    return h(num / den[..., None]).reshape(T, H * d)


def block_max(z, block_of, nb, positive_only=False):
    """max |z| per owner block: [T, nb] float64 (0 for an empty block)."""
    a = z.astype(F64)
    a = np.maximum(a, 0.0) if positive_only else np.abs(a)
    out = np.zeros((z.shape[0], nb))
    for b in range(nb):
        sel = block_of == b
        if sel.any():
            out[:, b] = a[:, sel].max(axis=1)
    return out


def ref_quant(z, clip, block_of=None, nb=1, fault=None, block=0):
    """scale = h(h(amax / 7) h(clip)); q = clamp(rn_even(h(z / scale)), -8, 7), low nibble first.  -> (q [T, n/2] int8, scale)."""
    z = np.asarray(z)
    T, n = z.shape
    if block_of is None:
        block_of, nb = np.zeros(n, np.int64), 1
    pm = block_max(z, block_of, nb, positive_only=fault == "amax_positive_only")
    if fault == "amax_drops_a_block":
        pm[:, block] = 0.0
    elif fault == "stale_block_maximum":      # block `block` still holds the previous token's maximum
        pm[:, block] = np.concatenate([[0.0], pm[:-1, block]])
    amax = pm.max(axis=1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s1 = (amax.astype(F32) / F32(7.0)).astype(F16)
        sc = (s1.astype(F32) * F32(F16(clip))).astype(F16)
        qf = (z.astype(F32) / sc.astype(F32)[:, None]).astype(F16).astype(F64)
    qf = np.where(np.isnan(qf), 0.0, qf)
    r = np.sign(qf) * np.floor(np.abs(qf) + 0.5) if fault == "round_half_away" else np.rint(qf)
    q = np.clip(r, -7 if fault == "clamp_minus_7" else -8, 7).astype(np.int64)
    lo, hi = (q[:, 1::2], q[:, 0::2]) if fault == "nibbles_swapped" else (q[:, 0::2], q[:, 1::2])
    return ((lo & 0xF) | ((hi & 0xF) << 4)).astype(np.uint8).view(np.int8), sc


def xp_offsets(T: int, K: int) -> np.ndarray:
    """common.cuh w4a16_xperm_offset(r, k, K): where element (r, k) sits in the fragment-major tile(s).  [T, K] int64."""
    r, k = np.arange(T)[:, None], np.arange(K)[None, :]
    rem, e = k & 127, k & 7
    pos = ((e & 3) << 1) | (e >> 2)
    one = ((((k >> 7) * 4 + ((rem >> 3) & 3)) * 64 + (rem >> 5) * 16 + (r & 15)) << 3) + pos
    return (r >> 4) * 16 * K + one


def xp_tile(z, fill) -> np.ndarray:
    """The tile buffer (16 or 32 rows) holding z [T, K]; rows no token owns keep `fill`."""
    T, K = z.shape
    out = np.full((16 if T <= 16 else 32) * K, fill, F16)
    out[xp_offsets(T, K).reshape(-1)] = z.reshape(-1)
    return out


FAULTS = ("amax_drops_a_block", "amax_positive_only", "clamp_minus_7", "round_half_away", "nibbles_swapped",
          "table_transposed", "scale_after_mix", "sequency_order", "wrong_split_stride", "stale_block_maximum")
QUANT_FAULTS = ("amax_drops_a_block", "amax_positive_only", "clamp_minus_7", "round_half_away", "nibbles_swapped",
                "stale_block_maximum")


# ------------------------------------------------------------------ owners of the row maximum

def owners(row: str, n: int, d: int = 0, P: int = 0) -> Tuple[np.ndarray, int]:
    """block_of [n], nblocks: which workgroup (spread forms, part_amax) or wave (the rest) reduces output element e."""
    e = np.arange(n)
    if row.startswith("smh.spread"):
        nb = int(row[row.index("NB") + 2:-1])
        return (e % P) // (P // nb), nb
    if row.startswith("smh.one"):
        return ((e // 8) % 1024) // 64, 16
    if row.startswith("hh.wide") or row.startswith("hhm.merge"):
        return (e // d) // 8, n // d // 8
    if row.startswith("hh.gen") or row.startswith("hhm.cols"):
        return ((e % d) // 2) // 64, 2 if d > 128 else 1
    if row.startswith("hhm.spread32") or row.startswith("hhx.spread"):
        return (e % d) // 16, 8
    if row.startswith("rq.row"):
        return (((e // 8) % 256) // 64, 4) if n % 8 == 0 else (((e // 2) % 256) // 64, 4)
    return np.zeros(n, np.int64), 1


# ------------------------------------------------------------------ cases

KINDS = ("pos", "neg", "ties")      # one maximum in one block, in rotation
TAIL = ("both", "over", "tiny", "sub", "zero")   # the last tokens of a case: all five from 10 tokens on, tiny / sub / zero from 6
A_SPIKE, UNIT = 4, 2.0 ** -4


@dataclass
class Case:
    name: str
    entry: str                      # fwht | hadk_mix | heads_hadamard | heads_hadamard_mix | heads_hadamard_merge | ..._spread | mlp | rq
    tier: str                       # exact | realistic
    T: int
    dims: Dict[str, int]            # the rest of the shape: N | K, M | heads, d[, K][, S] | I, K | K
    modes: Tuple[str, ...]          # f16, q, xp, amax
    ws: bool = False                # mlp: an exchange workspace is passed (the spread forms)
    gate: bool = False              # mlp: also through silu_mul_hadamard(gate_up)
    clip2: float = 0.9              # the second clip ratio of the quantising modes
    shift: int = 0
    nsplits_arg: Optional[int] = None   # heads_hadamard_merge, d != 128: the n_splits the caller passes (clamped to 4)
    kinds: Optional[Tuple[str, ...]] = None   # exact tier: the kind of every token, where the rotation is not wanted
    seed: int = 0

    @property
    def id(self):
        return f"{self.name}-{self.tier}"

    def routes(self) -> List[Tuple[str, str, object]]:
        """(entry point, mode, row) of every launch the GPU test makes for this case."""
        d, T, out = self.dims, self.T, []
        for mode in self.modes:
            quant, xp, amax = mode == "q", mode == "xp", mode == "amax"
            if self.entry == "fwht":
                out.append(("fwht", mode, route("fwht", rows=T, N=d["N"])))
            elif self.entry == "hadk_mix":
                out.append(("hadk_mix", mode, route("hadk_mix", T=T, K=d["K"], M=d["M"])))
            elif self.entry == "heads_hadamard":
                out.append((self.entry, mode, route(self.entry, T=T, heads=d["heads"], d=d["d"], quant=quant)))
            elif self.entry == "heads_hadamard_mix":
                out.append((self.entry, mode, route(self.entry, T=T, heads=d["heads"], d=d["d"], K=d["K"])))
            elif self.entry == "heads_hadamard_merge":
                S = d["S"] if self.nsplits_arg is None else self.nsplits_arg
                out.append((self.entry, mode, route(self.entry, T=T, heads=d["heads"], d=d["d"], S=S, quant=quant, xp=xp)))
            elif self.entry == "heads_hadamard_merge_spread":
                out.append((self.entry, mode, route(self.entry, T=T, heads=d["heads"], d=d["d"], S=d["S"])))
            elif self.entry == "heads_hadamard_mix_merge_spread":
                out.append((self.entry, mode, route(self.entry, T=T, heads=d["heads"], d=d["d"], K=d["K"], S=d["S"], amax=amax, xp=xp)))
            elif self.entry == "mlp":
                out.append(("mlp_hadamard", mode, route("mlp_hadamard", T=T, I=d["I"], K=d["K"], ws=self.ws, quant=quant, xp=xp)))
                if self.gate and not xp:
                    out.append(("silu_mul_hadamard", mode, route("silu_mul_hadamard", T=T, I=d["I"], K=d["K"], quant=quant)))
            elif self.entry == "rq":
                out.append(("rowabsmax_quant", mode, route("rowabsmax_quant", T=T, K=d["K"])))
        return out

    def geometry(self):
        """(n, K, P, heads, d): the output row of n elements; the transform is hadK (x) H_P over the heads (d > 0) or the row."""
        dm = self.dims
        if self.entry == "fwht":
            return dm["N"], 1, dm["N"], 0, 0
        if self.entry == "hadk_mix":
            return dm["K"] * dm["M"], dm["K"], 1, 0, 0
        if self.entry == "mlp":
            return dm["I"], dm["K"], dm["I"] // dm["K"], 0, 0
        if self.entry == "rq":
            return dm["K"], 1, 1, 0, 0
        K = dm.get("K", 1)
        return dm["heads"] * dm["d"], K, dm["heads"] // K, dm["heads"], dm["d"]

    def owners(self, row=None):
        n, K, P, heads, d = self.geometry()
        if row is None:   # the geometry of the quantising / amax row when there is one
            rs = {m: r for _, m, r in self.routes()}
            row = rs.get("q", rs.get("amax", next(iter(rs.values()))))
        return owners(row, n, d, P)


@dataclass
class Data:
    x: np.ndarray                   # the input rows fp16: [T, n] (mlp: act; heads: [T, heads d], merge forms: the merged rows)
    scale: float                    # had_scale
    had: Optional[np.ndarray]       # the table, float64 (None: K = 1)
    kinds: List[str] = field(default_factory=list)
    spikes: List[List[Tuple[int, int]]] = field(default_factory=list)   # per token: (output element, a) of every spike
    gate_up: Optional[np.ndarray] = None
    o: Optional[np.ndarray] = None  # merge forms: partials
    m: Optional[np.ndarray] = None
    l: Optional[np.ndarray] = None


def rand_hidden(rng, T, H, scale=1.0):
    x = rng.standard_normal((T, H)) * scale
    x[:, rng.integers(0, H, 8)] *= 20.0
    return x.astype(F16)


def _had_scale(c: Case) -> float:
    n, K, P, heads, d = c.geometry()
    if c.entry in ("hadk_mix", "rq"):
        return 1.0
    m = heads if heads else n
    return pow2_scale(m) if c.tier == "exact" else rsqrt_scale(m)


def _preimage(c: Case, e: int, had) -> np.ndarray:
    """The +-1 input row (length n) whose transform is one spike at output element e."""
    n, K, P, heads, d = c.geometry()
    if c.entry == "rq":
        v = np.zeros(n, np.int64)
        v[e] = 1
        return v
    if c.entry == "hadk_mix":
        i, j = divmod(e, c.dims["M"])
        v = np.zeros((K, c.dims["M"]), np.int64)
        v[:, j] = had[i].astype(np.int64) if had is not None else 1
        return v.reshape(-1)
    if heads:
        hd, col = divmod(e, d)
        i, j = divmod(hd, P)
        w = np.kron(had[i] if had is not None else np.ones(1), sylvester_row(j, P)).astype(np.int64)
        v = np.zeros((heads, d), np.int64)
        v[:, col] = w
        return v.reshape(-1)
    i, j = divmod(e, P)
    return np.kron(had[i] if had is not None else np.ones(1), sylvester_row(j, P)).astype(np.int64)


def _peak_unit(c: Case) -> int:
    """K P, the factor one unit of spike gains (1 for the entries without a transform of their own)."""
    n, K, P, heads, d = c.geometry()
    return {"rq": 1, "hadk_mix": K}.get(c.entry, K * P)


def _exact_rows(c: Case, rng, had) -> Data:
    n, K, P, heads, d = c.geometry()
    block_of, nb = c.owners()
    members = [np.flatnonzero(block_of == b) for b in range(nb)]
    live = [b for b in range(nb) if len(members[b])]
    scale = _had_scale(c)
    x = np.zeros((c.T, n), F64)
    kinds, spikes = [], []
    for t in range(c.T):
        kind = KINDS[(t + c.shift) % len(KINDS)]
        tail = TAIL if c.T >= 10 else (TAIL[2:] if c.T >= 6 else ())
        if t >= c.T - len(tail):
            kind = tail[t - (c.T - len(tail))]
        if c.kinds is not None:
            kind = c.kinds[t]
        unit = UNIT
        if kind == "over":    # the spike alone passes 65504 (twice over); y = h(wht scale) = z / K stays finite
            unit = 2.0 ** math.ceil(math.log2(65504.0 * 2 / (A_SPIKE * _peak_unit(c) * scale)))
            if c.entry == "rq" or K in (2, 3) or (A_SPIKE + 1) * unit > 60000.0:
                kind, unit = "pos", UNIT
        if n < 16 and kind in ("both", "ties"):
            kind = "neg"
        k = t + c.shift
        b = live[k % len(live)]
        last = (k // len(live) + k) % 2 == 1
        e = int(members[b][-1] if last else members[b][0])
        b2 = live[(live.index(b) + max(1, len(live) // 2)) % len(live)]
        e2 = int(members[b2][0] if last else members[b2][-1])
        if e2 == e:
            e2 = (e + n // 2 + 1) % n
        noise = rng.integers(-1, 2, n).astype(F64)
        if kind == "zero":
            sp, row = [], np.zeros(n)
        elif kind == "tiny":  # one input of 2^-24 / had_scale: every nonzero output is +-2^-24 (rq: 3 x 2^-24), so h(amax / 7) = 0
            sp, row = [], np.zeros(n)
            row[e] = 3.0 if c.entry == "rq" else 1.0
            unit = 2.0 ** -24 / scale
        elif kind == "sub":   # noise alone, scaled until y = h(wht unit scale) loses bits below 2^-24; inputs stay fp16 subnormals
            sp, row = [], rng.integers(-3, 4, n).astype(F64)
            unit = max(2.0 ** -25 / scale, 2.0 ** -20 if c.gate else 2.0 ** -24)
        elif kind == "ties":
            others = [a for k2 in range(1, 14, 2) for a in (k2, -k2)]
            pos = [e] + [int(p) for p in rng.choice(np.setdiff1d(np.arange(n), [e]), min(len(others), n - 1), replace=False)]
            sp = list(zip(pos, [14] + others))
            row = sum(a * _preimage(c, p, had).astype(F64) for p, a in sp) * A_SPIKE
        else:
            sp = [(e, -A_SPIKE)] if kind == "neg" else ([(e, A_SPIKE), (e2, -A_SPIKE)] if kind == "both" else [(e, A_SPIKE)])
            row = sum(a * _preimage(c, p, had).astype(F64) for p, a in sp) + noise
        x[t] = row * unit
        kinds.append(kind)
        spikes.append(sp)
    x16 = x.astype(F16)
    assert np.array_equal(x16.astype(F64), x), c.id      # the inputs are fp16 values
    return Data(x16, scale, had, kinds, spikes)


def _merge_partials(c: Case, rng, merged, exact: bool):
    """Partials (o, m, l) [T, H, S, ..] of the merged rows.  exact: equal maxima, sum l = 2^j, some splits empty -- the merge
    then returns `merged` bit for bit.  Otherwise random partials (merged is ignored)."""
    T, H, d, S = c.T, c.dims["heads"], c.dims["d"], c.dims["S"]
    if not exact:
        o = rng.standard_normal((T, H, S, d)) * 2.0
        m = rng.standard_normal((T, H, S)) * 3.0
        l = rng.random((T, H, S)) * 5.0 + 0.5
        if S > 1:
            m[0, 0, 1], o[0, 0, 1], l[0, 0, 1] = -np.inf, 0.0, 0.0
        return o.astype(F32), m.astype(F32), l.astype(F32)
    a = merged.astype(F64).reshape(T, H, d)
    o, m, l = np.zeros((T, H, S, d)), np.full((T, H, S), -np.inf), np.zeros((T, H, S))
    mval = rng.integers(-8, 9, (T, H)) * 0.25
    for t in range(T):
        for hd in range(H):
            live = np.flatnonzero(rng.random(S) < 0.7)
            if len(live) == 0:
                live = np.array([rng.integers(0, S)])
            lv = [1.0] + [2.0 ** max(0, i - 1) for i in range(1, len(live))]     # 1, 1, 2, 4, ..: the sum is a power of two
            rest = 0
            for i, s in enumerate(live):      # o_s = a (l_s + k_s) with sum k_s = 0: the numerator is a sum l exactly
                ks = int(rng.integers(-2, 3)) if i + 1 < len(live) else -rest
                rest += ks
                o[t, hd, s] = a[t, hd] * (lv[i] + ks)
                m[t, hd, s], l[t, hd, s] = mval[t, hd], lv[i]
    o32 = o.astype(F32)
    assert np.array_equal(o32.astype(F64), o)
    return o32, m.astype(F32), l.astype(F32)


def build(c: Case) -> Data:
    """The inputs of a case; exact tier: the built rows, with the placement asserted on the reference."""
    rng = np.random.default_rng(c.seed)
    n, K, P, heads, d = c.geometry()
    had = table(K) if c.entry != "fwht" and K > 1 else None
    merge = c.entry.startswith("heads_hadamard_m") and c.entry != "heads_hadamard_mix"
    if c.tier == "exact":
        dt = _exact_rows(c, rng, had)
        if c.gate:      # h(silu(16)) = 16 in fp16, so g = h(16 up) = act for up = act / 16
            up = (dt.x.astype(F64) / 16.0).astype(F16)
            assert np.array_equal(up.astype(F64) * 16.0, dt.x.astype(F64)), c.id
            dt.gate_up = np.concatenate([up, np.full_like(up, 16.0)], axis=1)
    else:
        sc = _had_scale(c)
        if c.entry == "mlp" and c.gate:
            gu = rand_hidden(rng, c.T, 2 * n, 2.0)
            dt = Data(ref_silu_mul(gu, n), sc, had, gate_up=gu)
        elif c.entry == "mlp":
            dt = Data(rand_hidden(rng, c.T, n, 1.0), sc, had)
        elif c.entry == "hadk_mix":
            dt = Data(rng.standard_normal((c.T, n)).astype(F16), sc, had)
        else:
            dt = Data(rand_hidden(rng, c.T, n, 0.5 if heads else 1.0), sc, had)
    if merge:
        dt.o, dt.m, dt.l = _merge_partials(c, rng, dt.x, c.tier == "exact")
        if c.tier == "exact":
            assert np.array_equal(ref_merge(dt.o, dt.m, dt.l).view(np.uint16), dt.x.view(np.uint16)), c.id
        else:
            dt.x = ref_merge(dt.o, dt.m, dt.l)
    if c.tier == "exact":
        check_built(c, dt, ref_rows(c, dt))
    return dt


def ref_rows(c: Case, dt: Data, fault=None) -> np.ndarray:
    """The fp16 output rows [T, n] of the case's transform, float64 reference."""
    n, K, P, heads, d = c.geometry()
    x = dt.x
    if fault == "wrong_split_stride" and dt.o is not None:
        x = ref_merge(dt.o, dt.m, dt.l, fault)
    if c.entry == "rq":
        return x
    if c.entry == "hadk_mix":
        M = c.dims["M"]
        hk = dt.had if dt.had is not None else np.ones((1, 1))
        hk = hk.T if fault == "table_transposed" else hk
        return h(np.einsum("ik,tkj->tij", hk, x.astype(F64).reshape(c.T, K, M))).reshape(c.T, n)
    if heads:
        return ref_heads(x, heads, dt.had, K, dt.scale, fault)
    return ref_transform(x, dt.had, K, dt.scale, fault)


def oracle_rows(oracle, c: Case, dt: Data) -> np.ndarray:
    """The fp16 output rows of the case as the CPU oracle (the `oracle` package, passed in) computes them."""
    n, K, P, heads, d = c.geometry()
    had16 = dt.had.astype(F16) if dt.had is not None else None
    if c.entry == "rq":
        return dt.x
    if c.entry == "fwht":
        return oracle.fwht(dt.x, dt.scale)
    if c.entry == "hadk_mix":
        hk = had16 if had16 is not None else np.ones((1, 1), F16)
        return oracle.hadk_mix(dt.x.reshape(c.T, K, c.dims["M"]), hk).reshape(c.T, n)
    if heads:
        return oracle.heads_hadamard(dt.x, heads, dt.scale, had16, K)
    return oracle.mlp_hadamard(dt.x, had16, K, dt.scale)


def check_built(c: Case, dt: Data, z: np.ndarray) -> None:
    """Every built row has the property it was built for, on the reference."""
    block_of, nb = c.owners()
    zz = z.astype(F64)
    peak_unit = _peak_unit(c) * dt.scale
    for t, (kind, sp) in enumerate(zip(dt.kinds, dt.spikes)):
        row = zz[t]
        if kind == "zero":
            assert not row.any(), (c.id, t)
        elif kind == "tiny":
            assert 0 < np.abs(row).max() <= 3 * 2.0 ** -24, (c.id, t)
            q, s = ref_quant(z[t:t + 1], 1.0)
            assert float(s[0]) == 0.0 and set(np.unique(unpack_i4(q))) <= {-8, 0, 7} and unpack_i4(q).any(), (c.id, t)
        elif kind == "sub":
            assert row.any() and (np.abs(row) < 2.0 ** -14).mean() > 0.9, (c.id, t)
        elif kind == "over":
            e = sp[0][0]
            assert np.isposinf(row[e]) and np.isfinite(np.delete(row, e)).all(), (c.id, t)
        elif kind == "ties":
            cc = A_SPIKE * UNIT * peak_unit
            assert all(row[e] == a * cc for e, a in sp) and np.count_nonzero(row) == len(sp), (c.id, t)
            _, s = ref_quant(z[t:t + 1], 1.0)
            assert float(s[0]) == 2 * cc, (c.id, t)
            assert all((row[e] / float(s[0]) * 2) % 2 == 1 for e, a in sp[1:]), (c.id, t)     # k + 1/2
        else:
            where = [e for e, a in sp]
            top = np.abs(row).max()
            rest = np.abs(np.delete(row, where)).max() if len(where) < len(row) else 0.0
            assert max(abs(row[e]) for e in where) == top and rest * 2 <= top, (c.id, t, kind, top, rest)
            if kind == "neg":
                assert row[where[0]] < 0 and row.max() * 2 <= top, (c.id, t)
            if kind == "both":    # the two spikes differ by the noise at most, on opposite sides, in different blocks
                assert row[where[0]] > 0 > row[where[1]] and abs(row[where[0]] + row[where[1]]) <= 2 * rest, (c.id, t)
                assert len(np.unique(block_of)) == 1 or block_of[where[0]] != block_of[where[1]], (c.id, t)


def _mk(name, entry, T, modes, tiers=("exact", "realistic"), **kw) -> List[Case]:
    dims = {k: kw.pop(k) for k in list(kw) if k in ("N", "K", "M", "heads", "d", "S", "I")}
    out = []
    for tier in tiers:
        seed = (sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 2 + (tier == "exact")) % (2 ** 31)
        out.append(Case(name, entry, tier, T, dims, tuple(modes), seed=seed, **kw))
    return out


def cases() -> List[Case]:
    cs: List[Case] = []
    # ---- fwht / hadk_mix (no quantiser: wiring, scale placement, overflow and subnormal rounding)
    for N, rows in ((1, 3), (2, 5), (128, 12), (256, 12), (512, 12), (4096, 12), (32768, 2)):
        cs += _mk(f"fwht-N{N}-r{rows}", "fwht", rows, ("f16",), N=N)
    for K, M, T in ((12, 64, 12), (28, 512, 3), (108, 128, 2), (140, 6, 2), (1, 5, 2), (40, 300, 2)):
        cs += _mk(f"mix-K{K}-M{M}", "hadk_mix", T, ("f16",), K=K, M=M)
    # ---- heads_hadamard: wide (d = 128) and generic forms; T covers every wave as owner of the maximum
    for heads, d, T in ((32, 128, 12), (64, 128, 12), (8, 2, 6), (8, 64, 7), (8, 130, 7), (8, 256, 6), (16, 66, 7), (16, 256, 6),
                        (32, 64, 7), (32, 192, 6), (64, 64, 6), (64, 136, 6), (16, 128, 2), (8, 128, 2)):
        cs += _mk(f"hh-{heads}x{d}-T{T}", "heads_hadamard", T, ("f16", "q"), heads=heads, d=d, clip2=0.9 if heads % 32 else 0.5)
    # ---- heads_hadamard_mix
    for heads, d, K, T in ((40, 128, 40, 12), (24, 128, 12, 3), (80, 64, 40, 2), (12, 2, 12, 2), (48, 32, 12, 2)):
        cs += _mk(f"hhx-{heads}x{d}-K{K}", "heads_hadamard_mix", T, ("f16",), heads=heads, d=d, K=K)
    # ---- heads_hadamard_merge.  32 x 128: T <= 128 spread (f16), quantiser one workgroup; T = 129: merge(NH32,f16)
    for T, S, modes in ((1, 1, ("f16", "q", "xp")), (12, 3, ("f16", "q", "xp")), (17, 8, ("f16", "xp")), (32, 2, ("xp",)),
                        (9, 9, ("f16", "q")), (128, 2, ("f16",)), (129, 2, ("f16", "q"))):
        cs += _mk(f"hhm-32x128-T{T}-S{S}", "heads_hadamard_merge", T, modes, heads=32, d=128, S=S, clip2=0.5 if S % 2 else 0.9)
    for T, S, modes in ((12, 3, ("f16", "q", "xp")), (17, 9, ("f16", "q", "xp")), (33, 1, ("f16",))):
        cs += _mk(f"hhm-64x128-T{T}-S{S}", "heads_hadamard_merge", T, modes, heads=64, d=128, S=S)
    for d, S, T, arg in ((64, 4, 12, 8), (64, 1, 2, None), (8, 2, 6, None), (136, 3, 7, None), (256, 2, 6, None), (120, 4, 2, 4)):
        cs += _mk(f"hhm-32x{d}-T{T}-S{S}", "heads_hadamard_merge", T, ("f16", "q"), heads=32, d=d, S=S, nsplits_arg=arg)
    # ---- heads_hadamard_merge_spread (fp16 rows + part_amax [T, 8]); T <= 4 feeds the hq quantiser
    for T, S, shift in ((4, 3, 0), (4, 2, 4), (1, 1, 5), (12, 9, 0), (128, 2, 0)):
        cs += _mk(f"hhms-T{T}-S{S}", "heads_hadamard_merge_spread", T, ("amax",), heads=32, d=128, S=S, shift=shift)
    # (four tokens with a zero-scale row and an all-zero row among them: what the hq quantiser gets of the tail kinds)
    cs += _mk("hhms-T4-S2-tail", "heads_hadamard_merge_spread", 4, ("amax",), tiers=("exact",), heads=32, d=128, S=2, shift=2,
              kinds=("pos", "tiny", "zero", "neg"))
    cs += _mk("hhxs-40-K40-T4-S2-tail", "heads_hadamard_mix_merge_spread", 4, ("amax",), tiers=("exact",), heads=40, d=128, K=40, S=2,
              shift=5, kinds=("tiny", "neg", "ties", "zero"))
    # ---- heads_hadamard_mix_merge_spread
    for heads, K, T, S, modes, shift in ((40, 40, 4, 2, ("f16", "amax", "xp"), 0), (40, 40, 4, 3, ("amax",), 4), (40, 40, 17, 1, ("f16", "amax", "xp"), 0),
                                         (40, 40, 32, 2, ("xp",), 0), (24, 12, 9, 9, ("f16", "amax", "xp"), 0), (48, 12, 3, 2, ("f16", "amax"), 5),
                                         (56, 28, 8, 1, ("f16", "amax"), 0), (12, 12, 2, 2, ("f16", "amax"), 3), (40, 40, 128, 1, ("amax",), 0)):
        cs += _mk(f"hhxs-{heads}-K{K}-T{T}-S{S}", "heads_hadamard_mix_merge_spread", T, modes, heads=heads, d=128, K=K, S=S, shift=shift)
    # ---- MLP, one workgroup per token: every (EPL, KH) through BOTH entries (silu_mul_hadamard and mlp_hadamard, no workspace)
    one = [(28, 128), (28, 256), (28, 512), (28, 1024), (44, 128), (44, 256), (44, 512), (12, 128), (12, 256), (12, 512), (12, 1024),
           (12, 2048), (108, 128), (1, 256), (40, 512), (20, 1024), (4, 2048), (1, 2048), (1, 128), (2, 128)]
    for i, (K, P) in enumerate(one):
        cs += _mk(f"mlp-had{K}xH{P}-T21", "mlp", 21, ("f16", "q", "xp"), I=K * P, K=K, gate=True, clip2=(0.9, 0.5)[i % 2])
    # ---- MLP with the exchange workspace: both sides of every token boundary of smh_spread
    for K, P, Ts in ((28, 1024, (1, 5, 16, 17)), (28, 512, (1, 3, 16, 17, 32, 33)), (108, 128, (1, 5, 16, 17, 32, 33))):
        for T in Ts:      # (the few-token cases start at block 11: the five blocks the 16-token case gives to both / over / tiny / sub / zero)
            cs += _mk(f"mlpws-had{K}xH{P}-T{T}", "mlp", T, ("f16", "q") + (("xp",) if T <= 32 else ()), I=K * P, K=K, ws=True,
                      shift=11 if T < 16 else 0, clip2=(0.9, 0.5)[T % 2])
    for T in (256, 257):        # QS_XWG_MAX_TOKENS
        cs += _mk(f"mlpws-had28xH512-T{T}", "mlp", T, ("q",), tiers=("exact",), I=14336, K=28, ws=True)
    cs += _mk("mlpws-had44xH128-T4", "mlp", 4, ("f16", "q"), I=5632, K=44, ws=True)      # a workspace, but no spread form
    # ---- the row-absmax quantiser itself
    for K, T in ((4096, 12), (2056, 8), (1002, 8), (6, 3), (5120, 2)):
        cs += _mk(f"rq-K{K}", "rq", T, ("q",), K=K, clip2=0.5 if K % 8 else 0.9)
    cs += _mk("rq-K512-clip0", "rq", 8, ("q",), K=512, clip2=0.0)     # clip 0: every scale is 0, every nonzero x is +-inf
    cs += _mk("hh-32x128-T8-clip0", "heads_hadamard", 8, ("f16", "q"), heads=32, d=128, clip2=0.0)
    return cs


# ------------------------------------------------------------------ what a case must give, and the named faults

TRANSFORM_FAULTS = ("table_transposed", "scale_after_mix", "sequency_order", "wrong_split_stride")
BLOCK_FAULTS = ("amax_drops_a_block", "stale_block_maximum")
XP_FILL = 123.0     # what the test leaves in the tile rows that no token owns


def reference(c: Case, dt: Data, fault: Optional[str] = None, block: int = 0) -> dict:
    """Every output of the case: "f16" rows [T, n]; ("q", clip) -> (bytes [T, n/2], scale [T]) for clip in (1.0, c.clip2);
    "amax" [T, 8] fp32 partial maxima; "xp" the fragment-major tile(s).  `fault`: the same with one named mutation."""
    assert fault is None or fault in FAULTS, fault
    z = ref_rows(c, dt, fault if fault in TRANSFORM_FAULTS else None)
    out = {"f16": z}
    block_of, nb = c.owners()
    if "q" in c.modes:
        for clip in (1.0, c.clip2):
            out[("q", clip)] = ref_quant(z, clip, block_of, nb, fault if fault in QUANT_FAULTS else None, block)
    if "amax" in c.modes:
        pm = block_max(z, block_of, nb, positive_only=fault == "amax_positive_only")
        if fault == "amax_drops_a_block":
            pm[:, block] = 0.0
        elif fault == "stale_block_maximum":
            pm[:, block] = np.concatenate([[0.0], pm[:-1, block]])
        out["amax"] = pm.astype(F32)
    if "xp" in c.modes:
        out["xp"] = xp_tile(z, XP_FILL)
    return out


def quant_tokens(dt: Data) -> np.ndarray:
    """The tokens whose quantised output is compared: all but the `over` rows (see the module docstring)."""
    return np.array([k != "over" for k in dt.kinds], bool) if dt.kinds else np.ones(dt.x.shape[0], bool)


def differs(c: Case, dt: Data, a: dict, b: dict, mode: str) -> bool:
    """Do two results of the case differ in what `mode` compares (bit for bit)?"""
    u16 = lambda v: np.ascontiguousarray(v).view(np.uint16)
    if mode == "f16":
        return not np.array_equal(u16(a["f16"]), u16(b["f16"]))
    if mode == "xp":
        return not np.array_equal(u16(a["xp"]), u16(b["xp"]))
    if mode == "amax":
        return not (np.array_equal(a["amax"], b["amax"]) and np.array_equal(u16(a["f16"]), u16(b["f16"])))
    keep = quant_tokens(dt)
    return any(not (np.array_equal(a[k][0][keep], b[k][0][keep]) and np.array_equal(u16(a[k][1][keep]), u16(b[k][1][keep])))
               for k in a if isinstance(k, tuple))


def fault_blocks(c: Case, fault: str, mode: str) -> List[int]:
    """The blocks a fault is tried on for (case, mode); empty: the fault does not apply there."""
    n, K, P, heads, d = c.geometry()
    merge = c.entry.startswith("heads_hadamard_m") and c.entry != "heads_hadamard_mix"
    block_of, nb = c.owners()
    live = [int(b) for b in np.unique(block_of)]
    if fault in BLOCK_FAULTS:
        rows = [r for _, m, r in c.routes() if m == mode]
        if mode not in ("q", "amax") or len(live) < 2:
            return []
        if fault == "stale_block_maximum" and not any(r.startswith("smh.spread") or mode == "amax" for r in rows):
            return []
        return live
    if fault in ("amax_positive_only",):
        return [0] if mode in ("q", "amax") else []
    if fault in ("clamp_minus_7", "round_half_away", "nibbles_swapped"):
        return [0] if mode == "q" else []
    if fault == "table_transposed":       # (the had28 table is symmetric: transposed, it is the same table)
        return [0] if K > 1 and c.entry != "rq" and not np.array_equal(table(K), table(K).T) else []
    if fault == "scale_after_mix":
        return [0] if K > 1 and c.entry not in ("rq", "hadk_mix") else []
    if fault == "sequency_order":
        return [0] if P >= 4 and c.entry not in ("rq", "hadk_mix") else []
    if fault == "wrong_split_stride":
        return [0] if merge and c.dims["S"] > 1 else []
    raise KeyError(fault)


# (entry point, keyword arguments of route, the code) of shapes every entry must refuse without launching
REFUSED = [
    ("fwht", dict(rows=2, N=3), -1), ("fwht", dict(rows=2, N=65536), -1), ("fwht", dict(rows=2, N=0), -1),
    ("hadk_mix", dict(T=2, K=0, M=8), -1), ("hadk_mix", dict(T=2, K=173, M=8), -1),
    ("heads_hadamard", dict(T=2, heads=12, d=128, quant=False), -1), ("heads_hadamard", dict(T=2, heads=32, d=3, quant=True), -1),
    ("heads_hadamard", dict(T=2, heads=32, d=258, quant=False), -1), ("heads_hadamard", dict(T=2, heads=128, d=128, quant=True), -1),
    ("heads_hadamard_mix", dict(T=2, heads=32, d=128, K=1), -1), ("heads_hadamard_mix", dict(T=2, heads=42, d=128, K=40), -1),
    ("heads_hadamard_mix", dict(T=2, heads=36, d=128, K=12), -1), ("heads_hadamard_mix", dict(T=2, heads=160, d=128, K=40), -2),
    ("heads_hadamard_merge", dict(T=2, heads=16, d=128, S=2, quant=False), -1),
    ("heads_hadamard_merge", dict(T=2, heads=32, d=12, S=2, quant=False), -1),
    ("heads_hadamard_merge", dict(T=2, heads=64, d=64, S=2, quant=True), -1),
    ("heads_hadamard_merge", dict(T=3, heads=32, d=128, S=2, quant=True, max_tokens=2), -1),
    ("heads_hadamard_merge", dict(T=2, heads=32, d=128, S=0, quant=False), -1),
    ("heads_hadamard_merge", dict(T=2, heads=64, d=128, S=2, quant=True, xp=True), -1),
    ("heads_hadamard_merge", dict(T=33, heads=64, d=128, S=2, quant=False, xp=True), -1),
    ("heads_hadamard_merge", dict(T=2, heads=32, d=64, S=2, quant=False, xp=True), -1),
    ("heads_hadamard_merge_spread", dict(T=129, heads=32, d=128, S=2), -1),
    ("heads_hadamard_merge_spread", dict(T=2, heads=64, d=128, S=2), -1),
    ("heads_hadamard_merge_spread", dict(T=2, heads=32, d=64, S=2), -1),
    ("heads_hadamard_mix_merge_spread", dict(T=129, heads=40, d=128, K=40, S=2, amax=True), -1),
    ("heads_hadamard_mix_merge_spread", dict(T=2, heads=40, d=64, K=40, S=2, amax=False), -1),
    ("heads_hadamard_mix_merge_spread", dict(T=2, heads=80, d=128, K=40, S=2, amax=False), -1),
    ("heads_hadamard_mix_merge_spread", dict(T=33, heads=40, d=128, K=40, S=2, amax=False, xp=True), -1),
    ("heads_hadamard_mix_merge_spread", dict(T=2, heads=40, d=128, K=40, S=2, amax=True, xp=True), -1),
    ("heads_hadamard_mix_merge_spread", dict(T=2, heads=36, d=128, K=12, S=2, amax=False), -1),
    ("silu_mul_hadamard", dict(T=2, I=1792, K=28, quant=True), -1),          # P = 64: no form
    ("silu_mul_hadamard", dict(T=2, I=10752, K=28, quant=False), -1),        # P = 384
    ("silu_mul_hadamard", dict(T=2, I=57344, K=28, quant=True), -2),         # had28 x H2048: 227 KB
    ("silu_mul_hadamard", dict(T=2, I=1000, K=28, quant=True), -1),          # I % K
    ("mlp_hadamard", dict(T=2, I=57344, K=28, ws=True, quant=False), -2),
    ("mlp_hadamard", dict(T=17, I=57344, K=28, ws=True, quant=False, xp=True), -2),
    ("mlp_hadamard", dict(T=33, I=14336, K=28, ws=True, quant=False, xp=True), -1),
    ("mlp_hadamard", dict(T=4, I=14336, K=28, ws=True, quant=True, xp=True), -1),
    ("mlp_hadamard", dict(T=2, I=2048, K=0, ws=False, quant=False), -1),
    ("mlp_hadamard", dict(T=2, I=45056, K=44, ws=False, quant=True), -2),
    ("rowabsmax_quant", dict(T=2, K=7), -1), ("rowabsmax_quant", dict(T=2, K=0), -1),
]

# the workspace-history sequence (one exchange workspace, tokens at different generations): (T, I, K)
HISTORY = [(32, 14336, 28), (3, 28672, 28), (32, 13824, 108), (17, 28672, 28), (1, 13824, 108), (16, 14336, 28)]
