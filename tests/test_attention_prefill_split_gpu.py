"""The context-split prompt attention (attention_prefill.hip: paged_attention_prefill_kernel<.., SPLIT = true>, family
ATTN_PREFILL_SPLIT of attention.hip: attn_form) against float64: a prompt-sized suffix behind a context that is already in the
paged cache, over several context splits of whole 64-key chunks.

Shapes are the smallest at which this form can go wrong: exactly two 64-row blocks and ragged last blocks, splits that lie
wholly behind the early rows (no prefix at all), prefixes around one chunk, contexts one key either side of S whole chunks,
mostly empty splits, ragged launches over narrow and wide block tables at every block size, one long context, and the other
head layouts.  Every case runs with `out` (the merge launch; a guard row behind the output) and without (the partials: none
NaN, l >= 0, every split that a row cannot see the neutral partial; their float64 merge; and the head transform over them).
Data, poison and reference are those of tests/attn_cases.py; a ragged launch keeps the LAST q rows of each sequence of a
uniform case, which sit at the same positions."""
import numpy as np
import pytest
import torch

import attn_cases as A
from test_kernels_gpu import assert_close_1e3
from test_kv_fp8_gpu import dequantise_f64, quantise

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CNT_SLOTS = 4096    # attention_common.cuh: QS_ATT_CNT_SLOTS
FA_KEYS = 64        # attention_common.cuh: QS_FA_KEYS
FAMILY_SPLIT = 6    # attention_common.cuh: ATTN_PREFILL_SPLIT


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from qspec_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _case(q_lens, ctx, heads, bs, S, regime, seed, width=None):
    """(Case at the longest q_len, q_lens per sequence)."""
    q_lens = (q_lens,) * len(ctx) if isinstance(q_lens, int) else tuple(q_lens)
    return A.make_case(ctx, max(q_lens), heads, bs, regime, S, True, seed, width=width, sink_last=True), q_lens


H32, H64, H40 = A.H32, A.H64, A.H40
RAGGED = ((40, 33, 1), (300, 2100, 517))
CASES = [
    # no prefix at all: the later splits lie wholly behind the early rows
    _case(32, (32,), H32, 16, 4, "smooth", 1), _case(33, (33,), H32, 16, 4, "peaked", 2), _case(47, (47,), H32, 8, 4, "sink", 3),
    # prefixes of 1, 63, 64 and 65 keys, two splits
    _case(32, (33, 95, 96, 97), H32, 16, 2, "negative", 4),
    # one key either side of S whole chunks
    _case(32, (191, 193), H32, 16, 3, "sink", 5), _case(33, (511, 513), H32, 32, 8, "peaked", 6),
    # mostly empty splits
    _case(32, (70,), H32, 16, 16, "future_trap", 7),
    # ragged launches: narrow and wide tables, every block size
    _case(*RAGGED, H32, 8, 4, "peaked", 8), _case(*RAGGED, H32, 16, 16, "sink", 9), _case(*RAGGED, H32, 32, 8, "negative", 10),
    _case(*RAGGED, H32, 8, 16, "smooth", 11, width=4096 // 8), _case(*RAGGED, H32, 16, 4, "future_trap", 12, width=4096 // 16),
    _case(*RAGGED, H32, 32, 16, "sink", 13, width=4096 // 32),
    # one long context
    _case(32, (4097,), H32, 16, 16, "sink", 14),
    # the other head layouts: group 8 (two row blocks at 16 tokens), no GQA (two row blocks and a ragged third)
    _case(16, (16, 400), H64, 16, 4, "peaked", 15), _case(128, (328,), H40, 16, 3, "sink", 16),
    _case(130, (130, 207), H40, 8, 4, "negative", 17),
]
FP8_CASES = [CASES[3], CASES[8], CASES[13]]


def _id(cq):
    c, q = cq
    return f"{c.regime}-h{c.nq}.{c.nkv}-bs{c.bs}-w{c.width}-q{','.join(map(str, q))}-S{c.n_splits}-ctx{','.join(map(str, c.ctx))}"


def _ragged(case, q_lens, d):
    """The launch arrays of the case with sequence s keeping its last q_lens[s] rows."""
    keep = np.concatenate([np.arange((s + 1) * case.q_len - q, (s + 1) * case.q_len) for s, q in enumerate(q_lens)])
    qkv = np.ascontiguousarray(d["qkv"][keep])
    q_start = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    return qkv, qkv[:, :case.nq * case.d], q_start


def _run(ops, case, q_lens, d, qkv, q_start, kc, vc, out, **scales):
    T, Tmax = int(q_start[-1]), len(case.ctx) * case.q_len
    assert ops.paged_attention_family(len(case.ctx), case.q_len, case.nq, case.nkv, case.d, case.bs, case.width, case.n_splits,
                                      out is not None) == FAMILY_SPLIT
    ws = torch.zeros(ops.paged_attention_workspace_bytes(Tmax, case.nq, case.d, case.n_splits), dtype=torch.uint8, device=DEV)
    ops.paged_attention(dev(qkv), d["row"], kc, vc, dev(d["bt"]), dev(d["ctx"]), dev(q_start), T, case.q_len, case.nq,
                        d["scale"], case.n_splits, ws, out, **scales)
    return ws


def _partials(case, ws, T):
    """(o [T, nq, S, d], (m, l) [T, nq, S, 2]): the workspace is laid out for Tmax = n_seqs * max_q_len tokens."""
    Tmax, nq, hd, S = len(case.ctx) * case.q_len, case.nq, case.d, case.n_splits
    f = host(ws.view(torch.float32))
    o = f[CNT_SLOTS:CNT_SLOTS + Tmax * nq * S * hd].reshape(Tmax, nq, S, hd)[:T]
    ml = f[CNT_SLOTS + Tmax * nq * S * hd:CNT_SLOTS + Tmax * nq * S * (hd + 2)].reshape(Tmax, nq, S, 2)[:T]
    return o, ml


def _check(ops, oracle, case, q_lens, d, kc, vc, ref_kc, ref_vc, **scales):
    qkv, q, q_start = _ragged(case, q_lens, d)
    T, nq, hd, S = int(q_start[-1]), case.nq, case.d, case.n_splits
    ref = A.ref_attention_f64(q, ref_kc, ref_vc, d["bt"], d["ctx"], q_start, d["scale"])
    # merged
    out = torch.full((T + 1, nq * hd), 7.0, dtype=torch.float16, device=DEV)
    _run(ops, case, q_lens, d, qkv, q_start, kc, vc, out[:T], **scales)
    assert_close_1e3(host(out[:T]), ref)
    assert torch.all(out[T] == 7.0)   # guard row
    # partials
    ws = _run(ops, case, q_lens, d, qkv, q_start, kc, vc, None, **scales)
    o, ml = _partials(case, ws, T)
    assert not np.isnan(o).any() and not np.isnan(ml).any()
    assert (ml[..., 1] >= 0).all()
    for s, (c, ql) in enumerate(zip(case.ctx, q_lens)):   # a split that starts past a row's position: the neutral partial
        L = -(-(-(-c // S)) // FA_KEYS) * FA_KEYS
        for i in range(ql):
            t, z0 = int(q_start[s]) + i, (c - ql + i) // L + 1
            assert (o[t, :, z0:] == 0).all() and np.isneginf(ml[t, :, z0:, 0]).all() and (ml[t, :, z0:, 1] == 0).all(), (s, i)
            assert np.isfinite(ml[t, :, :z0, 0]).all() and (ml[t, :, :z0, 1] > 0).all(), (s, i)
    assert_close_1e3(A.merge_partials_f64(o, ml).reshape(T, -1), ref)
    if nq in (32, 64):   # the head transform that merges the partials, against the transform of the merged rows
        scale = oracle.rsqrt_scale(nq)
        a = torch.full((T + 1, nq * hd), 7.0, dtype=torch.float16, device=DEV)
        b = torch.empty(T, nq * hd, dtype=torch.float16, device=DEV)
        ops.heads_hadamard_merged(ws, len(case.ctx) * case.q_len, S, T, nq, hd, scale, out_f16=a[:T])
        ops.heads_hadamard(out[:T], scale, out_f16=b, heads=nq)
        assert_close_1e3(host(a[:T]), host(b))
        assert torch.all(a[T] == 7.0)


@pytest.mark.parametrize("cq", CASES, ids=_id)
def test_split_prompt_attention_matches_float64(ops, oracle, cq):
    case, q_lens = cq
    d = A.build(case)
    _check(ops, oracle, case, q_lens, d, dev(d["kc"]), dev(d["vc"]), d["kc"], d["vc"])


@pytest.mark.parametrize("cq", FP8_CASES, ids=_id)
def test_split_prompt_attention_fp8_matches_float64_on_the_dequantised_cache(ops, oracle, cq):
    case, q_lens = cq
    d = A.build(case)
    ks, vs = 0.75, 1.5
    kc8, vc8 = quantise(d["kc"], ks), quantise(d["vc"], vs)
    _check(ops, oracle, case, q_lens, d, kc8.view(torch.uint8).to(DEV), vc8.view(torch.uint8).to(DEV), dequantise_f64(kc8, ks),
           dequantise_f64(vc8, vs), k_scale=ks, v_scale=vs)
