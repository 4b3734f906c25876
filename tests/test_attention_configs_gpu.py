"""ops.paged_attention against the float64 reference over the case matrix of tests/attn_cases.py: block sizes 8 / 16 / 32,
block tables narrower and wider than the 128 entries the register table holds, every context split count the engine
uses, verify-shaped queries, and score regimes far from the flat softmax of std-0.5 data (peaked, a sink key at either
end of the context, all-negative, keys the causal mask must keep out).  Every cache slot a sequence does not own holds
poison, every block no table names NaN.  Then the partials through the head transforms the model merges them in."""
import numpy as np
import pytest
import torch

import attn_cases as A
from test_kernels_gpu import assert_close_1e3

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CNT_SLOTS = 4096   # attention_common.cuh: QS_ATT_CNT_SLOTS, ints ahead of the partials in the workspace


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


def _launch(ops, case, d, out):
    T = case.T
    ws = torch.zeros(ops.paged_attention_workspace_bytes(T, case.nq, case.d, case.n_splits), dtype=torch.uint8, device=DEV)
    ops.paged_attention(dev(d["qkv"]), d["row"], dev(d["kc"]), dev(d["vc"]), dev(d["bt"]), dev(d["ctx"]),
                        dev(d["q_start"]), T, case.q_len, case.nq, d["scale"], case.n_splits, ws, out)
    return ws


def _partials(case, ws):
    """(o [T, nq, S, d], (m, l) [T, nq, S, 2]) as paged_attention(out = NULL) leaves them."""
    T, nq, hd = case.T, case.nq, case.d
    S = A.generic_splits(case.n_splits) if hd != 128 else case.n_splits
    f = host(ws.view(torch.float32))
    o = f[CNT_SLOTS:CNT_SLOTS + T * nq * S * hd].reshape(T, nq, S, hd)
    ml = f[CNT_SLOTS + T * nq * S * hd:CNT_SLOTS + T * nq * S * (hd + 2)].reshape(T, nq, S, 2)
    return o, ml


@pytest.mark.parametrize("case", A.GPU_CASES, ids=lambda c: c.id)
def test_paged_attention_matches_float64(ops, case):
    d = A.build(case)
    ref = A.ref_attention_f64(d["q"], d["kc"], d["vc"], d["bt"], d["ctx"], d["q_start"], d["scale"])
    T = case.T
    if case.merged:
        out = torch.full((T + 1, case.nq * case.d), 7.0, dtype=torch.float16, device=DEV)
        _launch(ops, case, d, out[:T])
        assert_close_1e3(host(out[:T]), ref)
        assert torch.all(out[T] == 7.0)   # guard row
    else:
        o, ml = _partials(case, _launch(ops, case, d, None))
        assert np.isfinite(o).all() and not np.isnan(ml).any()
        assert_close_1e3(A.merge_partials_f64(o, ml).reshape(T, -1), ref)


def _hadamard_ref(oracle, case, ref):
    from qspec_amd import hadamard_tables
    had_scale = oracle.rsqrt_scale(case.nq)
    hadK, K = hadamard_tables.get_hadK(case.nq)
    r16 = ref.astype(np.float16)
    if K == 1:
        return had_scale, None, 1, oracle.heads_hadamard(r16, case.nq, had_scale)
    return had_scale, hadK, K, oracle.heads_hadamard(r16, case.nq, had_scale, hadK.numpy().astype(np.float16), K)


CONSUMER_CASES = [
    # heads_hadamard_merged: 32 and 64 heads, verify and draft shapes
    ("merged", A.make_case((300, 1100, 5, 2049), 4, A.H32, 16, "sink", 8, False, 6000, sink_last=True)),
    ("merged", A.make_case((129, 700), 6, A.H32, 8, "peaked", 16, False, 6001, width=300)),
    ("merged", A.make_case((33, 4097), 4, A.H32, 32, "negative", 4, False, 6002)),
    ("merged", A.make_case((40, 2048, 9, 1), 1, A.H32, 16, "future_trap", 8, False, 6003)),
    ("merged", A.make_case((200, 1300), 4, A.H64, 8, "sink", 3, False, 6004, sink_last=True)),
    ("merged", A.make_case((17, 8191), 1, A.H64, 16, "peaked", 16, False, 6005)),
    ("merged", A.make_case((600, 2047), 6, A.H64, 32, "future_trap", 4, False, 6006, width=200)),
    # the draft pass's spread form (<= 4 tokens)
    ("spread", A.make_case((37, 600, 1500, 9), 1, A.H32, 16, "sink", 8, False, 6100, sink_last=True)),
    ("spread", A.make_case((2049, 5), 1, A.H32, 8, "negative", 16, False, 6101, width=512)),
    ("spread", A.make_case((4097,), 4, A.H32, 32, "peaked", 4, False, 6102)),
    # 40 heads (Llama-2-13B, had40): the mix spread form
    ("mix", A.make_case((300, 77, 1200), 1, A.H40, 16, "sink", 3, False, 6200, sink_last=True)),
    ("mix", A.make_case((1025,), 4, A.H40, 8, "peaked", 3, False, 6201, width=256)),
    ("mix", A.make_case((129, 2049), 1, A.H40, 32, "negative", 3, False, 6202)),
]


@pytest.mark.parametrize("form,case", CONSUMER_CASES, ids=[f"{f}-{c.id}" for f, c in CONSUMER_CASES])
def test_partials_through_the_head_transform_match_float64(ops, oracle, form, case):
    """The consumers the model merges the partials in: against the oracle head transform of the float64 attention
    rounded to fp16, within 1e-3 on the fp16 output."""
    d = A.build(case)
    ref = A.ref_attention_f64(d["q"], d["kc"], d["vc"], d["bt"], d["ctx"], d["q_start"], d["scale"])
    had_scale, hadK, K, ref_h = _hadamard_ref(oracle, case, ref)
    ws = _launch(ops, case, d, None)
    T, nq, hd, S = case.T, case.nq, case.d, case.n_splits
    out = torch.full((T + 1, nq * hd), 7.0, dtype=torch.float16, device=DEV)
    if form == "merged":
        assert K == 1
        ops.heads_hadamard_merged(ws, T, S, T, nq, hd, had_scale, out_f16=out[:T])
    elif form == "spread":
        assert K == 1 and ops.heads_hadamard_merged_spread_supported(T, nq, hd)
        pam = torch.full((T, 8), -1.0, dtype=torch.float32, device=DEV)
        ops.heads_hadamard_merged_spread(ws, T, S, T, nq, hd, had_scale, out[:T], pam)
        assert np.array_equal(host(pam).max(axis=1), np.abs(host(out[:T]).astype(np.float32)).max(axis=1))
    else:
        assert K > 1 and ops.heads_hadamard_mix_merged_spread_supported(T, nq, hd, K)
        ops.heads_hadamard_mix_merged_spread(ws, T, S, T, nq, hd, hadK.to(torch.float16).to(DEV), K, had_scale, out[:T])
    assert_close_1e3(host(out[:T]), ref_h)
    assert torch.all(out[T] == 7.0)
