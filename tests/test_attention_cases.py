"""CPU side of the paged-attention matrix (tests/attn_cases.py): the CPU oracle against the float64 reference on every
case of the GPU matrix with contexts <= 2048, the reference (and the oracle) blind to the poisoned slots, the regimes
doing what they claim, and the case list reaching every kernel instantiation paged_attention() (attention.hip) launches."""
import numpy as np
import pytest

import attn_cases as A

CPU_CASES = [c for c in A.GPU_CASES if max(c.ctx) <= 2048]


def _close_1e3(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = ~(np.abs(got - ref) <= 1e-3 * np.maximum(1.0, np.abs(ref)))
    assert not bad.any(), (np.nanmax(np.abs(got - ref)), int(bad.sum()))


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.id)
def test_oracle_attention_within_1e3_of_float64(oracle, case):
    d = A.build(case)
    args = (d["bt"], d["ctx"], d["q_start"], d["scale"])
    ref = A.ref_attention_f64(d["q"], d["kc"], d["vc"], *args)
    got = oracle.paged_attention(np.ascontiguousarray(d["q"]), d["kc"], d["vc"], *args)
    _close_1e3(got, ref)
    # every poisoned value re-drawn: neither the reference nor the oracle moves
    d2 = A.build(case, poison_seed=case.seed + 7)
    assert np.array_equal(d2["poisoned"], d["poisoned"])
    if d["poisoned"].any():
        assert not np.array_equal(d2["kc"][d["poisoned"]].view(np.uint16), d["kc"][d["poisoned"]].view(np.uint16))
    assert np.array_equal(A.ref_attention_f64(d2["q"], d2["kc"], d2["vc"], *args), ref)
    assert np.array_equal(oracle.paged_attention(np.ascontiguousarray(d2["q"]), d2["kc"], d2["vc"], *args).view(np.uint16),
                          got.view(np.uint16))


def test_reference_reads_only_owned_slots():
    """A key leaking from a poisoned slot or a NaN block into the float64 reference is visible at once."""
    case = A.make_case((5, 17, 40), 4, (8, 2, 128), 8, "smooth", 1, True, 7, width=12)
    d = A.build(case)
    assert d["poisoned"].any() and len(d["nan_blocks"]) > 0
    assert np.isnan(d["kc"][d["nan_blocks"]]).all() and np.isnan(d["vc"][d["nan_blocks"]]).all()
    assert (np.abs(d["kc"][d["poisoned"]].astype(np.float32)) > 5e4).all()
    # every padding entry names a poison block, every poisoned slot lies in a named block
    named = set(d["bt"].ravel().tolist())
    assert not named & set(d["nan_blocks"].tolist())
    ref = A.ref_attention_f64(d["q"], d["kc"], d["vc"], d["bt"], d["ctx"], d["q_start"], d["scale"])
    assert np.isfinite(ref).all()
    # one more key per sequence (the first poisoned slot past ctx): the reference must change by far more than 1e-3
    ctx2 = d["ctx"] + 1
    ref2 = A.ref_attention_f64(d["q"], d["kc"], d["vc"], d["bt"], ctx2, d["q_start"], d["scale"])
    assert np.abs(ref2 - ref).max() > 1.0


def test_regimes_have_the_claimed_scores():
    """peaked: logit std ~6; sink: one key > 90 % of every row's mass, > 20 above the rest; negative: every logit <= -30;
    future_trap: the masked keys of the verify window would score ~ +20 over the visible ones."""
    for regime, sink_last in [("peaked", False), ("sink", False), ("sink", True), ("negative", False), ("future_trap", False)]:
        for heads in ((32, 8, 128), (32, 4, 64)):
            case = A.make_case((300, 1100), 6, heads, 16, regime, 8, True, 11, sink_last=sink_last)
            d = A.build(case)
            _, L = A.ref_attention_f64(d["q"], d["kc"], d["vc"], d["bt"], d["ctx"], d["q_start"], d["scale"],
                                       return_logits=True)
            for S, c in zip(L, case.ctx):
                vis = S[np.isfinite(S)]
                P = np.exp(S - S.max(-1, keepdims=True))
                P /= P.sum(-1, keepdims=True)
                if regime == "peaked":
                    assert 4.5 < vis.std() < 7.5 and vis.max() > 18 and vis.min() < -18
                elif regime == "sink":
                    p = c - case.q_len if sink_last else 0
                    assert (P[..., p] > 0.9).all()
                    rest = np.delete(S, p, axis=-1)
                    assert (S[..., p] - np.where(np.isfinite(rest), rest, -np.inf).max(-1) > 20).all()
                elif regime == "negative":
                    assert vis.max() <= -30
                else:   # the logits the mask removes, against the visible ones of the same row
                    assert np.isneginf(S[:, 0, :, c - case.q_len + 1:]).all()
                    last = S[:, -1]     # the last query sees the whole window: the trap keys are its own past
                    assert (last[..., c - case.q_len + 1:].min(-1) - last[..., :c - case.q_len + 1].max(-1) > 15).all()


def test_matrix_covers_every_dispatch_row():
    """attention.hip: attn_form() at default knobs -- prefill kernel, paged_attention_kernel<PF, BT> with and
    without out, paged_attention_waves_kernel<BT, 4, FAST>, the generic head-size kernels -- each reached by at least
    one case of the GPU matrix (a pruned case list or a changed rule fails here)."""
    reached = set().union(*(A.path_rows(c) for c in A.GPU_CASES))
    assert A.REQUIRED_ROWS <= reached, sorted(A.REQUIRED_ROWS - reached)
    cs = A.GPU_CASES
    assert {c.bs for c in cs} == {8, 16, 32}
    assert set(A.REGIMES) <= {c.regime for c in cs}
    assert {1, 4, 6} <= {c.q_len for c in cs}
    assert set(A.SPLITS) <= {c.n_splits for c in cs}
    assert {(c.nq, c.nkv, c.d) for c in cs} >= {A.H32, A.H64, A.H40, A.HT}
    assert any(c.width <= 128 for c in cs) and any(c.width > 128 and min(c.ctx) < 64 for c in cs)
    lens = {x for c in cs for x in c.ctx}
    for bs in (8, 16, 32):
        assert {bs - 1, bs + 1} <= {x for c in cs if c.bs == bs for x in c.ctx}
    assert {1, 127, 128, 129, 2047, 2048, 2049, 4097, 8191} <= lens
    assert max(x for c in cs if c.d == 64 for x in c.ctx) <= 2048
    assert all(c.d == 128 for c in cs if max(c.ctx) > 2048)
    for regime in A.REGIMES:   # every regime reaches the in-kernel merge and the partials
        assert {True, False} <= {c.merged for c in cs if c.regime == regime}
    assert any(c.regime == "future_trap" and c.q_len > 1 and A.kernel_path(c).startswith("chunk") for c in cs)


def _function_body(src, signature):
    """The text between the braces of the function whose definition starts with `signature`."""
    i = src.index(signature)
    j = src.index("{", i + len(signature) - 1)
    depth, k = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            return src[j + 1:k]
        k += 1


def test_dispatch_rule_matches_the_kernel_source():
    """The Python rule restates attention.hip: attn_form(); the constants it copies (attention_common.cuh) and the conditions
    it mirrors are read back from the source, so that a change there without a change here fails.  Every condition of the
    launch plan lies inside attn_form() itself; the split clamp of the generic head sizes is the one-line function attn_form
    calls (hadamard.hip calls it too)."""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qspec_amd", "csrc")
    consts = open(os.path.join(csrc, "attention_common.cuh")).read()
    for name, v in (("QS_ATT_CHUNK", A.CHUNK), ("QS_FA_ROWS", A.FA_ROWS), ("QS_ATT_MAXR", A.MAXR),
                    ("QS_ATT_MAXSPLIT", A.MAXSPLIT)):
        assert f"#define {name} {v}" in consts, name
    src = open(os.path.join(csrc, "attention.hip")).read()
    form = _function_body(src, "static AttnForm attn_form(const AttnArgs& a) {")
    for cond in ("const int rows = a.max_q_len << f.group_log2;",
                 "if (fa_env && a.n_splits == 1 && rows >= 2 * QS_FA_ROWS)",
                 "((int64_t)a.max_blocks << f.bs_log2) > (int64_t)QS_ATT_CHUNK * a.n_splits",
                 "if (!a.out && (aw_env >= 0 ? aw_env != 0 : long_splits))",
                 "f.fast = f.bt && f.bs_log2 >= 4 && fast_env;",
                 "(size_t)a.n_seqs * a.nkv * f.n_rb * a.n_splits <= 256",
                 "f.bt = a.max_blocks <= 128;",
                 "const bool partials = !a.out || S > 1;",
                 "if (a.d % 8 == 0 && a.d >= 8)",
                 "const int S = paged_attention_generic_splits(a.n_splits);"):
        assert cond in form, cond
    assert "(n_splits > 4 ? 4 : n_splits)" in _function_body(src, "int paged_attention_generic_splits(int n_splits) {")
    # the dev knobs of the family are read in attn_form and nowhere else
    sources = [os.path.join(d, f) for d, _, fs in os.walk(csrc) for f in fs if f.endswith((".hip", ".cuh", ".h", ".inc"))]
    assert any(os.path.dirname(p) != csrc for p in sources)   # the experimental includes are among them
    for p in sources:
        text = open(p).read()
        text = text.replace(form, "") if p == os.path.join(csrc, "attention.hip") else text
        assert 'QS_DEV_KNOB("QSPEC_ATTN_' not in text, p
    assert form.count('QS_DEV_KNOB("QSPEC_ATTN_') == 5
