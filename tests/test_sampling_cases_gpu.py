"""sample_top_k_top_p (csrc/sampler.hip: topk_hist_kernel, topk_select_kernel<MINP>, topk_write_kernel<SEEDED>,
topk_token_kernel) against the float64 reference of tests/sampling_cases.py on its case matrix: every row has a boundary of
the selection where the kernel's walk over key positions branches (a thread's first / last key, a wave edge, runs of empty
threads, groups of equal logits, signed zeros, top_p = 1 over 60 nats).  Per row: the kept set `probs > 0` EQUAL to the
reference's (no boundary-group allowance: the parameters sit 1e-4 / 1e-3 away from every group), |probs - ref| <= PROB_BAR
(the measured oracle-to-float64 distance x 4, tests/test_sampling_cases.py), the row sum within 1e-5 of 1, the token equal.
The entry points -- plain, min_p, seeded with no sequence seeded, seeded + min_p -- agree bit for bit; a row's bits do not
depend on its neighbours, its row index or on what the workspace served before; the histogram is left zeroed."""
import numpy as np
import pytest
import torch

import sampling_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = sc.batches()
BATCH_IDS = [f"V{b[0].V}x{len(b)}-{b[0].name}" for b in BATCHES]
WHERE = {c.name: (i, j) for i, b in enumerate(BATCHES) for j, c in enumerate(b)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from qspec_amd import ops
    return ops


def _sample(ops, arrays, form, rows=None, ws=None):
    """One call of the entry point `form` on the rows `rows` of a batch -> (probs [n, V] fp32, token [n] int64, workspace).
    The outputs are pre-filled with -1: an element the kernels do not write shows as a negative probability."""
    lg, temp, top_k, top_p, min_p, E = [a if a is None or rows is None else a[rows] for a in arrays]
    n, V = lg.shape
    probs = torch.full((n, V), -1.0, dtype=torch.float32, device=DEV)
    tok = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    ws = ops.new_sample_workspace(n, DEV) if ws is None else ws
    kw = {}
    if "min_p" in form:
        kw["min_p"] = dev(min_p)
    if "seeded" in form:        # no sequence is seeded: E is injected, and every row is the engine-stream row
        kw.update(seq_seeds=torch.zeros(n, dtype=torch.int64, device=DEV), seq_seeded=torch.zeros(n, dtype=torch.int32, device=DEV),
                  base_pos=torch.zeros(n, dtype=torch.int32, device=DEV))
    ops.sample_top_k_top_p(dev(lg), probs, tok, dev(temp), dev(top_k), None if top_p is None else dev(top_p), exponential=dev(E),
                           workspace=ws, **kw)
    return host(probs), host(tok), ws


@pytest.fixture(scope="module")
def results(ops):
    """Every batch once through the min_p entry (the one form every case can take): batch index -> (probs, token)."""
    return [_sample(ops, sc.batch_arrays(b), "min_p")[:2] for b in BATCHES]


@pytest.mark.parametrize("case", sc.cases(), ids=[c.name for c in sc.cases()])
def test_selection_matches_the_float64_reference(results, case):
    i, j = WHERE[case.name]
    probs, tok = results[i]
    bad = sc.check_row(case.ref, probs[j], tok[j])
    err = float(np.abs(probs[j].astype(np.float64) - case.ref.probs).max())
    print(f"{case.name}: kept {(probs[j] > 0).sum()} / ref {case.ref.nonzero.sum()}, |dp| {err:.3g}, token {tok[j]} / ref {case.ref.token}")
    assert not bad, (case.name, bad)


def _same_bits(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: probs differ in rows " \
        f"{np.flatnonzero((got[0].view(np.uint32) != want[0].view(np.uint32)).any(1))}"
    assert np.array_equal(got[1], want[1]), f"{what}: tokens {got[1]} != {want[1]}"


@pytest.mark.parametrize("b", range(len(BATCHES)), ids=BATCH_IDS)
def test_entry_points_agree_bit_for_bit(ops, results, b):
    """plain and seeded (no min_p array) on the rows without a min_p, seeded + min_p on all: the bits of the min_p entry."""
    arrays = sc.batch_arrays(BATCHES[b])
    base = results[b]
    off = np.flatnonzero(arrays[4] == 0.0)
    if off.size:
        sub = (base[0][off], base[1][off])
        _same_bits(_sample(ops, arrays, "plain", off), sub, "plain")
        _same_bits(_sample(ops, arrays, "seeded", off), sub, "seeded")
        zeros = list(arrays)
        zeros[4] = np.zeros_like(arrays[4])
        _same_bits(_sample(ops, zeros, "min_p", off), sub, "min_p = 0")
    _same_bits(_sample(ops, arrays, "seeded_min_p"), base, "seeded + min_p")


@pytest.mark.parametrize("b", range(len(BATCHES)), ids=BATCH_IDS)
def test_rows_are_independent_and_the_histogram_is_left_zeroed(ops, results, b):
    arrays = sc.batch_arrays(BATCHES[b])
    base = results[b]
    n = len(BATCHES[b])
    perm = np.roll(np.arange(n)[::-1], 3)                       # every row at another index, next to other neighbours
    pr, tk, ws = _sample(ops, arrays, "min_p", perm)
    _same_bits((pr, tk), (base[0][perm], base[1][perm]), "permuted rows")
    hist = ws[:n * 65536 * 4].view(torch.int32)
    assert int(hist.abs().max().item()) == 0, "the histogram is not left zeroed"
    _same_bits(_sample(ops, arrays, "min_p", ws=ws)[:2], base, "second call on the same workspace")
    assert int(hist.abs().max().item()) == 0, "the histogram is not left zeroed by the second call"
