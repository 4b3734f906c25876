"""Every GEMM dispatch row (tests/gemm_cases.py) against a float64 reference, on both data tiers, through `ops`.

Every call writes into a NaN-prefilled output that sits in a flat buffer with a guard row and guard elements behind it:
an element no kernel writes fails the bar, a write past the last element changes the guard.  Every call runs twice and
must give the same bits (the split-K merges included)."""
import numpy as np
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD16, GUARD32 = 0x7E5A, 0x7FC0DEAD   # NaN payloads no kernel produces
STATS = {}   # (row, tier) -> [max ulps, correctly rounded count, element count, sum of signed errors]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from qspec_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(shape, dtype):
    """(out view, flat buffer, guard start): out prefilled with NaN (or a poison int), one guard row + 64 elements behind."""
    n = int(np.prod(shape))
    extra = shape[-1] + 64
    if dtype == torch.float16:
        flat = torch.full((n + extra,), float("nan"), dtype=dtype, device=DEV)
        flat[n:].view(torch.int16).fill_(GUARD16)
    elif dtype == torch.float32:
        flat = torch.full((n + extra,), float("nan"), dtype=dtype, device=DEV)
        flat[n:].view(torch.int32).fill_(GUARD32)
    else:
        flat = torch.full((n + extra,), -0x55555556, dtype=dtype, device=DEV)
        flat[n:].fill_(GUARD32)
    return flat[:n].view(*shape), flat, n


def _guard_intact(flat, n):
    g = flat[n:].view(torch.int16 if flat.dtype == torch.float16 else torch.int32).cpu().numpy()
    want = GUARD16 if flat.dtype == torch.float16 else GUARD32
    return bool((g == want).all())


def _call(ops, case, d, t, out):
    M, N, K = case.M, case.N, case.K
    if case.op == "a4":
        ops.rowwise_scaled_linear_cutlass_s4s4_unified(t["xq"], t["xs"], t["wq"], t["ws"], t.get("bias"), out)
    elif case.op == "w16":
        ops.w4a16_linear(t["x"], t["wq"], t["ws"], out, t.get("bias"))
    elif case.op == "f16":
        ops.linear_f16(t["x"], t["w"], out)
    elif case.op == "a4.ipart":
        ops.rowwise_scaled_linear_s4s4_partial(t["xq"], t["wq"], out, out.shape[0])
    elif case.op == "w16.partial_raw":
        ops.w4a16_linear_partial(t["x"], t["wq"], out, out.shape[0])
    elif case.op == "w16.ksliced_raw":
        ops.w4a16_linear_ksliced_raw(t["x"], t["wq"], out, case.k0, case.k1)
    else:
        raise ValueError(case.op)


def run_case(ops, case, tier):
    """Inputs, two calls (same bits), guard check.  Returns (output as numpy, data dict)."""
    d = G.make_data(case, tier)
    t = {k: dev(v) for k, v in d.items() if k in ("xq", "xs", "wq", "ws", "x", "w", "bias")}
    M, N, K = case.M, case.N, case.K
    if case.op == "a4.ipart":
        S = G.a4_ipart_slices(M, N, K)
        shape, dtype = (S, M, N), torch.int32
    elif case.op == "w16.partial_raw":
        S = G.w16_linear_partial_slices(M, N, K)
        shape, dtype = (S, M, N), torch.float32
    elif case.op == "w16.ksliced_raw":
        shape, dtype = (M, N), torch.float32
    else:
        shape, dtype = (M, N), torch.float16
    outs = []
    for _ in range(2):
        out, flat, n = _guarded(shape, dtype)
        _call(ops, case, d, t, out)
        torch.cuda.synchronize()
        assert _guard_intact(flat, n), f"{case.id} {tier}: a write past the output"
        outs.append(out.cpu().numpy())
    u = np.uint16 if dtype == torch.float16 else np.uint32
    assert np.array_equal(outs[0].view(u), outs[1].view(u)), f"{case.id} {tier}: a second call gave other bits"
    return outs[0], d


def _check(case, tier, out, d):
    label = f"{case.id} {tier}"
    if case.op in ("a4.ipart", "w16.partial_raw"):
        # each slice against the float64 sum of its own K range, then the slices' sum
        S = out.shape[0]
        Ks = case.K // S
        for s in range(S):
            ds = dict(d)
            if case.op == "a4.ipart":
                ds["ref"] = G._dot_rows(G._f64(G.unpack_i4(d["xq"][:, s * Ks // 2:(s + 1) * Ks // 2])),
                                        lambda n0, n1: G._f64(G.unpack_i4(d["wq"][n0:n1, s * Ks // 2:(s + 1) * Ks // 2])), case.N)[0]
            else:
                xs_ = d["x"][:, s * Ks:(s + 1) * Ks]
                ws_ = d["wq"][:, s * Ks // 2:(s + 1) * Ks // 2]
                ds["ref"] = G.ref_w4a16_raw(xs_, ws_)
                ds["abs"] = G._dot_rows(np.abs(G._f64(xs_)), lambda n0, n1: np.abs(G._f64(G.unpack_i4(ws_[n0:n1]))), case.N)[0]
            G.check_raw(out[s], ds, f"{label} slice {s}")
        return
    if case.op == "w16.ksliced_raw":
        G.check_raw(out, d, label)
        return
    mx, crf, se = G.check_f16(out, d, label)
    for row in set(case.rows):
        st = STATS.setdefault((row, tier), [0.0, 0, 0, 0.0])
        st[0] = max(st[0], mx)
        st[1] += int(round(crf * out.size))
        st[2] += out.size
        st[3] += float(se.sum())


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_gemm_case(ops, case):
    for tier in ("exact", "realistic"):
        out, d = run_case(ops, case, tier)
        _check(case, tier, out, d)


def test_bias_through_the_linear_method(ops):
    """QSpecLinearMethod.apply(layer, x, bias) for a W4A4 and a W4A16 layer (vLLM models with biased projections)."""
    from qspec_amd.quantization import QSpecLinearMethod
    from qspec_amd.quarot_nn import PackedQuantizedTensor
    for case in (G.Case("a4", 5, 6144, 4096, "mixed"), G.Case("w16", 5, 6144, 4096, "mixed"),
                 G.Case("w16", 24, 12288, 1024, "dominant")):
        for tier in ("exact", "realistic"):
            d = G.make_data(case, tier)
            layer = torch.nn.Module()
            layer.weight = torch.nn.Parameter(dev(d["wq"]), requires_grad=False)
            layer.weight_scales = torch.nn.Parameter(dev(d["ws"].reshape(-1, 1)), requires_grad=False)
            method = QSpecLinearMethod(None)
            if case.op == "a4":
                x = PackedQuantizedTensor(dev(d["xq"]), dev(d["xs"].reshape(-1, 1)))
            else:
                x = dev(d["x"])
            out = method.apply(layer, x, dev(d["bias"]))
            torch.cuda.synchronize()
            G.check_f16(out.cpu().numpy(), d, f"apply {case.id} {tier}")


def test_shared_workspace_across_slice_and_block_counts(ops):
    """One stream, one workspace: calls with different K-slice and block counts interleaved, then the first again --
    same bits; the ticket counters at the front of the workspace end all zero."""
    seq = [G.Case("w16", 1, 256, 14336), G.Case("w16", 16, 4112, 1536), G.Case("w16", 17, 128, 768),
           G.Case("w16", 1, 64, 8192, "mixed"), G.Case("w16", 32, 12288, 4096, "cancel"), G.Case("w16", 2, 128, 13824),
           G.Case("w16", 16, 12288, 4096, "dominant")]
    assert [c.rows[0] for c in seq] == ["w16.partial(4)", "w16.partial(3)", "w16.tiled(1,S)", "w16.gen2d(1,S)",
                                        "w16.gen2d(2,S)", "w16.partial(3)", "w16.gen2d(1,S)"]
    data = [G.make_data(c, "realistic") for c in seq]
    args = [(dev(d["x"]), dev(d["wq"]), dev(d["ws"]), dev(d["bias"]) if "bias" in d else None) for d in data]
    outs = []
    for c, (x, wq, ws_, b) in zip(seq + seq[:1], args + args[:1]):   # enqueued back to back, read afterwards
        outs.append(torch.full((c.M, c.N), float("nan"), dtype=torch.float16, device=DEV))
        ops.w4a16_linear(x, wq, ws_, outs[-1], b)
    torch.cuda.synchronize()
    for c, d, out in zip(seq, data, outs):
        G.check_f16(out.cpu().numpy(), d, c.id)
    assert np.array_equal(outs[0].cpu().numpy().view(np.uint16), outs[-1].cpu().numpy().view(np.uint16))
    ws = ops.w4a16_workspace(torch.device(DEV))
    torch.cuda.synchronize()
    assert int(ws[:G.W16_CNT_BYTES].view(torch.int32).abs().max().item()) == 0


def test_rounding_bias_per_row(ops):
    """Mean signed error over all of a row's realistic-tier elements within 0.02 + 1.2 / sqrt(n) ulps; prints the
    per-row table (max ulps, fraction correctly rounded, mean signed error) of both tiers."""
    for case in G.CASES:   # rows whose cases did not run in this session (a -k selection)
        if case.op in ("a4", "w16", "f16") and any((r, "realistic") not in STATS for r in case.rows):
            for tier in ("exact", "realistic"):
                out, d = run_case(ops, case, tier)
                _check(case, tier, out, d)
    lines, bad = [], []
    for row in G.ROWS:
        for tier in ("exact", "realistic"):
            if (row, tier) not in STATS:
                continue
            mx, ncr, n, sse = STATS[(row, tier)]
            mean = sse / n
            lines.append(f"{row:22s} {tier:9s} n={n:9d} max={mx:5.3f} ulp  cr={ncr / n:8.6f}  mean={mean:+.5f} ulp")
            if tier == "realistic" and abs(mean) > G.bias_bar(n):
                bad.append((row, mean, G.bias_bar(n)))
    print("\n" + "\n".join(lines))
    assert not bad, bad
