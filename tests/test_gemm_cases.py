"""The GEMM case matrix itself (no GPU): it reaches every dispatch row, its dispatch rule agrees with the library's own
host-side predicates, its float64 references agree with the oracle, its exact tier keeps every fp32 partial sum exact,
and its bars reject the kernel faults they are there to catch."""
from collections import Counter
from itertools import product

import numpy as np
import pytest

import gemm_cases as G


def test_cases_reach_every_row():
    reached = Counter(r for c in G.CASES for r in set(c.rows))
    assert set(reached) == set(G.ROWS), (set(G.ROWS) - set(reached), set(reached) - set(G.ROWS))
    thin = {r: n for r, n in reached.items() if n < 2}
    assert not thin, thin
    biased = {r for c in G.CASES if c.bias for r in c.rows}
    assert G.BIAS_ROWS <= biased, G.BIAS_ROWS - biased
    assert len({c.id for c in G.CASES}) == len(G.CASES)


def test_cases_cover_the_edges():
    ks_a4 = {c.K for c in G.CASES if c.rows[0] in ("a4.stream1", "a4.stream2", "a4.longk")}
    assert ks_a4 >= {128 * nw * ub for nw, ub in G.A4_STREAM_SHAPES} | {28672}
    ks_w16 = {c.K for c in G.CASES if c.rows[0].startswith("w16.stream16")}
    assert ks_w16 == {128 * nw * ub for nw, ub in G.W16_STREAM_SHAPES}
    # a tile count the 256-workgroup cap splits unevenly, on every streaming family
    for fam in ("a4.longk", "a4.stream1", "a4.stream2", "w16.stream16", "w16.partial", "f16.stream", "f16.longk"):
        assert any(c.rows[0].startswith(fam) and (c.N // 16) > 256 and (c.N // 16) % 256 for c in G.CASES), fam
    # N not a multiple of 16 on the first-generation fp16 kernel, at M <= 16 and above
    assert any(c.rows[0] == "f16.gen1" and c.N % 16 for c in G.CASES)
    assert any("f16.gen2" in c.rows and c.N % 16 for c in G.CASES)
    # 33..64 rows and a remainder pass on the W4A4 first-generation kernel
    assert any(c.rows == ("a4.gen4", "a4.gen1") for c in G.CASES)
    # the smallest and largest M of each M range
    Ms = {c.M for c in G.CASES}
    assert Ms >= {1, 16, 17, 32, 33, 64, 65}


def test_pack_unpack_match_the_oracle(oracle):
    rng = np.random.default_rng(0)
    q = rng.integers(-8, 8, (7, 256)).astype(np.int8)
    q[0, :4] = (-8, 7, 7, -8)
    q[1] = -8
    q[2] = 7
    p = G.pack_i4(q)
    assert np.array_equal(p, oracle.pack_i4(q))
    assert np.array_equal(G.unpack_i4(p), q)
    assert np.array_equal(oracle.unpack_i4(p), q)
    b = np.arange(256, dtype=np.uint8).view(np.int8).reshape(1, 256)   # every byte value
    assert np.array_equal(G.unpack_i4(b), oracle.unpack_i4(b))


def _grid():
    Ms = (1, 2, 4, 15, 16, 17, 20, 31, 32, 33, 48, 64, 65, 100, 130, 200, 423, 512)
    Ns = (16, 48, 64, 128, 192, 4096, 4112, 6144, 12288, 14336, 16384, 28672)
    Ks = (128, 384, 512, 768, 1024, 1408, 1536, 2048, 3584, 4096, 4608, 5120, 5632, 7168, 8192, 8320, 9216, 10240,
          13824, 14336, 28672)
    return product(Ms, Ns, Ks)


def test_route_agrees_with_the_library_predicates():
    from qspec_amd import _lib
    lib = _lib.load()
    for M, N, K in _grid():
        assert bool(lib.qspec_rowwise_scaled_linear_s4s4_residual_supported(M, N, K)) == G.a4_stream_supported(M, N, K), (M, N, K)
        assert (G.route("a4", M, N, K)[0] in ("a4.stream1", "a4.stream2", "a4.longk")) == G.a4_stream_supported(M, N, K)
        assert lib.qspec_rowwise_scaled_linear_s4s4_partial_slices(M, N, K) == G.a4_ipart_slices(M, N, K), (M, N, K)
        S = lib.qspec_w4a16_linear_partial_slices(M, N, K)
        assert S == G.w16_linear_partial_slices(M, N, K), (M, N, K)
        row = G.route("w16", M, N, K)[0]
        if row.startswith("w16.partial("):
            assert row == f"w16.partial({S})", (M, N, K, row, S)
        if row.startswith("w16.tiled("):
            assert row.endswith(",S)") == (S > 1), (M, N, K, row, S)
        for op in ("a4", "w16", "f16"):
            for bias in ((False, True) if op != "f16" else (False,)):
                for r in G.route(op, M, N, K, bias):
                    assert r in G.ROWS, (op, M, N, K, bias, r)
                    if bias:
                        assert r in G.BIAS_ROWS, (op, M, N, K, r)


@pytest.mark.parametrize("op,M,N,K,bias", [("a4", 3, 48, 256, True), ("a4", 20, 64, 512, False),
                                           ("w16", 3, 48, 256, True), ("w16", 17, 32, 640, False),
                                           ("f16", 5, 40, 256, False), ("f16", 18, 24, 512, False)])
def test_references_agree_with_the_oracle(oracle, op, M, N, K, bias):
    c = G.Case(op, M, N, K, "mixed" if bias else "")
    for tier in ("exact", "realistic"):
        d = G.make_data(c, tier)
        if op == "a4":
            o = oracle.gemm_w4a4(d["xq"], d["xs"], d["wq"], d["ws"], d.get("bias"))
        elif op == "w16":
            o = oracle.gemm_w4a16(d["x"], d["wq"], d["ws"], d.get("bias"))
        else:
            o = oracle.gemm_f16(d["x"], d["w"])
        # the oracle sums in double and rounds through fp32: its own error is within the bars
        G.check_f16(o, d, f"oracle {c.id} {tier}")


def test_exact_tier_keeps_every_partial_sum_exact():
    """By construction for every case (|x| <= R, |w| <= 8; |x|, |w| <= A / 8, A / 16), and measured on the small ones."""
    for c in G.CASES:
        if c.op in ("a4", "a4.ipart"):
            continue   # integer products, int32 sums
        if c.op == "f16":
            A = max(1, min(32, int(np.sqrt((1 << 24) // c.K)) - 1))
            assert c.K * A * A < 2 ** 24, c.id
        else:
            assert 8 * G.exact_w4a16_range(c.K) * c.K < 2 ** 22, c.id
        if c.N * c.K <= 1 << 22:
            d = G.make_data(c, "exact")
            assert G.exact_budget_ok(d), c.id
            raw = d["ref"]
            if c.op == "w16":
                raw = (raw - (d["bias"].astype(np.float64) if "bias" in d else 0)) / d["ws"].astype(np.float64)
            if c.K >= 1024:   # the sums need more significant bits than fp16 has
                assert np.abs(raw).max() / d["u"] > 2 ** 11, c.id


# ------------------------------------------------------------------ the bars have teeth

def _kernel(d, mode, S=4):
    """A numpy W4A16 'kernel' (fp32 sums, scale, bias add, fp16 store) with one deliberate fault."""
    x = d["x"].astype(np.float32)
    w = G.unpack_i4(d["wq"]).astype(np.float32)
    ws = d["ws"].astype(np.float32)
    b = d["bias"].astype(np.float32) if "bias" in d else None
    K = x.shape[1]
    if mode == "drop_chunk":
        x = x.copy()
        x[:, 48:64] = 0
    if mode == "scale_first":   # h(s w) before the sum: the reference's BitBLAS order
        acc = x @ (w * ws[:, None]).astype(np.float16).astype(np.float32).T
        v = acc
    else:
        parts = [x[:, s * K // S:(s + 1) * K // S] @ w[:, s * K // S:(s + 1) * K // S].T for s in range(S)]
        if mode == "fp16_partial":
            parts = [p.astype(np.float16).astype(np.float32) for p in parts]
        acc = parts[0]
        for p in parts[1:]:
            acc = acc + p
        v = acc * ws
    if b is not None:
        v = v + (S * b if mode == "bias_per_slice" else b)
    h = v.astype(np.float16)
    if mode == "truncate":
        over = np.abs(h.astype(np.float32)) > np.abs(v)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h


_TEETH_CASES = (G.Case("w16", 8, 256, 4096, "mixed"), G.Case("w16", 16, 128, 14336, "dominant"), G.Case("w16", 4, 512, 2048))


@pytest.mark.parametrize("tier", ["exact", "realistic"])
def test_a_correct_kernel_passes_the_bars(tier):
    for c in _TEETH_CASES:
        G.check_f16(_kernel(G.make_data(c, tier), "none"), G.make_data(c, tier), c.id)


@pytest.mark.parametrize("mode", ["truncate", "drop_chunk", "bias_per_slice", "scale_first", "fp16_partial"])
def test_the_bars_reject_a_faulty_kernel(mode):
    for c in _TEETH_CASES:
        if mode == "bias_per_slice" and not c.bias:
            continue
        for tier in ("exact", "realistic"):
            if mode in ("scale_first", "fp16_partial") and tier == "realistic":
                continue   # below the realistic tier's summation budget by design; the exact tier catches them
            d = G.make_data(c, tier)
            with pytest.raises(AssertionError):
                G.check_f16(_kernel(d, mode), d, c.id)


def test_the_rounding_bias_bar_rejects_a_biased_kernel():
    """Rounding toward +inf on every store passes a max-error bar but not the mean signed error over a row."""
    c = G.Case("w16", 16, 512, 4096)
    d = G.make_data(c, "realistic")
    _, se, _ = G.errors(_kernel(d, "none"), d["ref"])
    assert abs(se.mean()) <= G.bias_bar(se.size)
    x = d["x"].astype(np.float32) @ G.unpack_i4(d["wq"]).astype(np.float32).T * d["ws"].astype(np.float32)
    up = x.astype(np.float16)
    up = np.where(up.astype(np.float32) < x, np.nextafter(up, np.float16(np.inf)), up)
    _, se2, _ = G.errors(up, d["ref"])
    assert abs(se2.mean()) > G.bias_bar(se2.size)
