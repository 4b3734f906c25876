"""CPU checks of tests/hadamard_cases.py: the restated dispatch reaches every reachable row, every built row has the property
it was built for, the float64 reference equals the oracle on the exact tier (and stays within the measured distance on the
realistic one), reproduces the golden transforms, and every named fault is caught on every row it applies to."""
import functools
import os

import numpy as np
import pytest

import hadamard_cases as hc

CASES = hc.cases()
EXACT = [c for c in CASES if c.tier == "exact"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@functools.lru_cache(maxsize=None)
def built(i):
    c = CASES[i]
    dt = hc.build(c)          # (asserts the placement of every built row on the reference)
    return dt, hc.reference(c, dt)


def index(c):
    return CASES.index(c)


def test_route_reaches_every_reachable_row():
    reach = {}
    for c in CASES:
        for entry, mode, row in c.routes():
            assert isinstance(row, str) and row in hc.ALL_ROWS, (c.id, entry, mode, row)
            reach.setdefault(row, []).append(f"{c.id}[{mode}]")
    print()
    for row in hc.ALL_ROWS:
        if row in hc.UNREACHABLE:
            print(f"{row:40s} unreachable: {hc.UNREACHABLE[row]}")
        else:
            ids = reach.get(row, [])
            print(f"{row:40s} {len(ids):3d}  {' '.join(ids[:6])}{' ...' if len(ids) > 6 else ''}")
    assert not [r for r in hc.ALL_ROWS if r not in hc.UNREACHABLE and r not in reach]
    assert not [r for r in hc.UNREACHABLE if r in reach]
    # every smh row in all of its modes; both tiers on every row
    for row, ids in reach.items():
        if row.startswith("smh."):
            want = {"q", "f16"} | ({"xp"} if "gate" not in row else set())
            assert want <= {i[i.index("[") + 1:-1] for i in ids}, (row, ids)
        assert any("-exact[" in i for i in ids), row
        assert any("-realistic[" in i for i in ids), row


def test_token_boundaries_of_the_spread_forms():
    r = lambda T, I, K: hc.route("mlp_hadamard", T=T, I=I, K=K, ws=True, quant=True)
    assert [r(T, 28672, 28) for T in (16, 17)] == ["smh.spread28(P1024,NB16)", "smh.one(EPL16,KH28,preact)"]
    assert [r(T, 14336, 28) for T in (32, 33)] == ["smh.spread28(P512,NB8)", "smh.one(EPL8,KH28,preact)"]
    assert [r(T, 13824, 108) for T in (16, 17, 32, 33)] == ["smh.spread108(P128,NB16)", "smh.spread108(P128,NB8)",
                                                            "smh.spread108(P128,NB8)", "smh.one(EPL2,KH0,preact)"]
    assert [r(T, 14336, 28) for T in (256, 257)] == ["smh.one(EPL8,KH28,preact)"] * 2
    h = lambda T, q: hc.route("heads_hadamard_merge", T=T, heads=32, d=128, S=2, quant=q)
    assert [h(128, False), h(129, False), h(2, True)] == ["hhm.spread32(f16)", "hhm.merge(NH32,f16)", "hhm.merge(NH32,quant)"]
    have = {(c.entry, c.T, c.dims.get("I"), c.ws) for c in CASES}
    for T, I in ((16, 28672), (17, 28672), (32, 14336), (33, 14336), (16, 13824), (17, 13824), (32, 13824), (33, 13824),
                 (256, 14336), (257, 14336)):
        assert ("mlp", T, I, True) in have, (T, I)
    assert [(T, I, K) for T, I, K in hc.HISTORY] and [r(T, I, K) for T, I, K in hc.HISTORY] == [
        "smh.spread28(P512,NB8)", "smh.spread28(P1024,NB16)", "smh.spread108(P128,NB8)", "smh.one(EPL16,KH28,preact)",
        "smh.spread108(P128,NB16)", "smh.spread28(P512,NB8)"]


def test_refused_shapes_and_supported_queries():
    for entry, kw, code in hc.REFUSED:
        assert hc.route(entry, **kw) == code, (entry, kw)
    assert hc.route("fwht", rows=0, N=3) == "noop"
    for T in (0, 1, 16, 17, 32, 33, 128, 129):
        for heads, d, K in ((32, 128, 1), (40, 128, 40), (24, 128, 12), (64, 128, 1), (32, 64, 1), (80, 128, 40), (36, 128, 12)):
            if T:
                ok = isinstance(hc.route("heads_hadamard_merge_spread", T=T, heads=heads, d=d, S=1), str)
                assert ok == hc.heads_merge_spread_supported(T, heads, d)
                if K > 1:
                    ok = isinstance(hc.route("heads_hadamard_mix_merge_spread", T=T, heads=heads, d=d, K=K, S=1, amax=False), str)
                    assert ok == hc.heads_mix_merge_spread_supported(T, heads, d, K)
        for I, K in ((14336, 28), (28672, 28), (13824, 108), (57344, 28), (5632, 44), (1792, 28), (2048, 1), (24576, 12)):
            if T and hc.mlp_xp_supported(T, I, K):     # what the query promises, the entry launches
                assert isinstance(hc.route("mlp_hadamard", T=T, I=I, K=K, ws=True, quant=False, xp=True), str), (T, I, K)


@pytest.mark.parametrize("c", EXACT, ids=lambda c: c.id)
def test_built_rows_and_oracle_on_the_exact_tier(oracle, c):
    """build() asserts every row's property; the oracle gives the float64 reference's bits on this tier."""
    dt, ref = built(index(c))
    assert np.array_equal(bits(hc.oracle_rows(oracle, c, dt)), bits(ref["f16"])), c.id
    keep = hc.quant_tokens(dt)
    for key, (q, s) in ((k, v) for k, v in ref.items() if isinstance(k, tuple)):
        q0, s0 = oracle.rowabsmax_quant_i4(ref["f16"][keep], key[1])
        assert np.array_equal(q0, q[keep]) and np.array_equal(bits(s0), bits(s[keep])), (c.id, key)
    if c.gate:
        assert np.array_equal(bits(hc.ref_silu_mul(dt.gate_up, c.dims["I"])), bits(dt.x))
        assert np.array_equal(bits(oracle.silu_mul(dt.gate_up, c.dims["I"])), bits(dt.x))
    if "xp" in c.modes:     # the tile is a permutation of the rows
        T, n = ref["f16"].shape
        off = hc.xp_offsets(T, n).reshape(-1)
        assert len(np.unique(off)) == T * n and off.max() < ref["xp"].size
        assert np.array_equal(bits(ref["xp"][off]), bits(ref["f16"]).reshape(-1))
    with np.errstate(invalid="ignore"):
        if any(k == "over" for k in dt.kinds):
            assert np.isinf(ref["f16"].astype(np.float64)).any(), c.id
        if any(k == "sub" for k in dt.kinds):
            z = np.abs(ref["f16"][dt.kinds.index("sub")].astype(np.float64))
            assert ((z > 0) & (z < 2.0 ** -14)).any(), c.id


FAMILY = {"fwht": "fwht", "hadk_mix": "hadk_mix", "mlp": "mlp", "rq": "rq"}


def test_oracle_distance_on_the_realistic_tier(oracle):
    """max |oracle - reference| / max |oracle| per family and the fraction of fp16 values that differ: printed, and held
    against the constants recorded in hadamard_cases.ORACLE_DIST."""
    worst = {}
    silu = [0, 0]
    for i, c in enumerate(CASES):
        if c.tier != "realistic":
            continue
        dt, ref = built(i)
        if c.gate:
            silu[0] += int((bits(oracle.silu_mul(dt.gate_up, c.dims["I"])) != bits(dt.x)).sum())
            silu[1] += dt.x.size
        o = hc.oracle_rows(oracle, c, dt).astype(np.float64)
        r = ref["f16"].astype(np.float64)
        dist = np.abs(o - r).max() / max(np.abs(o).max(), 1e-30)
        frac = float((bits(ref["f16"]) != bits(hc.oracle_rows(oracle, c, dt))).mean())
        fam = FAMILY.get(c.entry, "heads")
        w = worst.get(fam, (0.0, 0.0, ""))
        worst[fam] = (max(w[0], dist), max(w[1], frac), c.id if dist >= w[0] else w[2])
    print()
    for fam, (dist, frac, cid) in sorted(worst.items()):
        print(f"ORACLE_DIST[{fam!r}] = {dist:.3e}   (differing fp16 values: at most {frac:.2%}; worst case {cid})")
    print(f"SILU_DIFF = {silu[0] / silu[1]:.3e}   ({silu[0]} of {silu[1]} values of silu_mul differ)")
    for fam, (dist, frac, cid) in sorted(worst.items()):
        assert dist <= hc.ORACLE_DIST[fam], (fam, dist, cid)
    assert silu[0] / silu[1] <= hc.SILU_DIFF


def test_reference_reproduces_the_golden_transforms(golden_dir):
    g = np.load(os.path.join(golden_dir, "hadamard.npz"))
    from qspec_amd import hadamard_tables
    for n in (32, 512, 14336, 28672, 13824, 40, 80):
        hadK, K = hadamard_tables.get_hadK(n)
        had = np.array(g[f"had{K}"], np.float64) if K > 1 else None
        assert K == 1 or np.array_equal(had @ had.T, K * np.eye(K))
        x = g[f"x_{n}"]
        w = hc.wht(x.reshape(x.shape[0], K, n // K))
        y = (np.einsum("ik,tkj->tij", had, w) if K > 1 else w).reshape(x.shape[0], n) / np.sqrt(n)
        # (the golden rows went through the reference's fp32 tables and scale: 2^-23 of the largest value per step)
        assert np.allclose(y, g[f"y_{n}"], rtol=0, atol=1e-6 * np.abs(g[f"y_{n}"]).max()), n
    # and the one-hot statement the built rows rest on: the preimage of e_j is a +-1 row whose image is one spike of K P
    for K, P in ((28, 512), (108, 128), (1, 64)):
        had = hc.table(K)
        for e in (0, K * P - 1, (K * P) // 3):
            i, j = divmod(e, P)
            pre = np.kron(had[i] if had is not None else np.ones(1), hc.sylvester_row(j, P))
            w = hc.wht(pre.reshape(1, K, P))
            z = (np.einsum("ik,tkj->tij", had, w) if K > 1 else w).reshape(-1)
            assert set(np.abs(pre)) == {1.0} and z[e] == K * P and np.count_nonzero(z) == 1


def test_every_named_fault_is_caught_on_every_row_it_applies_to():
    """For every row, every fault that applies to it (and, for the block faults, every owner block) changes what at least one
    exact-tier case of that row compares."""
    todo = {}       # (row, mode, fault, block) -> caught
    by_case = {}
    for i, c in enumerate(CASES):
        if c.tier != "exact":
            continue
        for entry, mode, row in c.routes():
            for fault in hc.FAULTS:
                for b in hc.fault_blocks(c, fault, mode):
                    todo.setdefault((row, mode, fault, b), False)
                    by_case.setdefault(i, set()).add((row, mode, fault, b))
    for i, keys in by_case.items():
        c = CASES[i]
        dt, ref = built(i)
        memo = {}
        for key in sorted(keys):
            row, mode, fault, b = key
            if todo[key]:
                continue
            if (fault, b) not in memo:
                memo[(fault, b)] = hc.reference(c, dt, fault, b)
            todo[key] = hc.differs(c, dt, ref, memo[(fault, b)], mode)
    missed = [k for k, v in todo.items() if not v]
    print(f"\n{len(todo)} (row, mode, fault, block) combinations, {len(missed)} not caught")
    for fault in hc.FAULTS:
        rows = sorted({k[0] for k in todo if k[2] == fault})
        print(f"  {fault:22s} applies to {len(rows):3d} rows")
    assert not missed, missed[:20]
