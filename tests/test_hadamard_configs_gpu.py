"""Every launch form of hadamard.hip and of the row-absmax quantiser against tests/hadamard_cases.py: the exact tier bit for
bit against the float64 reference, the realistic tier against the oracle's bits (merge forms with unequal maxima:
hadamard_cases.MERGE_BAR), on rows built to put the row maximum into every workgroup's and wave's share.

These cases strictly contain the random-row tests of test_kernels_gpu.py (test_hadamard_mix_bit_exact,
test_heads_hadamard_bit_exact, test_silu_mul_hadamard_bit_exact, test_heads_hadamard_mix_bit_exact and the one-split half of
test_spread_table_factor_head_transform_bit_exact_on_given_partials): same entries, same bar, their shapes among the cases
here.  Those tests stay."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import hadamard_cases as hc
from test_kernels_gpu import _attn_partials_ws     # given partials in an attention workspace (not copied)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = hc.cases()


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def of(entry):
    return [c for c in CASES if c.entry == entry]


@functools.lru_cache(maxsize=None)
def _built(i):
    return hc.build(CASES[i])


def expected(oracle, c):
    """(dt, want, merge_bar): want as hadamard_cases.reference gives it -- the float64 reference on the exact tier, the
    oracle's bits on the realistic one; merge_bar: None, or the absolute bar of a merge form with unequal maxima."""
    dt = _built(CASES.index(c))
    if c.tier == "exact":
        return dt, hc.reference(c, dt), None
    merge = dt.o is not None
    if c.gate:      # the oracle's own SiLU (1.5e-4 of its values differ from the float64 one: hadamard_cases.SILU_DIFF)
        dt = dataclasses.replace(dt, x=oracle.silu_mul(dt.gate_up, c.dims["I"]))
    z = hc.oracle_rows(oracle, c, dt)
    want = {"f16": z}
    block_of, nb = c.owners()
    if "q" in c.modes:
        for clip in (1.0, c.clip2):
            want[("q", clip)] = oracle.rowabsmax_quant_i4(z, clip)
    if "amax" in c.modes:
        want["amax"] = hc.block_max(z, block_of, nb).astype(np.float32)
    if "xp" in c.modes:
        want["xp"] = hc.xp_tile(z, hc.XP_FILL)
    bar = hc.MERGE_BAR * max(1.0, float(np.abs(z.astype(np.float64)).max())) if merge else None
    return dt, want, bar


def check_rows(got, want, bar, what):
    if bar is None:
        assert np.array_equal(bits(got), bits(want)), what
    else:
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        print(f"{what}: max |out - ref| = {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (what, err, bar)


def check_quant(c, dt, q, s, want, bar, z_ref, what):
    keep = hc.quant_tokens(dt)
    q0, s0 = want
    if bar is None:
        assert np.array_equal(bits(s)[keep], bits(s0)[keep]), (what, "scale")
        assert np.array_equal(q[keep], q0[keep]), (what, "int4 bytes")
        return
    # unequal maxima: the rows are within `bar` of the reference, so (clip 1) scale = h(h(amax / 7)) is within bar / 7 and two
    # fp16 roundings of amax / 7, and q scale is within scale (1/2 + 2^-9: the rounding of h(z / scale) below 8) + bar of it
    z, sc = z_ref.astype(np.float64), s.astype(np.float64)
    s_ref = np.abs(z).max(axis=1) / 7.0
    assert (np.abs(sc - s_ref) <= bar / 7.0 + s_ref * 2.0 ** -9).all(), (what, "scale")
    deq = hc.unpack_i4(q).astype(np.float64) * sc[:, None]
    assert (np.abs(deq - z) <= sc[:, None] * (0.5 + 2.0 ** -9) + bar).all(), (what, "int4 bytes")


def _tile(T, n):
    return torch.full(((16 if T <= 16 else 32) * n,), hc.XP_FILL, dtype=torch.float16, device=DEV)


def _qbuf(T, n):
    return (torch.full((T, n // 2), 0x55, dtype=torch.int8, device=DEV), torch.full((T,), -3.0, dtype=torch.float16, device=DEV))


def _fbuf(T, n):
    return torch.full((T, n), hc.XP_FILL, dtype=torch.float16, device=DEV)


def _clips(c, bar):
    return (1.0,) if bar is not None else (1.0, c.clip2)


def _hk(dt):
    return dev(dt.had.astype(np.float16)) if dt.had is not None else None


# ------------------------------------------------------------------ fwht / hadk_mix / rowabsmax_quant

@pytest.mark.parametrize("c", of("fwht"), ids=lambda c: c.id)
def test_fwht(ops, oracle, c):
    dt, want, _ = expected(oracle, c)
    out = _fbuf(c.T, c.dims["N"])
    ops.faster_fast_hadamard_transform(dev(dt.x), dt.scale, out)
    check_rows(host(out), want["f16"], None, c.id)


@pytest.mark.parametrize("c", of("hadk_mix"), ids=lambda c: c.id)
def test_hadamard_mix(ops, oracle, c):
    dt, want, _ = expected(oracle, c)
    K, M = c.dims["K"], c.dims["M"]
    hk = _hk(dt) if K > 1 else torch.ones(1, 1, dtype=torch.float16, device=DEV)
    out = _fbuf(c.T, K * M).view(c.T, K, M)
    ops.hadamard_mix(dev(dt.x.reshape(c.T, K, M)), hk, out)
    check_rows(host(out).reshape(c.T, K * M), want["f16"], None, c.id)


@pytest.mark.parametrize("c", of("rq"), ids=lambda c: c.id)
def test_rowabsmax_quant(ops, oracle, c):
    dt, want, _ = expected(oracle, c)
    for clip in (1.0, c.clip2):
        q, s = _qbuf(c.T, c.dims["K"])
        ops.fuse_sym_quant(dev(dt.x), s, q, clip)
        check_quant(c, dt, host(q), host(s), want[("q", clip)], None, None, (c.id, clip))


# ------------------------------------------------------------------ head transforms

@pytest.mark.parametrize("c", of("heads_hadamard"), ids=lambda c: c.id)
def test_heads_hadamard(ops, oracle, c):
    dt, want, _ = expected(oracle, c)
    heads, n = c.dims["heads"], c.dims["heads"] * c.dims["d"]
    x = dev(dt.x)
    out = _fbuf(c.T, n)
    ops.heads_hadamard(x, dt.scale, out_f16=out, heads=heads)
    check_rows(host(out), want["f16"], None, c.id)
    for clip in (1.0, c.clip2):
        q, s = _qbuf(c.T, n)
        ops.heads_hadamard(x, dt.scale, q=q, scale=s, clip_ratio=clip, heads=heads)
        check_quant(c, dt, host(q), host(s), want[("q", clip)], None, None, (c.id, clip))


@pytest.mark.parametrize("c", of("heads_hadamard_mix"), ids=lambda c: c.id)
def test_heads_hadamard_mix(ops, oracle, c):
    dt, want, _ = expected(oracle, c)
    heads, d = c.dims["heads"], c.dims["d"]
    out = _fbuf(c.T, heads * d)
    ops.heads_hadamard_mix(dev(dt.x.reshape(c.T, heads, d)), _hk(dt), c.dims["K"], dt.scale, out)
    check_rows(host(out), want["f16"], None, c.id)


def _partials(ops, c, dt):
    return _attn_partials_ws(ops, c.T, c.dims["heads"], c.dims["d"], c.dims["S"], dt.o, dt.m, dt.l)


@pytest.mark.parametrize("c", of("heads_hadamard_merge"), ids=lambda c: c.id)
def test_heads_hadamard_merged(ops, oracle, c):
    """Merge + head transform on GIVEN partials against the reference -- not against the GPU's two-launch form."""
    dt, want, bar = expected(oracle, c)
    T, heads, d, S = c.T, c.dims["heads"], c.dims["d"], c.dims["S"]
    n, ws = heads * d, _partials(ops, c, dt)
    ns = S if c.nsplits_arg is None else c.nsplits_arg
    if "f16" in c.modes:
        out = _fbuf(T, n)
        ops.heads_hadamard_merged(ws, T, ns, T, heads, d, dt.scale, out_f16=out)
        check_rows(host(out), want["f16"], bar, c.id)
    if "q" in c.modes:
        for clip in _clips(c, bar):
            q, s = _qbuf(T, n)
            ops.heads_hadamard_merged(ws, T, ns, T, heads, d, dt.scale, q=q, scale=s, clip_ratio=clip)
            check_quant(c, dt, host(q), host(s), want[("q", clip)], bar, want["f16"], (c.id, clip))
    if "xp" in c.modes:
        tile = _tile(T, n)
        ops.heads_hadamard_merged(ws, T, ns, T, heads, d, dt.scale, out_f16=tile, xp=True)
        check_rows(host(tile), want["xp"], bar, (c.id, "xp"))


@pytest.mark.parametrize("c", of("heads_hadamard_merge_spread"), ids=lambda c: c.id)
def test_heads_hadamard_merged_spread(ops, oracle, c):
    dt, want, bar = expected(oracle, c)
    T, heads, d, S = c.T, c.dims["heads"], c.dims["d"], c.dims["S"]
    assert ops.heads_hadamard_merged_spread_supported(T, heads, d) == isinstance(c.routes()[0][2], str)
    out, pam = _fbuf(T, heads * d), torch.full((T, 8), -1.0, dtype=torch.float32, device=DEV)
    ops.heads_hadamard_merged_spread(_partials(ops, c, dt), T, S, T, heads, d, dt.scale, out, pam)
    check_rows(host(out), want["f16"], bar, c.id)
    _check_part_amax(host(pam), want["amax"], bar, c.id)


def _check_part_amax(pam, want, bar, what):
    """Each of the eight partial maxima, not only their maximum."""
    if bar is None:
        assert np.array_equal(pam.view(np.uint32), want.view(np.uint32)), (what, "part_amax")
    else:       # |max a - max b| <= max |a - b|
        assert (np.abs(pam.astype(np.float64) - want.astype(np.float64)) <= bar).all(), (what, "part_amax")


@pytest.mark.parametrize("c", of("heads_hadamard_mix_merge_spread"), ids=lambda c: c.id)
def test_heads_hadamard_mix_merged_spread(ops, oracle, c):
    dt, want, bar = expected(oracle, c)
    T, heads, d, S, K = c.T, c.dims["heads"], c.dims["d"], c.dims["S"], c.dims["K"]
    assert ops.heads_hadamard_mix_merged_spread_supported(T, heads, d, K) == hc.heads_mix_merge_spread_supported(T, heads, d, K)
    n, ws, hk = heads * d, _partials(ops, c, dt), _hk(dt)
    if "f16" in c.modes:
        out = _fbuf(T, n)
        ops.heads_hadamard_mix_merged_spread(ws, T, S, T, heads, d, hk, K, dt.scale, out)
        check_rows(host(out), want["f16"], bar, c.id)
    if "amax" in c.modes:
        out, pam = _fbuf(T, n), torch.full((T, 8), -1.0, dtype=torch.float32, device=DEV)
        ops.heads_hadamard_mix_merged_spread(ws, T, S, T, heads, d, hk, K, dt.scale, out, pam)
        check_rows(host(out), want["f16"], bar, (c.id, "amax"))
        _check_part_amax(host(pam), want["amax"], bar, c.id)
    if "xp" in c.modes:
        tile = _tile(T, n)
        ops.heads_hadamard_mix_merged_spread(ws, T, S, T, heads, d, hk, K, dt.scale, tile, xp=True)
        check_rows(host(tile), want["xp"], bar, (c.id, "xp"))


# ------------------------------------------------------------------ the MLP transform, both entries

def _mlp_modes(ops, c, dt, want, workspace):
    T, I, K = c.T, c.dims["I"], c.dims["K"]
    act, hk = dev(dt.x), _hk(dt)
    if "f16" in c.modes:
        out = _fbuf(T, I)
        ops.mlp_hadamard(act, hk, K, dt.scale, out_f16=out, workspace=workspace)
        check_rows(host(out), want["f16"], None, (c.id, "mlp_hadamard"))
    if "q" in c.modes:
        for clip in (1.0, c.clip2):
            q, s = _qbuf(T, I)
            ops.mlp_hadamard(act, hk, K, dt.scale, q=q, scale=s, clip_ratio=clip, workspace=workspace)
            check_quant(c, dt, host(q), host(s), want[("q", clip)], None, None, (c.id, "mlp_hadamard", clip))
    if "xp" in c.modes:
        tile = _tile(T, I)
        ops.mlp_hadamard(act, hk, K, dt.scale, out_f16=tile, workspace=workspace, xp=True)
        check_rows(host(tile), want["xp"], None, (c.id, "mlp_hadamard xp"))   # against the reference, not the plain GPU output


@pytest.mark.parametrize("c", of("mlp"), ids=lambda c: c.id)
def test_mlp_hadamard_and_silu_mul_hadamard(ops, oracle, c):
    """mlp_hadamard(act) in every mode of the case; cases with gate_up also run silu_mul_hadamard(gate_up) and
    act = silu_mul(gate_up) on the GPU: the same bits from both entries on every row that both reach."""
    dt, want, _ = expected(oracle, c)
    T, I, K = c.T, c.dims["I"], c.dims["K"]
    xws = ops.xwg_workspace(DEV) if c.ws else None
    assert not c.ws or xws is not None, "the spread forms need the exchange workspace (QSPEC_XWG_SPREAD=0?)"
    assert ops.mlp_hadamard_act_layout_supported(T, I, K) == hc.mlp_xp_supported(T, I, K)
    if hc.mlp_xp_supported(T, I, K):
        assert isinstance(hc.route("mlp_hadamard", T=T, I=I, K=K, ws=True, quant=False, xp=True), str)
    _mlp_modes(ops, c, dt, want, xws)
    if c.gate:
        gu, hk = dev(dt.gate_up), _hk(dt)
        act = torch.empty(T, I, dtype=torch.float16, device=DEV)
        ops.silu_mul(gu, act)
        assert np.array_equal(bits(host(act)), bits(dt.x)), (c.id, "silu_mul")
        out = _fbuf(T, I)
        ops.silu_mul_hadamard(gu, hk, K, dt.scale, out_f16=out)
        check_rows(host(out), want["f16"], None, (c.id, "silu_mul_hadamard"))
        for clip in (1.0, c.clip2):
            q, s = _qbuf(T, I)
            ops.silu_mul_hadamard(gu, hk, K, dt.scale, q=q, scale=s, clip_ratio=clip)
            check_quant(c, dt, host(q), host(s), want[("q", clip)], None, None, (c.id, "silu_mul_hadamard", clip))
    if c.ws:
        w = ops.xwg_error_word(DEV)
        assert w is not None and int(host(w).max()) == 0


def test_exchange_workspace_history(ops, oracle):
    """One exchange workspace through a sequence the engine produces: tokens 0..2 pass more generations than tokens 3..31,
    the three spread forms alternate with a one-workgroup launch in between.  Every launch gives the reference bytes."""
    xws = ops.xwg_workspace(DEV)
    assert xws is not None
    seen = []
    for step, (T, I, K) in enumerate(hc.HISTORY):
        c = hc.Case(f"history{step}", "mlp", "exact", T, {"I": I, "K": K}, ("q",), ws=True, shift=step, clip2=(0.9, 0.5)[step % 2],
                    seed=1000 + step)
        seen.append(c.routes()[0][2])
        dt = hc.build(c)
        want = hc.reference(c, dt)
        hk = _hk(dt)
        for clip in (1.0, c.clip2):
            q, s = _qbuf(T, I)
            ops.mlp_hadamard(dev(dt.x), hk, K, dt.scale, q=q, scale=s, clip_ratio=clip, workspace=xws)
            check_quant(c, dt, host(q), host(s), want[("q", clip)], None, None, (c.id, clip))
    assert sum("spread" in r for r in seen) == 5 and sum("smh.one" in r for r in seen) == 1, seen
    assert int(host(ops.xwg_error_word(DEV)).max()) == 0


# ------------------------------------------------------------------ the quantiser in the o_proj prologue

HQ = [c for c in CASES if c.tier == "exact" and c.T <= 4 and "amax" in c.modes and c.dims["heads"] in (32, 40)]


@pytest.mark.parametrize("c", HQ, ids=lambda c: c.id)
def test_spread_rows_and_partial_maxima_through_the_hq_quantiser(ops, oracle, c):
    """rowwise_scaled_linear_s4s4_residual_hq on the spread head forms' rows and partial maxima at clip != 1, the row maximum in
    a different one of the eight blocks per token: the oracle's rowabsmax_quant_i4(., clip) -> gemm_w4a4 -> add_f16."""
    dt, want, _ = expected(oracle, c)
    T, heads, d, S = c.T, c.dims["heads"], c.dims["d"], c.dims["S"]
    Kd, N = heads * d, 512
    assert ops.rowwise_scaled_linear_s4s4_residual_hq_supported(T, N, Kd)
    rng = np.random.default_rng(c.seed)
    wq, wsc = rng.integers(-128, 128, (N, Kd // 2)).astype(np.int8), (rng.random(N) * 0.01 + 0.001).astype(np.float16)
    resid = rng.standard_normal((T, N)).astype(np.float16)
    out, pam = _fbuf(T, Kd), torch.full((T, 8), -1.0, dtype=torch.float32, device=DEV)
    if "K" in c.dims:
        ops.heads_hadamard_mix_merged_spread(_partials(ops, c, dt), T, S, T, heads, d, _hk(dt), c.dims["K"], dt.scale, out, pam)
    else:
        ops.heads_hadamard_merged_spread(_partials(ops, c, dt), T, S, T, heads, d, dt.scale, out, pam)
    spike = [t for t, k in enumerate(dt.kinds) if k in ("pos", "neg", "ties")]
    assert len(set(np.argmax(host(pam)[spike], axis=1))) == len(spike)         # every such token's maximum in a block of its own
    _check_part_amax(host(pam), want["amax"], None, c.id)
    for clip in (0.9, 0.5):
        h1 = dev(resid)
        ops.rowwise_scaled_linear_s4s4_residual_hq(out, pam, clip, dev(wq), dev(wsc), h1, h1)
        q0, s0 = oracle.rowabsmax_quant_i4(want["f16"], clip)
        ref = oracle.add_f16(resid, oracle.gemm_w4a4(q0, s0, wq, wsc))
        assert np.array_equal(bits(host(h1)), bits(ref)), (c.id, clip)


# ------------------------------------------------------------------ refused shapes

SENT = 77.0


def _refused_call(ops, entry, a):
    """Launch the entry at a refused shape with buffers large enough for a kernel that would run all the same; returns the
    output buffers."""
    T = a.get("T", a.get("rows"))
    f = lambda *shape: torch.full(shape, SENT, dtype=torch.float16, device=DEV)
    i8 = lambda *shape: torch.full(shape, 0x55, dtype=torch.int8, device=DEV)
    if entry == "fwht":
        x, out = f(T, max(a["N"], 1)), f(T, max(a["N"], 1))
        return [out], lambda: ops._call("qspec_fast_hadamard_transform", x.data_ptr(), 1.0, out.data_ptr(), T, a["N"], ops._stream())
    if entry == "hadk_mix":
        K, M = max(a["K"], 1), a["M"]
        y, hk, out = f(T, K, M), f(K, K), f(T, K, M)
        return [out], lambda: ops._call("qspec_hadamard_mix", y.data_ptr(), hk.data_ptr(), out.data_ptr(), T, a["K"], M, ops._stream())
    if entry == "heads_hadamard":
        n = a["heads"] * a["d"]
        x, out, q, s = f(T, a["heads"], a["d"]), f(T, n + 2), i8(T, n // 2 + 2), f(T)
        if a["quant"]:
            return [q, s], lambda: ops.heads_hadamard(x, 0.25, q=q, scale=s)
        return [out], lambda: ops.heads_hadamard(x, 0.25, out_f16=out)
    if entry == "heads_hadamard_mix":
        heads, d, K = a["heads"], a["d"], a["K"]
        x, out, hk = f(T, heads, d), f(T, heads, d), f(max(K, 1), max(K, 1))
        return [out], lambda: ops.heads_hadamard_mix(x, hk, K, 0.25, out)
    if entry.startswith("heads_hadamard_m"):
        heads, d, S = a["heads"], a["d"], a["S"]
        mt = a.get("max_tokens", T)
        ws = torch.zeros(ops.paged_attention_workspace_bytes(max(T, mt), heads, d, max(S, 1)), dtype=torch.uint8, device=DEV)
        n = heads * d
        out, q, s, pam = f(32 * n if a.get("xp") else T * n), i8(T, n // 2), f(T), torch.full((T, 8), SENT, dtype=torch.float32, device=DEV)
        if entry == "heads_hadamard_merge":
            kw = dict(q=q, scale=s) if a["quant"] else dict(out_f16=out)
            if a.get("xp"):
                kw["out_f16"] = out
            return [out, q, s], lambda: ops.heads_hadamard_merged(ws, mt, S, T, heads, d, 0.25, xp=bool(a.get("xp")), **kw)
        if entry == "heads_hadamard_merge_spread":
            return [out, pam], lambda: ops.heads_hadamard_merged_spread(ws, mt, S, T, heads, d, 0.25, out, pam)
        K = a["K"]
        hk = f(K, K)
        return [out, pam], lambda: ops.heads_hadamard_mix_merged_spread(ws, mt, S, T, heads, d, hk, K, 0.25, out,
                                                                         pam if a["amax"] else None, xp=bool(a.get("xp")))
    if entry in ("silu_mul_hadamard", "mlp_hadamard"):
        I, K = a["I"], a["K"]
        hk = f(max(K, 1), max(K, 1))
        out, q, s = f(32 * I if a.get("xp") else T * I), i8(T, I // 2), f(T)
        kw = dict(q=q, scale=s) if a["quant"] else dict(out_f16=out.view(-1, I)[:T] if not a.get("xp") else out)
        if a.get("xp"):
            kw["out_f16"] = out
        if entry == "silu_mul_hadamard":
            x = f(T, 2 * I)
            return [out, q, s], lambda: ops.silu_mul_hadamard(x, hk, K, 0.25, **kw)
        x = f(T, I)
        xws = ops.xwg_workspace(DEV) if a["ws"] else None
        return [out, q, s], lambda: ops.mlp_hadamard(x, hk, K, 0.25, workspace=xws, xp=bool(a.get("xp")), **kw)
    if entry == "rowabsmax_quant":
        K = a["K"]
        x, q, s = f(T, K + 2), i8(T, K // 2 + 2), f(T)
        return [q, s], lambda: ops._call("qspec_fuse_sym_quant", x.data_ptr(), s.data_ptr(), q.data_ptr(), 1.0, T, K, ops._stream())
    raise KeyError(entry)


C_ENTRY = {"fwht": "qspec_fast_hadamard_transform", "hadk_mix": "qspec_hadamard_mix", "heads_hadamard": "qspec_heads_hadamard",
           "heads_hadamard_mix": "qspec_heads_hadamard_mix", "heads_hadamard_merge": "qspec_heads_hadamard_merged",
           "heads_hadamard_merge_spread": "qspec_heads_hadamard_merged_spread",
           "heads_hadamard_mix_merge_spread": "qspec_heads_hadamard_mix_merged_spread", "silu_mul_hadamard": "qspec_silu_mul_hadamard",
           "mlp_hadamard": "qspec_mlp_hadamard", "rowabsmax_quant": "qspec_fuse_sym_quant"}


@pytest.mark.parametrize("entry,a,code", hc.REFUSED, ids=[f"{e}-{i}" for i, (e, _, _) in enumerate(hc.REFUSED)])
def test_refused_shapes_raise_and_launch_nothing(ops, entry, a, code):
    assert hc.route(entry, **a) == code
    if entry == "mlp_hadamard":
        assert ops.mlp_hadamard_act_layout_supported(a["T"], a["I"], a["K"]) == hc.mlp_xp_supported(a["T"], a["I"], a["K"])
        if a.get("xp") and not a["quant"]:       # (the query knows nothing of the quantiser: xp with q is refused by the entry)
            assert not ops.mlp_hadamard_act_layout_supported(a["T"], a["I"], a["K"])
    if entry == "heads_hadamard_merge_spread":
        assert not ops.heads_hadamard_merged_spread_supported(a["T"], a["heads"], a["d"])
    outs, call = _refused_call(ops, entry, a)
    before = [o.clone() for o in outs]
    with pytest.raises(RuntimeError, match=C_ENTRY[entry]):
        call()
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert torch.equal(o, b), (entry, a)


def test_zero_tokens_launch_nothing(ops):
    assert hc.route("mlp_hadamard", T=0, I=14336, K=28, ws=True, quant=True) == "noop"
    e = torch.empty(0, 14336, dtype=torch.float16, device=DEV)
    hk = torch.ones(28, 28, dtype=torch.float16, device=DEV)
    ops.mlp_hadamard(e, hk, 28, 0.125, out_f16=torch.empty_like(e))
    ops.heads_hadamard(torch.empty(0, 4096, dtype=torch.float16, device=DEV), 0.25, out_f16=torch.empty(0, 4096, dtype=torch.float16, device=DEV), heads=32)
    ops.fuse_sym_quant(torch.empty(0, 64, dtype=torch.float16, device=DEV), torch.empty(0, dtype=torch.float16, device=DEV),
                       torch.empty(0, 32, dtype=torch.int8, device=DEV))
    torch.cuda.synchronize()
