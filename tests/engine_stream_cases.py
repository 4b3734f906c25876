"""Fixed-seed inputs and float64 references for the engine (unseeded) Philox stream tests: shared by
tests/test_engine_stream_cpu.py (which bounds the share of skipped rows before any GPU run) and
tests/test_engine_stream_gpu.py.  numpy only."""
import numpy as np

from philox_ref import engine_r0, exp_noise_f64, u01_closed_open

# every key and counter word is live: the seed's high half is non-zero and the offset is beyond 2^32
SEED = 0x5DEECE66D1234567
OFFSET = (7 << 32) | 0x89ABCDEF
FLT_MIN = float(np.finfo(np.float32).tiny)
MIN_GAP = 1e-3        # rows whose float64 top-2 relative gap is below it are skipped: the kernel's log is __logf
MAX_SKIPPED = 0.10


def softmax32(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _argmax_with_gap(val):
    top2 = np.sort(val, -1)[..., -2:]
    ok = (top2[..., 1] - top2[..., 0]) / top2[..., 1] >= MIN_GAP
    return val.argmax(-1), ok


def uniform_case(offset=OFFSET, B=64, k=3, V=64):
    """One-hot draft (p[x] = 1), q[x] = u (rejected: u < u is false) or the next float above u (accepted), where
    u = (r0 >> 8) / 2^24 with c0 = 0xFFFFFFFF, c1 = b * k + i: pins the accept uniform bit for bit."""
    rng = np.random.default_rng(41)
    ids = rng.integers(0, V, (B, k))
    bk = np.arange(B * k).reshape(B, k)
    u = u01_closed_open(engine_r0(0xFFFFFFFF, bk, SEED, offset))
    acc_want = rng.integers(0, 2, (B, k)).astype(bool) & (u > 0)
    thr = np.where(acc_want, np.nextafter(u, np.float32(2)), u).astype(np.float32)
    dp = np.zeros((B, k, V), np.float32)
    np.put_along_axis(dp, ids[..., None], 1.0, -1)
    tq = np.full((B, k + 1, V), 0.01, np.float32)
    np.put_along_axis(tq[:, :k], ids[..., None], thr[..., None], -1)
    return dict(tq=tq, dp=dp, ids=ids, bonus=rng.integers(0, V, B), accepted=acc_want)


def recovered_case(offset=OFFSET, B=32, k=3, V=512):
    """Dense q and p, every draft token forced rejected (q[x] = 0):
    recovered = argmax_v (max(q - p, FLT_MIN) / S) / -log(((r0 >> 8) + 0.5) / 2^24), c0 = v, c1 = b * k + i, in float64."""
    rng = np.random.default_rng(42)
    tq = softmax32(rng.normal(0, 2, (B, k + 1, V)))
    dp = softmax32(rng.normal(0, 2, (B, k, V)))
    ids = rng.integers(0, V, (B, k))
    np.put_along_axis(tq[:, :k], ids[..., None], 0.0, -1)
    f = np.maximum(tq[:, :k].astype(np.float64) - dp.astype(np.float64), FLT_MIN)
    S = f.sum(-1, keepdims=True)
    bk = np.arange(B * k).reshape(B, k, 1)
    e = exp_noise_f64(engine_r0(np.arange(V).reshape(1, 1, V), bk, SEED, offset))
    recovered, ok = _argmax_with_gap(f / S / e)
    return dict(tq=tq, dp=dp, ids=ids, bonus=rng.integers(0, V, B), recovered=recovered, ok=ok)


def sampled_case(offset=OFFSET, T=128, V=512):
    """Temperature 1, no top-k / top-p: token = argmax_v softmax(logits)_v / -log(u_v), c0 = v, c1 = 0x40000000 | t."""
    rng = np.random.default_rng(43)
    logits = rng.normal(0, 1, (T, V)).astype(np.float16)
    x = logits.astype(np.float64)
    p = np.exp(x - x.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    c1 = (0x40000000 | np.arange(T)).reshape(T, 1)
    e = exp_noise_f64(engine_r0(np.arange(V).reshape(1, V), c1, SEED, offset))
    token, ok = _argmax_with_gap(p / e)
    return dict(logits=logits, probs=p, token=token, ok=ok)
