"""Token logprobs (include/qspec_hip.h, "Logprobs"): a float64 numpy restatement of the two entry points' semantics, the case
list the CPU and the GPU test share, and the ONE comparison both use (tests/test_logprobs_cpu.py feeds it deliberately faulty
variants, tests/test_logprobs_gpu.py the kernels' outputs).

A case is a WIDE host buffer [rows, width] and the view x = wide[:, off:off + vocab] the kernel is given: with off > 0 or
width > vocab the rows are strided and mis-aligned for 16-byte loads, and what lies around them holds large values that must
never be seen."""
from collections import namedtuple

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
MAX_LOGPROBS = 32

Result = namedtuple("Result", "logprob rank top_ids top_logprobs")
Case = namedtuple("Case", "name kind wide off vocab tokens num_top")


def case_input(c):
    return c.wide[:, c.off:c.off + c.vocab]


def ref_token_logprobs(x, tokens, num_top, kind, *, fault=None, wide=None):
    """x [rows, vocab]: fp32 probabilities (kind "probs") or fp16 logits (kind "logits"); tokens [rows] int64.
    lp: probs log(max(p, FLT_MIN)); logits l - (m + log(sum exp(l - m))) -- in float64 on the float32 / float16 VALUES.
    rank = 1 + #{v: x[v] > x[token]}; the num_top largest inputs in descending order, ties lowest id first; surplus entries
    (num_top > vocab) id -1 / -inf; a token outside [0, vocab): logprob 0.0, rank -1.
    fault (tests only): "rank_ge" counts >= in the rank, "ties_high" orders ties highest id first, "lse_stride" takes the
    logits' normaliser over the whole row of `wide` instead of the vocab."""
    rows, vocab = x.shape
    lp_tok, rank = np.zeros(rows), np.full(rows, -1, dtype=np.int64)
    top_ids = np.full((rows, num_top), -1, dtype=np.int64)
    top_lp = np.full((rows, num_top), -np.inf)
    n = min(num_top, vocab)
    for r in range(rows):
        v = x[r].astype(np.float64)
        if kind == "probs":
            lp = np.log(np.maximum(v, FLT_MIN))
        else:
            src = wide[r].astype(np.float64) if fault == "lse_stride" else v
            m = src.max()
            with np.errstate(divide="ignore"):
                lp = v - (m + np.log(np.exp(src - m).sum()))
        t = int(tokens[r])
        if 0 <= t < vocab:
            lp_tok[r] = lp[t]
            rank[r] = 1 + int(((v >= v[t]) if fault == "rank_ge" else (v > v[t])).sum())
        if n:
            if fault == "ties_high":
                order = (vocab - 1 - np.argsort(-v[::-1], kind="stable"))[:n]
            else:
                order = np.argsort(-v, kind="stable")[:n]
            top_ids[r, :n] = order
            top_lp[r, :n] = lp[order]
    return Result(lp_tok, rank, top_ids, top_lp)


def compare(got, ref, kind):
    """The check of both tests: ranks and top ids exact (ties included), logprobs within |lp - ref| <= 1e-5 + 1e-6 |ref|
    (probs: logf within a few fp32 ulp at magnitudes up to 87) or 1e-4 absolute (logits: the bar tests/test_oracle_golden.py
    puts on sm_logprobs); infinite reference entries (surplus, -inf logits) must match exactly.  Returns a list of complaints."""
    bad = []
    if not np.array_equal(np.asarray(got.rank, dtype=np.int64), ref.rank):
        bad.append(f"rank {np.asarray(got.rank).tolist()} != {ref.rank.tolist()}")
    if not np.array_equal(np.asarray(got.top_ids, dtype=np.int64).reshape(ref.top_ids.shape), ref.top_ids):
        bad.append("top ids differ")
    for name, g, w in (("logprob", got.logprob, ref.logprob), ("top_logprobs", got.top_logprobs, ref.top_logprobs)):
        g, w = np.asarray(g, dtype=np.float64).reshape(w.shape), np.asarray(w, dtype=np.float64)
        fin = np.isfinite(w)
        if not np.array_equal(g[~fin], w[~fin]):
            bad.append(f"{name}: infinite entries differ")
        tol = 1e-5 + 1e-6 * np.abs(w[fin]) if kind == "probs" else 1e-4
        err = np.abs(g[fin] - w[fin])
        if not np.all(err <= tol):     # (a NaN fails too)
            bad.append(f"{name}: max error {np.nanmax(err) if err.size else 0:.3g}")
    return bad


# ---------------------------------------------------------------------- data

def _logits(rng, data, rows, vocab):
    if data == "normal":      # rounded to fp16: many exact ties at V = 128256
        return (rng.standard_normal((rows, vocab)) * 3.0).astype(np.float16)
    if data == "equal":
        return np.full((rows, vocab), 1.5, dtype=np.float16)
    if data == "peaked":      # -inf nearly everywhere
        x = np.full((rows, vocab), -np.inf, dtype=np.float16)
        for r in range(rows):
            ids = rng.choice(vocab, size=min(vocab, 3), replace=False)
            x[r, ids] = rng.standard_normal(len(ids)).astype(np.float16) * 4
        return x
    if data == "plateau":     # three members of the top value above tie groups of ~V/3: the N-th best sits inside a large group
        x = rng.choice(np.array([0.5, 1.0, 1.5], dtype=np.float16), size=(rows, vocab))
        for r in range(rows):
            x[r, rng.choice(vocab, size=min(vocab, 3), replace=False)] = 2.0
        return x
    raise ValueError(data)


def _softmax32(logits):
    v = logits.astype(np.float64)
    e = np.exp(v - v.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def _tokens(rng, x):
    """Per row in turn: the argmax, the argmin, a member of a tie group, id vocab - 1, a random id; one -1 per case (and one id
    past the vocabulary where there are rows to spare)."""
    rows, vocab = x.shape
    out = np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        v = x[r].astype(np.float64)
        pick = r % 5
        if pick == 0:
            out[r] = int(np.argmax(v))
        elif pick == 1:
            out[r] = int(np.argmin(v))
        elif pick == 2:
            vals, first, counts = np.unique(v, return_index=True, return_counts=True)
            tied = np.flatnonzero(counts > 1)
            if len(tied):
                val = vals[tied[len(tied) // 2]]
                out[r] = int(np.flatnonzero(v == val)[1])     # its second member
            else:
                out[r] = int(rng.integers(vocab))
        elif pick == 3:
            out[r] = vocab - 1
        else:
            out[r] = int(rng.integers(vocab))
    out[rows - 1 if rows < 5 else 4] = -1
    if rows > 9:
        out[9] = vocab + 3
    return out


# (vocab, rows, num_top, data, pad, off): vocab 1 / 7 (surplus entries), 2048 / 2049 (the tail behind the 16-byte loads, one
# element past a wave's share), 32000, 128256; rows 1 / 5 / 33; every num_top of 0, 1, 5, 20, 32; pad / off: strided, shifted rows
_SPECS = [
    (1, 1, 0, "normal", 0, 0), (1, 5, 5, "normal", 0, 0),
    (7, 5, 20, "normal", 0, 0), (7, 1, 1, "equal", 3, 1), (7, 33, 5, "peaked", 2, 0),
    (2048, 5, 5, "normal", 0, 0), (2048, 33, 1, "normal", 3, 0), (2048, 1, 20, "plateau", 0, 0),
    (2049, 5, 20, "normal", 5, 1), (2049, 1, 32, "equal", 0, 0), (2049, 5, 0, "peaked", 0, 0),
    (32000, 5, 5, "normal", 0, 0), (32000, 33, 20, "peaked", 1, 0), (32000, 1, 32, "normal", 8, 3),
    (32000, 5, 32, "plateau", 3, 2),
    (128256, 5, 20, "normal", 0, 0), (128256, 1, 0, "normal", 0, 0), (128256, 5, 32, "equal", 0, 0),
    (128256, 5, 5, "peaked", 0, 0), (128256, 33, 5, "normal", 3, 1), (128256, 1, 1, "plateau", 0, 0),
]


def _one_hot(rng, rows, vocab):
    x = np.zeros((rows, vocab), dtype=np.float32)      # p = 0 elsewhere: the FLT_MIN clamp
    x[np.arange(rows), rng.integers(vocab, size=rows)] = 1.0
    return x


_CASES = None


def cases():
    """The shared case list (built once, never modified)."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    for kind in ("logits", "probs"):
        for i, (vocab, rows, num_top, data, pad, off) in enumerate(_SPECS):
            rng = np.random.default_rng(1000 + i)
            logits = _logits(rng, data, rows, vocab)
            if kind == "logits":
                x, fill = logits, np.float16(60000.0)
            else:
                # the processed distributions: softmax of the logits cases (equal probabilities stay exact ties)
                x, fill = _softmax32(logits), np.float32(2.0)
            wide = np.full((rows, off + vocab + pad), fill, dtype=x.dtype)
            wide[:, off:off + vocab] = x
            wide.setflags(write=False)
            out.append(Case(f"{kind}-v{vocab}-r{rows}-n{num_top}-{data}" + ("-strided" if pad or off else ""), kind, wide, off,
                            vocab, _tokens(rng, x), num_top))
        if kind == "probs":
            for i, (vocab, rows, num_top) in enumerate(((7, 5, 5), (2049, 5, 20), (128256, 5, 5))):
                rng = np.random.default_rng(2000 + i)
                x = _one_hot(rng, rows, vocab)
                x.setflags(write=False)
                out.append(Case(f"probs-v{vocab}-r{rows}-n{num_top}-onehot", kind, x, 0, vocab, _tokens(rng, x), num_top))
    _CASES = out
    return out


_REFS = {}


def reference(c):
    """ref_token_logprobs of a case, computed once and shared."""
    if c.name not in _REFS:
        _REFS[c.name] = ref_token_logprobs(case_input(c), c.tokens, c.num_top, c.kind)
    return _REFS[c.name]
