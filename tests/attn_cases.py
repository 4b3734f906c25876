"""Paged-attention cases for the parity tests: a float64 reference, a case builder over block size, block-table width,
context split count and score regime, and the launch plan of attention.hip: attn_form() restated in Python so
that a test can assert that the case list reaches every kernel instantiation.

Every case poisons what no kernel may read.  Slots past a sequence's context in its last block and the blocks named by
its table's padding entries hold finite poison (K and V = +-60000): in the product the padding entries name real blocks
of other sequences, so a key that leaked into the softmax would be finite and large, not NaN.  Blocks that no table
entry names hold NaN.

Regimes (scale . q . k, the logits):
  smooth       q, k, v ~ N(0, 0.5): logit std ~0.25, an almost flat softmax
  peaked       q ~ N(0, 12): logit std ~6, range ~ +-25
  sink         one key per sequence with > 90 % of the mass (~27 above the rest): at position 0, or (sink_last) at the
               last position every query sees -- the last chunk of the last split, so that the earlier partials are
               rescaled by exp(-delta), delta >= 20
  negative     every logit <= -30 (a running max initialised to 0 or to a finite floor underflows every weight)
  future_trap  the keys of the verify window after the first query's position score ~ +22 over the rest: only the
               causal mask keeps them out of the earlier queries' rows
"""
import math
from dataclasses import dataclass
from itertools import product

import numpy as np

POISON = 60000.0
REGIMES = ("smooth", "peaked", "sink", "negative", "future_trap")
SPLITS = (16, 8, 4, 3, 1)            # every value engine.n_splits_for returns for the BASELINE configs
CHUNK, FA_ROWS, MAXR, MAXSPLIT = 128, 64, 16, 64   # attention_common.cuh: QS_ATT_CHUNK, QS_FA_ROWS, QS_ATT_MAXR, QS_ATT_MAXSPLIT


@dataclass(frozen=True)
class Case:
    ctx: tuple           # context length per sequence (the q_len new tokens included)
    q_len: int           # query tokens per sequence: 1 (draft), k + 1 (verify), or prompt-sized
    nq: int
    nkv: int
    d: int
    bs: int              # KV block size
    width: int           # block-table entries per sequence (set on its own, >= the longest context's blocks)
    regime: str
    n_splits: int
    merged: bool         # out given (the kernel merges its splits) or out = NULL (partials left in the workspace)
    seed: int
    sink_last: bool = False

    @property
    def id(self):
        c = ",".join(map(str, self.ctx))
        return (f"{self.regime}{'-last' if self.sink_last else ''}-h{self.nq}.{self.nkv}.{self.d}-bs{self.bs}-w{self.width}"
                f"-q{self.q_len}-S{self.n_splits}-{'out' if self.merged else 'part'}-ctx{c}")

    @property
    def T(self):
        return len(self.ctx) * self.q_len


def make_case(ctx, q_len, heads, bs, regime, n_splits, merged, seed, width=None, sink_last=False):
    """width None: the tightest table (longest context's blocks + 1, as the older tests size it)."""
    nq, nkv, d = heads
    ctx = tuple(max(int(c), q_len) for c in ctx)
    need = max(-(-c // bs) for c in ctx)
    w = need + 1 if width is None else max(width, need)
    return Case(ctx, q_len, nq, nkv, d, bs, w, regime, n_splits, merged, seed, sink_last and regime == "sink")


# ------------------------------------------------------------------ data

def build(case, poison_seed=None):
    """-> dict(q [T, nq*d] fp16 (a view of a fused qkv row, stride row), qkv, row, kc, vc [nb, bs, nkv, d] fp16,
    bt [n_seqs, width] int32, ctx int32, q_start int32, scale, poisoned (bool mask over the cache slots)).
    poison_seed re-draws the poison values (and only those)."""
    rng = np.random.default_rng(case.seed)
    nq, nkv, d, bs, W = case.nq, case.nkv, case.d, case.bs, case.width
    n_seqs = len(case.ctx)
    need = [-(-c // bs) for c in case.ctx]
    n_real = sum(need)
    n_pad = n_seqs * W - n_real
    n_pool = min(n_pad, 8)            # blocks the padding entries name (shared between sequences, as in the product)
    n_nan = 3
    nb = n_real + n_pool + n_nan
    ids = rng.permutation(nb).astype(np.int32)
    real, pool, nan_ids = ids[:n_real], ids[n_real:n_real + n_pool], ids[n_real + n_pool:]
    bt = np.empty((n_seqs, W), np.int32)
    o = 0
    for s, n in enumerate(need):
        bt[s, :n] = real[o:o + n]
        o += n
        if W > n:
            bt[s, n:] = pool[rng.integers(0, n_pool, W - n)]
    shape = (nb, bs, nkv, d)
    kc = (rng.standard_normal(shape, dtype=np.float32) * 0.5)
    vc = (rng.standard_normal(shape, dtype=np.float32) * 0.5)
    T = case.T
    row = (nq + 2 * nkv) * d                      # q is read from the fused qkv row, as the model passes it
    q = rng.standard_normal((T, nq, d), dtype=np.float32) * 0.5
    rd = math.sqrt(d)
    q_start = (np.arange(n_seqs + 1) * case.q_len).astype(np.int32)

    def slot(s, p):                               # -> (block, offset) arrays for positions p of sequence s
        p = np.asarray(p)
        return bt[s, p // bs], p % bs

    if case.regime == "peaked":
        q *= 24.0                                 # q ~ N(0, 12): logit std 12 * 0.5 = 6
    elif case.regime in ("sink", "negative", "future_trap"):
        a = 2.0 if case.regime != "negative" else math.sqrt(45.0 / rd)
        q += a                                    # a common direction (all ones) in every query
        for s, c in enumerate(case.ctx):
            if case.regime == "sink":
                p = c - case.q_len if case.sink_last else 0       # seen by every query of the sequence
                blk, off = slot(s, [p])
                kc[blk, off] = 27.0 / (a * rd)    # logit ~ 27 above the rest (which are ~ N(0, 1))
            elif case.regime == "future_trap" and case.q_len > 1:
                blk, off = slot(s, np.arange(c - case.q_len + 1, c))
                kc[blk, off] = 22.0 / (a * rd)
        if case.regime == "negative":
            kc -= a                               # logits ~ -45 +- 1.5
    kc, vc = kc.astype(np.float16), vc.astype(np.float16)
    qkv = np.zeros((T, row), np.float16)
    qkv[:, :nq * d] = q.reshape(T, nq * d).astype(np.float16)
    qkv[:, nq * d:] = (rng.standard_normal((T, 2 * nkv * d), dtype=np.float32)).astype(np.float16)
    # poison: every slot no sequence owns; NaN in the blocks no table entry names
    owned = np.zeros((nb, bs), bool)
    for s, c in enumerate(case.ctx):
        blk, off = slot(s, np.arange(c))
        owned[blk, off] = True
    poisoned = ~owned
    poisoned[nan_ids] = False
    prng = np.random.default_rng(case.seed + 1 if poison_seed is None else poison_seed)
    npois = int(poisoned.sum())
    for cache in (kc, vc):
        cache[poisoned] = (prng.choice([-POISON, POISON], (npois, nkv, d))
                           * (1.0 - 0.01 * prng.random((npois, nkv, d)))).astype(np.float16)
        cache[nan_ids] = np.nan
    return dict(q=qkv[:, :nq * d], qkv=qkv, row=row, kc=kc, vc=vc, bt=bt, ctx=np.array(case.ctx, np.int32),
                q_start=q_start, scale=d ** -0.5, poisoned=poisoned, nan_blocks=nan_ids)


# ------------------------------------------------------------------ float64 reference

def ref_attention_f64(q, kc, vc, bt, ctx, q_start, scale, return_logits=False):
    """Causal varlen paged attention in float64: query i of sequence s (position ctx[s] - q_len_s + i) attends to the
    keys 0 .. its position, read from the slots bt[s, pos // bs] * bs + pos % bs for pos < ctx[s] -- and nothing else.
    q [T, nq*d] -> [T, nq*d] float64 (and, with return_logits, the per-sequence [nkv, q_len, group, ctx] logits with
    the causal mask applied as -inf)."""
    nb, bs, nkv, d = kc.shape
    T = q.shape[0]
    nq = q.shape[1] // d
    g = nq // nkv
    out = np.zeros((T, nq, d))
    logits = []
    for s in range(len(ctx)):
        c, t0, t1 = int(ctx[s]), int(q_start[s]), int(q_start[s + 1])
        ql = t1 - t0
        if ql == 0:
            continue
        p = np.arange(c)
        blk, off = bt[s, p // bs], p % bs
        K = kc[blk, off].astype(np.float64).transpose(1, 0, 2)          # [nkv, ctx, d]
        V = vc[blk, off].astype(np.float64).transpose(1, 0, 2)
        Q = q[t0:t1].astype(np.float64).reshape(ql, nkv, g, d).transpose(1, 0, 2, 3)   # [nkv, ql, g, d]
        S = np.einsum("hqgd,hkd->hqgk", Q, K) * scale
        qpos = c - ql + np.arange(ql)
        S = np.where(p[None, None, None, :] <= qpos[None, :, None, None], S, -np.inf)
        m = S.max(axis=-1, keepdims=True)
        P = np.exp(S - m)
        O = np.einsum("hqgk,hkd->hqgd", P, V) / P.sum(axis=-1)[..., None]
        out[t0:t1] = O.transpose(1, 0, 2, 3).reshape(ql, nq, d)
        logits.append(S)
    out = out.reshape(T, nq * d)
    return (out, logits) if return_logits else out


def merge_partials_f64(o, ml):
    """o [T, nq, S, d], ml [T, nq, S, 2] (m, l) -> sum_s w_s o_s / sum_s w_s l_s, w_s = e^(m_s - M), in float64."""
    o, ml = o.astype(np.float64), ml.astype(np.float64)
    m, l = ml[..., 0], ml[..., 1]
    M = m.max(axis=2, keepdims=True)
    w = np.where(np.isneginf(m), 0.0, np.exp(m - M))
    return (w[..., None] * o).sum(axis=2) / (w * l).sum(axis=2)[..., None]


# ------------------------------------------------------------------ launch plan of attention.hip: attn_form()

def generic_splits(n_splits):
    """attention.hip: paged_attention_generic_splits."""
    return 1 if n_splits < 1 else min(n_splits, 4)


def kernel_path(c):
    """The kernel instantiation paged_attention() launches for case c at default knobs, as a label."""
    n_seqs, group = len(c.ctx), c.nq // c.nkv
    if c.d != 128:
        if c.d % 8 == 0:
            S = generic_splits(c.n_splits)
            if not c.merged:
                return "generic_vec partials"
            return "generic_vec S=1" if S == 1 else "generic_vec S>1 + merge"
        assert c.merged, "the generic kernel needs out"
        return "generic"
    rows = c.q_len * group
    if c.n_splits == 1 and rows >= 2 * FA_ROWS:
        return "prefill"
    n_rb = -(-rows // MAXR)
    bt_reg = c.width <= 128
    long_splits = c.width * c.bs > CHUNK * c.n_splits
    if not c.merged and long_splits:
        fast = bt_reg and c.bs >= 16
        return f"waves<{'TF'[not bt_reg]},4,{'TF'[not fast]}>"
    pf = n_seqs * c.nkv * n_rb * c.n_splits <= 256
    return f"chunk<{'TF'[not pf]},{'TF'[not bt_reg]}>" + (" out" if c.merged else " partials")


def path_rows(c):
    """The rows of the coverage table case c reaches (kernel_path plus the conditions the table asks for)."""
    p = kernel_path(c)
    rows = {p}
    if p == "prefill":
        rows.add(f"prefill bs{c.bs}")
        if c.width > 128:
            rows.add("prefill wide")
    if p.startswith("waves") and c.q_len in (4, 6):
        rows.add(p + " verify")
    return rows


REQUIRED_ROWS = {"prefill bs8", "prefill bs32", "prefill wide",
                 *(f"chunk<{pf},{bt}> {m}" for pf, bt, m in product("TF", "TF", ("out", "partials"))),
                 "waves<T,4,T> verify", "waves<T,4,F> verify", "waves<F,4,F> verify",
                 "generic_vec S=1", "generic_vec S>1 + merge", "generic_vec partials", "generic"}


# ------------------------------------------------------------------ the matrix

H32, H64, H40, HT = (32, 8, 128), (64, 8, 128), (40, 40, 128), (32, 4, 64)


def _boundary_sets(bs, S):
    """Context sets of one launch: 1 key, block boundaries +-1, 128-key chunk boundaries +-1, split boundaries
    (128 * n_splits: one chunk per split below, two above) +-1, 2047 / 2048 / 2049."""
    return [(1, bs - 1, bs, bs + 1),
            (127, 128, 129, 3 * bs + 1),
            (CHUNK * S - 1, CHUNK * S, CHUNK * S + 1),
            (2047, 2048, 2049)]


def gpu_cases():
    cases = []
    # 1. every block size x regime x q_len at the Llama-3-8B head layout: boundaries, split counts, table widths, both
    #    output forms rotate through the combinations
    for i, (bs, regime, q_len) in enumerate(product((8, 16, 32), REGIMES, (1, 4, 6))):
        S = SPLITS[i % len(SPLITS)]
        ctx = _boundary_sets(bs, S)[i % 4]
        wide = (i // 2) % 2 == 1
        width = max(129, 2 * max(ctx) // bs + 3) if wide else None
        cases.append(make_case(ctx, q_len, H32, bs, regime, S, i % 2 == 0, 1000 + i, width=width,
                               sink_last=regime == "sink" and i % 3 != 0))
    # 2. short contexts in wide tables (the engine sizes the table from max_model_len)
    for i, (bs, q_len) in enumerate(product((8, 16, 32), (1, 4, 6))):
        cases.append(make_case((1, 5, 37, 200), q_len, H32, bs, REGIMES[i % 5], SPLITS[i % 5], i % 2 == 1, 2000 + i,
                               width=4096 // bs, sink_last=True))
    # 3. long contexts: 4097 (every block size), 8191 (block size 16)
    for i, (ctx, bs, regime, q_len, S) in enumerate([
            ((4097, 33), 8, "peaked", 4, 8), ((4097,), 16, "sink", 6, 16), ((4097, 100), 32, "negative", 1, 4),
            ((4097,), 16, "future_trap", 6, 3), ((8191,), 16, "sink", 4, 8), ((8191, 17), 16, "peaked", 1, 16),
            ((8191,), 16, "negative", 6, 4), ((4097,), 32, "sink", 4, 1)]):
        for merged in (True, False):
            cases.append(make_case(ctx, q_len, H32, bs, regime, S, merged, 3000 + 2 * i + merged, sink_last=True))
    # 4. the other head layouts: 64 heads (group 8), 40 heads (no GQA, 3 splits), head size 64 (contexts <= 2048)
    for i, (regime, q_len, bs) in enumerate(product(REGIMES, (1, 4), (8, 16, 32))):
        ctx = ((1, 129, 700), (bs + 1, 2047), (255, 256, 257))[i % 3]
        cases.append(make_case(ctx, q_len, H64, bs, regime, SPLITS[i % 5], i % 2 == 0, 4000 + i, sink_last=i % 2 == 1,
                               width=300 if i % 4 == 3 else None))
        cases.append(make_case(ctx[:2], q_len, H40, bs, regime, 3, i % 2 == 1, 4100 + i, sink_last=i % 2 == 0))
        cases.append(make_case(((1, 64, 65), (bs - 1, 600, 2048), (2047, 300))[i % 3], q_len, HT, bs, regime,
                               (1, 3, 8)[i % 3], i % 4 != 3, 4200 + i, width=(None, 2048 // bs)[i % 2],
                               sink_last=i % 2 == 1))
    # 5. the rows of the dispatch table the rotation above may miss
    for i, bs in enumerate((8, 16, 32)):             # prompt-sized queries (prefill kernel), narrow and wide tables
        cases.append(make_case((40, 300), 40, H32, bs, ("sink", "peaked", "future_trap")[i], 1, True, 5000 + i, sink_last=True))
        cases.append(make_case((33, 2100), 33, H32, bs, ("negative", "future_trap", "smooth")[i], 1, i != 1, 5010 + i,
                               width=4096 // bs))
    cases += [
        # in-kernel merge and short-split partials, PF x BT: PF = false above 256 workgroups
        make_case((300, 70, 129), 6, H32, 16, "future_trap", 16, True, 5100),                     # chunk<F,T> out
        make_case((300, 70, 129), 6, H32, 16, "negative", 16, True, 5101, width=200),             # chunk<F,F> out
        make_case((300, 70, 129), 6, H32, 16, "sink", 16, False, 5102, sink_last=True),           # chunk<F,T> partials
        make_case((300, 70, 129), 6, H32, 8, "peaked", 16, False, 5103, width=200),               # chunk<F,F> partials
        make_case((500,), 4, H32, 16, "negative", 8, True, 5104),                                 # chunk<T,T> out
        make_case((500,), 4, H32, 8, "future_trap", 16, True, 5105, width=250),                   # chunk<T,F> out
        make_case((500,), 4, H32, 16, "sink", 8, False, 5106),                                    # chunk<T,T> partials
        make_case((500,), 6, H32, 8, "negative", 16, False, 5107, width=250),                     # chunk<T,F> partials
        # keys over waves: <T,4,T> (width <= 128, bs >= 16), <T,4,F> (bs 8), <F,4,F> (width > 128)
        make_case((1500, 9), 4, H32, 16, "future_trap", 4, False, 5200),
        make_case((900, 9), 6, H32, 8, "negative", 4, False, 5201),
        make_case((1500, 9), 6, H32, 32, "sink", 3, False, 5202, width=300, sink_last=True),
        # generic head sizes: even d, d % 8 != 0 (no vector loads)
        make_case((1, 17, 300), 4, (4, 2, 66), 16, "peaked", 8, True, 5300),
        make_case((700, 33), 1, (4, 2, 66), 8, "negative", 1, True, 5301, width=200),
    ]
    return cases


GPU_CASES = gpu_cases()
