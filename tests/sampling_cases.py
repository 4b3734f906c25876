"""The case matrix of the top-k / top-p / min_p selection (csrc/sampler.hip: topk_hist_kernel, topk_select_kernel<MINP>,
topk_write_kernel<SEEDED>, topk_token_kernel) and its float64 reference.  Plain numpy: no GPU, no oracle import.

The selection does not sort: it histograms the row's fp16 keys and one 1024-thread workgroup walks the 65536 key POSITIONS
(pos = 65535 - key, descending logit order), 64 consecutive positions per thread, 4096 per wave.  Its off-by-ones live where
that walk branches: at a thread's first / last position, at a wave edge, across runs of empty threads, inside groups of
equal logits.  The rows here are therefore built from (position, count) groups, so that a boundary sits exactly on such a
place, and every parameter of a row is derived from the row: top_p is the midpoint between the cumulative fractions on
either side of the intended boundary group, min_p the geometric mean of the two neighbouring probability ratios, the
exponential noise is redrawn until the winning token leads by 1e-3.  No row needs to be excused by the GPU test.

  pos_of / value_at     fp16 value <-> position; -0.0 has the position of +0.0 (equal logits are ONE group)
  build_row             (position, count) groups -> a shuffled fp16 row
  ref_select            the reference: float64, on groups of equal value
  model_select          a model of the kernel's walk (per-thread prefixes, the "first key of a later thread" offer, the
                        denominator from the thread that owns pos_last) with named faults: what the bars must catch
  check_row             the checks the GPU test applies to a row (tests/test_sampling_cases.py applies them to the model)
  cases / batches       the matrix
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64

POS_ZERO = 32767          # +0.0 and -0.0
POS_NEG_INF = 64512
KEYS_PER_THREAD = 64      # 64 threads = 4096 positions per wave

# |GPU probs - float64 probs| allowed per token.  Measured, not chosen (test_prob_bar_is_measured): the largest
# |oracle.sample_top_k_top_p probs - ref_select probs| over the cases whose kept sets agree is 1.951e-7 (fp32 arithmetic,
# the oracle's own expf, an fp64 denominator: the arithmetic the kernel restates; the T=0.3 row sets it, where the fp32
# quotient logit / T near 30 carries half an ulp, 1e-6, into the exponent); the kernel sums its mass in another,
# hierarchical order and rounds z to fp32 once, about one fp32 ulp each and nothing more: 4x the measured distance.
PROB_BAR = 7.8e-7
SUM_BAR = 1e-5            # |row sum - 1|

GAP_TOP_P = 1e-4          # every group's cumulative fraction is at least this far from top_p
GAP_MIN_P = 1e-3          # every group's exp(l - max) is at least this far from min_p, relative
GAP_E = 1e-3              # best p / E over second best >= 1 + GAP_E
UNDERFLOW = -86.0         # the fp32 exp of the product (qexpf) is 0 below: such a token's fp32 probability is 0
CLEAR_ZONE = (-110.0, -75.0)   # no finite token of any case has l - max in here: "probability > 0" is never in doubt

FAULTS = ("k_off_by_one", "split_signed_zero", "mask_max_group", "later_thread_not_offered", "empty_thread_denominator",
          "p_one_absorbs_tail", "minp_masks_max", "boundary_group_split")


# ---------------------------------------------------------------------- positions
def positions(logits, split_zero: bool = False) -> np.ndarray:
    """fp16 array -> int64 positions (65535 - tk_key); NaN -> -1.  split_zero: -0.0 keeps its own key (position 32768)."""
    b = np.ascontiguousarray(logits, dtype=F16).view(np.uint16).astype(np.int64)
    if not split_zero:
        b = np.where(b == 0x8000, 0, b)
    key = np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)
    pos = 65535 - key
    nan = (b & 0x7FFF) > 0x7C00
    return np.where(nan, -1, pos)


def pos_of(value) -> int:
    p = int(positions(np.array([value], F16))[0])
    assert p >= 0, "NaN has no position"
    return p


def value_at(pos: int) -> np.float16:
    key = 65535 - int(pos)
    b = (key & 0x7FFF) if key & 0x8000 else (~key & 0xFFFF)
    return np.array([b], np.uint16).view(F16)[0]


_VALUES = np.array([value_at(p) for p in range(65536)], F16).astype(F64)    # position -> logit (NaN patterns included)


def th(thread: int, j: int) -> int:
    """Position j of thread `thread`."""
    assert 0 <= j < KEYS_PER_THREAD
    return KEYS_PER_THREAD * thread + j


def build_row(groups, V: int, seed: int, neg_zeros: int = 0) -> np.ndarray:
    """(position, count) groups in descending logit order -> fp16 row [V] in shuffled token order.  Positive finite values
    sit at positions 1024 .. 32767, negative finite ones from 32769 up, -inf at 64512.  neg_zeros: how many members of the
    zero group are -0.0."""
    last, vals = -1, []
    for pos, cnt in groups:
        assert pos > last and cnt > 0, (pos, cnt)
        assert 1024 <= pos <= POS_ZERO or POS_ZERO + 1 < pos <= POS_NEG_INF, pos
        last = pos
        v = np.full(cnt, value_at(pos), F16)
        if pos == POS_ZERO and neg_zeros:
            assert 0 < neg_zeros < cnt     # both signs present
            v[:neg_zeros] = F16(-0.0)
        vals.append(v)
    row = np.concatenate(vals)
    assert row.size == V, (row.size, V)
    assert neg_zeros == 0 or any(p == POS_ZERO for p, _ in groups)
    return row[np.random.default_rng(seed).permutation(V)]


# ---------------------------------------------------------------------- the float64 reference
@dataclass
class Sel:
    kept: np.ndarray            # [V] bool: what the selection rule keeps (-inf and NaN tokens never)
    nonzero: np.ndarray         # kept, and the fp32 probability is not 0 (exp(l - max) does not underflow)
    probs: np.ndarray           # [V] float64
    token: int
    best: float                 # the largest and the second largest p / E (p for a greedy row)
    second: float
    pos_k: int = -1             # position of the top-k group
    pos_p: Optional[int] = None     # position of the first group top-p masks (inside top-k), or None
    pos_mp: Optional[int] = None    # position of the first group min_p masks, or None
    prev_k: int = -1            # positions of the groups just above them
    prev_p: Optional[int] = None
    tightest: str = ""          # which of top_k / top_p / min_p set the last kept group ("" = none binds)
    gap_p: float = np.inf
    gap_mp: float = np.inf
    boundary_count: int = 1     # tokens in the last kept group
    d: np.ndarray = None        # [V] l - max


def _groups(logits, temperature):
    x = np.asarray(logits, F16).astype(F64)
    ok = ~np.isnan(x)
    t32 = F32(1.0 if temperature is None else temperature)
    greedy = bool(t32 < F32(1e-5))
    div = 1.0 if greedy else float(t32)
    neg, inv_ok, cnt = np.unique(-x[ok], return_inverse=True, return_counts=True)     # -0.0 == +0.0: one group
    vals = -neg
    inv = np.full(x.size, -1, np.int64)
    inv[ok] = inv_ok.ravel()
    l = vals / div
    with np.errstate(invalid="ignore"):
        r = np.exp(l - l[0])           # exp(l - max) per group; 0 for -inf
    return vals, cnt, inv, l, r, greedy


def ref_select(logits, temperature, top_k, top_p, min_p, E=None) -> Sel:
    """The selection in float64 on groups of equal value.
    l = float64(logit) / float64(float32 temperature) (divisor 1 when temperature < 1e-5: a greedy row).
    top-k: the group at which the descending cumulative count reaches k (k <= 0 or k > V: V); Z_k = the mass down to and
    including it.  top-p: the first group, never the maximum group, whose strictly larger groups hold >= p Z_k is masked
    with everything below it; top_p >= 1 (or None) masks nothing.  min_p: groups with exp(l - max) < min_p are masked,
    never the maximum group; greedy rows ignore it.  probs = float64 softmax over what is left; token = argmax(p / E), or
    argmax(p) for a greedy row, the first index on ties."""
    vals, cnt, inv, l, r, greedy = _groups(logits, temperature)
    V, G = inv.size, vals.size
    k = int(-1 if top_k is None else top_k)
    if k <= 0 or k > V:
        k = V
    cum = np.cumsum(cnt)
    gk = G - 1 if k > cum[-1] else int(np.searchsorted(cum, k))
    w = cnt * r
    incl = np.cumsum(w)
    above = np.concatenate([[0.0], incl[:-1]])
    zk = incl[gk]
    last, tight = gk, ("top_k" if gk < G - 1 and np.isfinite(l[gk + 1]) else "")
    p = 1.0 if top_p is None else float(F32(top_p))
    gp = None
    gap_p = np.inf
    if p < 1.0:
        frac = above / zk
        hit = np.flatnonzero(frac[1:gk + 1] >= p)
        if hit.size:
            gp = int(hit[0]) + 1
            if gp - 1 < last:
                last, tight = gp - 1, "top_p"
        if gk >= 1:
            gap_p = float(np.abs(frac[1:gk + 1] - p).min())
    mp = 0.0 if (min_p is None or greedy) else float(F32(min_p))
    gm = None
    gap_mp = np.inf
    if mp > 0.0:
        hit = np.flatnonzero(r[1:] < mp)
        if hit.size:
            gm = int(hit[0]) + 1
            if gm - 1 < last:
                last, tight = gm - 1, "min_p"
        fin = r[1:][r[1:] > 0]
        if fin.size:
            gap_mp = float(np.abs(fin / mp - 1.0).min())
    gkept = (np.arange(G) <= last) & np.isfinite(l)
    z = float((w * gkept).sum())
    gprob = np.where(gkept, r / z, 0.0)
    kept = np.zeros(V, bool)
    probs = np.zeros(V, F64)
    d = np.full(V, -np.inf)
    okm = inv >= 0
    kept[okm] = gkept[inv[okm]]
    probs[okm] = gprob[inv[okm]]
    with np.errstate(invalid="ignore"):
        d[okm] = (l - l[0])[inv[okm]]
    score = probs if (greedy or E is None) else probs / np.asarray(E, F32).astype(F64)
    token = int(np.argmax(score))
    top2 = np.sort(score)[-2:] if V > 1 else np.array([0.0, score[0]])
    P = lambda g: None if g is None else int(positions(np.array([vals[g]], F16))[0])
    return Sel(kept=kept, nonzero=kept & (d >= UNDERFLOW), probs=probs, token=token, best=float(top2[1]), second=float(top2[0]),
               pos_k=P(gk), pos_p=P(gp), pos_mp=P(gm), prev_k=P(gk - 1) if gk >= 1 else -1, prev_p=P(gp - 1) if gp else None,
               tightest=tight, gap_p=gap_p, gap_mp=gap_mp, boundary_count=int(cnt[last]), d=d)


# ---------------------------------------------------------------------- a model of the kernel's walk, with faults
def model_select(logits, temperature, top_k, top_p, min_p, E=None, fault: Optional[str] = None) -> Tuple[np.ndarray, int]:
    """topk_select_kernel + topk_write_kernel restated position by position -> (probs [V] float64, token).
    1024 threads own 64 descending positions each; exclusive prefixes of counts and mass (waves summed in wave order);
    the thread whose count range holds k walks for the top-k key; for top-p the thread in which the mass above crosses
    p Z_k walks, threads behind it offer their first key without a walk, the smallest position wins; min_p is one more
    boundary; the denominator comes from the thread that owns pos_last, which may be an empty one.
    fault=None is the intended kernel (signed zeros one key, top_p >= 1 skips the search); each named fault is one way
    to get it wrong."""
    assert fault is None or fault in FAULTS, fault
    lg = np.asarray(logits, F16)
    V = lg.size
    pos = positions(lg, split_zero=(fault == "split_signed_zero"))
    valid = pos >= 0
    cnt = np.bincount(pos[valid], minlength=65536).astype(np.int64)
    t32 = F32(1.0 if temperature is None else temperature)
    greedy = bool(t32 < F32(1e-5))
    temp = 1.0 if greedy else float(t32)
    kk = int(-1 if top_k is None else top_k)
    if kk <= 0 or kk > V:
        kk = V
    pp = 1.0 if top_p is None else float(F32(top_p))
    ne = np.flatnonzero(cnt)
    pos_max = int(ne[0])
    mx = _VALUES[pos_max] / temp
    dpos = np.full(65536, -np.inf)
    dpos[ne] = _VALUES[ne] / temp - mx
    epos = np.where(dpos >= UNDERFLOW, np.exp(dpos), 0.0)          # qexpf: 0 below -86
    wpos = cnt * epos
    c_loc = cnt.reshape(1024, 64).sum(1)
    m_loc = np.cumsum(wpos.reshape(1024, 64), axis=1)[:, -1]       # (sequential sums throughout: np.sum adds pairwise)
    c_ex = np.cumsum(c_loc) - c_loc
    m_ex = np.zeros(1024)
    wave_mass = np.cumsum(m_loc.reshape(16, 64), axis=1)[:, -1]
    for wv in range(16):
        inc = np.cumsum(m_loc[64 * wv:64 * wv + 64])
        ex = inc - m_loc[64 * wv:64 * wv + 64]
        for w2 in range(wv):
            ex = ex + wave_mass[w2]
        m_ex[64 * wv:64 * wv + 64] = ex
    first = np.full(1024, -1, np.int64)
    for p_ in ne[::-1]:
        first[p_ >> 6] = p_
    live = np.flatnonzero(c_loc)

    # (a) top-k
    ke = kk + 1 if fault == "k_off_by_one" else kk
    pos_k, zk, split = None, None, None
    for t in live:
        if c_ex[t] < ke <= c_ex[t] + c_loc[t]:
            run, mrun = c_ex[t], m_ex[t]
            for j in range(64):
                q = 64 * t + j
                if cnt[q]:
                    if run < ke <= run + cnt[q]:
                        pos_k, zk = q, mrun + wpos[q]
                        if fault == "boundary_group_split" and run + cnt[q] > ke:
                            split = (q, int(ke - run))          # keep exactly k tokens
                            zk = mrun + split[1] * epos[q]
                    run += cnt[q]
                    mrun += wpos[q]
    if pos_k is None:           # fewer than k tokens with a key: everything is kept
        pos_k, zk = 65535, m_ex[1023] + m_loc[1023]

    # (b) top-p
    pos_p = None
    if pp < 1.0 or fault == "p_one_absorbs_tail":
        thr = pp * zk
        incl = fault == "mask_max_group"       # "mass down to and including" compared, the maximum group not exempt
        for t in live:
            if not (m_ex[t] + m_loc[t] >= thr and 64 * t <= pos_k):
                continue
            best = None
            if m_ex[t] >= thr and (incl or first[t] != pos_max):
                if fault == "later_thread_not_offered":
                    continue
                if first[t] <= pos_k:
                    best = int(first[t])
            else:
                mrun = m_ex[t]
                for j in range(64):
                    q = 64 * t + j
                    if cnt[q]:
                        above = mrun + wpos[q] if incl else mrun
                        if best is None and q <= pos_k and (incl or q != pos_max) and above >= thr:
                            best = q
                        mrun += wpos[q]
            if best is not None and (pos_p is None or best < pos_p):
                pos_p = best

    # (b') min_p
    pos_mp = None
    mp = 0.0 if (min_p is None or greedy) else float(F32(min_p))
    if mp > 0.0:
        for q in ne:
            below = (epos[q] <= mp) if fault == "minp_masks_max" else (epos[q] < mp and q != pos_max)
            if below:
                pos_mp = int(q)
                break

    pos_last = pos_k if pos_p is None else min(pos_k, pos_p - 1)
    if pos_mp is not None:
        pos_last = min(pos_last, pos_mp - 1)

    # (c) the denominator, from the thread that owns pos_last
    z = np.nan                   # never published
    tl = pos_last >> 6
    if 0 <= tl < 1024 and not (fault == "empty_thread_denominator" and c_loc[tl] == 0):
        z = m_ex[tl]
        for q in np.flatnonzero(cnt[64 * tl:pos_last + 1]):
            z = z + wpos[64 * tl + q]
    keep = valid & (pos <= pos_last)
    if split is not None and pos_last == split[0]:
        members = np.flatnonzero(pos == split[0])
        keep[members[split[1]:]] = False
        z -= (members.size - split[1]) * epos[split[0]]
    with np.errstate(all="ignore"):
        probs = np.where(keep, epos[np.where(valid, pos, 0)] / z, 0.0)
        score = probs if (greedy or E is None) else probs / np.asarray(E, F32).astype(F64)
    token = int(np.argmax(np.where(np.isnan(score), -np.inf, score)))
    return probs, token


# ---------------------------------------------------------------------- the checks of the GPU test
def check_row(ref: Sel, probs, token) -> List[str]:
    """What the GPU test asserts of one row, as a list of failures (empty: the row passes)."""
    probs = np.asarray(probs, F64)
    bad = []
    if np.isnan(probs).any() or np.isinf(probs).any() or (probs < 0).any():
        return [f"{int((~np.isfinite(probs)).sum())} non-finite / {int((probs < 0).sum())} negative probabilities"]
    got = probs > 0
    if not np.array_equal(got, ref.nonzero):
        extra, miss = np.flatnonzero(got & ~ref.nonzero), np.flatnonzero(~got & ref.nonzero)
        bad.append(f"kept set: {got.sum()} tokens, want {ref.nonzero.sum()} ({extra.size} extra {extra[:4]}, {miss.size} missing {miss[:4]})")
    err = float(np.abs(probs - ref.probs).max())
    if not err <= PROB_BAR:
        bad.append(f"|probs - ref| = {err:.3e} > {PROB_BAR:.1e}")
    if not abs(float(probs.sum()) - 1.0) <= SUM_BAR:
        bad.append(f"row sum {probs.sum():.8f}")
    if int(token) != ref.token:
        bad.append(f"token {int(token)}, want {ref.token}")
    return bad


# ---------------------------------------------------------------------- the cases
@dataclass
class Case:
    name: str
    logits: np.ndarray          # [V] fp16
    temperature: float
    top_k: int
    top_p: Optional[float]      # None: the call passes no top_p array at all
    min_p: float
    E: np.ndarray               # [V] fp32 exponential noise (ones for a greedy row)
    tags: Tuple[str, ...]
    ref: Sel = field(repr=False, default=None)

    @property
    def V(self) -> int:
        return self.logits.size


TAGS = (
    # top-k
    "tk_first_key", "tk_last_key", "tk_inside_group_last_key", "tk_exact_group_end", "tk_next_same_thread", "tk_next_thread",
    "tk_next_after_empty_threads", "tk_next_across_wave", "k=1", "k=V-1", "k=V", "k=V+5", "k=0", "k=-1", "k_exceeds_finite",
    "k1_tie_at_max",
    # top-p
    "tp_mid_thread", "tp_later_thread_adjacent", "tp_later_thread_one_empty", "tp_later_thread_many_empty", "tp_across_wave",
    "tp_pos_last_in_empty_thread", "tp_first_masked_last_key", "tp_max_alone_same_thread", "tp_max_alone_later_thread",
    "tp_above_top_k", "tk_above_top_p", "tp_1e-6", "tp_one_wide", "tp_none_wide",
    # min_p
    "mp_binding", "mp_not_binding", "mp_first_key", "mp_last_key", "mp_one", "mp_zero", "tightest_top_k", "tightest_top_p",
    "tightest_min_p",
    # signed zeros
    "sz_top_k", "sz_top_p", "sz_min_p", "sz_max_small_p",
    # values
    "subnormals", "fp16_ceiling", "neg_inf_every_third", "T=0.05", "T=0.3", "T=1.0", "T=2.0", "greedy", "negative_edge",
    "nan_takes_no_part",
    # sizes
    "V=1", "V=7", "V=64", "V=1003", "V=16384", "V=16385", "V=40000", "V=131080_uniform",
)

FILL_POS = pos_of(-12.0)      # the filler group that brings a row to its V: far below everything a case is about


def _finish(name, logits, T, k, p, mp, tags, seed) -> Case:
    """Derive the parameters from the row, draw E, attach the reference.  p / mp: a number, None, or ("g", i): the
    boundary lies just above group i (descending group index): that group is the first one masked."""
    logits = np.asarray(logits, F16)
    vals, cnt, inv, l, r, greedy = _groups(logits, T)
    V = logits.size
    kk = V if (k <= 0 or k > V) else k
    cum = np.cumsum(cnt)
    gk = len(cnt) - 1 if kk > cum[-1] else int(np.searchsorted(cum, kk))
    if isinstance(p, tuple):
        g = p[1]
        incl = np.cumsum(cnt * r)
        above = np.concatenate([[0.0], incl[:-1]]) / incl[gk]
        assert 1 <= g <= gk + 1, (name, g, gk)
        hi = above[g] if g <= gk else 1.0
        p = float(F32(0.5 * (above[g - 1] + hi)))
    if isinstance(mp, tuple):
        g = mp[1]
        assert g >= 1 and r[g] > 0
        mp = float(F32(np.sqrt(r[g - 1] * r[g])))
    p, mp = (None if p is None else float(F32(p))), float(F32(mp))      # what the fp32 parameter arrays will hold
    sel = ref_select(logits, T, k, p, mp)
    assert sel.gap_p >= GAP_TOP_P, (name, sel.gap_p)
    assert sel.gap_mp >= GAP_MIN_P, (name, sel.gap_mp)
    fin = sel.d[np.isfinite(sel.d)]
    assert not ((fin > CLEAR_ZONE[0]) & (fin < CLEAR_ZONE[1])).any(), (name, "a token in the underflow zone")
    if greedy:
        E = np.ones(V, F32)
    else:
        while True:
            E = np.random.default_rng(seed).exponential(1.0, V).astype(F32)
            E = np.maximum(E, F32(1e-6))
            s = np.sort(sel.probs / E.astype(F64))
            if V == 1 or s[-1] >= (1.0 + GAP_E) * s[-2]:
                break
            seed += 1000
    return Case(name, logits, float(F32(T)), int(k), p, float(mp), E, tuple(tags), ref_select(logits, T, k, p, mp, E))


def _grp(name, groups, tags, V=1003, T=1.0, k=-1, p=1.0, mp=0.0, seed=0, neg_zeros=0, fill=FILL_POS) -> Case:
    """A row of (position, count) groups plus the filler group that brings it to V tokens."""
    n = sum(c for _, c in groups)
    groups = list(groups)
    if n < V:
        assert fill > groups[-1][0]
        groups.append((fill, V - n))
    return _finish(name, build_row(groups, V, 7919 * seed + 11, neg_zeros), T, k, p, mp, tags, seed)


def _gauss(V, seed, sigma=3.0, clip=9.0):
    return np.clip(np.random.default_rng(seed).standard_normal(V) * sigma, -clip, clip).astype(F16)


_CASES: Optional[List[Case]] = None


def cases() -> List[Case]:
    global _CASES
    if _CASES is not None:
        return _CASES
    c: List[Case] = []
    P = pos_of
    A = 250           # a thread of wave 3 (values ~2.7), above the threads the boundaries sit in
    hi = (th(A, 10), 3)

    # ------------------------------------------------ top-k
    c.append(_grp("tk_first_key", [hi, (th(260, 0), 2), (th(260, 5), 4)], ["tk_first_key"], k=5, seed=1))
    c.append(_grp("tk_last_key", [hi, (th(260, 63), 1), (th(261, 0), 4)], ["tk_last_key"], k=4, seed=2))
    c.append(_grp("tk_inside_group_last_key", [hi, (th(260, 63), 5), (th(261, 7), 2)], ["tk_inside_group_last_key"], k=5, seed=3))
    c.append(_grp("tk_exact_group_end", [hi, (th(260, 20), 4), (th(260, 21), 2)], ["tk_exact_group_end"], k=7, seed=4))
    c.append(_grp("tk_next_same_thread", [(th(260, 3), 3), (th(260, 9), 4), (th(260, 40), 2)], ["tk_next_same_thread"], k=4, seed=5))
    c.append(_grp("tk_next_thread", [(th(260, 3), 3), (th(261, 9), 4), (th(263, 0), 2)], ["tk_next_thread"], k=4, seed=6))
    c.append(_grp("tk_next_after_empty_threads", [(th(260, 3), 3), (th(265, 9), 4), (th(266, 0), 2)],
                  ["tk_next_after_empty_threads"], k=4, seed=7))
    c.append(_grp("tk_next_across_wave", [(4 * 4096 - 1, 3), (4 * 4096, 4), (4 * 4096 + 1, 2)], ["tk_next_across_wave"], k=4, seed=8))
    c.append(_grp("tk_next_across_wave_negative", [hi, (12 * 4096 - 1, 3), (12 * 4096, 4), (12 * 4096 + 64, 2)],
                  ["tk_next_across_wave", "negative_edge"], k=7, seed=9, fill=P(-14.0)))
    seven = [(P(v), 1) for v in (2.5, 1.5, 0.75, 0.25, -0.5, -1.25, -3.0)]
    for k in (1, 6, 7, 12, 0, -1):
        tag = {1: "k=1", 6: "k=V-1", 7: "k=V", 12: "k=V+5", 0: "k=0", -1: "k=-1"}[k]
        c.append(_grp(f"tk_{tag}", seven, [tag, "V=7"], V=7, k=k, p=1.0, seed=10 + (k & 15)))
    c.append(_grp("tk_k=V-1_tie_at_the_bottom", seven[:5] + [(P(-1.25), 2)], ["k=V-1", "V=7"], V=7, k=6, seed=29))
    c.append(_grp("tk_k_exceeds_finite", [(P(2.0), 1), (P(1.0), 2), (P(-1.0), 1), (POS_NEG_INF, 3)], ["k_exceeds_finite"],
                  V=7, k=6, seed=30))
    c.append(_grp("tk_k1_tie_at_max", [(th(260, 63), 3), (th(261, 0), 2)], ["k1_tie_at_max", "k=1"], k=1, seed=31))

    # ------------------------------------------------ top-p (single tokens around 1.5 .. 2.7: every group carries mass)
    one = lambda *ps: [(q, 1) for q in ps]
    c.append(_grp("tp_mid_thread", one(th(258, 5), th(260, 10), th(260, 20), th(260, 30), th(262, 3)), ["tp_mid_thread"],
                  p=("g", 3), seed=40))
    c.append(_grp("tp_later_thread_adjacent", one(th(258, 5), th(260, 10), th(260, 40), th(261, 7), th(262, 3)),
                  ["tp_later_thread_adjacent"], p=("g", 3), seed=41))
    c.append(_grp("tp_later_thread_one_empty", one(th(258, 5), th(260, 10), th(260, 40), th(262, 7), th(262, 9)),
                  ["tp_later_thread_one_empty"], p=("g", 3), seed=42))
    c.append(_grp("tp_later_thread_many_empty", one(th(258, 5), th(260, 10), th(260, 40), th(270, 7), th(275, 9)),
                  ["tp_later_thread_many_empty"], p=("g", 3), seed=43))
    c.append(_grp("tp_across_wave", one(th(250, 5), 4 * 4096 - 70, 4 * 4096 - 1, 4 * 4096, 4 * 4096 + 1), ["tp_across_wave"],
                  p=("g", 3), seed=44))
    c.append(_grp("tp_across_wave_negative", one(P(0.5), P(-1.0), 12 * 4096 - 1, 12 * 4096, 12 * 4096 + 3),
                  ["tp_across_wave", "negative_edge"], p=("g", 3), seed=45, fill=P(-14.0)))
    c.append(_grp("tp_pos_last_in_empty_thread", one(th(258, 5), th(260, 10), th(260, 40), th(262, 0), th(262, 1)),
                  ["tp_pos_last_in_empty_thread"], p=("g", 3), seed=46))
    c.append(_grp("tp_first_masked_last_key", one(th(258, 5), th(260, 10), th(260, 40), th(260, 63), th(261, 0)),
                  ["tp_first_masked_last_key"], p=("g", 3), seed=47))
    c.append(_grp("tp_max_alone_same_thread", [(th(260, 3), 2), (th(260, 9), 1), (th(261, 9), 1)], ["tp_max_alone_same_thread"],
                  p=("g", 1), seed=48))
    c.append(_grp("tp_max_alone_later_thread", [(th(260, 3), 2), (th(263, 0), 1), (th(263, 9), 1)], ["tp_max_alone_later_thread"],
                  p=("g", 1), seed=49))
    six = one(th(255, 1), th(257, 2), th(259, 3), th(261, 4), th(263, 5), th(265, 6))
    c.append(_grp("tp_above_top_k", six, ["tp_above_top_k"], k=5, p=("g", 2), seed=50))
    c.append(_grp("tk_above_top_p", six, ["tk_above_top_p"], k=2, p=("g", 2), seed=51))
    c.append(_grp("tp_groups_whole", [(th(258, 5), 2), (th(260, 10), 3), (th(260, 40), 5), (th(262, 0), 4), (th(262, 1), 2)],
                  ["tp_pos_last_in_empty_thread"], p=("g", 3), seed=57))       # the last kept and the first masked group: 5 and 4 tokens
    c.append(_grp("tp_groups_whole_top_k_inside", [(th(258, 5), 2), (th(260, 10), 3), (th(260, 63), 5), (th(261, 0), 4), (th(270, 1), 6)],
                  ["tp_later_thread_adjacent"], k=16, p=("g", 3), seed=58))    # k ends inside a group that top-p masks
    c.append(_grp("tp_1e-6",[(th(255, 1), 2)] + six[1:], ["tp_1e-6"], p=1e-6, seed=52))
    wide = np.linspace(30.0, -30.0, 1003).astype(F16)          # 60 nats at T = 1: the tail weighs < 1/2 ulp of the mass above it
    wide = wide[np.random.default_rng(53).permutation(1003)]
    c.append(_finish("tp_one_wide", wide, 1.0, -1, 1.0, 0.0, ["tp_one_wide"], 53))
    c.append(_finish("tp_none_wide", wide, 1.0, -1, None, 0.0, ["tp_none_wide"], 54))
    peak = np.clip(np.random.default_rng(55).standard_normal(1003) * 4.0, -12.0, 12.0).astype(F16)
    peak[500] = F16(30.0)                                       # N(0, 4^2) with one logit at 30, T = 0.7: 60 nats again
    c.append(_finish("tp_one_peaked", peak, 0.7, -1, 1.0, 0.0, ["tp_one_wide"], 55))
    c.append(_finish("tp_one_wide_top_k", wide, 1.0, 900, 1.0, 0.0, ["tp_one_wide"], 56))

    # ------------------------------------------------ min_p
    c.append(_grp("mp_binding", six, ["mp_binding"], mp=("g", 3), seed=60))
    c.append(_grp("mp_not_binding", six, ["mp_not_binding"], mp=1e-12, seed=61))
    c.append(_grp("mp_first_key", one(th(255, 1), th(259, 30), th(262, 0), th(262, 1)), ["mp_first_key", "mp_binding"],
                  mp=("g", 2), seed=62))
    c.append(_grp("mp_last_key", one(th(255, 1), th(259, 30), th(262, 63), th(263, 0)), ["mp_last_key", "mp_binding"],
                  mp=("g", 2), seed=63))
    c.append(_grp("mp_across_wave", one(th(250, 5), 4 * 4096 - 1, 4 * 4096, 4 * 4096 + 1), ["mp_first_key", "mp_binding"], T=0.3,
                  mp=("g", 2), seed=69))
    c.append(_grp("mp_one", [(th(255, 1), 2)] + six[1:], ["mp_one"], mp=1.0, seed=64))
    c.append(_grp("mp_zero", six, ["mp_zero"], k=4, mp=0.0, seed=65))
    c.append(_grp("tightest_top_k", six, ["tightest_top_k"], k=2, p=("g", 2), mp=("g", 5), seed=66))
    c.append(_grp("tightest_top_p", six, ["tightest_top_p"], k=5, p=("g", 2), mp=("g", 4), seed=67))
    c.append(_grp("tightest_min_p", six, ["tightest_min_p"], k=5, p=("g", 4), mp=("g", 2), seed=68))

    # ------------------------------------------------ signed zeros: +0.0 and -0.0 are one group
    Z = POS_ZERO
    c.append(_grp("sz_top_k", [(P(3.0), 1), (P(2.0), 1), (P(1.0), 1), (Z, 4), (P(-1.0), 1), (P(-2.0), 1)], ["sz_top_k"],
                  k=4, neg_zeros=2, seed=70))
    c.append(_grp("sz_top_p_last_kept", [(P(2.0), 1), (P(1.0), 1), (Z, 4), (P(-1.0), 1), (P(-2.0), 1)], ["sz_top_p"],
                  p=("g", 3), neg_zeros=1, seed=71))
    c.append(_grp("sz_top_p_first_masked", [(P(2.0), 1), (P(1.0), 1), (Z, 4), (P(-1.0), 1)], ["sz_top_p"],
                  p=("g", 2), neg_zeros=2, seed=72))
    c.append(_grp("sz_min_p_last_kept", [(P(2.0), 1), (P(1.0), 1), (Z, 4), (P(-1.0), 1), (P(-2.0), 1)], ["sz_min_p"],
                  mp=("g", 3), neg_zeros=2, seed=73))
    c.append(_grp("sz_min_p_first_masked", [(P(2.0), 1), (P(1.0), 1), (Z, 4), (P(-1.0), 1)], ["sz_min_p"],
                  mp=("g", 2), neg_zeros=3, seed=74))
    c.append(_grp("sz_max_small_p", [(Z, 4), (P(-1.0), 1), (P(-2.0), 2)], ["sz_max_small_p"], p=0.01, neg_zeros=2, seed=75))
    c.append(_grp("sz_max_top_k_1", [(Z, 4), (P(-1.0), 1), (P(-2.0), 2)], ["sz_top_k", "k=1"], k=1, neg_zeros=3, seed=76))

    # ------------------------------------------------ values
    sub = np.arange(1, 502, dtype=np.uint16)                   # every positive and negative fp16 subnormal up to 501 * 2^-24
    sub = np.concatenate([sub, sub | 0x8000, np.array([0], np.uint16)]).view(F16)
    sub = sub[np.random.default_rng(80).permutation(1003)]
    c.append(_finish("subnormals", sub, 2e-5, 50, 1.0, 0.0, ["subnormals"], 80))
    top = _gauss(1003, 81)
    top[17] = F16(60000.0)
    c.append(_finish("fp16_ceiling", top, 1.0, -1, 0.9, 0.0, ["fp16_ceiling"], 81))
    third = _gauss(1003, 82)
    third[::3] = F16(-np.inf)
    c.append(_finish("neg_inf_every_third", third, 0.8, 40, ("g", 12), 0.0, ["neg_inf_every_third"], 82))
    holes = _gauss(1003, 79)
    holes[7::50] = F16(np.nan)                                  # a NaN logit takes no part: no key, no count towards k, probability 0
    c.append(_finish("nan_takes_no_part", holes, 0.9, 30, ("g", 8), 0.0, ["nan_takes_no_part"], 79))
    cold = np.random.default_rng(83).uniform(-4.0, 1.5, 1003).astype(F16)
    cold[np.arange(7) * 100 + 3] = np.array([8.0, 7.5, 7.0, 6.5, 6.0, 5.5, 5.0], F16)   # everything else underflows at T = 0.05
    c.append(_finish("T=0.05", cold, 0.05, -1, 1.0, 0.0, ["T=0.05"], 83))
    c.append(_finish("T=0.05_top_p", cold, 0.05, 5, ("g", 1), 0.0, ["T=0.05"], 84))
    c.append(_finish("T=0.3", _gauss(1003, 85), 0.3, 100, ("g", 6), 0.0, ["T=0.3", "V=1003"], 85))
    c.append(_finish("T=1.0", _gauss(1003, 86), 1.0, 300, ("g", 40), ("g", 30), ["T=1.0", "V=1003"], 86))
    c.append(_finish("T=2.0", _gauss(1003, 87), 2.0, 800, ("g", 200), 0.0, ["T=2.0", "V=1003"], 87))
    c.append(_finish("greedy", _gauss(1003, 88), 0.0, -1, 1.0, 0.0, ["greedy"], 88))
    c.append(_grp("greedy_tie_at_max", [(th(260, 63), 3), (th(261, 0), 2)], ["greedy"], T=0.0, mp=0.3, seed=97))
    # (a greedy row ignores a min_p it still carries and takes the first index of the maximum group)
    c.append(_grp("tk_last_key_negative", [hi, (P(-0.25), 2), (th(730, 63), 1), (th(731, 0), 4)], ["tk_last_key", "negative_edge"],
                  k=6, seed=89, fill=P(-14.0)))

    # ------------------------------------------------ sizes
    c.append(_finish("V=1", np.array([1.5], F16), 0.7, 3, 0.5, 0.1, ["V=1"], 90))
    c.append(_finish("V=64", _gauss(64, 91), 0.9, 20, ("g", 8), 0.0, ["V=64"], 91))
    c.append(_finish("V=64_min_p", _gauss(64, 92), 1.1, -1, 1.0, ("g", 10), ["V=64", "mp_binding"], 92))
    for V, seed in ((16384, 93), (16385, 94), (40000, 95)):       # one histogram chunk exactly, one token more, three chunks
        c.append(_finish(f"V={V}", _gauss(V, seed), 0.8, 500, ("g", 60), 0.0, [f"V={V}"], seed))
    c.append(_finish("V=131080_uniform", np.full(131080, 0.25, F16), 1.0, 5, 0.3, 0.0, ["V=131080_uniform"], 96))
    # nine histogram chunks, eight tokens in the last one, 131080 counts in one bin: the group stays whole

    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    _CASES = c
    return c


def batches(max_rows: int = 17) -> List[List[Case]]:
    """The cases grouped by V (and by whether the call passes a top_p array) into calls of at most 17 rows: rows of a call
    differ in every parameter, and the row index reaches past 16."""
    by = {}
    for x in cases():
        by.setdefault((x.V, x.top_p is None), []).append(x)
    out = []
    for rows in by.values():
        for i in range(0, len(rows), max_rows):
            out.append(rows[i:i + max_rows])
    return out


def batch_arrays(rows: List[Case]):
    """-> logits [n, V] fp16, temperature [n] fp32, top_k [n] int32, top_p [n] fp32 or None, min_p [n] fp32, E [n, V] fp32."""
    top_p = None if rows[0].top_p is None else np.array([x.top_p for x in rows], F32)
    return (np.stack([x.logits for x in rows]), np.array([x.temperature for x in rows], F32),
            np.array([x.top_k for x in rows], np.int32), top_p, np.array([x.min_p for x in rows], F32),
            np.stack([x.E for x in rows]))
