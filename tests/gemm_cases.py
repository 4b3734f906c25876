"""GEMM cases for the parity tests: float64 references, the host-side dispatch rule of every GEMM entry restated in
Python, and a case list that reaches every row of that rule -- the GEMM counterpart of attn_cases.py.

Rows (what `route` returns; the product build's defaults: stream cap 256, QSPEC_TILED_MIN_M 17, head LDS-DMA on, the
W4A16 workspace always passed):
  W4A4  rowwise_scaled_linear_cutlass_s4s4_unified
    a4.longk        gemm_stream_w4a4.hip gemm_w4a4_longk_kernel           no bias, M 1..16, K = 28672
    a4.stream1      gemm_w4a4_stream_kernel, one token tile          no bias, M 1..16, K in stream_shape
    a4.stream2      gemm_w4a4_stream_kernel, two token tiles         no bias, M 17..32, K in stream_shape with NW >= 8
    a4.gen{1,2,4}   gemm.hip gemm_w4a4_kernel<MT>                    the rest, one launch per 64-row pass
  W4A16 w4a16_linear
    w16.stream16(NW,UB)   gemm_w4a16_stream_kernel                   no bias, M 1..16, K in stream16_shape
    w16.partial(S)        the same kernel over K / S + the finish     no bias, M 1..16, K / S in stream16_shape
    w16.tiled(MT,1|S)     gemm_tiled.hip (+ the finish when S > 1)    no bias, M >= 17, N % 128, K % 256, K >= 512
    w16.gen2d(MT,1|S)     gemm.hip gemm_w4a16_2d_kernel               N % 64, M <= 32, N / 64 >= 192 or K >= 8192
    w16.gen{16,32}        gemm.hip gemm_w4a16_kernel<MT>              the rest, one launch per 32-row pass
  fp16  linear_f16
    f16.sdma / f16.sdma2  gemm_f16_sdma_kernel / gemm_f16_sdma2_kernel   K = 4096, >= 4 tiles per workgroup
    f16.longk             gemm_f16_longk_kernel                      M <= 16, K = 8192
    f16.stream(NW,UB)     gemm_f16_stream_kernel                     M <= 16, K in {1024, 2048, 4096, 5120}
    f16.tiled(MT)         gemm_tiled.hip gemm_f16_tiled_kernel<MT>   M > 16, N % 32, K % 256, K >= 512
    f16.gen{1,2}          gemm.hip gemm_f16_kernel<MT>               the rest, one launch per 32-row pass
  raw partial sums
    a4.ipart          rowwise_scaled_linear_s4s4_partial   (int32 K-slice sums)
    w16.partial_raw   w4a16_linear_partial                 (fp32 K-slice sums; stream form at M <= 16, tiled above)
    w16.ksliced_raw   w4a16_linear_ksliced_raw             (fp32 sums of a K range; stream form or gemm.hip EPI_RAW)

Two data tiers per case:
  exact      every product lies on a grid of step u and the sum of |products| stays below 2^24 u, so every fp32 partial
             sum is exact in any order; the sums themselves go far past what fp16 holds exactly.  Bars: W4A4 / W4A16
             within 1 fp16 ulp and correctly rounded on all but max(1, 0.1 %) of the elements; fp16 bit-exact.
             Where a bias is added, both tiers also allow 2^-22 (|acc s| + |bias|): the fp32 epilogue's own roundings,
             which show where the bias cancels the product.  A rounding that is not the correct one is excused only
             where r lies within the epilogue's fp32 roundings of an fp16 rounding boundary (double rounding).
  realistic  activations with outlier channels, realistic scales.  Bars: within 1 ulp16(r) + 2^-20 sum|x w| s,
             correctly rounded on all but max(1, 1 %), and a mean signed error per row within 0.02 + 1.2 / sqrt(n) ulps.
"""
import math
from dataclasses import dataclass

import numpy as np

# ------------------------------------------------------------------ constants of the product build

STREAM_CAP = 256            # stream_common.cuh stream_cap()
TILED_MIN_M = 17            # capi.hip tiled_min_m()
W16_CNT_BYTES = 8192        # gemm.hip QS_W16_CNT_SLOTS * sizeof(int): the ticket counters at the front of the workspace
W16_CNT_SLOTS = 2048
W16_PART_BYTES = 32 * 1024 * 1024
W16_WS_BYTES = W16_CNT_BYTES + W16_PART_BYTES

# gemm_stream_w4a4.hip QS_W4A4_SHAPES: K / 128 = NW * UB
A4_STREAM_SHAPES = ((8, 4), (16, 7), (8, 8), (8, 5), (4, 4), (4, 2), (4, 7), (12, 9), (4, 11))
# gemm_stream_w4a16.hip QS_W4A16_SHAPES16
W16_STREAM_SHAPES = ((8, 4), (8, 8), (8, 5), (4, 4), (4, 2), (8, 7), (4, 7), (4, 1), (4, 9), (4, 11))
F16_STREAM = {4096: (8, 16), 2048: (8, 8), 1024: (4, 8), 5120: (8, 20)}   # gemm_f16_stream(); 8192 is the longk kernel


# ------------------------------------------------------------------ int4 packing (independent of the oracle)

def pack_i4(q):
    """[.., K] int values in [-8, 7] -> [.., K/2] int8, byte j = (q[2j] & 0xF) | (q[2j+1] << 4)."""
    q = np.asarray(q).astype(np.int16)
    lo, hi = q[..., 0::2] & 0xF, (q[..., 1::2] & 0xF) << 4
    return (lo | hi).astype(np.uint8).view(np.int8)


_NIB = np.arange(16, dtype=np.int16)
_NIB = np.where(_NIB >= 8, _NIB - 16, _NIB)
_UNPACK = np.stack([_NIB[np.arange(256) & 0xF], _NIB[np.arange(256) >> 4]], axis=1).astype(np.int8)   # byte -> (lo, hi)


def unpack_i4(p):
    """[.., K/2] packed bytes -> [.., K] int8 (two's complement nibbles, low nibble first)."""
    b = np.ascontiguousarray(p).view(np.uint8)
    return _UNPACK[b].reshape(b.shape[:-1] + (2 * b.shape[-1],))


# ------------------------------------------------------------------ float64 references (BLAS matmul)

_CHUNK = 2048   # weight rows per block: the float64 copy of a wide layer stays small


def _dot_rows(x64, w_rows_fn, N):
    """x64 [M, K] float64; w_rows_fn(n0, n1) -> [n1 - n0, K] float64.  Returns (sum x w [M, N], sum |x w| [M, N])."""
    M = x64.shape[0]
    s = np.empty((M, N)); a = np.empty((M, N))
    ax = np.abs(x64)
    for n0 in range(0, N, _CHUNK):
        n1 = min(N, n0 + _CHUNK)
        w = w_rows_fn(n0, n1)
        s[:, n0:n1] = x64 @ w.T
        a[:, n0:n1] = ax @ np.abs(w).T
    return s, a


def _f64(a):
    return np.asarray(a).astype(np.float64)


def ref_w4a4(xq, xs, wq, ws, bias=None, with_abs=False):
    """(sum_k x w) xs ws (+ bias), float64; xq [M, K/2], wq [N, K/2] packed."""
    x = _f64(unpack_i4(xq))
    s, a = _dot_rows(x, lambda n0, n1: _f64(unpack_i4(wq[n0:n1])), wq.shape[0])
    scale = _f64(xs).reshape(-1, 1) * _f64(ws).reshape(1, -1)
    r = s * scale
    if bias is not None:
        r = r + _f64(bias).reshape(1, -1)
    return (r, a * np.abs(scale)) if with_abs else r


def ref_w4a16(x, wq, ws, bias=None, with_abs=False):
    """(sum_k x w) ws (+ bias), float64; x [M, K] fp16, wq [N, K/2] packed."""
    s, a = _dot_rows(_f64(x), lambda n0, n1: _f64(unpack_i4(wq[n0:n1])), wq.shape[0])
    sc = _f64(ws).reshape(1, -1)
    r = s * sc
    if bias is not None:
        r = r + _f64(bias).reshape(1, -1)
    return (r, a * np.abs(sc)) if with_abs else r


def ref_w4a16_raw(x, wq):
    """Unscaled sum_k x w, float64 (what the raw partial entries sum in fp32)."""
    return _dot_rows(_f64(x), lambda n0, n1: _f64(unpack_i4(wq[n0:n1])), wq.shape[0])[0]


def ref_f16(x, w, with_abs=False):
    s, a = _dot_rows(_f64(x), lambda n0, n1: _f64(w[n0:n1]), w.shape[0])
    return (s, a) if with_abs else s


# ------------------------------------------------------------------ dispatch rule (capi.hip + launchers) restated

def a4_stream_shape(K):
    if K % 128:
        return None
    for nw, ub in A4_STREAM_SHAPES:
        if K // 128 == nw * ub:
            return nw, ub
    return None


def w16_stream_shape(K):
    if K % 128:
        return None
    for nw, ub in W16_STREAM_SHAPES:
        if K // 128 == nw * ub:
            return nw, ub
    return None


def a4_stream_lds(M, K, NW, MT):
    """gemm_stream_w4a4.hip stream_lds_bytes() for the (xq, xs) prologue (no staged rows)."""
    NG, RB = NW // 4, (4 if NW == 4 else (2 if NW == 8 else 1))
    return 64 + 2 * NW * MT * 1024 + MT * 1024 + 3 * NG * RB * 32 * 4


def a4_stream_supported(M, N, K):
    """gemm_w4a4_stream_supported(M, N, K, ln=false) == qspec_rowwise_scaled_linear_s4s4_residual_supported."""
    if 1 <= M <= 16 and N % 16 == 0 and K == 28672:
        return True
    sh = a4_stream_shape(K)
    if not (1 <= M <= 32) or N % 16 or K > (1 << 19) or sh is None:
        return False
    if M > 16 and sh[0] < 8:
        return False
    return a4_stream_lds(M, K, sh[0], 2 if M > 16 else 1) <= 160 * 1024


def a4_ipart_slices(M, N, K):
    """gemm_w4a4_stream_partial_slices == qspec_rowwise_scaled_linear_s4s4_partial_slices."""
    if M < 17 or M > 32 or N % 32 or N // 16 > STREAM_CAP:
        return 0
    return 2 if K == 14336 else 0


def w16_stream_supported(M, N, K):
    return 1 <= M <= 16 and N % 16 == 0 and w16_stream_shape(K) is not None


def w16_stream_partial_slices(M, N, K):
    """gemm_w4a16_stream_partial_slices: four slices first, then two, then three."""
    if w16_stream_supported(M, N, K):
        return 0
    for S in (4, 2, 3):
        if K % S == 0 and w16_stream_supported(M, N, K // S):
            return S
    return 0


def w16_tiled_supported(M, N, K):
    return M >= 1 and N % 128 == 0 and K % 256 == 0 and K >= 512


def w16_tiled_plan(M, N, K, part_bytes):
    """gemm_tiled.hip gemm_w4a16_tiled_plan (the cost model, same double arithmetic) -> (MT, S)."""
    unit = 512 if K % 512 == 0 else 256
    best, bmt, bs = 1e30, 1, 1
    for mt in range(1, 5):
        mb = (M + 32 * mt - 1) // (32 * mt)
        for sl in range(1, 9):
            if K % (sl * unit):
                continue
            if sl > 1 and sl * M * N * 4 > part_bytes:
                continue
            wgs = float((N // 128) * mb * sl)
            steps = float(K // sl // 64)
            rounds = float((int(wgs) + 511) // 512)
            share = 1.0 if wgs > 256 else 0.62
            comp = rounds * steps * (0.06 + 0.265 * mt) * share
            traffic = (float(N) * K / 2 * mb) / 5.5e6
            t = (comp if comp > traffic else traffic) + 4.0
            if sl > 1:
                t += 1.5 + float(sl) * M * N * 8 / 5e6
            if t < best:
                best, bmt, bs = t, mt, sl
    return bmt, bs


def w16_tiled_partial_slices(M, N, K):
    if not w16_tiled_supported(M, N, K):
        return 0
    S = w16_tiled_plan(M, N, K, W16_WS_BYTES - 8192)[1]
    return S if S > 1 else 0


def w16_linear_partial_slices(M, N, K):
    """qspec_w4a16_linear_partial_slices."""
    if M > 16:
        return w16_tiled_partial_slices(M, N, K) if M >= TILED_MIN_M else 0
    return w16_stream_partial_slices(M, N, K)


def w16_tiled_variant(M, N, K, MT, S):
    """tiled_launch(): (MT, RING, NT) of gemm_w4a16_tiled_kernel."""
    mblocks = (M + 32 * MT - 1) // (32 * MT)
    NT = 2 if (N % 256 == 0 and (N // 256) * mblocks * S >= 192) else 1
    RING = 8 if (K % 512 == 0 and NT == 1) else 4
    return MT, RING, NT


def w16_gen2d_plan(M, N, K):
    """launch_w4a16 2-D branch: (MT, S) or None."""
    if not (N % 64 == 0 and M <= 32 and (N // 64 >= 192 or K >= 8192)):
        return None
    nblocks, nrounds, MT = N // 64, (K // 128 + 3) // 4, (1 if M <= 16 else 2)
    S = 1
    if nblocks <= W16_CNT_SLOTS:
        S = min(8, (256 + nblocks - 1) // nblocks)
        while S > 1 and nrounds // S < 2:
            S -= 1
        while S > 1 and S * nblocks * 4 * MT * 256 * 4 > W16_PART_BYTES:
            S -= 1
    rounds_per = (nrounds + S - 1) // S
    return MT, (nrounds + rounds_per - 1) // rounds_per


def f16_stream_grid(N):
    ntiles = N // 16
    if ntiles <= 256:
        return ntiles
    per = (ntiles + 255) // 256
    return (ntiles + per - 1) // per


def f16_stream_supported(M, N, K):
    if 16 < M <= 32 and K == 4096 and N % 16 == 0 and N // 16 >= 4 * f16_stream_grid(N):
        return True
    return 1 <= M <= 16 and N % 16 == 0 and K in (1024, 2048, 4096, 5120, 8192)


def f16_tiled_mt(M):
    blocks = (M + 127) // 128
    per = (M + blocks - 1) // blocks
    return (per + 31) // 32


def _gen_passes(M, step, names):
    """One launch per `step`-row pass; names[i] for a pass of <= (i + 1) * 16 rows (the last name above that)."""
    out = []
    for mb in range(0, M, step):
        rows = M - mb
        out.append(names[min((rows - 1) // 16, len(names) - 1)])
    return tuple(out)


def route(op, M, N, K, bias=False):
    """Rows that one call of `op` launches, in launch order (a tuple: the first-generation kernels loop over row
    passes, so M = 80 on the W4A4 path is ('a4.gen4', 'a4.gen1')).  op: 'a4', 'w16', 'f16', 'a4.ipart',
    'w16.partial_raw', 'w16.ksliced_raw' (K = the K range)."""
    if op == "a4":
        assert N % 16 == 0 and K % 128 == 0
        if not bias and a4_stream_supported(M, N, K):
            if K == 28672 and M <= 16:
                return ("a4.longk",)
            return ("a4.stream1",) if M <= 16 else ("a4.stream2",)
        return _gen_passes(M, 64, ("a4.gen1", "a4.gen2", "a4.gen4"))
    if op == "w16":
        assert N % 16 == 0 and K % 128 == 0
        if not bias and w16_stream_supported(M, N, K):
            return ("w16.stream16(%d,%d)" % w16_stream_shape(K),)
        S = 0 if bias else w16_stream_partial_slices(M, N, K)
        if S > 0 and S * M * N * 4 + 8192 <= W16_WS_BYTES:
            return (f"w16.partial({S})",)
        if not bias and M >= TILED_MIN_M and w16_tiled_supported(M, N, K):
            MT, S = w16_tiled_plan(M, N, K, W16_WS_BYTES - 8192)
            return (f"w16.tiled({MT},{'S' if S > 1 else 1})",)
        p = w16_gen2d_plan(M, N, K)
        if p is not None:
            return (f"w16.gen2d({p[0]},{'S' if p[1] > 1 else 1})",)
        return _gen_passes(M, 32, ("w16.gen16", "w16.gen32"))
    if op == "f16":
        assert K % 32 == 0
        if f16_stream_supported(M, N, K):
            if M > 16:
                return ("f16.sdma2",)
            if K == 4096 and N // 16 >= 4 * min_grid_f16(N):
                return ("f16.sdma",)
            if K == 8192:
                return ("f16.longk",)
            return ("f16.stream(%d,%d)" % F16_STREAM[K],)
        if M > 16 and N % 32 == 0 and K % 256 == 0 and K >= 512:
            return (f"f16.tiled({f16_tiled_mt(M)})",)
        return _gen_passes(M, 32, ("f16.gen1", "f16.gen2"))
    if op == "a4.ipart":
        assert a4_ipart_slices(M, N, K) > 1
        return ("a4.ipart",)
    if op == "w16.partial_raw":
        assert w16_linear_partial_slices(M, N, K) > 1
        return ("w16.partial_raw",)
    if op == "w16.ksliced_raw":
        assert M <= 32
        return ("w16.ksliced_raw",)
    raise ValueError(op)


def min_grid_f16(N):
    """gemm_f16_stream's grid at M <= 16 (the stream cap, 256)."""
    ntiles = N // 16
    if ntiles <= STREAM_CAP:
        return ntiles
    per = (ntiles + STREAM_CAP - 1) // STREAM_CAP
    return (ntiles + per - 1) // per


ROWS = (
    ["a4.longk", "a4.stream1", "a4.stream2", "a4.gen1", "a4.gen2", "a4.gen4"]
    + ["w16.stream16(%d,%d)" % s for s in W16_STREAM_SHAPES]
    + [f"w16.partial({S})" for S in (2, 3, 4)]
    + [f"w16.tiled({mt},{s})" for mt in (1, 2, 3, 4) for s in (1, "S")]
    + [f"w16.gen2d({mt},{s})" for mt in (1, 2) for s in (1, "S")]
    + ["w16.gen16", "w16.gen32"]
    + ["f16.sdma", "f16.sdma2", "f16.longk"] + ["f16.stream(%d,%d)" % v for v in F16_STREAM.values()]
    + [f"f16.tiled({mt})" for mt in (1, 2, 3, 4)] + ["f16.gen1", "f16.gen2"]
    + ["a4.ipart", "w16.partial_raw", "w16.ksliced_raw"]
)
BIAS_ROWS = {"a4.gen1", "a4.gen2", "a4.gen4", "w16.gen16", "w16.gen32", "w16.gen2d(1,1)", "w16.gen2d(1,S)",
             "w16.gen2d(2,1)", "w16.gen2d(2,S)"}


# ------------------------------------------------------------------ the case list

@dataclass(frozen=True)
class Case:
    op: str
    M: int
    N: int
    K: int
    bias: str = ""       # "" (none), "dominant", "mixed", "cancel"
    k0: int = 0          # w16.ksliced_raw: the K range [k0, k1) of a K-wide layer
    k1: int = 0

    @property
    def id(self):
        b = f"-b{self.bias}" if self.bias else ""
        r = f"-k{self.k0}:{self.k1}" if self.k1 else ""
        return f"{self.op}-M{self.M}-N{self.N}-K{self.K}{b}{r}"

    @property
    def rows(self):
        return route(self.op, self.M, self.N, self.k1 - self.k0 if self.k1 else self.K, bool(self.bias))

    @property
    def seed(self):
        tag = sum(ord(ch) * (i + 1) for i, ch in enumerate(self.op + self.bias))
        return (self.M * 1000003 + self.N * 7919 + self.K * 31 + self.k0 + tag) & 0x7FFFFFFF


def _cases():
    c = []
    A, W, F = "a4", "w16", "f16"
    # W4A4 streaming forms: M edges, every built K, uneven tiles per workgroup (N = 4112: 257 tiles over 256 workgroups)
    c += [Case(A, 1, 64, 28672), Case(A, 16, 4112, 28672)]
    for K, M, N in ((4096, 1, 4112), (14336, 16, 256), (8192, 5, 512), (5120, 16, 4112), (2048, 1, 1024),
                    (1024, 16, 4112), (3584, 7, 256), (13824, 3, 128), (5632, 16, 96)):
        c.append(Case(A, M, N, K))
    for K, M, N in ((4096, 17, 4112), (14336, 32, 512), (8192, 24, 256), (5120, 32, 4112), (13824, 17, 64)):
        c.append(Case(A, M, N, K))
    # W4A4 first-generation kernel: bias at every MT, N > 4096 too; K not built; NW = 4 shapes at 17..32 rows;
    # 33..64 rows and a remainder pass
    c += [Case(A, 1, 6144, 4096, "mixed"), Case(A, 16, 28672, 128, "dominant"), Case(A, 4, 256, 1408),
          Case(A, 17, 28672, 256, "cancel"), Case(A, 32, 6144, 1024, "mixed"), Case(A, 24, 512, 2048),
          Case(A, 33, 6144, 512, "dominant"), Case(A, 64, 256, 4096, "mixed"), Case(A, 80, 4112, 256, "cancel"),
          Case(A, 65, 128, 1408), Case(A, 100, 64, 4096)]
    # W4A16 streaming (M 1 / 16 at every built K, N = 4112 on the Llama shapes)
    for K in (512, 1024, 2048, 3584, 4096, 4608, 5120, 5632, 7168, 8192):
        c.append(Case(W, 1, 4112 if K in (4096, 5120) else 128, K))
        c.append(Case(W, 16, 4112 if K in (1024, 3584) else 256, K))
    # K slices of a built length: 4 (14336, 28672), 2 (9216, 10240), 3 (1536, 13824)
    c += [Case(W, 1, 256, 14336), Case(W, 16, 128, 28672), Case(W, 3, 1024, 14336),
          Case(W, 16, 256, 9216), Case(W, 1, 4112, 10240),
          Case(W, 16, 4112, 1536), Case(W, 2, 128, 13824)]
    # M-tiled W4A16: MT 1..4, K-sliced and not, ragged last token block
    c += [Case(W, 17, 128, 512), Case(W, 17, 128, 768), Case(W, 32, 4096, 4096), Case(W, 33, 14336, 4096),
          Case(W, 65, 8192, 1024), Case(W, 97, 512, 2048), Case(W, 200, 256, 1024), Case(W, 423, 1536, 6144),
          Case(W, 321, 6144, 4608), Case(W, 100, 12288, 10240)]
    c += [Case(W, M, N, K) for (M, N, K) in _TILED_EXTRA]
    # W4A16 2-D split-K kernel: bias at MT 1 / 2 and S 1 / > 1, and the no-bias shapes no other form takes
    c += [Case(W, 1, 64, 8192, "mixed"), Case(W, 16, 12288, 4096, "dominant"), Case(W, 4, 12288, 1024, "cancel"),
          Case(W, 16, 16384, 1024, "mixed"), Case(W, 17, 128, 8192, "dominant"), Case(W, 32, 12288, 4096, "cancel"),
          Case(W, 32, 12288, 1024, "mixed"), Case(W, 24, 16384, 512, "dominant"), Case(W, 8, 192, 8320),
          Case(W, 20, 256, 8320)]
    # W4A16 16 / 32-row kernel: bias, K / N no other form takes, 32-row passes
    c += [Case(W, 1, 4096, 4096, "dominant"), Case(W, 16, 96, 1408, "mixed"), Case(W, 5, 48, 384),
          Case(W, 17, 4096, 1024, "cancel"), Case(W, 32, 112, 896, "mixed"), Case(W, 40, 64, 640),
          Case(W, 33, 256, 4096, "dominant"), Case(W, 65, 80, 384)]
    # fp16: LDS-DMA lm_head forms, long K, the streaming forms, M-tiled, first-generation kernel (N % 16 != 0 too)
    c += [Case(F, 1, 12352, 4096), Case(F, 16, 16400, 4096), Case(F, 17, 12480, 4096), Case(F, 32, 16384, 4096),
          Case(F, 17, 12304, 4096)]
    c += [Case(F, 1, 32, 8192), Case(F, 16, 4112, 8192)]
    for K in (1024, 2048, 4096, 5120):
        c += [Case(F, 1, 4112 if K != 5120 else 64, K), Case(F, 16, 1040 if K != 1024 else 4112, K)]
    c += [Case(F, 17, 96, 512), Case(F, 32, 4096, 4096), Case(F, 33, 1024, 2048), Case(F, 64, 160, 768),
          Case(F, 65, 64, 1024), Case(F, 96, 128, 512), Case(F, 97, 256, 512), Case(F, 200, 96, 1024)]
    c += [Case(F, 1, 1000, 4096), Case(F, 16, 120, 256), Case(F, 5, 4104, 1536), Case(F, 17, 1000, 2048),
          Case(F, 32, 13, 512), Case(F, 40, 48, 256), Case(F, 70, 100, 96)]
    # raw partial sums
    c += [Case("a4.ipart", 17, 64, 14336), Case("a4.ipart", 32, 4096, 14336)]
    c += [Case("w16.partial_raw", 16, 256, 14336), Case("w16.partial_raw", 1, 4112, 1536),
          Case("w16.partial_raw", *_TILED_SLICED)]
    c += [Case("w16.ksliced_raw", 4, 1024, 8192, k0=4096, k1=8192), Case("w16.ksliced_raw", 16, 4112, 8192, k0=0, k1=4096),
          Case("w16.ksliced_raw", 20, 256, 4096, k0=1024, k1=3072), Case("w16.ksliced_raw", 32, 128, 8192, k0=2048, k1=6400)]
    return c


_TILED_EXTRA = ()   # (M, N, K) filled in below by search where the hand-picked shapes miss a (MT, S) row
_TILED_SLICED = (17, 128, 768)   # the smallest shape the tiled plan cuts into K slices
CASES = None


def _find_tiled_extra():
    """Small shapes (weights <= 8 MB) for every tiled (MT, S) row the hand-picked list misses: smallest weights first."""
    want = {r for r in ROWS if r.startswith("w16.tiled")}
    have = {}
    for cs in _cases():
        for r in set(cs.rows):
            have[r] = have.get(r, 0) + 1
    extra = []
    for M in (17, 32, 33, 64, 65, 96, 97, 128, 130, 200, 384, 400, 512):
        for K in (512, 768, 1024, 1536, 2048, 3072, 4096, 8192, 14336):
            for N in (128, 256, 512, 1024, 2048, 4096, 8192, 14336):
                if N * K // 2 > 8 << 20:
                    continue
                r = route("w16", M, N, K)[0]
                if r in want and have.get(r, 0) < 2:
                    have[r] = have.get(r, 0) + 1
                    extra.append((M, N, K))
    return tuple(extra)


_TILED_EXTRA = _find_tiled_extra()
CASES = _cases()
REACHABLE_ROWS = sorted({r for cs in CASES for r in cs.rows})


# ------------------------------------------------------------------ data

def _rng(case, tier):
    return np.random.default_rng([case.seed, 0 if tier == "exact" else 1])


def rand_hidden(rng, T, H, scale=1.0):
    x = rng.standard_normal((T, H)) * scale
    x[:, rng.integers(0, H, 8)] *= 20.0   # a few outlier channels, as in real LLM activations
    return x.astype(np.float16)


def rand_packed(rng, rows, K):
    """Packed int4 rows with uniform nibbles over the full range [-8, 7]."""
    return rng.integers(0, 256, (rows, K // 2), dtype=np.uint8).view(np.int8)


def exact_w4a16_range(K):
    """R: activations j / 4 in [-R, R] keep sum |x w| <= 8 R K < 2^22 (u = 1/4)."""
    return max(1, min(256, (1 << 19) // K - 1))


def make_bias(rng, kind, acc):
    """kind: 'dominant' (|bias| >> |acc s|), 'mixed' (random sign, comparable size) or 'cancel' (bias ~ -acc s of row 0,
    so that row's outputs are tiny differences).  acc: the float64 product without bias [M, N]."""
    N = acc.shape[1]
    mag = np.abs(acc).max(axis=0) + 1e-3
    if kind == "dominant":
        b = (rng.random(N) * 8 + 8) * mag * np.where(rng.random(N) < 0.5, -1, 1)
    elif kind == "mixed":
        b = rng.standard_normal(N) * mag
    elif kind == "cancel":   # three quarters of row 0 cancel (a full cancellation leaves only fp32 rounding noise)
        b = -0.75 * acc[0]
    else:
        raise ValueError(kind)
    return np.clip(b, -60000, 60000).astype(np.float16)


def make_data(case, tier):
    """Inputs and the float64 reference of one case.  Returns a dict: the input arrays, 'ref' [M, N] (float64), 'abs'
    (sum |x w| s, for the summation budget), 'u' (exact tier: the product grid step) and 'kind' of the output."""
    rng = _rng(case, tier)
    M, N, K = case.M, case.N, case.K
    d = {"tier": tier, "op": case.op}
    if case.op in ("a4", "a4.ipart"):
        xq, wq = rand_packed(rng, M, K), rand_packed(rng, N, K)
        if tier == "exact":
            xs = (rng.random(M) * 0.1 + 0.01).astype(np.float16)
            ws = (rng.random(N) * 0.01 + 0.001).astype(np.float16)
        else:   # the per-token scale of a quantised hidden row (absmax / 7), channel scales of a real checkpoint
            xs = (np.abs(rand_hidden(rng, M, 64)).astype(np.float32).max(axis=1) / 7).astype(np.float16)
            ws = (np.abs(rng.standard_normal(N)) * 0.002 + 0.0005).astype(np.float16)
        d.update(xq=xq, wq=wq, xs=xs, ws=ws)
        if case.op == "a4.ipart":
            d["ref"] = _dot_rows(_f64(unpack_i4(xq)), lambda n0, n1: _f64(unpack_i4(wq[n0:n1])), N)[0]
            d["kind"] = "i32"
            return d
        r, a = ref_w4a4(xq, xs, wq, ws, with_abs=True)
        if case.bias:
            b = make_bias(rng, case.bias, r)
            d["bias"] = b
            r = r + _f64(b)
        d.update(ref=r, abs=a, kind="f16", u=None)
        return d
    if case.op in ("w16", "w16.partial_raw", "w16.ksliced_raw"):
        wq = rand_packed(rng, N, K)
        if tier == "exact":
            R = exact_w4a16_range(K)
            x = (rng.integers(-4 * R, 4 * R + 1, (M, K)) / 4).astype(np.float16)
            ws = (rng.random(N) * 0.004 + 0.0005).astype(np.float16)
            d["u"] = 0.25
        else:
            x = rand_hidden(rng, M, K)
            ws = (np.abs(rng.standard_normal(N)) * 0.002 + 0.0005).astype(np.float16)
            d["u"] = None
        d.update(x=x, wq=wq, ws=ws)
        if case.op != "w16":
            k0, k1 = (case.k0, case.k1) if case.k1 else (0, K)
            d["ref"] = ref_w4a16_raw(x[:, k0:k1], wq[:, k0 // 2:k1 // 2])
            d["abs"] = _dot_rows(np.abs(_f64(x[:, k0:k1])), lambda n0, n1: np.abs(_f64(unpack_i4(wq[n0:n1, k0 // 2:k1 // 2]))), N)[0]
            d["abs_raw"] = d["abs"]
            d["kind"] = "f32"
            return d
        s, a = _dot_rows(_f64(x), lambda n0, n1: _f64(unpack_i4(wq[n0:n1])), N)
        d["abs_raw"] = a
        r, a = s * _f64(ws), a * _f64(ws)
        if case.bias:
            b = make_bias(rng, case.bias, r)
            d["bias"] = b
            r = r + _f64(b)
        d.update(ref=r, abs=a, kind="f16")
        return d
    if case.op == "f16":
        if tier == "exact":
            A = max(1, min(32, int(math.isqrt((1 << 24) // K)) - 1))
            x = (rng.integers(-A, A + 1, (M, K)) / 8).astype(np.float16)
            w = (rng.integers(-A, A + 1, (N, K), dtype=np.int8) / 16).astype(np.float16)
            d["u"] = 1.0 / 128
        else:
            x = rand_hidden(rng, M, K)
            w = (rng.standard_normal((N, K), dtype=np.float32) * 0.02).astype(np.float16)
            d["u"] = None
        r, a = ref_f16(x, w, with_abs=True)
        d.update(x=x, w=w, ref=r, abs=a, abs_raw=a, kind="f16")
        return d
    raise ValueError(case.op)


def exact_budget_ok(d):
    """The exact-tier premise: sum |x w| < 2^24 u (every fp32 partial sum of the products is exact in any order)."""
    if d["tier"] != "exact" or d.get("u") is None:
        return True
    return float(d["abs_raw"].max()) < 2.0 ** 24 * d["u"]


# ------------------------------------------------------------------ bars

def ulp16(r):
    """fp16 ulp at |r| (the spacing above float16(|r|); subnormal spacing 2^-24 near zero)."""
    h = np.abs(np.asarray(r, np.float64)).astype(np.float16)
    h = np.where(np.isfinite(h), h, np.float16(65504))
    return np.spacing(h).astype(np.float64)


def errors(out, ref):
    """(|out - r| in fp16 ulps of r, signed error in ulps, correctly rounded mask)."""
    o = np.asarray(out).astype(np.float64)
    u = ulp16(ref)
    e = (o - ref) / u
    cr = np.asarray(out).view(np.uint16) == np.asarray(ref, np.float64).astype(np.float16).view(np.uint16)
    return np.abs(e), e, cr


def check_f16(out, d, label=""):
    """The bars of an fp16 output (raises AssertionError).  Returns (max ulps, correctly-rounded fraction, signed errors)."""
    ref = d["ref"]
    out = np.asarray(out)
    assert out.shape == ref.shape and out.dtype == np.float16, (out.shape, out.dtype)
    ae, se, cr = errors(out, ref)
    n = ref.size
    exact = d["tier"] == "exact"
    if d["kind"] == "f16" and exact and d.get("op") == "f16":
        bad = ~cr
        assert not bad.any(), f"{label}: fp16 exact tier not bit-exact: {int(bad.sum())} / {n} (max {np.nanmax(ae):.2f} ulp)"
    # fp32 epilogue: (acc s) and the bias add round in fp32 before the fp16 store.  Where a bias cancels the product those
    # roundings (2^-24 of |acc s| and of |bias|, three at most) are what is left of r: measured up to 16 ulp16(r) on a few
    # elements in 10^5 of a random-sign bias, all within 2^-22 (|acc s| + |bias|).
    u = ulp16(ref)
    epi = np.zeros_like(ref)
    if "bias" in d:
        b = d["bias"].astype(np.float64).reshape(1, -1)
        epi = 2.0 ** -22 * (np.abs(ref - b) + np.abs(b)) / u
    fp32 = epi if exact else epi + 2.0 ** -20 * d["abs"] / u   # the fp32 budget in ulps
    lim = 1.0 + fp32
    over = ~(ae <= lim)   # NaN fails
    assert not over.any(), (f"{label}: {int(over.sum())} / {n} elements over the bar, worst {np.nanmax(ae - lim) + 1:.2f} "
                            f"ulp at {np.unravel_index(int(np.nanargmax(np.where(np.isnan(ae), np.inf, ae - lim))), ref.shape)}")
    # a rounding that is not the correct one counts against the bar unless r lies within the epilogue's fp32 roundings
    # (2^-22 |r|, and the bias term above) of an fp16 rounding boundary: there the fp32 result may round either way
    to_boundary = 0.5 - np.abs(ref - ref.astype(np.float16).astype(np.float64)) / u
    excused = to_boundary <= epi + 2.0 ** -22 * np.abs(ref) / u
    allowed = max(1, int((0.001 if exact else 0.01) * n))
    ncr = int((~cr & ~excused).sum())
    assert ncr <= allowed, f"{label}: {ncr} / {n} elements not correctly rounded (allowed {allowed})"
    return float(ae.max()), float(cr.mean()), se


def check_raw(out, d, label=""):
    """Raw partial sums: int32 exact; fp32 exact in the exact tier, within the fp32 summation budget otherwise."""
    ref = d["ref"]
    out = np.asarray(out)
    if d["kind"] == "i32":
        assert out.dtype == np.int32 and np.array_equal(out.astype(np.int64), ref.astype(np.int64)), f"{label}: int32 sums differ"
        return
    assert out.dtype == np.float32
    if d["tier"] == "exact":
        bad = out.astype(np.float64) != ref
        assert not bad.any(), f"{label}: {int(bad.sum())} / {ref.size} fp32 sums not exact"
    else:
        bad = ~(np.abs(out.astype(np.float64) - ref) <= 2.0 ** -20 * d["abs"] + 2.0 ** -24 * np.abs(ref))
        assert not bad.any(), f"{label}: {int(bad.sum())} / {ref.size} fp32 sums over the budget"


def bias_bar(n):
    """Mean signed error (ulps) allowed over n elements of one row."""
    return 0.02 + 1.2 / math.sqrt(n)
