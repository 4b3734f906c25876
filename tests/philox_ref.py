"""numpy Philox4x32-10 and the two counter layouts of csrc/sampler.hip (include/qspec_hip.h): the per-request seeded
stream and the engine's own (unseeded) stream.  No torch, no GPU."""
import numpy as np

M32 = 0xFFFFFFFF


def philox_words(c0, c1, c2, c3, k0, k1):
    """The four output words of Philox4x32-10 for broadcastable uint32-valued arrays (Salmon et al., SC'11)."""
    u = np.uint64
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=u) for x in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    m = u(M32)
    for _ in range(10):
        p0 = u(0xD2511F53) * c0
        p1 = u(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> u(32)) ^ c1 ^ k0, p1 & m, (p0 >> u(32)) ^ c3 ^ k1, p0 & m
        k0 = (k0 + u(0x9E3779B9)) & m
        k1 = (k1 + u(0xBB67AE85)) & m
    return c0, c1, c2, c3


def philox_r0(c0, c1, c2, c3, k0, k1):
    """First output word of Philox4x32-10 for broadcastable uint32-valued arrays."""
    return philox_words(c0, c1, c2, c3, k0, k1)[0]


def seeded_r0(c0, seed, base_pos, stream, j):
    seed = np.asarray(seed, dtype=np.uint64)
    c1 = np.uint64(0x80000000) | (np.uint64(stream) << np.uint64(16)) | np.asarray(j, dtype=np.uint64)
    return philox_r0(c0, c1, np.asarray(base_pos, dtype=np.uint64), 0, seed & np.uint64(M32), seed >> np.uint64(32))


def engine_r0(c0, c1, seed, offset):
    """The engine stream: key = seed, counter = (c0, c1, offset lo, offset hi).  seed / offset: Python ints < 2^64;
    c1 = b * k + i for the rejection sampler, 0x40000000 | row for the sampler."""
    seed, offset = int(seed), int(offset)
    assert 0 <= seed < 2 ** 64 and 0 <= offset < 2 ** 64
    return philox_r0(c0, c1, offset & M32, offset >> 32, seed & M32, seed >> 32)


def u01_closed_open(r0):
    """The accept uniform: (r0 >> 8) / 2^24 in [0, 1), exact in fp32."""
    return (np.asarray(r0, np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def exp_noise_f64(r0):
    """The per-token noise: -log(((r0 >> 8) + 0.5) / 2^24), float64."""
    return -np.log(((np.asarray(r0, np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0)
