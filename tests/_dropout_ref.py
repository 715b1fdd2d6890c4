"""The stream of the critics' dropout masks (CurlSacAgent(critic_dropout=p)) restated in NumPy from its specification
(DESIGN.md 7e), not from the kernels: Philox4x32-10 on a four-word counter and the keep mask of one launch."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """``ctr``: four uint64 arrays of one shape holding 32-bit words (c0..c3); ``key`` = (k0, k1) Python ints.  Returns
    the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & LO for c in ctr)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # (32 x 32 -> 64 bits: no overflow of uint64)
        n0 = (p1 >> S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & LO, n2, p0 & LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def keep_mask(seed, counter, tag, nb, B, H, p):
    """bool [nb, B, H]: True where element (twin z, row r, feature f) of the pass (seed S, phase counter O, tag t) is
    kept."""
    S, O, t = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1), int(tag)
    z, r, f = np.meshgrid(np.arange(nb, dtype=np.uint64), np.arange(B, dtype=np.uint64), np.arange(H, dtype=np.uint64),
                          indexing="ij")
    chunks = np.uint64((H + 255) // 256)
    e = ((z * np.uint64(B) + r) * chunks + (f >> np.uint64(8))) * np.uint64(64) + (f & np.uint64(63))
    c2 = np.full(e.shape, O & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(e.shape, (((O >> 32) << 8) | t) & 0xFFFFFFFF, dtype=np.uint64)
    words = np.stack(philox4x32_10((e & LO, e >> S32, c2, c3), (S & 0xFFFFFFFF, S >> 32)), axis=-1)
    word = np.take_along_axis(words, ((f >> np.uint64(6)) & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]
    u = (word >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)  # exact: 24 bits
    return u >= np.float32(p)
