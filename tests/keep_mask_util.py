"""The keep decision of the dropout mask generator, restated in numpy uint64 (plain helper, like gpu_util.py).

include/amdnuwa.h (amdnuwa_keep_mask_linear) states the function; this file is its CPU restatement and the oracle of the generator kernels:
Philox4x32-10 with the standard constants, key = the two 32-bit seed words, and for the logical element e (64-bit)

    word = output word (e mod 4) of Philox(counter = (floor(e / 4) mod 2^32, floor(e / 4) >> 32, 0, 0), key);    keep  <=>  word >= thr

with thr = min(2^32 - 1, round(p * 2^32)).  The three logical-index maps follow."""
import math

import numpy as np

U = np.uint64
M32 = U(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = U(0xD2511F53), U(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = U(0x9E3779B9), U(0xBB67AE85)
S32 = U(32)

# (counter, key) -> the four output words, in order
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or ints) holding 32-bit words, key: two ints -> the four output word arrays (uint64 holding 32 bits)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=U) for c in counter)
    k0, k1 = U(key[0]) & M32, U(key[1]) & M32
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2                    # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def keep_threshold(p):
    return min(0xFFFFFFFF, int(math.floor(float(p) * 4294967296.0 + 0.5)))


def element_words(e, seed):
    """the 32-bit word that decides each logical element of the uint64 array e"""
    e = np.asarray(e, dtype=U)
    grp = e >> U(2)
    zero = np.zeros_like(grp)
    w = philox4x32_10((grp & M32, grp >> S32, zero, zero), seed)
    return np.choose((e & U(3)).astype(np.int64), w)


def keep_of(e, thr, seed):
    """boolean keep decisions of the logical elements e"""
    return element_words(e, seed) >= U(thr)


def ff_elements(R, C, e0=0):
    """FeedForward mask [R, C]: e = r * C + c"""
    return (U(e0) + np.arange(R * C, dtype=U)).reshape(R, C)


def attn_elements(B, nq, J, heads, e0=0):
    """window / SparseCross2DNA mask [B, nq, J, heads]: e = ((b * nq + i) * J + j) * heads + g, the storage index"""
    return (U(e0) + np.arange(B * nq * J * heads, dtype=U)).reshape(B, nq, J, heads)


def cattn_elements(B, n, T, heads, b_first=0):
    """cattn mask in the attention-map order (b, g, i, j) of ops.cattn_pack_keep's argument, j = 0 the null slot:
    e = ((b * n + i) * (T + 1) + j) * 8 + g with b counted from b_first"""
    b = (U(b_first) + np.arange(B, dtype=U))[:, None, None, None]
    g = np.arange(heads, dtype=U)[None, :, None, None]
    i = np.arange(n, dtype=U)[None, None, :, None]
    j = np.arange(T + 1, dtype=U)[None, None, None, :]
    return ((b * U(n) + i) * U(T + 1) + j) * U(8) + g


def linear_keep(count, thr, seed, e0=0):
    """what amdnuwa_keep_mask_linear writes: uint8 0 / 1 of the elements e0 .. e0 + count - 1"""
    return keep_of(U(e0) + np.arange(count, dtype=U), thr, seed).astype(np.uint8)


def cattn_keep(B, n, T, heads, thr, seed, b_first=0):
    """boolean mask (b, heads, i, j) whose ops.cattn_pack_keep is what amdnuwa_keep_mask_cattn writes"""
    return keep_of(cattn_elements(B, n, T, heads, b_first), thr, seed)
