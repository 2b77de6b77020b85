"""The host statement of the project's random stream: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
easy as 1, 2, 3", SC 2011), written from the published algorithm in numpy.  It neither imports nor compiles csrc/ph_device.h.

Every device draw is a function of four values: a 64-bit key, a 64-bit counter, a row and a block (philox_uniform4: all four
words) or component (philox_uniform: word 0).  The counter words are (row, block, counter lo, counter hi), the key words
(key lo, key hi) -- the layout csrc/ph_device.h documents.  A uniform is the top 24 bits of a word times 2**-24, exact in float32.
Rows, blocks, keys and counters broadcast against each other; the result has the broadcast shape with the four words last."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57             # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85             # the key schedule's Weyl increments (golden ratio, sqrt(3) - 1)
_MASK32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
MASK64 = 0xFFFFFFFFFFFFFFFF


def _u64(x):
    """any integer array or Python integer below 2**64 as uint64 (object route: numpy refuses large Python ints otherwise)"""
    return np.asarray(x, dtype=object).astype(np.uint64) if not isinstance(x, np.ndarray) else x.astype(np.uint64)


def philox4x32_10_words(c0, c1, c2, c3, k0, k1) -> np.ndarray:
    """ten rounds on the counter words (c0..c3) under the key words (k0, k1), all 32-bit values -> (..., 4) uint32"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(x) & _MASK32 for x in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2         # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + np.uint64(W0)) & _MASK32, (k1 + np.uint64(W1)) & _MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox4x32_10(key64, counter64, row, block) -> np.ndarray:
    """the four words of the project's call (key, counter, row, block) -> (n, 4) uint32 (or the broadcast shape + (4,))"""
    key64, counter64 = _u64(key64), _u64(counter64)
    return philox4x32_10_words(_u64(row), _u64(block), counter64 & _MASK32, counter64 >> _S32, key64 & _MASK32, key64 >> _S32)


def to_uniform(words) -> np.ndarray:
    """(word >> 8) * 2**-24 as float32: exact, in [0, 1)"""
    return ((np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def uniform4(key64, counter64, row, block) -> np.ndarray:
    """philox_uniform4: the four uniforms of one call"""
    return to_uniform(philox4x32_10(key64, counter64, row, block))


def uniform(key64, counter64, row, comp) -> np.ndarray:
    """philox_uniform: word 0 of the call whose block slot holds the component"""
    return to_uniform(philox4x32_10(key64, counter64, row, comp)[..., 0])


def epoch_key(seed: int, epoch: int) -> int:
    """csrc/ph_launch.h epoch_key: the splitmix64 finaliser of seed + golden * (epoch + 1), in Python integers"""
    z = (int(seed) + 0x9E3779B97F4A7C15 * ((int(epoch) + 1) & MASK64)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


# ---- what the consumers make of their uniforms --------------------------------------------------------------------------------------
def inverse_cdf(probs64: np.ndarray, u: np.ndarray) -> np.ndarray:
    """action = the number of prefix sums <= u, over the first K - 1 edges (the last edge is 1 by construction)"""
    edges = np.cumsum(np.asarray(probs64, np.float64), axis=1)[:, :-1]
    return (edges <= np.asarray(u, np.float64)[:, None]).sum(axis=1).astype(np.int64)


def near_edge(probs64: np.ndarray, u: np.ndarray, margin: float) -> np.ndarray:
    """rows whose uniform lies within `margin` of an inner CDF edge"""
    edges = np.cumsum(np.asarray(probs64, np.float64), axis=1)[:, :-1]
    if edges.shape[1] == 0:
        return np.zeros(len(edges), bool)
    return (np.abs(edges - np.asarray(u, np.float64)[:, None]) < margin).any(axis=1)


def box_muller(u1, u2, dtype=np.float64) -> np.ndarray:
    """sqrt(-2 log(max(u1, 1e-30))) cos(2 pi u2), computed in `dtype`"""
    u1, u2 = np.asarray(u1).astype(dtype), np.asarray(u2).astype(dtype)
    return np.sqrt(dtype(-2.0) * np.log(np.maximum(u1, dtype(1.0e-30)))) * np.cos(dtype(2.0 * np.pi) * u2)


LIAR_DICE, LIAR_SIDES = 6, 6                 # dice per player, sides (LiarEnv)
FIRST_MOVER_BLOCK = 100
ADAP_SALT = 0xADA9C0DE                         # csrc/ph_adap.hip, ph_adapmult.hip: key = epoch_key((seed ^ salt) + epoch, minibatch)


def liar_deal(key64, counter64, tables) -> np.ndarray:
    """the hands of `tables` dealt at (key, counter): (n, 12) int32, counts of sides 0..5 of the ego's six dice, then the
    partner's.  Die d is word d % 4 of block d // 4 at row = table; side = min(int(float32(u) * float32(6)), 5)."""
    tables = np.asarray(tables, np.int64)
    hands = np.zeros((len(tables), 2 * LIAR_SIDES), np.int32)
    u = np.concatenate([uniform4(key64, counter64, tables, b) for b in range(2 * LIAR_DICE // 4)], axis=1)   # (n, 12): die d
    side = np.minimum((u * np.float32(LIAR_SIDES)).astype(np.float32).astype(np.int64), LIAR_SIDES - 1)
    for d in range(2 * LIAR_DICE):
        np.add.at(hands, (np.arange(len(tables)), (0 if d < LIAR_DICE else LIAR_SIDES) + side[:, d]), 1)
    return hands


def liar_ego_first(key64, counter64, tables, probegostart: float) -> np.ndarray:
    return uniform(key64, counter64, np.asarray(tables, np.int64), FIRST_MOVER_BLOCK) < np.float32(probegostart)
