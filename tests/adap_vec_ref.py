"""The numpy statement of what an ADAP seat adds to a device-resident game (csrc/ph_adap_vec.h), over tests/philox_ref.py: the five
context samplers of the reference's adap/util.py:42-89 drawn per table from the project's Philox stream, and the row
features(observation) ++ context.  It neither imports nor compiles the engine's text."""
from __future__ import annotations

import numpy as np

from tests import philox_ref as R

ADAP_VEC_SALT = 0xC0A7E87D5A17ADA9      # key = the learner's policy seed ^ this constant
SAMPLERS = ("l2", "unit_square", "positive_square", "categorical", "natural_numbers")


def draw_contexts(sampler: str, context_size: int, seed: int, counter: int, tables) -> np.ndarray:
    """(len(tables), C) float32: the context of every table in `tables` drawn at (seed, counter).  Component k is
    philox_uniform(seed ^ salt, counter, table, k); every operation is one float32 operation, in the order written."""
    tables = np.asarray(tables, np.int64)
    C, key = int(context_size), (int(seed) ^ ADAP_VEC_SALT) & R.MASK64
    f32 = np.float32
    if sampler in ("categorical", "natural_numbers"):
        u = R.uniform(key, counter, tables, 0)
        v = np.minimum((u * f32(C)).astype(np.float32).astype(np.int64), C - 1)
        out = np.zeros((len(tables), C), np.float32)
        if sampler == "categorical":
            out[np.arange(len(tables)), v] = 1.0
        else:
            out[:, 0] = v.astype(np.float32)
        return out
    u = np.stack([R.uniform(key, counter, tables, k) for k in range(C)], axis=1).astype(np.float32)
    if sampler == "positive_square":
        return u
    c = (u * f32(2.0) - f32(1.0)).astype(np.float32)
    if sampler == "unit_square":
        return c
    assert sampler == "l2"
    ss = np.zeros(len(tables), np.float32)
    for k in range(C):                                      # the sum in component order, a product and a sum per step
        ss = (ss + (c[:, k] * c[:, k]).astype(np.float32)).astype(np.float32)
    return (c / np.sqrt(ss).astype(np.float32)[:, None]).astype(np.float32)


def one_hot_features(nvec, obs) -> np.ndarray:
    """SB3 preprocess_obs + FlattenExtractor of (n, D) stored observations of a MultiDiscrete(nvec) space, out-of-range components
    clamped"""
    obs = np.asarray(obs, np.float32)
    parts = []
    for i, k in enumerate(nvec):
        idx = np.clip(obs[:, i].astype(np.int64), 0, int(k) - 1)
        parts.append(np.eye(int(k), dtype=np.float32)[idx])
    return np.concatenate(parts, axis=1)


def rows(nvec, obs, contexts) -> np.ndarray:
    """(n, F + C): nvec None = a Box observation, its values unchanged"""
    obs = np.asarray(obs, np.float32)
    feats = obs if nvec is None else one_hot_features(nvec, obs)
    return np.concatenate([feats, np.asarray(contexts, np.float32)], axis=1)
