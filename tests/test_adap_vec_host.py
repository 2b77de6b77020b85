"""not-gpu: what an ADAP seat adds to the device-resident games, pinned without a device -- ph_adap_vec_host (the text the kernels of
csrc/ph_adap_vec.hip run, csrc/ph_adap_vec.h) against the numpy statement tests/adap_vec_ref.py, the trainer's plan and refusals, and
the header's declarations.  tests/test_gpu_adap_vec.py holds the kernels to ph_adap_vec_host bit for bit."""
import os
import re

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat
from pantheonrl_amd import spaces as sp
from pantheonrl_amd import trainer
from pantheonrl_amd.envs import vec as V
from tests import adap_vec_ref as A
from tests.philox_ref import ADAP_SALT

N = 300
COUNTERS = (0, 9, 2 ** 33 + 1)
SEED = 0x1234567


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("sampler", A.SAMPLERS)
def test_samplers_are_the_numpy_statement(sampler, C):
    if sampler == "natural_numbers" and C != 1:
        with pytest.raises(nat.NativeError, match="context_size == 1"):
            nat.adap_vec_host(C, N, sampler=sampler, seed=SEED, counter=0)
        return
    for counter in COUNTERS:
        got, _ = nat.adap_vec_host(C, N, sampler=sampler, seed=SEED, counter=counter)
        want = A.draw_contexts(sampler, C, SEED, counter, np.arange(N))
        assert got.shape == (N, C) and np.array_equal(bits(got), bits(want)), (sampler, C, counter)
        if sampler == "l2":
            assert np.all(np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(axis=1)) - 1.0) < 1e-6)
        if sampler == "categorical":
            assert np.all((got == 0) | (got == 1)) and np.all(got.sum(axis=1) == 1)
        if sampler == "natural_numbers":
            assert not got.any()
        if sampler == "unit_square":
            assert got.min() >= -1 and got.max() < 1
        if sampler == "positive_square":
            assert got.min() >= 0 and got.max() < 1


@pytest.mark.parametrize("sampler", ["l2", "categorical"])
def test_only_flagged_tables_change_and_the_draw_is_a_function_of_its_arguments(sampler):
    C = 3
    rng = np.random.default_rng(1)
    flags = (rng.random(N) < 0.4).astype(np.uint8)
    before = rng.standard_normal((N, C)).astype(np.float32)
    got, _ = nat.adap_vec_host(C, N, sampler=sampler, seed=SEED, counter=9, redraw=flags, contexts=before)
    full = A.draw_contexts(sampler, C, SEED, 9, np.arange(N))
    assert np.array_equal(bits(got), bits(np.where(flags[:, None] != 0, full, before)))
    again, _ = nat.adap_vec_host(C, N, sampler=sampler, seed=SEED, counter=9, redraw=flags, contexts=before)
    assert np.array_equal(bits(got), bits(again))
    if sampler == "l2":                                  # (a categorical draw may come out the same: three values)
        base, _ = nat.adap_vec_host(C, N, sampler=sampler, seed=SEED, counter=9)
        for other in (dict(counter=10), dict(counter=9 + 2 ** 32), dict(counter=9, seed=SEED + 1)):
            moved, _ = nat.adap_vec_host(C, N, sampler=sampler, **{"seed": SEED, **other})
            assert not (bits(moved) == bits(base)).all(axis=1).any(), other


def test_the_salt_is_its_own():
    assert nat.ADAP_VEC_SALT == A.ADAP_VEC_SALT
    assert nat.ADAP_VEC_SALT not in (ADAP_SALT, V.POOL_SEED_SALT, 0)
    text = open(os.path.join(os.path.dirname(nat.__file__), "csrc", "ph_adap_vec.h")).read()
    assert "ADAP_VEC_SALT = 0x%Xull" % nat.ADAP_VEC_SALT in text
    for seed in (0, 5, 2 ** 40 + 3):                     # another key than the policy's, the loss term's and the pool's of that seed
        assert len({seed, seed ^ ADAP_SALT, seed ^ V.POOL_SEED_SALT, seed ^ nat.ADAP_VEC_SALT}) == 4


# ---- row build -------------------------------------------------------------------------------------------------------------------
def adap_features(space, obs):
    """AdapPolicy.features without a device: the method reads nothing but `_nvec`"""
    from pantheonrl_amd.adap import AdapPolicy
    kind = sp._kind(space)
    stub = type("Stub", (), {})()
    stub._nvec = None if kind == "Box" else ([int(space.n)] if kind == "Discrete" else [int(v) for v in space.nvec])
    return AdapPolicy.features(stub, th.as_tensor(obs)).numpy(), stub._nvec


def liar_obs(rng, n):
    nvec = np.asarray(V.VecLiarsDice.observation_space.nvec)
    return (rng.random((n, len(nvec))) * nvec).astype(np.int64).astype(np.float32)


@pytest.mark.parametrize("case", ["liar", "rps", "box", "clamped"])
def test_rows_are_adap_policy_features_then_the_context(case):
    rng = np.random.default_rng(2)
    n, C = 37, 3
    if case in ("liar", "clamped"):
        space, obs = V.VecLiarsDice.observation_space, liar_obs(rng, n)
        if case == "clamped":
            obs[3, 7], obs[5, 0], obs[9, 29] = 99.0, -2.0, 12.0       # above nvec, below 0, one past the last category
    elif case == "rps":
        space, obs = V.VecRPS.observation_space, np.zeros((n, 1), np.float32)
    else:
        space, obs = sp.Box(-np.inf, np.inf, (6,)), rng.standard_normal((n, 6)).astype(np.float32)
    ctx = A.draw_contexts("l2", C, SEED, 4, np.arange(n))
    feats, nvec = adap_features(space, obs)
    want = np.concatenate([feats, ctx], axis=1)
    assert np.array_equal(want, A.rows(nvec, obs, ctx))                 # the numpy statement says the same
    _, got = nat.adap_vec_host(C, n, contexts=ctx, env_space=nat.env_space_of(space), obs=obs)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    assert got.shape[1] == {"liar": 273, "clamped": 273, "rps": 4, "box": 9}[case]
    # inactive tables keep what the plane held
    active = (rng.random(n) < 0.5).astype(np.uint8)
    sentinel = np.full_like(want, -7.5)
    _, part = nat.adap_vec_host(C, n, contexts=ctx, env_space=nat.env_space_of(space), obs=obs, active=active, rows=sentinel)
    assert np.array_equal(bits(part), bits(np.where(active[:, None] != 0, want, sentinel)))


def test_misuse_is_an_error_string():
    with pytest.raises(nat.NativeError, match="context_size"):
        nat.adap_vec_host(0, 4, sampler="l2")
    with pytest.raises(nat.NativeError, match="context_size"):
        nat.adap_vec_host(nat.ADAP_VEC_MAX_CONTEXT + 1, 4, sampler="l2")
    with pytest.raises(nat.NativeError, match="n must be positive"):
        nat.check(nat.load().ph_adap_vec_host(None, 3, 0, 1, 0, 0, None, None, None, None, None, 0))


# ---- the trainer's plan ------------------------------------------------------------------------------------------------------------
def test_adap_pairings_are_planned_without_a_device(monkeypatch):
    monkeypatch.setattr(nat, "Context", None)
    plan = trainer.adap_plan(trainer.parse_cli(["LiarsDice-v0", "ADAP", "ADAP", "--n-envs", "8", "--share-latent"]))
    assert (plan["ego"], plan["alt"], plan["share_latent"]) == ("ADAP", "ADAP", True)
    plan = trainer.adap_plan(trainer.parse_cli(["RPS-v0", "ADAP", "PPO", "--n-envs", "8", "--env-config", '{"log_interval": 3}']))
    assert (plan["ego"], plan["alt"], plan["share_latent"], plan["log_interval"]) == ("ADAP", "PPO", False, 3)
    plan = trainer.adap_plan(trainer.parse_cli(["LiarsDice-v0", "PPO", "ADAP", "--n-envs", "8", "--alt-config",
                                                '{"context_size": 4, "context_sampler": "categorical"}']))
    assert (plan["ego"], plan["alt"], plan["share_latent"]) == ("PPO", "ADAP", False)
    # no ADAP seat: today's plans
    assert trainer.adap_plan(trainer.parse_cli(["LiarsDice-v0", "PPO", "PPO", "--n-envs", "8"])) is None


@pytest.mark.parametrize("argv,word", [
    (["LiarsDice-v0", "ADAP_MULT", "ADAP_MULT", "--n-envs", "8"], "ADAP_MULT"),
    (["RPS-v0", "PPO", "ADAP_MULT", "--n-envs", "8"], "ADAP_MULT"),
    (["BlockEnv-v0", "ADAP", "ADAP", "--n-envs", "8"], "block worlds"),
    (["BlockEnv-v1", "PPO", "ADAP", "--n-envs", "8"], "block worlds"),
    (["LiarsDice-v0", "PPO", "PPO", "ADAP", "--n-envs", "8"], "pool of"),
    (["LiarsDice-v0", "ADAP", "ADAP", "ADAP", "--n-envs", "8"], "pool of"),
    (["LiarsDice-v0", "ADAP", "DEFAULT", "--n-envs", "8"], "each from PPO and ADAP"),
    (["LiarsDice-v0", "ADAP", "ADAP", "--n-envs", "8", "--record", "f.npy"], "--record"),
    (["LiarsDice-v0", "PPO", "ADAP", "--n-envs", "8", "--share-latent"], "both agents must be ADAP"),
])
def test_what_adap_seats_cannot_do_is_an_env_exception_before_a_device_is_touched(monkeypatch, argv, word):
    monkeypatch.setattr(nat, "Context", None)            # touching a device would be a TypeError, not an EnvException
    with pytest.raises(trainer.EnvException, match=word):
        trainer.run(argv)


# ---- the header --------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_seat():
    root = os.path.dirname(os.path.dirname(os.path.abspath(nat.__file__)))
    text = open(os.path.join(root, "include", "pantheon_hip.h")).read()
    for name in ("ph_adap_rows", "ph_adap_context_draw", "ph_adap_vec_host", "ph_liar_selfplay_step_adap"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in nat.SIGNATURES and hasattr(nat.load(), name)
    seat = re.search(r"typedef struct ph_adap_seat \{(.*?)\} ph_adap_seat;", text, re.S)
    assert seat is not None
    for field, _ in nat.PhAdapSeat._fields_:
        assert re.search(r"\b%s\b" % field, seat.group(1)), field
    assert "#define PH_ABI_VERSION 7" in text and "still 7: + ph_adap_rows" in text
