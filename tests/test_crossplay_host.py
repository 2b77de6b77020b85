"""not-gpu: the device-resident cross-play evaluation of Liar's Dice -- the new symbols of the C ABI, the host statement of the
statistics, the 7-step bound of a game and what the two command lines refuse before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pantheonrl_amd import _native as nat
from pantheonrl_amd import crossplay as xcli
from pantheonrl_amd import tester
from pantheonrl_amd.envs.crossplay import (MAX_STEPS_PER_GAME, all_pairs, check_pairs, crossplay_stats, pair_of_tables)
from pantheonrl_amd.envs.liar import LiarEnv
from pantheonrl_amd.trainer import EnvException

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "pantheon_hip.h")).read()


# ---- 1. symbols and structs --------------------------------------------------------------------------------------------------------
def test_crossplay_symbols_are_declared_and_exported():
    lib = nat.load()
    for name in ("ph_liar_xplay_step", "ph_xplay_stats"):
        assert re.search(r"^int\s+" + name + r"\s*\(", HEADER, flags=re.M), name
        assert hasattr(lib, name) and name in nat.SIGNATURES
    assert HEADER.count("tester.py:41-63") >= 3                      # the struct and both entry points cite the loop they vectorise
    assert lib.ph_abi_version() == 7                                  # additive: the version stays
    assert int(re.search(r"#define PH_ABI_VERSION (\d+)", HEADER).group(1)) == 7
    body = re.search(r"typedef struct ph_liar_xplay \{(.*?)\} ph_liar_xplay;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip(" *") for n in re.sub(r"^(?:const\s+)?(?:unsigned\s+)?(?:long\s+long|[a-z_]+)\s", "", decl).split(",")]
    assert [n for n, _ in nat.PhLiarXplay._fields_] == names
    assert len(names) == 35 and C.sizeof(nat.PhLiarXplay) == 8 * 34     # 8-byte slots; n_pairs and episodes_per_table share one
    # host-side misuse needs no device: a null context is an error string, not a crash
    assert lib.ph_liar_xplay_step(None, None, 0, 0) != 0 and b"null" in lib.ph_last_error()
    assert lib.ph_xplay_stats(None, None, None, None, 0, 0, 0, None) != 0 and b"null" in lib.ph_last_error()


# ---- 2. the statistics' host statement ------------------------------------------------------------------------------------------
def test_crossplay_stats_is_mean_std_and_count_per_pair():
    E, G, P = 7, 3, 3                       # pair 0: tables 0, 3, 6; pair 1: tables 1, 4; pair 2: tables 2, 5
    pot = pair_of_tables(E, P)
    assert pot.tolist() == [0, 1, 2, 0, 1, 2, 0] and pot.dtype == np.int32
    rng = np.random.default_rng(0)
    returns = rng.choice(np.array([-1.0, 1.0, 0.5, -0.25], np.float32), size=(E, G))
    lengths = rng.integers(1, 8, size=(E, G)).astype(np.int32)
    st = crossplay_stats(returns, lengths, pot, P)
    for p in range(P):
        r = returns[pot == p].astype(np.float64).reshape(-1)
        assert st["count"][p] == r.size == G * [3, 2, 2][p]
        assert st["sum"][p] == r.sum() and st["sumsq"][p] == (r * r).sum()        # quarters: every sum is exact
        assert st["mean"][p] == np.mean(r)
        # sqrt(E[x^2] - mean^2) against numpy's two-pass form: both are float64 evaluations of values of order 1
        assert abs(st["std"][p] - np.std(r)) < 1e-14
        assert st["mean_length"][p] == lengths[pot == p].mean()
    # a pair with ONE table; a pair without games reports nan, not a crash
    one = crossplay_stats(returns[:3], lengths[:3], pair_of_tables(3, 3), 3)
    assert one["count"].tolist() == [G] * 3 and one["mean"][1] == np.mean(returns[1].astype(np.float64))
    none = crossplay_stats(returns, lengths, pot, P, games=np.array([0, 1, 2, 0, 3, 2, 0]))
    assert none["count"].tolist() == [0.0, 4.0, 4.0] and np.isnan(none["mean"][0]) and np.isnan(none["std"][0])
    assert none["sum"][1] == float(returns[1, 0]) + float(returns[4].astype(np.float64).sum())
    # +-1 returns: the standard deviation of a win rate
    pm = np.array([[1, 1, -1, -1], [1, 1, 1, -1]], np.float32)
    s = crossplay_stats(pm, np.ones((2, 4), np.int32), np.array([0, 0]), 1)
    assert s["mean"][0] == 0.25 and s["std"][0] == np.std(pm.astype(np.float64)) == np.sqrt(1 - 0.25 ** 2) and s["count"][0] == 8


def test_pairs_default_to_the_whole_matrix_and_need_a_table_each():
    assert all_pairs(3) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
    assert check_pairs(16, 4, None).tolist() == [list(p) for p in all_pairs(4)]
    assert check_pairs(2, 3, [(2, 2), (0, 1)]).tolist() == [[2, 2], [0, 1]]               # a diagonal pair is legal
    with pytest.raises(nat.NativeError, match="at least as many tables"):
        check_pairs(8, 3, None)                                                         # P = 9 > E = 8
    with pytest.raises(nat.NativeError, match="at least as many tables"):
        pair_of_tables(3, 4)
    with pytest.raises(nat.NativeError, match="outside"):
        check_pairs(8, 2, [(0, 2)])
    with pytest.raises(nat.NativeError, match="1..8"):
        check_pairs(128, 9, None)


# ---- 3. the step bound ---------------------------------------------------------------------------------------------------------
def _ego_steps(env, moves):
    """play one game of `env` with `moves()` for both seats -> ego moves until done (the partner is a plain callback)"""
    from pantheonrl_amd.common import Agent

    class Script(Agent):
        def get_action(self, obs, record=True):
            return moves()

        def update(self, reward, done):
            pass
    if not env.partners[0]:
        env.add_partner_agent(Script())
    env.reset()
    n, done = 0, False
    while not done:
        _, _, done, _ = env.step(moves())
        n += 1
        assert n <= MAX_STEPS_PER_GAME
    return n


def test_no_game_takes_more_than_seven_ego_steps():
    rng = np.random.default_rng(3)
    env = LiarEnv()
    seen = set()
    for _ in range(300):
        seen.add(_ego_steps(env, lambda: np.array([rng.integers(0, 7), rng.integers(0, 12)])))
    assert max(seen) <= MAX_STEPS_PER_GAME == 7 and len(seen) > 1
    # the strictly raising line: counts 0..11 fill the 12 moves of the history, the 13th move can only be a call
    for probegostart, want in ((1.0, 7), (0.0, 7)):
        env = LiarEnv(probegostart=probegostart)
        count = iter(range(64))
        n = _ego_steps(env, lambda: np.array([0, min(next(count), 11)]))
        if probegostart == 1.0:
            assert n == want            # ego bids 0, 2, .., 10 (6 moves), partner 1, 3, .., 11; the ego's 7th move is the call
        else:
            assert n <= want


# ---- 4. refusals before a device is touched ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,word", [
    (["RPS-v0", "PPO", "DEFAULT", "--ego-load", "m", "--n-envs", "8"], "LiarsDice-v0, not RPS-v0"),
    (["BlockEnv-v0", "PPO", "DEFAULT", "--ego-load", "m", "--n-envs", "8"], "LiarsDice-v0, not BlockEnv-v0"),
    (["LiarsDice-v0", "BC", "DEFAULT", "--ego-load", "m", "--n-envs", "8"], "not BC against DEFAULT"),
    (["LiarsDice-v0", "PPO", "BC", "--ego-load", "m", "--alt-load", "m", "--n-envs", "8"], "not PPO against BC"),
    (["LiarsDice-v0", "PPO", "ADAP", "--ego-load", "m", "--alt-load", "m", "--n-envs", "8"], "not PPO against ADAP"),
    (["LiarsDice-v0", "PPO", "DEFAULT", "--ego-load", "m", "--n-envs", "8", "--framestack", "2"], "--framestack"),
    (["LiarsDice-v0", "PPO", "DEFAULT", "--ego-load", "m", "--n-envs", "8", "--record", "f"], "--record"),
    (["LiarsDice-v0", "PPO", "DEFAULT", "--ego-load", "m", "--n-envs", "0"], "at least 1"),
])
def test_tester_n_envs_refusals_come_before_a_device_is_touched(argv, word, monkeypatch):
    monkeypatch.setattr(nat, "Context", None)            # touching a device would be a TypeError, not an EnvException
    monkeypatch.setattr(tester, "gen_load", None)
    with pytest.raises(EnvException, match=word):
        tester.run(argv)


def test_crossplay_cli_refusals_and_sizes():
    with pytest.raises(EnvException, match="at most 8 agents, not 9"):
        xcli.plan(xcli.build_parser().parse_args(["LiarsDice-v0", "--agents"] + ["DEFAULT"] * 9))
    with pytest.raises(EnvException, match="LiarsDice-v0, not RPS-v0"):
        xcli.plan(xcli.build_parser().parse_args(["RPS-v0", "--agents", "DEFAULT"]))
    with pytest.raises(EnvException, match="at least 9"):
        xcli.plan(xcli.build_parser().parse_args(["LiarsDice-v0", "--agents", "a", "b", "DEFAULT", "--n-envs", "8"]))
    size = xcli.plan(xcli.build_parser().parse_args(["LiarsDice-v0", "--agents", "a", "b", "DEFAULT", "--n-envs", "256", "-t", "1000"]))
    assert size == dict(n_members=3, n_pairs=9, episodes_per_table=36)        # 28 tables per pair at least: ceil(1000 / 28)


def test_tester_without_n_envs_parses_as_before():
    argv = ["RPS-v0", "PPO", "DEFAULT", "--ego-load", "models/ego", "--alt-config", '{"r": 1}', "-t", "7", "--seed", "3"]
    args = tester.build_parser().parse_args(argv)
    before = dict(env="RPS-v0", ego="PPO", alt="DEFAULT", total_episodes=7, device="cuda", seed=3, ego_config={}, alt_config={"r": 1},
                  env_config={}, framestack=1, record=None, render=False, ego_load="models/ego", alt_load=None)
    got = dict(vars(args))
    assert got.pop("n_envs") == 1 and got == before
    tester.input_check(args)                                 # and the host path's own checks still take it
