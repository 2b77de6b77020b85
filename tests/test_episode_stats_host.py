"""not-gpu: the episode statistics' host side -- the NumPy oracle on hand-worked columns, the C ABI's declaration and export, the
`log_interval` key of --env-config in both planning paths, and the window / total arithmetic of `EpisodeStats.read`."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from pantheonrl_amd import _native as nat
from pantheonrl_amd import trainer
from pantheonrl_amd.episode_stats import EpisodeStats, episode_report, episode_summary
from tests.episode_stats_oracle import EpisodeOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "pantheon_hip.h")).read()


def test_oracle_on_three_hand_worked_columns():
    """Two scans of T = 3 over three tables.
    column 0 (valid): rewards 1 2 | 3, then 4 5 6: ends after rows 1 and 2 of scan A and after row 2 of scan B
        -> episodes (3, len 2), (3, len 1), (15, len 3)
    column 1 (valid): rewards .5 .25 .125 then 1 -1 2, one end after row 0 of scan B: the episode spans both scans
        -> episode (.5 + .25 + .125 + 1 = 1.875, len 4); (-1 + 2, len 2) stays in the carry
    column 2 (carry_valid = 0): rewards 7 8 9 then 1 1 1, ends after row 1 of scan A and row 1 of scan B: the game in progress at
        the attach is dropped -> only (9 + 1 + 1 = 11, len 3); the carry holds (1, len 1)"""
    o = EpisodeOracle(3)
    o.valid[2] = False
    rew_a = np.array([[1, .5, 7], [2, .25, 8], [3, .125, 9]], np.float32)
    st_a = np.array([[9, 9, 9], [0, 0, 0], [1, 0, 1]], np.float32)          # row 0's own flags are never read
    o.scan(rew_a, st_a, np.array([1, 0, 0], np.float32))
    assert o.episodes == [(0, 3.0, 2), (0, 3.0, 1)]
    assert o.ret.tolist() == [0.0, 0.875, 9.0] and o.len.tolist() == [0, 3, 1] and o.valid.tolist() == [True, True, True]
    rew_b = np.array([[4, 1, 1], [5, -1, 1], [6, 2, 1]], np.float32)
    st_b = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    o.scan(rew_b, st_b, np.array([1, 0, 0], np.float32))
    assert o.episodes == [(0, 3.0, 2), (0, 3.0, 1), (0, 1.875, 4), (0, 11.0, 3), (0, 15.0, 3)]
    assert o.ret.tolist() == [0.0, 1.0, 1.0] and o.len.tolist() == [0, 2, 1]
    want = np.array([[5.0, 33.875, 9 + 9 + 1.875 ** 2 + 121 + 225, 13.0]])
    assert np.array_equal(o.stats(), want)
    assert (o.bounds() > 0).all() and (o.bounds() < 1e-11).all()


def test_oracle_sums_in_float32_and_replays_members():
    o = EpisodeOracle(1)
    rew = np.array([[1e8], [1.0], [-1e8]], np.float32)
    o.scan(rew, np.zeros((3, 1), np.float32), np.ones(1, np.float32))
    assert o.episodes == [(0, 0.0, 3)]                 # (1e8 + 1) rounds to 1e8 in float32: a float64 sum would leave 1
    # robin over K = 3 from member 2: every end advances the member; the random rule draws the deal counter's Philox word
    from pantheonrl_amd.envs.vec import POOL_RESAMPLE_BLOCK, philox_word0, pool_resample
    ends = np.ones((4, 2), np.float32)
    o = EpisodeOracle(2, K=3, member=[2, 0]).scan(np.ones((4, 2), np.float32), ends, np.ones(2, np.float32))
    assert [m for m, _, _ in o.episodes] == [2, 0, 0, 1, 1, 2, 2, 0] and o.member.tolist() == [0, 1]
    o = EpisodeOracle(2, K=8, member=[5, 5], rule="random", pool_seed=77).scan(np.ones((2, 2), np.float32), ends[:2], np.ones(2, np.float32),
                                                                               counter0=40, epoch=3)
    w0 = philox_word0(77, 40 + (3 << 32), np.arange(2), POOL_RESAMPLE_BLOCK)
    w1 = philox_word0(77, 41 + (3 << 32), np.arange(2), POOL_RESAMPLE_BLOCK)
    first = [pool_resample(5, 8, "random", int(w)) for w in w0]
    assert [m for m, _, _ in o.episodes] == [5, 5] + first
    assert o.member.tolist() == [pool_resample(0, 8, "random", int(w)) for w in w1]


def test_entry_point_is_declared_and_exported():
    lib = nat.load()
    assert re.search(r"^int\s+ph_episode_stats\s*\(ph_ctx \*ctx, const ph_episode_scan \*scan\);", HEADER, flags=re.M)
    assert re.search(r"typedef struct ph_episode_scan \{", HEADER) and "} ph_episode_scan;" in HEADER
    assert int(re.search(r"#define PH_EPISODE_NSTAT (\d+)", HEADER).group(1)) == nat.EPISODE_NSTAT == 4
    assert hasattr(lib, "ph_episode_stats")
    assert nat.SIGNATURES["ph_episode_stats"] == [C.c_void_p, C.POINTER(nat.PhEpisodeScan)]
    body = HEADER[HEADER.index("typedef struct ph_episode_scan {"):HEADER.index("} ph_episode_scan;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*?\b([A-Za-z_0-9]+)\s*(?:,\s*\*?([A-Za-z_0-9]+)\s*)?;", body)
    names = [n for pair in fields for n in pair if n]
    assert names == [f[0] for f in nat.PhEpisodeScan._fields_]
    # x86-64 layout of the header's struct: 8-byte pointers, ints padded up to them
    assert C.sizeof(nat.PhEpisodeScan) == 96 and nat.PhEpisodeScan.stats.offset == 88 and nat.PhEpisodeScan.pool_seed.offset == 72
    assert lib.ph_episode_stats(None, None) != 0 and b"null" in lib.ph_last_error()
    assert "agents.py:132-158" in HEADER and "ep_info_buffer" in HEADER


def test_log_interval_is_popped_in_both_planning_paths_and_the_arguments_stay():
    args = trainer.parse_cli(["LiarsDice-v0", "PPO", "PPO", "DEFAULT", "--n-envs", "8", "--env-config",
                              '{"log_interval": 3, "resample": "random", "probegostart": 0.25}'])
    plan = trainer.pool_plan(args)
    assert plan["log_interval"] == 3 and plan["resample"] == "random" and plan["env_config"] == {"probegostart": 0.25}
    assert args.env_config == {"log_interval": 3, "resample": "random", "probegostart": 0.25}
    args = trainer.parse_cli(["LiarsDice-v0", "PPO", "PPO", "--n-envs", "8", "--env-config", '{"log_interval": 0, "probegostart": 1.0}'])
    assert trainer.pool_plan(args) is None
    assert trainer.vectorised_plan(args) == (0, {"probegostart": 1.0})
    assert args.env_config == {"log_interval": 0, "probegostart": 1.0}
    args = trainer.parse_cli(["RPS-v0", "PPO", "PPO", "--n-envs", "8"])
    assert trainer.vectorised_plan(args) == (trainer.LOG_INTERVAL, {}) and trainer.LOG_INTERVAL == 10
    assert trainer.pool_plan(trainer.parse_cli(["LiarsDice-v0", "PPO", "DEFAULT", "--n-envs", "8"]))["log_interval"] == 10
    for bad in ("-1", "2.5", '"often"', "true"):
        args = trainer.parse_cli(["RPS-v0", "PPO", "PPO", "--n-envs", "8", "--env-config", '{"log_interval": %s}' % bad])
        with pytest.raises(trainer.EnvException, match="log_interval"):
            trainer.vectorised_plan(args)
    assert "log_interval" not in {a.dest for a in trainer.build_parser()._actions}      # an --env-config key, not a flag


class _FakeStats(EpisodeStats):
    """EpisodeStats over a host array in place of the device accumulator"""

    def __init__(self, K):
        self.pool = False
        self._init_host(K)
        self.block = np.zeros((K, nat.EPISODE_NSTAT))

    def _fetch_totals(self):
        return self.block.copy()


def test_read_reports_the_window_against_the_totals():
    s = _FakeStats(2)
    rep = s.read()
    for part in (rep["window"], rep["total"]):                  # nothing ended: zeros, no NaN anywhere
        assert part["count"] == 0 and part["mean"] == 0.0 and part["std"] == 0.0 and part["mean_length"] == 0.0
        assert all(m == dict(count=0, mean=0.0, std=0.0, mean_length=0.0) for m in part["members"])
    # member 0: returns 1, 3 (lengths 2, 4); member 1: nothing
    s.block[0] = (2, 4, 10, 6)
    rep = s.read()
    assert rep["window"] == rep["total"]
    assert rep["total"]["members"][0] == dict(count=2, mean=2.0, std=1.0, mean_length=3.0)
    assert rep["total"]["members"][1]["count"] == 0 and not math.isnan(rep["total"]["members"][1]["mean"])
    assert rep["total"]["count"] == 2 and rep["total"]["mean"] == 2.0
    # then member 0: 5 (length 1); member 1: -1, -1 (lengths 3, 3)
    s.block[0] += (1, 5, 25, 1)
    s.block[1] += (2, -2, 2, 6)
    peek = s.read(reset_window=False)
    rep = s.read()
    assert peek == rep                                           # a peek leaves the window open
    w, t = rep["window"], rep["total"]
    assert w["members"][0] == dict(count=1, mean=5.0, std=0.0, mean_length=1.0)
    assert w["members"][1] == dict(count=2, mean=-1.0, std=0.0, mean_length=3.0)
    assert w["count"] == 3 and w["mean"] == 1.0 and w["mean_length"] == 7 / 3
    assert w["std"] == pytest.approx(math.sqrt(27 / 3 - 1.0), rel=1e-15)
    assert t["count"] == 5 and t["mean"] == 7 / 5 and t["members"][0]["count"] == 3
    assert t["std"] == pytest.approx(math.sqrt(37 / 5 - (7 / 5) ** 2), rel=1e-15)
    assert s.read()["window"]["count"] == 0 and s.read()["total"] == t
    # a variance that rounds below zero is clamped, not a NaN
    assert 0.02999999999999999 / 3.0 - (0.3 / 3.0) ** 2 < 0
    assert episode_summary(np.array([3.0, 0.3, 0.02999999999999999, 3.0]))["std"] == 0.0
    assert episode_report(np.zeros((3, 4)))["members"][2]["count"] == 0


def test_agents_carry_no_statistics_unless_attached():
    import inspect

    from pantheonrl_amd import vec
    src = inspect.getsource(vec.VecOnPolicyAgent)
    assert "self.episode_stats = None" in src
    body = inspect.getsource(vec.VecOnPolicyAgent.compute_returns)
    assert body.index("flush_rewards()") < body.index("episode_stats.scan()")
