"""Episode returns and lengths of device-resident training, per pool member.

The host paths log `rollout/ep_rew_mean` / `rollout/ep_len_mean` out of SB3's Monitor records (reference
pantheonrl/common/agents.py:132-158).  The device-resident paths play their games without the host, so the same figures are
computed on the device, behind the rollout: every such path seats the ego as a rectangular `VecOnPolicyAgent`, and once its
buffer is full the reward plane and the episode-start plane hold every game of the rollout.  `EpisodeStats.scan()` is ONE launch
over those two planes (`ph_episode_stats`, csrc/ph_episode.hip), called by `VecOnPolicyAgent.compute_returns()`; nothing is added
to a step.  Games that span rollouts are carried per table from one scan to the next.

For the partner pool the member at seat 1 is replayed instead of logged: the scan credits an ending game to the member it holds
for the table and advances it with the step's own resample rule under the step's own counter, so after a scan its members must
equal `env.partnerid` -- `read()` checks exactly that.

The figures are over ALL episodes that ended in the window, over all tables -- not SB3's mean over a deque of the last 100 (with E
tables ending games in the same step "the last 100" has no defined order).  Partner-side returns are not reported.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch as th

from . import _native as nat


def episode_summary(block: np.ndarray) -> dict:
    """(count, sum, sum of squares, sum of lengths) f64 -> count, mean, population std, mean length; zeros where nothing ended"""
    n, s, q, l = (float(v) for v in block)
    if n <= 0:
        return dict(count=0, mean=0.0, std=0.0, mean_length=0.0)
    mean = s / n
    return dict(count=int(round(n)), mean=mean, std=math.sqrt(max(q / n - mean * mean, 0.0)), mean_length=l / n)


def episode_report(block: np.ndarray) -> dict:
    """(K, 4) running sums -> the overall summary with a `members` list of per-member summaries"""
    block = np.asarray(block, np.float64).reshape(-1, nat.EPISODE_NSTAT)
    out = episode_summary(block.sum(axis=0))
    out["members"] = [episode_summary(row) for row in block]
    return out


class EpisodeStats:
    """Owns the carries and accumulators of one ego's episode statistics and launches the scan (see the module docstring).

    `ego`: the VecOnPolicyAgent; `env`: the partner pool (VecLiarPartnerPool) when games are to be credited to members, else None
    or any other environment (it only gets the `episode_stats` attribute).  Attached before the ego's first step every table is
    valid; attached later the game each table has in progress is dropped when it ends."""

    def __init__(self, ego, env=None):
        self.ego, self.env = ego, env
        model = ego.model
        pol, rb = model.policy, model.rollout_buffer
        self.dev, self.E = pol.device, ego.E
        self.pool = env is not None and hasattr(env, "partnerid")
        if self.pool and rb.pos != 0:
            raise nat.NativeError("EpisodeStats: attach to a partner pool between rollouts (the ego's buffer holds rows of members "
                                  "that can no longer be replayed)")
        fresh = ego.num_timesteps == 0 and rb.pos == 0
        E, dev = self.E, self.dev
        self.carry_return = th.zeros(E, dtype=th.float32, device=dev)
        self.carry_length = th.zeros(E, dtype=th.int32, device=dev)
        self.carry_valid = th.full((E,), 1 if fresh else 0, dtype=th.uint8, device=dev)
        self.member = env.partnerid.clone() if self.pool else None       # copied on the device
        self._init_host(env.K if self.pool else 1)
        self.stats = th.zeros((self.K, nat.EPISODE_NSTAT), dtype=th.float64, device=dev)
        self._covered_step = None      # the last environment step the replayed members stand behind
        self._rbc = rb.c_struct()
        s = nat.PhEpisodeScan()
        s.rb, s.carry_return, s.carry_length = C.pointer(self._rbc), self.carry_return.data_ptr(), self.carry_length.data_ptr()
        s.carry_valid, s.n_members, s.member = self.carry_valid.data_ptr(), self.K, nat.ptr(self.member)
        s.resample = nat.POOL_RESAMPLE[env.resample] if self.pool else 0
        s.pool_seed = int(env.pool_seed) if self.pool else 0
        s.stats = self.stats.data_ptr()
        self._desc = s
        ego.episode_stats = self
        if env is not None:
            env.episode_stats = self

    def _init_host(self, n_members: int) -> None:
        self.K = int(n_members)
        self._prev = np.zeros((self.K, nat.EPISODE_NSTAT), np.float64)      # the running totals at the previous read

    def detach(self) -> None:
        self.ego.episode_stats = None

    # -- device side -----------------------------------------------------------------------------------------------------------------
    def scan(self) -> None:
        """one `ph_episode_stats` launch over the ego's buffer on the agent's stream; no allocation, no synchronisation (capturable
        once it ran outside capture)"""
        ego = self.ego
        rb, pol = ego.model.rollout_buffer, ego.model.policy
        last = ego._last_episode_starts
        if last.dtype != th.float32:
            raise nat.NativeError("EpisodeStats.scan: the ego's episode-start flags must be float32")
        s = self._desc
        s.T = int(rb.pos) or int(rb.buffer_size)       # the graph paths fill the whole buffer without moving `pos`
        s.last_dones = last.data_ptr()
        s.counter0 = int(self.env.row0_counter) if self.pool else 0
        nat.check(pol.ctx.lib.ph_episode_stats(pol.ctx.handle, C.byref(s)))
        if self.pool:
            # row t was step counter0 + t.  A scan from the step's own roll-over runs inside step c, before its deal: it covers c - 1
            self._covered_step = int(s.counter0) + int(s.T) - 1

    # -- host side -------------------------------------------------------------------------------------------------------------------
    def _fetch_totals(self) -> np.ndarray:
        """the one synchronisation of a read: the running totals, and for a pool the replayed members against the environment's"""
        th.cuda.synchronize(self.dev)
        totals = self.stats.cpu().numpy().copy()
        if self.pool and self._covered_step == self.env.steps_done:      # steps played since the scan have resampled since
            mine, theirs = self.member.cpu().numpy(), self.env.partnerid.cpu().numpy()
            bad = np.flatnonzero(mine != theirs)
            if len(bad):
                e = int(bad[0])
                raise nat.NativeError(f"EpisodeStats: the replayed member of table {e} is {int(mine[e])} but the pool holds "
                                      f"{int(theirs[e])} there: the statistics' attribution has lost step with the step's resample")
        return totals

    def _report(self, totals: np.ndarray, reset_window: bool) -> dict:
        totals = np.asarray(totals, np.float64).reshape(self.K, nat.EPISODE_NSTAT)
        out = dict(window=episode_report(totals - self._prev), total=episode_report(totals))
        if reset_window:
            self._prev = totals.copy()
        return out

    def read(self, reset_window: bool = True) -> dict:
        """-> {"window": ..., "total": ...}: count, mean, std (population), mean_length overall and under "members" per member --
        for the episodes that ended since the previous read (host-side differences of the running totals) and for the whole run"""
        return self._report(self._fetch_totals(), reset_window)


def record_episode_stats(logger, stats: EpisodeStats, iteration: int, num_timesteps: int, elapsed: float) -> dict:
    """one log record of the device-resident trainers: read the window and record it under SB3's keys"""
    rep = stats.read()
    win = rep["window"]
    logger.record("time/iterations", int(iteration))
    logger.record("time/fps", int(num_timesteps / max(elapsed, 1e-9)))
    logger.record("time/total_timesteps", int(num_timesteps))
    logger.record("rollout/ep_rew_mean", win["mean"])
    logger.record("rollout/ep_len_mean", win["mean_length"])
    logger.record("rollout/episodes", win["count"])
    if stats.pool:
        for i, m in enumerate(win["members"]):
            logger.record(f"rollout/ep_rew_mean_vs_{i}", m["mean"])
            logger.record(f"rollout/episodes_vs_{i}", m["count"])
    logger.dump(step=int(num_timesteps))
    return rep

