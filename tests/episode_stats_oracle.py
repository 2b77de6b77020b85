"""NumPy restatement of `ph_episode_stats` (csrc/ph_episode.hip): the checker of the episode-statistics tests.

An episode of table e ends at row t iff episode_starts[t + 1][e] is set (t + 1 < T) or last_dones[e] is (t = T - 1); its return is
the float32 sum of rewards[.][e] over its rows in row order, carry first; its length is its number of rows.  Games span scans: the
oracle carries (return, length, valid) per table.  With K > 1 an ending episode is credited to the member the oracle holds for the
table, which then advances by `envs.vec.pool_resample` -- for the random rule with word 0 of Philox block POOL_RESAMPLE_BLOCK keyed
(pool seed, counter0 + t + (epoch << 32), table).  Sums over episodes are float64, added in the order the episodes were found."""
import numpy as np

from pantheonrl_amd.envs.vec import POOL_RESAMPLE_BLOCK, philox_word0, pool_resample


class EpisodeOracle:
    def __init__(self, E, K=1, member=None, rule="robin", pool_seed=0, valid=True):
        self.E, self.K, self.rule, self.pool_seed = int(E), int(K), rule, int(pool_seed)
        self.ret = np.zeros(E, np.float32)
        self.len = np.zeros(E, np.int64)
        self.valid = np.full(E, bool(valid))
        self.member = np.zeros(E, np.int64) if member is None else np.asarray(member, np.int64).copy()
        self.episodes = []          # (member, float32 return, length) in the order found: row by row, table by table

    def scan(self, rewards, starts, last_dones, counter0=0, epoch=None):
        rewards = np.asarray(rewards, np.float32)
        T, E = rewards.shape
        assert E == self.E
        for t in range(T):
            self.ret = self.ret + rewards[t]            # float32 + float32: one rounding per row, as a sequential loop per column
            assert self.ret.dtype == np.float32
            self.len += 1
            ended = np.flatnonzero((starts[t + 1] if t + 1 < T else last_dones) != 0)
            if not len(ended):
                continue
            words = None
            if self.K > 1 and self.rule == "random":
                c = int(counter0) + t + ((int(epoch) << 32) if epoch is not None else 0)
                words = philox_word0(self.pool_seed, c, ended, POOL_RESAMPLE_BLOCK)
            for j, e in enumerate(ended):
                if self.valid[e]:
                    self.episodes.append((int(self.member[e]), np.float32(self.ret[e]), int(self.len[e])))
                self.ret[e], self.len[e], self.valid[e] = 0.0, 0, True
                if self.K > 1:
                    self.member[e] = pool_resample(int(self.member[e]), self.K, self.rule, None if words is None else int(words[j]))
        return self

    def stats(self):
        """(K, 4) float64: count, sum, sum of squares, sum of lengths per member, added sequentially in float64"""
        out = np.zeros((self.K, 4), np.float64)
        for m, r, l in self.episodes:
            x = np.float64(r)
            out[m] += (1.0, x, x * x, float(l))
        return out

    def bounds(self):
        """(K, 2) float64: what any float64 summation order of the member's n returns / squared returns may differ by from another:
        n * 2**-52 * sum |x| and n * 2**-52 * sum x**2 (each of the n - 1 additions rounds by at most 2**-53 of a partial sum that
        is itself at most the sum of magnitudes, in either order: twice that covers both)"""
        out = np.zeros((self.K, 2), np.float64)
        n = np.zeros(self.K)
        for m, r, _ in self.episodes:
            x = abs(np.float64(r))
            out[m] += (x, x * x)
            n[m] += 1
        return out * n[:, None] * 2.0 ** -52
