"""Cross-play evaluation of Liar's Dice with every table on the device: `tester.py` of the reference (tester.py:41-63 -- play a
loaded ego against a loaded or default partner for a number of games, print the mean and standard deviation of the ego's returns)
for a whole population at once.

`VecLiarCrossPlay` seats BOTH players of E tables from one population of M <= 8 members (`FrozenVecPartner`, `ClonedVecPartner`,
`VecLiarDefaultPartner`)
and plays a list of ordered pairs (i, j) -- member i at seat 0 (the ego), member j at seat 1 (the partner).  `crossplay_stats` is the
host statement of the per-pair reduction `ph_xplay_stats` runs on the device.

`VecBlockCrossPlay` is the same evaluation for the block worlds, whose seats have different spaces: a population of planners, a
population of constructors (frozen policies and scripted constructors), a list of (planner, constructor) pairs.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch as th

from .. import _native as nat
from ..spaces import make_spec
from .vec import (AdapFrozenVecPartner, ClonedVecPartner, FrozenVecPartner, TowerFrozenVecPartner, VecLiarDefaultPartner,
                  VecLiarsDice, VecLiarStep, check_liar_member_policy)

MAX_STEPS_PER_GAME = 7       # 12 bids and a call: at most 7 moves of the ego, whoever opens


def all_pairs(n_members: int) -> List[Tuple[int, int]]:
    """every ordered pair (ego, partner) of the population, row major -- the diagonal included"""
    return [(i, j) for i in range(int(n_members)) for j in range(int(n_members))]


def check_pairs(n_envs: int, n_members: int, pairs: Optional[Sequence[Sequence[int]]]) -> np.ndarray:
    """-> (P, 2) int32.  None = all M^2 ordered pairs; more pairs than tables, or a member out of range, is refused"""
    if not 1 <= int(n_members) <= nat.PH_MAX_POOL:
        raise nat.NativeError(f"cross-play: the population holds 1..{nat.PH_MAX_POOL} members, not {n_members}")
    arr = np.asarray(all_pairs(n_members) if pairs is None else [tuple(p) for p in pairs], np.int64).reshape(-1, 2)
    if len(arr) < 1:
        raise nat.NativeError("cross-play: the pair list is empty")
    if len(arr) > int(n_envs):
        raise nat.NativeError(f"cross-play: {len(arr)} pairs need at least as many tables, not n_envs = {n_envs} (table e plays "
                              "pairs[e % P])")
    if arr.min() < 0 or arr.max() >= int(n_members):
        raise nat.NativeError(f"cross-play: a pair names a member outside 0..{int(n_members) - 1}")
    return arr.astype(np.int32)


def pair_of_tables(n_envs: int, n_pairs: int) -> np.ndarray:
    """table e plays pair e % P for the whole evaluation"""
    if int(n_pairs) > int(n_envs):
        raise nat.NativeError(f"cross-play: {n_pairs} pairs need at least as many tables, not n_envs = {n_envs}")
    return (np.arange(int(n_envs)) % int(n_pairs)).astype(np.int32)


def crossplay_stats(returns, lengths, pair_of_table, n_pairs: int, games=None) -> dict:
    """The per-pair reduction in plain numpy: over a pair's tables in ascending order and each table's games in ascending order,
    float64 count / sum / sum of squares / sum of lengths (running sums, the order `ph_xplay_stats` adds in), and from them the
    mean, the POPULATION standard deviation (np.std, what tester.py:54 prints) and the mean length.  `games` (E): how many games
    of each table count (None = all G)."""
    returns, lengths = np.asarray(returns), np.asarray(lengths)
    pair_of_table = np.asarray(pair_of_table)
    E, G = returns.shape
    games = np.full(E, G, np.int64) if games is None else np.clip(np.asarray(games, np.int64), 0, G)
    out = {k: np.zeros(int(n_pairs), np.float64) for k in ("count", "sum", "sumsq", "sum_length")}
    for p in range(int(n_pairs)):
        tables = np.nonzero(pair_of_table == p)[0]
        r = np.concatenate([returns[e, :games[e]] for e in tables] + [np.zeros(0)]).astype(np.float64)
        ln = np.concatenate([lengths[e, :games[e]] for e in tables] + [np.zeros(0)]).astype(np.float64)
        out["count"][p] = float(len(r))
        if len(r):
            out["sum"][p] = np.cumsum(r)[-1]
            out["sumsq"][p] = np.cumsum(r * r)[-1]
            out["sum_length"][p] = np.cumsum(ln)[-1]
    out.update(derived_stats(out["count"], out["sum"], out["sumsq"], out["sum_length"]))
    return out


def derived_stats(count, total, sumsq, sum_length) -> dict:
    """mean, population standard deviation and mean length from the four sums (nan where nothing was played)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = total / count
        std = np.sqrt(np.maximum(sumsq / count - mean * mean, 0.0))
        return dict(mean=mean, std=std, mean_length=sum_length / count)


class CrossPlayResult:
    """What `VecLiarCrossPlay.run` returns: the logs, the table -> pair assignment and the per-pair statistics."""

    def __init__(self, n_members, pairs, pair_of_table, returns, lengths, stats, steps):
        self.n_members, self.pairs, self.pair_of_table = int(n_members), np.asarray(pairs), np.asarray(pair_of_table)
        self.returns, self.lengths, self.steps = returns, lengths, int(steps)
        self.count, self.sum, self.sumsq, self.sum_length = (stats[:, i].copy() for i in range(nat.XPLAY_NSTAT))
        for k, v in derived_stats(self.count, self.sum, self.sumsq, self.sum_length).items():
            setattr(self, k, v)

    def matrix(self, name: str = "mean") -> np.ndarray:
        """(M, M): entry [i, j] = statistic `name` of the pair (ego i, partner j); nan where the pair was not played (a pair
        listed twice reports its last entry)"""
        out = np.full((self.n_members, self.n_members), np.nan)
        for (i, j), v in zip(self.pairs, getattr(self, name)):
            out[i, j] = v
        return out


class VecLiarCrossPlay(VecLiarStep):
    """tester.py:41-63 for a population: n_envs Liar's Dice tables resident on the device, both seats held by members of ONE
    population of M <= 8 frozen 64-64 policies (`FrozenVecPartner`), frozen net_arch towers (`TowerFrozenVecPartner`), frozen ADAP
    checkpoints under a stated or a per-table sampled latent (`AdapFrozenVecPartner`), behavioural clones (`ClonedVecPartner`: the shared 32-32 trunk of
    bc.py) and scripted players (`VecLiarDefaultPartner`); the same object
    may sit in either seat, or in both.

    The choices this class pins:
    * table e plays `pairs[e % P]` = (ego member, partner member) for the whole evaluation -- no resampling; P > n_envs is refused;
      diagonal pairs are legal; `pairs=None` is all M^2 ordered pairs, row major;
    * every table plays exactly `episodes_per_table` games and then goes idle: masked out of every forward and pass, its state and
      logs never change again (taking "the first N games to finish" would favour short games);
    * one step c >= 1 is one MultiAgentEnv.step of every playing table: seat 0's forward (Philox counter 3c), its move; seat 1's
      reply where the game goes on (3c + 1), its move and the ends of games -- log the return and length at [e, games[e]], count
      the game, then deal the next one (dice counter c) or retire the table (`tables_left` -= 1); seat 1's opening where it
      starts the new game (3c + 2).  The constructor's deal is step 0 (dice counter 0, opening counter 2).  A member draws under
      its own seed with row = table, so the seats' counters are disjoint even when one member holds both;
    * a game's return is the sum of the ego rewards MultiAgentEnv.step returns over it (the ego's transition plus the reply's),
      accumulated in float32; its length is the number of ego moves;
    * per pair, count / sum / sum of squares / sum of lengths are float64 sums in ascending table then game order, without
      atomics: two runs give the same bits.

    native=True: one `ph_liar_xplay_step` per step -- three bucket passes, three grouped forwards, three book-keeping launches,
    whatever M is, no host synchronisation.  native=False: the readable walk (VecLiarStep) -- per-member `ph_policy_forward` / `ph_bc_forward` /
    `ph_liar_default_actions`, `VecLiarsDice.player_step`, torch masks, the same counters; bitwise the native step."""

    def __init__(self, n_envs: int, members, pairs=None, episodes_per_table: int = 1, seed: int = 0, probegostart: float = 0.5,
                 native: bool = True, record: int = 0):
        members = list(members)
        self.pairs = check_pairs(n_envs, len(members), pairs)
        if int(episodes_per_table) < 1:
            raise nat.NativeError("VecLiarCrossPlay: episodes_per_table must be at least 1")
        self.G, self.M, self.P = int(episodes_per_table), len(members), len(self.pairs)
        self.members = members
        dev = None
        for m in members:
            if isinstance(m, VecLiarDefaultPartner):
                continue
            if not isinstance(m, (FrozenVecPartner, ClonedVecPartner)):
                raise nat.NativeError("VecLiarCrossPlay: members are FrozenVecPartner / ClonedVecPartner / VecLiarDefaultPartner "
                                      f"(learners train in VecLiarPartnerPool), not {type(m).__name__}")
            check_liar_member_policy(m.policy, type(self).__name__, towers=isinstance(m, TowerFrozenVecPartner),
                                     adap=isinstance(m, AdapFrozenVecPartner))
            dev = dev or m.policy.device
        dev = dev or th.device("cuda", th.cuda.current_device())
        self.ctx = nat.Context(dev.index or 0)
        self.spec = make_spec(VecLiarsDice.observation_space, VecLiarsDice.action_space)
        self._init_game(n_envs, self.ctx, dev, seed, probegostart, native)
        self.pair_of_table = pair_of_tables(self.E, self.P)
        self._seat_members = [sorted(set(self.pairs[:, s].tolist())) for s in (0, 1)]     # who can move at seat 0 / seat 1
        E, G = self.E, self.G
        self.ego_id = th.as_tensor(self.pairs[self.pair_of_table, 0].copy()).to(dev)
        self.alt_id = th.as_tensor(self.pairs[self.pair_of_table, 1].copy()).to(dev)
        self.ego_actions = th.zeros((E, 2), dtype=th.int32, device=dev)
        self.alt_actions = th.zeros((E, 2), dtype=th.int32, device=dev)
        self.games = th.zeros(E, dtype=th.int32, device=dev)
        self.playing = th.ones(E, dtype=th.uint8, device=dev)
        self.tables_left = th.full((1,), E, dtype=th.int32, device=dev)
        self.ep_return = th.zeros(E, dtype=th.float32, device=dev)
        self.ep_length = th.zeros(E, dtype=th.int32, device=dev)
        self.returns = th.zeros((E, G), dtype=th.float32, device=dev)
        self.lengths = th.zeros((E, G), dtype=th.int32, device=dev)
        self.stats = th.zeros((self.P, nat.XPLAY_NSTAT), dtype=th.float64, device=dev)
        if record:
            self.start_recording(record)          # the move log (VecLiarStep.start_recording), from the first openings on
        self._first_deal()

    def _contexts(self):
        return [self.ctx] + [m.policy.ctx for m in self.members if isinstance(m, (FrozenVecPartner, ClonedVecPartner))]

    def _counters(self, c: int):
        return 3 * c, 3 * c + 1, 3 * c + 2

    # -- the engine-side step ------------------------------------------------------------------------------------------------------
    def _build_native(self) -> None:
        self._pairs_arr = (C.c_int * (2 * self.P))(*[int(v) for v in self.pairs.reshape(-1)])
        s = self._fill_game(nat.PhLiarXplay(), book=False)
        s.spec = C.pointer(self.spec)
        self.towers = any(isinstance(m, TowerFrozenVecPartner) for m in self.members)      # a tower member: the step needs the archs
        self.adaps = any(isinstance(m, AdapFrozenVecPartner) for m in self.members)       # a frozen ADAP member: archs and descriptions
        s.members, s.n_members = self._member_arrays(self.members, self.towers or self.adaps, self.adaps), self.M
        s.pairs, s.n_pairs, s.episodes_per_table = self._pairs_arr, self.P, self.G
        for name in ("ego_id", "alt_id", "ego_actions", "alt_actions", "games", "playing", "tables_left", "ep_return", "ep_length",
                     "returns", "lengths"):
            setattr(s, name, getattr(self, name).data_ptr())
        self._desc = s

    def _native_call(self, counter: int, deal_only: bool = False) -> None:
        self._bind()
        # the widest entry point; an array no member needs is None (`_member_arrays`): the narrow entry points' own forward
        nat.check(self.ctx.lib.ph_liar_xplay_step_adap(self.ctx.handle, C.byref(self._desc), self._member_arch_arr,
                                                       self._member_adap_arr, int(counter), int(deal_only)))

    # -- the walk's hooks ----------------------------------------------------------------------------------------------------------
    def _seat_act(self, seat: int, obs: th.Tensor, mask: th.Tensor, counter: int) -> th.Tensor:
        """the forward of every member that can sit at `seat`, Philox counter `counter`; member k's move lands in the tables of
        `mask` it holds that seat of"""
        ids, out = (self.ego_id, self.ego_actions) if seat == 0 else (self.alt_id, self.alt_actions)
        return self._members_act(self._seat_members[seat], ids, obs, mask, counter, out)

    def _live(self) -> th.Tensor:
        return self.playing

    def _seat_member(self, seat: int) -> th.Tensor:
        return self.ego_id if seat == 0 else self.alt_id

    def _game_end(self, reward: th.Tensor, done: th.Tensor) -> th.Tensor:
        """the step's return and length; at the end of a game the log entry, the count, the budget -> the tables dealt again"""
        G, playing = self.G, self.playing.bool()
        self.ep_return.copy_(th.where(playing, self.ep_return + reward, self.ep_return))
        self.ep_length.add_(playing.to(th.int32))
        slot = self.games.clamp(max=G - 1).long()[:, None]
        self.returns.scatter_(1, slot, th.where(done, self.ep_return, self.returns.gather(1, slot)[:, 0])[:, None])
        self.lengths.scatter_(1, slot, th.where(done, self.ep_length, self.lengths.gather(1, slot)[:, 0])[:, None])
        self.games.add_(done.to(th.int32))
        self.ep_return.copy_(th.where(done, th.zeros_like(self.ep_return), self.ep_return))
        self.ep_length.copy_(th.where(done, th.zeros_like(self.ep_length), self.ep_length))
        spent = done & (self.games >= G)
        self.playing.copy_((playing & ~spent).to(th.uint8))
        self.tables_left.sub_(spent.sum().to(th.int32))
        return (done & ~spent).to(th.uint8)

    # -- one vectorised MultiAgentEnv.step of the playing tables -------------------------------------------------------------------
    def step(self) -> None:
        self.steps_done += 1
        if self.native:
            self._native_call(self.steps_done)
        else:
            self._walk(self.steps_done)

    def left(self) -> int:
        """tables with budget left (synchronises)"""
        return int(self.tables_left.item())

    def compute_stats(self) -> np.ndarray:
        """`ph_xplay_stats` over the logs so far -> (P, 4) float64: count, sum, sum of squares, sum of lengths"""
        self._bind()
        nat.check(self.ctx.lib.ph_xplay_stats(self.ctx.handle, self.returns.data_ptr(), self.lengths.data_ptr(), self.games.data_ptr(),
                                              self.E, self.G, self.P, self.stats.data_ptr()))
        return self.stats.cpu().numpy()

    def run(self, chunk: int = 8) -> CrossPlayResult:
        """play every table's budget out: `chunk` steps at a time with nothing on the host in between, then one read of
        `tables_left`.  A game takes at most 7 steps, so more than 7 * G steps can only be a bug: that raises."""
        limit = MAX_STEPS_PER_GAME * self.G
        while self.left() > 0:
            if self.steps_done >= limit:
                raise nat.NativeError(f"VecLiarCrossPlay: {self.left()} tables still play after {limit} steps "
                                      f"(a game takes at most {MAX_STEPS_PER_GAME})")
            for _ in range(min(int(chunk), limit - self.steps_done)):
                self.step()
        stats = self.compute_stats()
        return CrossPlayResult(self.M, self.pairs, self.pair_of_table, self.returns.cpu().numpy(), self.lengths.cpu().numpy(), stats,
                               self.steps_done)


# ---- the block worlds: every planner with every constructor ----------------------------------------------------------------------
BLOCK_STEPS_PER_GAME = 200     # default step cap per game of the budget: only the planner's last token ends a game, nothing bounds one


def block_pairs(n_envs: int, n_planners: int, n_constructors: int, pairs: Optional[Sequence[Sequence[int]]]) -> np.ndarray:
    """-> (P, 2) int32 of (planner, constructor).  None = all planner x constructor pairs, row major; more pairs than tables, an
    empty list, or a member out of range is refused"""
    for name, count in (("planners", n_planners), ("constructors", n_constructors)):
        if not 1 <= int(count) <= nat.PH_MAX_POOL:
            raise nat.NativeError(f"block cross-play: a seat holds 1..{nat.PH_MAX_POOL} {name}, not {count}")
    every = [(i, j) for i in range(int(n_planners)) for j in range(int(n_constructors))]
    arr = np.asarray(every if pairs is None else [tuple(p) for p in pairs], np.int64).reshape(-1, 2)
    if len(arr) < 1:
        raise nat.NativeError("block cross-play: the pair list is empty")
    if len(arr) > int(n_envs):
        raise nat.NativeError(f"block cross-play: {len(arr)} pairs need at least as many tables, not n_envs = {n_envs} (table e plays "
                              "pairs[e % P])")
    if arr.min() < 0 or arr[:, 0].max() >= int(n_planners) or arr[:, 1].max() >= int(n_constructors):
        raise nat.NativeError(f"block cross-play: a pair names a member outside 0..{int(n_planners) - 1} x 0..{int(n_constructors) - 1}")
    return arr.astype(np.int32)


def check_block_member(member, variant: int, seat: int, who: str) -> None:
    """a member of a block-world evaluation is a frozen 64-64 policy on that seat's spaces or -- at the constructor's seat -- a
    scripted constructor of that variant; everything else is refused by name"""
    from ..ppo import require_mlp_kernels
    from ..vec import is_tower
    from .vec import VecBlockScriptedPartner, VecBlockWorld
    seat_name = ("planner", "constructor")[seat]
    if isinstance(member, VecBlockScriptedPartner):
        if seat == 0:
            raise nat.NativeError(f"{who}: a scripted constructor does not sit at the planner's seat")
        if member.variant != int(variant):
            raise nat.NativeError(f"{who}: the scripted constructor is {VecBlockWorld.GAMES[member.variant]}'s, not "
                                  f"{VecBlockWorld.GAMES[int(variant)]}'s")
        return
    if isinstance(member, VecLiarDefaultPartner):
        raise nat.NativeError(f"{who}: VecLiarDefaultPartner is the Liar's Dice player; a block world's scripted constructor is "
                              "VecBlockScriptedPartner(variant, rule)")
    if isinstance(member, ClonedVecPartner):
        raise nat.NativeError(f"{who}: a BC clone (ClonedVecPartner, FeedForward32Policy) does not sit in the block worlds' cross-play")
    if isinstance(member, AdapFrozenVecPartner):
        raise nat.NativeError(f"{who}: an ADAP checkpoint (AdapFrozenVecPartner) does not sit in the block worlds' cross-play")
    if isinstance(member, TowerFrozenVecPartner) or (isinstance(member, FrozenVecPartner) and is_tower(member.policy)):
        raise nat.NativeError(f"{who}: a net_arch tower (ArchActorCriticPolicy) does not sit in the block worlds' cross-play")
    if not isinstance(member, FrozenVecPartner):
        raise nat.NativeError(f"{who}: members are FrozenVecPartner / VecBlockScriptedPartner (learners train in VecBlockSelfPlay), "
                              f"not {type(member).__name__}")
    policy = member.policy
    if policy.spec.act.kind == nat.PH_SPACE_BOX:
        raise nat.NativeError(f"{who}: a policy with Box actions does not play a block world")
    require_mlp_kernels(policy, who)
    spaces = VecBlockWorld.seat_spaces(variant)[seat]
    want = nat.layout_of(make_spec(spaces.observation_space, spaces.action_space))
    lay = policy.layout
    if (lay.D, lay.F, lay.A, lay.L) != (want.D, want.F, want.A, want.L):
        raise nat.NativeError(f"{who}: the policy does not play on {VecBlockWorld.GAMES[int(variant)]}'s {seat_name} spaces")


class BlockCrossPlayResult(CrossPlayResult):
    """What `VecBlockCrossPlay.run` returns: CrossPlayResult with a planner x constructor matrix, the games each table logged and the
    number of budgeted games that did not finish under the step cap."""

    def __init__(self, n_planners, n_constructors, pairs, pair_of_table, returns, lengths, games, stats, steps):
        super().__init__(n_planners, pairs, pair_of_table, returns, lengths, stats, steps)
        self.n_planners, self.n_constructors = int(n_planners), int(n_constructors)
        self.games = np.asarray(games)
        self.unfinished = int(returns.shape[0] * returns.shape[1] - self.games.sum())

    def matrix(self, name: str = "mean") -> np.ndarray:
        """(planners, constructors): entry [i, j] = statistic `name` of the pair (planner i, constructor j); nan where the pair was
        not played"""
        out = np.full((self.n_planners, self.n_constructors), np.nan)
        for (i, j), v in zip(self.pairs, getattr(self, name)):
            out[i, j] = v
        return out


class VecBlockCrossPlay:
    """tester.py:41-63 for a block world and two populations: n_envs tables of BlockEnv-v0 (variant 0) or BlockEnv-v1 (variant 1)
    resident on the device, the planner's seat held by one of up to 8 frozen 64-64 policies (`FrozenVecPartner`), the constructor's
    by one of up to 8 frozen policies or scripted constructors (`VecBlockScriptedPartner`).

    * table e plays `pairs[e % P]` = (planner, constructor) for the whole evaluation; `pairs=None` is every planner x constructor
      pair, row major; P > n_envs is refused;
    * every table plays exactly `games` games and then goes idle: masked out of every launch, its state and logs frozen;
    * one step c >= 1: the planners' forward (Philox counter 2c), the token; on the end token the game's return (f32 sum of ego
      rewards) and length (planner tokens) are logged at [e, games[e]], the game counted, and the next world generated (world counter
      c) or the table retired (`tables_left` -= 1); otherwise the constructors' forward (2c + 1) and their move.  The first worlds
      use world counter 0.  A member draws under its own seed with row = table;
    * a game ends only when the planner says its last token, so nothing bounds one: `run` stops at a step cap and reports the games
      that did not finish; the statistics cover the logged games only.

    native=True: one `ph_block_xplay_step` per step -- two bucket passes, two grouped forwards, two book-keeping launches and one more
    when a constructor is scripted, whatever the number of members, no host synchronisation.  native=False: the readable walk --
    `ph_policy_forward` per member over all rows, `ph_block_scripted_actions`, `ph_block_step` / `ph_block_reset` / `ph_block_obs`,
    torch masks, the same counters; bitwise the native step."""

    def __init__(self, variant: int, n_envs: int, planners, constructors, pairs=None, games: int = 1, seed: int = 0,
                 native: bool = True):
        from .vec import VecBlockScriptedPartner, VecBlockWorld
        self.variant = int(variant)
        if self.variant not in (0, 1):
            raise nat.NativeError("VecBlockCrossPlay: variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)")
        self.planners, self.constructors = list(planners), list(constructors)
        self.pairs = block_pairs(n_envs, len(self.planners), len(self.constructors), pairs)
        if int(games) < 1:
            raise nat.NativeError("VecBlockCrossPlay: games must be at least 1")
        self.E, self.G, self.P, self.native = int(n_envs), int(games), len(self.pairs), bool(native)
        self.seed = int(seed)
        dev = None
        for seat, members in enumerate((self.planners, self.constructors)):
            for k, m in enumerate(members):
                check_block_member(m, self.variant, seat, f"VecBlockCrossPlay: {('planner', 'constructor')[seat]} {k}")
                if not isinstance(m, VecBlockScriptedPartner):
                    dev = dev or m.policy.device
        dev = dev or th.device("cuda", th.cuda.current_device())
        self.dev = dev
        self.ctx = nat.Context(dev.index or 0)
        self.env = VecBlockWorld(self.variant, self.E, self.ctx, dev)
        ego_spaces, alt_spaces = VecBlockWorld.seat_spaces(self.variant)
        self.ego_spec = make_spec(ego_spaces.observation_space, ego_spaces.action_space)
        self.alt_spec = make_spec(alt_spaces.observation_space, alt_spaces.action_space)
        self.pair_of_table = pair_of_tables(self.E, self.P)
        self._seat_members = [sorted(set(self.pairs[:, s].tolist())) for s in (0, 1)]
        E, G = self.E, self.G
        A = len(alt_spaces.action_space.nvec)
        self.ego_id = th.as_tensor(self.pairs[self.pair_of_table, 0].copy()).to(dev)
        self.alt_id = th.as_tensor(self.pairs[self.pair_of_table, 1].copy()).to(dev)
        self.ego_actions = th.zeros(E, dtype=th.int32, device=dev)
        self.alt_actions = th.zeros((E, A), dtype=th.int32, device=dev)
        self.obs_ego = th.zeros((E, self.env.D_ego), dtype=th.float32, device=dev)
        self.obs_alt = th.zeros((E, self.env.D_alt), dtype=th.float32, device=dev)
        self.games = th.zeros(E, dtype=th.int32, device=dev)
        self.playing = th.ones(E, dtype=th.uint8, device=dev)
        self.running = th.zeros(E, dtype=th.uint8, device=dev)
        self.tables_left = th.full((1,), E, dtype=th.int32, device=dev)
        self.ep_return = th.zeros(E, dtype=th.float32, device=dev)
        self.ep_length = th.zeros(E, dtype=th.int32, device=dev)
        self.returns = th.zeros((E, G), dtype=th.float32, device=dev)
        self.lengths = th.zeros((E, G), dtype=th.int32, device=dev)
        self._stats = th.zeros((self.P, nat.XPLAY_NSTAT), dtype=th.float64, device=dev)
        self.steps_done = 0
        self._ctxs = [self.ctx] + [m.policy.ctx for m in self.planners + self.constructors if isinstance(m, FrozenVecPartner)]
        self._bind()
        if self.native:
            self._build_native()
            nat.check(self.ctx.lib.ph_block_xplay_step(self.ctx.handle, C.byref(self._desc), 0, 1))
        else:
            self.env.reset(self.seed, 0)
            self.env.observe(True, self.obs_ego)

    @property
    def state(self) -> th.Tensor:
        """(E, 12) int32 packed tables"""
        return self.env.state

    def _bind(self):
        stream = th.cuda.current_stream(self.dev).cuda_stream
        for ctx in self._ctxs:
            ctx.set_stream(stream)

    # -- the engine-side step ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _member_array(members):
        arr = (nat.PhPoolMember * len(members))()
        for c, m in zip(arr, members):
            c.kind = m.kind
            if m.kind == nat.PH_POOL_SCRIPTED:
                c.seed = m.rule                   # (a scripted member's `seed` holds its rule)
            else:
                c.params, c.seed = m.policy.params.data_ptr(), m.policy._seed
        return arr

    def _build_native(self) -> None:
        self._pairs_arr = (C.c_int * (2 * self.P))(*[int(v) for v in self.pairs.reshape(-1)])
        self._planner_arr, self._constructor_arr = self._member_array(self.planners), self._member_array(self.constructors)
        s = nat.PhBlockXplay()
        s.n, s.variant = self.E, self.variant
        s.ego_spec, s.alt_spec = C.pointer(self.ego_spec), C.pointer(self.alt_spec)
        s.state, s.world_seed = self.env.state.data_ptr(), self.seed
        s.planners, s.n_planners = self._planner_arr, len(self.planners)
        s.constructors, s.n_constructors = self._constructor_arr, len(self.constructors)
        s.pairs, s.n_pairs, s.episodes_per_table = self._pairs_arr, self.P, self.G
        for name in ("ego_id", "alt_id", "ego_actions", "alt_actions", "obs_ego", "obs_alt", "games", "playing", "tables_left",
                     "ep_return", "ep_length", "returns", "lengths", "running"):
            setattr(s, name, getattr(self, name).data_ptr())
        self._desc = s

    # -- the walk: the per-call entry points with torch masks ------------------------------------------------------------------------
    def _seat_act(self, seat: int, obs: th.Tensor, mask: th.Tensor, counter: int) -> None:
        """the forward of every member that can sit at `seat` over all rows, Philox counter `counter`; member k's move lands in the
        tables of `mask` it holds that seat of"""
        from .vec import VecBlockScriptedPartner
        members, ids, out = ((self.planners, self.ego_id, self.ego_actions) if seat == 0 else
                             (self.constructors, self.alt_id, self.alt_actions))
        for k in self._seat_members[seat]:
            m = members[k]
            mk = (mask.bool() & (ids == k)).to(th.uint8)
            if isinstance(m, VecBlockScriptedPartner):
                m.get_action(obs, mk, out, self.ctx)
                continue
            m.policy._counter = counter - 1
            a = m.get_action(obs, mk)
            if seat == 0:
                out.copy_(th.where(mk.bool(), a[:, 0], out))
            else:
                out.copy_(th.where(mk.bool()[:, None], a, out))

    def _walk(self, c: int) -> None:
        env, G = self.env, self.G
        playing = self.playing.clone()
        pb = playing.bool()
        self._seat_act(0, self.obs_ego, playing, 2 * c)
        obs_alt, rew, done = env.player_step(self.ego_actions, True, playing)
        d = done.bool() & pb                                       # (rows of idle tables are stale)
        # the token counts; the end token logs the game, counts it, and spends the budget or starts the next world
        self.ep_return.copy_(th.where(pb, self.ep_return + rew[:, 0], self.ep_return))
        self.ep_length.add_(pb.to(th.int32))
        slot = self.games.clamp(max=G - 1).long()[:, None]
        self.returns.scatter_(1, slot, th.where(d, self.ep_return, self.returns.gather(1, slot)[:, 0])[:, None])
        self.lengths.scatter_(1, slot, th.where(d, self.ep_length, self.lengths.gather(1, slot)[:, 0])[:, None])
        self.games.add_(d.to(th.int32))
        self.ep_return.copy_(th.where(d, th.zeros_like(self.ep_return), self.ep_return))
        self.ep_length.copy_(th.where(d, th.zeros_like(self.ep_length), self.ep_length))
        spent = d & (self.games >= G)
        self.playing.copy_((pb & ~spent).to(th.uint8))
        self.tables_left.sub_(spent.sum().to(th.int32))
        again = (d & ~spent).to(th.uint8)
        env.reset(self.seed, c, again)
        env.observe(True, self.obs_ego, again)
        # the constructor moves where the game goes on
        rb = pb & ~d
        running = rb.to(th.uint8)
        self.running.copy_(th.where(pb, running, self.running))
        self.obs_alt.copy_(th.where(rb[:, None], obs_alt, self.obs_alt))
        self._seat_act(1, self.obs_alt, running, 2 * c + 1)
        obs_ego, _, _ = env.player_step(self.alt_actions, False, running)
        self.obs_ego.copy_(th.where(rb[:, None], obs_ego, self.obs_ego))

    # -- one vectorised MultiAgentEnv.step of the playing tables -------------------------------------------------------------------
    def step(self) -> None:
        self.steps_done += 1
        self._bind()
        if self.native:
            nat.check(self.ctx.lib.ph_block_xplay_step(self.ctx.handle, C.byref(self._desc), self.steps_done, 0))
        else:
            self._walk(self.steps_done)

    def left(self) -> int:
        """tables with budget left (synchronises)"""
        return int(self.tables_left.item())

    def compute_stats(self) -> np.ndarray:
        """`ph_xplay_stats` over the logs so far -> (P, 4) float64: count, sum, sum of squares, sum of lengths"""
        self._bind()
        nat.check(self.ctx.lib.ph_xplay_stats(self.ctx.handle, self.returns.data_ptr(), self.lengths.data_ptr(), self.games.data_ptr(),
                                              self.E, self.G, self.P, self._stats.data_ptr()))
        return self._stats.cpu().numpy()

    def result(self) -> BlockCrossPlayResult:
        stats = self.compute_stats()
        return BlockCrossPlayResult(len(self.planners), len(self.constructors), self.pairs, self.pair_of_table,
                                    self.returns.cpu().numpy(), self.lengths.cpu().numpy(), self.games.cpu().numpy(), stats,
                                    self.steps_done)

    def stats(self) -> dict:
        """per pair: count, mean, population standard deviation and mean length of the logged games; `unfinished`: budgeted games
        that have not finished"""
        res = self.result()
        return dict(count=res.count, mean=res.mean, std=res.std, mean_length=res.mean_length, unfinished=res.unfinished)

    def run(self, max_steps: Optional[int] = None, chunk: int = 8) -> BlockCrossPlayResult:
        """play the budgets out, `chunk` steps at a time with nothing on the host in between, then one read of `tables_left`; stops
        after `max_steps` steps in all (default 200 per game of the budget) and reports what did not finish"""
        limit = BLOCK_STEPS_PER_GAME * self.G if max_steps is None else int(max_steps)
        while self.steps_done < limit and self.left() > 0:
            for _ in range(min(int(chunk), limit - self.steps_done)):
                self.step()
        return self.result()
