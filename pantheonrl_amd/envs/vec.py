"""Device-resident vectorised games: E independent copies stepped by one kernel launch.

`VecRPS` is the n_envs = E form of RPSEnv (reference pantheonrl/envs/rpsgym/rps.py:33-48): both seats act simultaneously
on the constant observation [0], payoffs follow the integer rule (ego - alt + 3) % 3, every episode lasts one step.
`selfplay_iteration` is the vectorised counterpart of `trainer.py RPS-v0 PPO PPO`: two learning agents, every callback
of the reference's step loop (multiagentenv.py:149-170) applied to E-long device tensors.

`VecLiarsDice` holds the state of E Liar's Dice tables on the device and applies `LiarEnv.player_step`
(liar.py:58-83) through `ph_liar_step`; dice are rolled on the host with the reference's draw order so a Python
`LiarEnv` fed the same dice is the bit-exact checker.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch as th

from .. import _native as nat
from ..spaces import Discrete, MultiDiscrete
from ..bc import FeedForward32Policy
from ..ppo import require_mlp_kernels
from ..vec import AdapSeat, VecOnPolicyAgent, is_adap, is_tower, require_tower_lds


class VecRPS:
    observation_space = Discrete(1)
    action_space = Discrete(3)

    def __init__(self, n_envs: int, ctx: nat.Context, device):
        self.E, self.ctx, self.device = n_envs, ctx, device
        self.obs = th.zeros((n_envs, 1), dtype=th.float32, device=device)      # NULL_OBS for every env, both seats
        self.dones = th.ones(n_envs, dtype=th.float32, device=device)          # one-step episodes: always done
        self.ego_rew = th.zeros(n_envs, dtype=th.float32, device=device)
        self.alt_rew = th.zeros(n_envs, dtype=th.float32, device=device)

    def step(self, ego_actions: th.Tensor, alt_actions: th.Tensor):
        """(E,) or (E,1) int32 device tensors -> (ego rewards, partner rewards, dones) device tensors"""
        self.ctx.set_stream(th.cuda.current_stream(self.device).cuda_stream)
        nat.check(self.ctx.lib.ph_rps_step(self.ctx.handle, ego_actions.data_ptr(), alt_actions.data_ptr(),
                                           self.ego_rew.data_ptr(), self.alt_rew.data_ptr(), self.E))
        return self.ego_rew, self.alt_rew, self.dones


def selfplay_iteration(env: VecRPS, ego: VecOnPolicyAgent, alt: VecOnPolicyAgent, n_steps: int) -> None:
    """n_steps simultaneous steps of E games, then both learners consume their rollouts."""
    ego.bind_stream()
    alt.bind_stream()
    for _ in range(n_steps):
        a0 = ego.get_action(env.obs)
        a1 = alt.get_action(env.obs)
        r0, r1, d = env.step(a0, a1)
        ego.update(r0, d)
        alt.update(r1, d)
        ego.flush_rewards()   # env.ego_rew / alt_rew are reused next step: apply now instead of deferring
        alt.flush_rewards()
    ego.learn_from_buffer()
    alt.learn_from_buffer()


class VecLiarsDice:
    N_SIDES, N_DICE, MAX_MOVES = 6, 6, 12
    observation_space = MultiDiscrete([7] * 6 + [7, 12] * 12)
    action_space = MultiDiscrete([7, 12])

    def __init__(self, n_envs: int, ctx: nat.Context, device):
        self.E, self.ctx, self.device = n_envs, ctx, device
        i32 = lambda *s: th.zeros(*s, dtype=th.int32, device=device)  # noqa: E731
        self.hands, self.history, self.nmoves = i32(n_envs, 12), i32(n_envs, 24), i32(n_envs)
        self.obs_next = th.zeros((n_envs, 30), dtype=th.float32, device=device)
        self.rewards = th.zeros((n_envs, 2), dtype=th.float32, device=device)
        self.done = th.zeros(n_envs, dtype=th.uint8, device=device)

    def reset(self, hands: np.ndarray) -> None:
        """hands (E, 12): ego histogram then partner histogram (roll them with envs.liar.roll_hand for reference order)"""
        self.hands.copy_(th.as_tensor(np.asarray(hands, np.int32)))
        self.history.zero_()
        self.nmoves.zero_()

    def player_step(self, actions: th.Tensor, is_ego: th.Tensor, active: th.Tensor = None):
        """actions (E,2) int32, is_ego (E) uint8, active (E) uint8 or None -> (obs of the other player, rewards (E,2), done)"""
        self.ctx.set_stream(th.cuda.current_stream(self.device).cuda_stream)
        nat.check(self.ctx.lib.ph_liar_step(self.ctx.handle, self.hands.data_ptr(), self.history.data_ptr(),
                                            self.nmoves.data_ptr(), actions.data_ptr(), is_ego.data_ptr(),
                                            nat.ptr(active), self.obs_next.data_ptr(), self.rewards.data_ptr(),
                                            self.done.data_ptr(), self.E))
        return self.obs_next, self.rewards, self.done


class RaggedVecOnPolicyAgent:
    """OnPolicyAgent for the PARTNER seat of a vectorised turn-based game.

    In a turn-based game the partner does not act in every environment at every vectorised step (a game may end on the
    ego's move, a new game may start with either player), so its rollout buffer cannot advance one row per step.  Each
    environment e owns column e of the (T, E) buffer and its own write row `pos[e]`; the learner trains
    when every column is full, which is the E-environment reading of "train before acting once the buffer is full"
    (agents.py:126).  Per environment the callbacks keep the reference's semantics:
      * a recorded action opens its row for late additive rewards until the agent is asked to act again (agents.py:198),
      * `episode_start` of a row = an episode ended since the previous recorded row (agents.py:176,197),
      * GAE bootstraps with V of the last recorded observation and dones = "the game ended before the next action"
        (agents.py:127-130, quirk D-1).
    `min_full` (default E = wait for every column) lowers the trigger: the learner trains as soon as that many columns are
    full, on exactly the full columns (compacted into a (T, n) buffer, `ph_buffer_compact_columns`), and only those columns
    start over.  Round-robin partner selection needs this: an environment spends whole episodes with other partners, so
    waiting for all columns starves the learner and drops the transitions that keep arriving in already-full columns.
    """

    def __init__(self, model):
        self.model = model
        pol, rb = model.policy, model.rollout_buffer
        self._require_kernels(pol)
        E, lay, dev = rb.n_envs, pol.layout, pol.device
        self.E, self.T = E, rb.buffer_size
        u8 = lambda v: th.full((E,), v, dtype=th.uint8, device=dev)  # noqa: E731
        self.pos = th.zeros(E, dtype=th.int32, device=dev)
        self.actions = th.zeros((E, lay.A), dtype=th.int32, device=dev)
        self.values = th.zeros(E, dtype=th.float32, device=dev)
        self.log_probs = th.zeros(E, dtype=th.float32, device=dev)
        self.boundary, self.term, self.open = u8(1), u8(0), u8(0)
        self.iteration = 0
        self.num_timesteps = 0
        self.min_full = E
        self._compact = {}          # n -> RolloutBuffer (T, n) reused between partial updates
        self._lib, self._h = pol.ctx.lib, pol.ctx.handle
        self._spec, self._rb = C.byref(pol.spec), C.byref(rb.c_struct())

    def _require_kernels(self, pol) -> None:
        require_mlp_kernels(pol, type(self).__name__)     # ph_policy_forward_ragged and the self-play steps read a ph_layout vector

    def get_action(self, obs: th.Tensor, rec_mask: th.Tensor) -> th.Tensor:
        """forward in every env; record the transition where rec_mask is set and the column still has room"""
        pol = self.model.policy
        pol._bind()
        room = self.pos < self.T
        can = (rec_mask.bool() & room).to(th.uint8)
        blocked = rec_mask.bool() & ~room
        es = self.boundary.to(th.float32)
        pol._counter += 1
        nat.check(pol._native_forward_ragged(       # the entry point of the policy's network (ppo.py)
            pol.params.data_ptr(), obs.data_ptr(), None, pol._seed, pol._counter, 0,
            self.actions.data_ptr(), self.values.data_ptr(), self.log_probs.data_ptr(), self._rb, self.pos.data_ptr(),
            can.data_ptr(), es.data_ptr()))
        nat.check(self._lib.ph_ragged_advance(self._h, self._rb, self.pos.data_ptr(), can.data_ptr()))
        canb = can.bool()
        self.boundary = th.where(canb, th.zeros_like(self.boundary), self.boundary)
        self.term = th.where(canb, th.zeros_like(self.term), self.term)
        self.open = th.where(canb, th.ones_like(self.open), th.where(blocked, th.zeros_like(self.open), self.open))
        self.num_timesteps += int(self.E)
        return self.actions

    def update(self, reward: th.Tensor, done: th.Tensor, mask: th.Tensor) -> None:
        """credit `reward` to the last recorded action of the envs in `mask` (whose rows are still open); remember the
        episode boundaries"""
        self.model.policy._bind()
        m = (mask.bool() & self.open.bool())
        m8 = m.to(th.uint8)
        nat.check(self._lib.ph_buffer_add_reward_ragged(self._h, self._rb, self.pos.data_ptr(), reward.data_ptr(),
                                                        m8.data_ptr()))
        d = done.bool()
        self.boundary = (self.boundary.bool() | d).to(th.uint8)
        self.term = (self.term.bool() | (m & d)).to(th.uint8)

    def full(self) -> bool:
        return int((self.pos >= self.T).sum().item()) >= min(self.min_full, self.E)

    def _learn_from_columns(self, cols: th.Tensor) -> None:
        """GAE + PPO update on the full columns `cols` only; the other columns keep filling"""
        from ..ppo import RolloutBuffer
        model, rb = self.model, self.model.rollout_buffer
        pol = model.policy
        n = int(cols.numel())
        sub = self._compact.get(n)
        if sub is None:
            sub = self._compact[n] = RolloutBuffer(rb.buffer_size, rb.observation_space, rb.action_space, rb.device, pol.ctx,
                                                   pol.spec, gae_lambda=rb.gae_lambda, gamma=rb.gamma, n_envs=n)
        pol._bind()
        cols32 = cols.to(th.int32).contiguous()
        nat.check(self._lib.ph_buffer_compact_columns(self._h, self._spec, self._rb, C.byref(sub.c_struct()),
                                                      cols32.data_ptr(), n))
        last_v = self.values.index_select(0, cols).contiguous()
        dones = self.term.to(th.float32).index_select(0, cols).contiguous()
        nat.check(self._lib.ph_gae(self._h, C.byref(sub.c_struct()), last_v.data_ptr(), dones.data_ptr(), rb.gamma,
                                   rb.gae_lambda, int(rb.gae_mode)))
        sub.pos, sub.full = sub.buffer_size, True
        model.rollout_buffer = sub
        try:
            model.train(sync_stats=False)
        finally:
            model.rollout_buffer = rb
        self.pos[cols] = 0
        self.open[cols] = 0
        self.term[cols] = 0
        self.iteration += 1

    def learn_from_buffer(self) -> None:
        model, rb = self.model, self.model.rollout_buffer
        ready = self.pos >= self.T
        if not bool(ready.all().item()):
            self._learn_from_columns(th.nonzero(ready).reshape(-1))
            return
        model.policy._bind()
        dones = self.term.to(th.float32)
        nat.check(self._lib.ph_gae(self._h, self._rb, self.values.data_ptr(), dones.data_ptr(), rb.gamma, rb.gae_lambda,
                                   int(rb.gae_mode)))
        rb.pos, rb.full = rb.buffer_size, True
        model.train(sync_stats=False)
        rb.pos, rb.full = 0, False
        self.pos.zero_()
        self.open.zero_()
        self.term.zero_()
        self.iteration += 1


class TowerRaggedVecOnPolicyAgent(RaggedVecOnPolicyAgent):
    """RaggedVecOnPolicyAgent for `policy_kwargs=dict(net_arch=...)` (ArchActorCriticPolicy): the class is what it accepts, a tower
    whose forward carve fits the CU.  get_action runs the ragged forward the policy names (the tower kernels), and the updates end
    in model.train(), which dispatches to ph_arch_train."""

    def _require_kernels(self, pol) -> None:
        if not is_tower(pol):
            raise nat.NativeError(f"{type(self).__name__}: {type(pol).__name__} is not a net_arch tower policy; use "
                                  "RaggedVecOnPolicyAgent")
        require_tower_lds(pol, type(self).__name__)


class AdapRaggedVecOnPolicyAgent(AdapSeat, RaggedVecOnPolicyAgent):
    """RaggedVecOnPolicyAgent whose model is an ADAP learner over an AdapPolicy (vec.py: AdapSeat): get_action builds the rows of
    the tables asked to move from the game's raw observations and records them; update gives a fresh context to the tables in
    which the agent is paid `done` (the tables of `mask` whose game ended), unless a latent syncer's contexts are read."""

    def __init__(self, model, latent_syncer=None):
        super().__init__(model)
        self._init_adap(latent_syncer)

    def get_action(self, obs: th.Tensor, rec_mask: th.Tensor) -> th.Tensor:
        return super().get_action(self.build_rows(obs, rec_mask), rec_mask)

    def update(self, reward: th.Tensor, done: th.Tensor, mask: th.Tensor) -> None:
        super().update(reward, done, mask)
        self._paid_done(mask.bool() & done.bool())


def ragged_agent_for(model, latent_syncer=None) -> RaggedVecOnPolicyAgent:
    """the ragged vectorised agent class that runs `model`'s policy"""
    if is_adap(model.policy):
        return AdapRaggedVecOnPolicyAgent(model, latent_syncer)
    return (TowerRaggedVecOnPolicyAgent if is_tower(model.policy) else RaggedVecOnPolicyAgent)(model)


def adap_seat(agent):
    """the ph_adap_seat of a seat's agent for the `_adap` step entry point: a pointer, or None (the seat stays on its kernels)"""
    return C.pointer(agent.seat_struct()) if isinstance(agent, AdapSeat) else None


def seat_arch(agent):
    """the ph_arch of a seat's policy for the `_arch` step entry points: a pointer, or None (the 64-wide kernels)"""
    pol = agent.model.policy
    return C.pointer(pol.arch) if is_tower(pol) else None


# ---- a pool of partners at seat 1 (MultiAgentEnv.add_partner_agent / resample_*, multiagentenv.py:92-147) -----------------------
POOL_SEED_SALT = 0x9001C0DE9001C0DE          # the resample stream's own Philox key: pool seed = dice seed ^ this constant
POOL_RESAMPLE_BLOCK = 101                    # Philox block of the resample word (the dice use blocks 0..2, the first mover 100)


def pool_resample(prev: int, n_members: int, rule: str = "robin", word: int = None) -> int:
    """the member that sits at a table's next game.  "robin": the next one in turn (resample_round_robin; applied at the first
    deal too, so every table starts at 1 % K -- SURVEY quirk D-9).  "random": the 32-bit `word` scaled to [0, K) without a
    division -- `word` is word 0 of Philox block POOL_RESAMPLE_BLOCK keyed (pool seed, deal counter, table)."""
    if rule == "robin":
        return (int(prev) + 1) % int(n_members)
    if rule != "random":
        raise ValueError(f"resample must be 'robin' or 'random', not {rule!r}")
    return ((int(word) & 0xFFFFFFFF) * int(n_members)) >> 32


def philox_word0(seed: int, counter: int, rows: np.ndarray, block: int) -> np.ndarray:
    """word 0 of Philox4x32-10 for the counters (row, block, counter lo, counter hi) under the key `seed`: the host statement of
    what the kernels draw (csrc/ph_device.h)"""
    mask = np.uint64(0xFFFFFFFF)
    c0 = np.asarray(rows, np.uint64) & mask
    c1 = np.full_like(c0, int(block) & 0xFFFFFFFF)
    c2 = np.full_like(c0, int(counter) & 0xFFFFFFFF)
    c3 = np.full_like(c0, (int(counter) >> 32) & 0xFFFFFFFF)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & mask, p1 & mask, \
            ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & mask, p0 & mask
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0.astype(np.uint32)


class FrozenVecPartner:
    """A pool member that plays a fixed policy: the E-table form of StaticPolicyAgent (agents.py:54-79).  It samples like any
    forward (its own Philox key and counter), records nothing, and `update` is a no-op."""
    kind = nat.PH_POOL_FROZEN

    def __init__(self, policy):
        self._require_kernels(policy)
        self.policy = policy
        self._out = {}

    def _require_kernels(self, policy) -> None:
        """what this member class accepts (the subclasses override it)"""
        if isinstance(policy, FeedForward32Policy):
            # its ph_bc_layout vector (one shared 32-32 trunk) is a sixth of the 64-64 ph_layout vector the frozen forward reads
            raise nat.NativeError(f"{type(self).__name__}: a FeedForward32Policy (the shared 32-32 trunk of behavioural cloning) is "
                                  "not a 64-64 policy; seat it as ClonedVecPartner(policy)")
        require_mlp_kernels(policy, type(self).__name__)

    def _rows(self, obs: th.Tensor) -> th.Tensor:
        """what the forward reads: the game's observations (the ADAP member builds its rows from them)"""
        return obs

    def _forward(self, obs: th.Tensor, seed: int) -> th.Tensor:
        """every frozen member's move, written once: the output buffers of n rows (allocated at the first call with that n), the
        policy's engine context on the current stream, the next Philox counter, and ONE forward of the member's rows through the
        entry point the policy names for its network (ppo.py: `_native_forward`) under the key `seed` -- no buffer, no mask,
        nothing recorded"""
        pol = self.policy
        n = int(obs.shape[0])
        out = self._out.get(n)
        if out is None:
            out = self._out[n] = (th.zeros((n, pol.layout.A), dtype=th.int32, device=pol.device),
                                  th.zeros(n, dtype=th.float32, device=pol.device), th.zeros(n, dtype=th.float32, device=pol.device))
        pol._bind()
        pol._counter += 1
        nat.check(pol._native_forward(
            pol.params.data_ptr(), self._rows(obs).data_ptr(), n, None, None, None, seed, pol._counter,
            0, out[0].data_ptr(), None, out[1].data_ptr(), out[2].data_ptr(), None, None, None, 0, None, None, 0))
        return out[0]

    def get_action(self, obs: th.Tensor, rec_mask: th.Tensor = None) -> th.Tensor:
        return self._forward(obs, self.policy._seed)

    def update(self, reward, done, mask=None) -> None:
        return None


class TowerFrozenVecPartner(FrozenVecPartner):
    """FrozenVecPartner for `policy_kwargs=dict(net_arch=...)` (ArchActorCriticPolicy): a fixed tower policy as a pool / population
    member.  In the native steps its rows run the tower tiles of the grouped forward (pool_tower_kernel); `get_action` is the walk's
    form, one tower forward over all rows (the base class's, through the policy's entry point) -- the same bits row by row."""

    def _require_kernels(self, policy) -> None:
        who = type(self).__name__
        if not is_tower(policy):
            raise nat.NativeError(f"{who}: {type(policy).__name__} is not a net_arch tower policy; use FrozenVecPartner")
        require_tower_lds(policy, who)


def frozen_partner_for(policy) -> FrozenVecPartner:
    """the frozen member class that plays `policy`"""
    return (TowerFrozenVecPartner if is_tower(policy) else FrozenVecPartner)(policy)


def check_adap_member_policy(policy, who: str) -> None:
    """a frozen ADAP member plays the additive AdapPolicy on its 64-64 towers: AdapPolicyMult and net_arch are refused by name"""
    from ..adap import AdapPolicyMult
    if isinstance(policy, AdapPolicyMult):
        raise nat.NativeError(f"{who}: AdapPolicyMult (ADAP_MULT) has no device-resident form; an ADAP member is the additive AdapPolicy")
    if not is_adap(policy):
        raise nat.NativeError(f"{who}: {type(policy).__name__} is not an AdapPolicy")
    if is_tower(policy) or getattr(policy, "net_arch", None) is not None:
        raise nat.NativeError(f"{who}: an AdapPolicy with policy_kwargs net_arch is not a member: ADAP members play the 64-64 towers")
    require_mlp_kernels(policy, who)
    C_, lay = int(policy.context_size), policy.layout
    if not 1 <= C_ <= nat.ADAP_VEC_MAX_CONTEXT:
        raise nat.NativeError(f"{who}: context_size must be 1..{nat.ADAP_VEC_MAX_CONTEXT}, not {C_}")
    if (lay.D, lay.A, lay.L) != (270 + C_, 2, 19) or policy.spec.obs.kind != nat.PH_SPACE_BOX:
        raise nat.NativeError(f"{who}: the ADAP checkpoint must play on the Liar's Dice spaces (a Box of 270 + context_size = "
                              f"{270 + C_} row components, 2 action components, 19 logits), not (D, A, L) = {(lay.D, lay.A, lay.L)}")


class AdapFrozenVecPartner(FrozenVecPartner):
    """A frozen ADAP checkpoint as a pool / population member: the reference's `FIXED '{"type":"ADAP","location":...,"latent_val":
    [...]}'` partner (trainer.py:140-147: ADAP.load, then policy.set_context) for E tables.  `latent` is
      * an array of context_size floats -- the stated form: one latent serves every table; or
      * the string "sample" -- every table owns a context of this member, drawn on the device with `context_sampler` (the
        checkpoint's own) at every deal of that table, the first included: one member is a whole population of partners.
    The member owns the (E, C) context tensor (`contexts`, allocated by the pool / population it joins).  Its Philox key `seed` --
    the policy's, unless the population had to tell two ADAP members apart -- keys its moves and, under the ADAP salt, its contexts.
    In the native steps its rows run the ADAP tiles of the grouped forward (pool_adap_kernel); `get_action` is the walk's form, the
    row build (`ph_adap_rows`) plus the base class's one forward over all rows -- the same bits row by row."""

    def _require_kernels(self, policy) -> None:
        check_adap_member_policy(policy, type(self).__name__)

    def __init__(self, policy, latent, context_sampler: str = "l2"):
        who = type(self).__name__
        super().__init__(policy)
        self.context_size = int(policy.context_size)
        self.sampled = isinstance(latent, str)
        if self.sampled:
            if latent != "sample":
                raise nat.NativeError(f"{who}: latent is a list of context_size numbers or the string \"sample\", not {latent!r}")
            if context_sampler not in nat.CONTEXT_SAMPLERS:
                raise nat.NativeError(f"{who}: unknown context sampler {context_sampler!r}")
            if context_sampler == "natural_numbers" and self.context_size != 1:
                raise nat.NativeError(f"{who}: context_sampler 'natural_numbers' needs context_size 1")
            self.latent = None
        else:
            self.latent = np.asarray(latent, np.float32).reshape(-1)
            if self.latent.size != self.context_size:
                raise nat.NativeError(f"{who}: the latent holds {self.latent.size} numbers, the checkpoint's context_size is "
                                      f"{self.context_size}")
        self.context_sampler, self.sampler = context_sampler, nat.CONTEXT_SAMPLERS[context_sampler]
        self.seed = int(policy._seed)
        self.env_space = nat.env_space_of(policy.observation_space)
        self.contexts = self.rows = None

    def attach(self, n_envs: int) -> None:
        """the member's contexts of `n_envs` tables: every row the latent (stated), or zeros until the first deal draws (sampled).
        One object, one population: the contexts (and the seed the population gives) are the member's state, so joining a second
        population of the same size shares them with the first, and one of another size is refused."""
        if self.contexts is not None:
            if int(self.contexts.shape[0]) != int(n_envs):
                raise nat.NativeError(f"{type(self).__name__}: this member holds the contexts of {int(self.contexts.shape[0])} tables of "
                                      f"the population it joined; build another AdapFrozenVecPartner for one of {int(n_envs)} tables")
            return
        dev = self.policy.device
        self.contexts = th.zeros((int(n_envs), self.context_size), dtype=th.float32, device=dev)
        if not self.sampled:
            self.contexts.copy_(th.as_tensor(self.latent).to(dev).expand(int(n_envs), -1))
        self.rows = th.zeros((int(n_envs), self.policy.layout.D), dtype=th.float32, device=dev)

    def adap_struct(self) -> "nat.PhPoolAdap":
        """this member for the `_adap` entry points (the policy keeps the spec alive)"""
        s = nat.PhPoolAdap()
        s.spec, s.context_size, s.sampler = C.pointer(self.policy.spec), self.context_size, self.sampler
        s.contexts, s.draw = self.contexts.data_ptr(), int(self.sampled)
        return s

    def redraw(self, flags, counter: int) -> None:
        """the walk's redraw: a fresh context, drawn at `counter`, for the tables flagged in `flags` (uint8) -- the launch of the
        native step under the same mask"""
        if not self.sampled:
            return
        pol = self.policy
        pol._bind()
        nat.check(pol.ctx.lib.ph_adap_context_draw(pol.ctx.handle, self.sampler, self.context_size, self.seed, int(counter),
                                                   nat.ptr(flags), self.contexts.data_ptr(), int(self.contexts.shape[0])))

    def _rows(self, obs: th.Tensor) -> th.Tensor:
        """features(observation) ++ the table's context, built on the device (the shared body has bound the stream)"""
        pol = self.policy
        nat.check(pol.ctx.lib.ph_adap_rows(pol.ctx.handle, C.byref(self.env_space), self.context_size, obs.data_ptr(),
                                           self.contexts.data_ptr(), None, self.rows.data_ptr(), int(obs.shape[0])))
        return self.rows

    def get_action(self, obs: th.Tensor, rec_mask: th.Tensor = None) -> th.Tensor:
        n = int(obs.shape[0])
        if self.contexts is None or int(self.contexts.shape[0]) != n:
            raise nat.NativeError(f"{type(self).__name__}: attach({n}) first: the member owns one context per table")
        return self._forward(obs, self.seed)


def attach_adap_members(members, n_envs: int) -> None:
    """give every ADAP member of a pool / population its contexts of n_envs tables, and a Philox key of its own: two ADAP members
    with one seed -- the same file loaded twice -- would draw one stream of contexts (and of moves), so a later one is moved to
    seed + k * the golden-ratio word until it is free"""
    taken = set()
    for k, m in enumerate(members):
        if not isinstance(m, AdapFrozenVecPartner):
            continue
        seed = int(m.policy._seed)
        while seed in taken:
            seed = (seed + (k + 1) * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
        taken.add(seed)
        m.seed = seed
        m.attach(n_envs)


class ClonedVecPartner:
    """A pool / population member that plays a behavioural clone: a `FeedForward32Policy` (bc.py: one shared 32-32 tanh trunk,
    parameters in ph_bc_layout) on the Liar's Dice spaces -- the "human proxy" partner of the reference's workflow (train, record,
    bctrainer, play the clone).  Like FrozenVecPartner it samples under its own Philox key and counter, records nothing, and `update`
    is a no-op.  In the native steps its rows run the clone tile of the grouped forward; `get_action` is the walk's form, one
    `ph_bc_forward` over all rows -- the same bits row by row.  It does not share FrozenVecPartner's body: the clone's forward
    returns actions only (one output buffer, no value or log-probability planes) and its policy has no `_bind`, so a shared helper
    would branch per caller."""
    kind = nat.PH_POOL_CLONE

    def __init__(self, policy):
        who = type(self).__name__
        if not isinstance(policy, FeedForward32Policy):
            raise nat.NativeError(f"{who}: takes a FeedForward32Policy (bc.reconstruct_policy), not {type(policy).__name__}; a 64-64 "
                                  "ActorCriticPolicy is seated as FrozenVecPartner")
        lay = policy.layout
        if (lay.D, lay.A, lay.L) != (30, 2, 19) or policy.spec.obs.kind == nat.PH_SPACE_BOX:
            raise nat.NativeError(f"{who}: the clone must play on the Liar's Dice spaces (30 one-hot observation components, 2 action "
                                  f"components, 19 logits), not (D, A, L) = {(lay.D, lay.A, lay.L)}")
        self.policy = policy
        self._out = {}

    def get_action(self, obs: th.Tensor, rec_mask: th.Tensor = None) -> th.Tensor:
        pol = self.policy
        n = int(obs.shape[0])
        out = self._out.get(n)
        if out is None:
            out = self._out[n] = th.zeros((n, pol.layout.A), dtype=th.int32, device=pol.device)
        pol.ctx.set_stream(th.cuda.current_stream(pol.device).cuda_stream)
        pol._counter += 1
        nat.check(pol._native_forward(pol.params.data_ptr(), obs.data_ptr(), n, None, None, None, pol._seed, pol._counter, 0,
                                      out.data_ptr(), None, None, None, None))
        return out

    def update(self, reward, done, mask=None) -> None:
        return None


def check_liar_member_policy(policy, who: str, towers: bool = False, adap: bool = False) -> None:
    """a pool / population member's policy runs on the grouped forward's kernels and plays on the Liar's Dice spaces: the 64-64
    layout through `require_mlp_kernels`, a clone's through its BC layout (ClonedVecPartner has checked the one-hot observation);
    `towers`: a net_arch tower whose forward carve fits the CU is taken too (tower tiles of the grouped forward); `adap`: the policy
    is held by an AdapFrozenVecPartner -- the additive AdapPolicy over Box(270 + C) rows (ADAP tiles).  The pool classes state both
    as class attributes (`accepts_towers` / `accepts_adaps`, read in VecLiarPartnerPool._check_member); cross-play, which seats
    every member kind, states them per member."""
    from ..adap import AdapPolicy
    if adap:
        check_adap_member_policy(policy, who)
        return
    if isinstance(policy, AdapPolicy):
        raise nat.NativeError(f"{who}: an AdapPolicy sits in a pool or population only as AdapFrozenVecPartner(policy, latent) -- a "
                              "frozen checkpoint under a latent, in liar_pool_for's pool or a VecLiarCrossPlay; an ADAP learner or "
                              "an ADAP ego does not")
    if towers and is_tower(policy):
        require_tower_lds(policy, who)
    elif not isinstance(policy, FeedForward32Policy):
        require_mlp_kernels(policy, who)
    lay = policy.layout
    if (lay.D, lay.A, lay.L) != (30, 2, 19):
        raise nat.NativeError(f"{who}: every member plays on the Liar's Dice spaces")


class VecLiarDefaultPartner:
    """The scripted pool member: LiarDefaultAgent (envs/liar.py) for E tables, integer-exact (`ph_liar_default_actions`)."""
    kind = nat.PH_POOL_SCRIPTED

    def get_action(self, obs: th.Tensor, rec_mask: th.Tensor, out: th.Tensor, ctx: nat.Context) -> th.Tensor:
        """writes the rule's move into `out` (E, 2) int32 where rec_mask is set; the other rows keep what they hold"""
        nat.check(ctx.lib.ph_liar_default_actions(ctx.handle, obs.data_ptr(), nat.ptr(rec_mask), out.data_ptr(), int(obs.shape[0])))
        return out

    def update(self, reward, done, mask=None) -> None:
        return None


# ---- Liar's Dice resident on the device: self-play, a pool of partners at seat 1, cross-play evaluation ------------------------
class LiarRecording:
    """What `VecLiarStep.recorded` returns: the tables' move streams concatenated in table order -- per table exactly the rows
    `TurnBasedRecorder` (common/wrappers.py) produces, [obs 30 | action 2 | flag].
      transitions    TurnBasedTransitions on the host (write_transition gives the reference's .npy)
      obs/acts/flags (N, 30) / (N, 2) / (N,) float32 device tensors, views of `rows` (N, 33)
      member         (N,) int32 device: who moved (cross-play: the population index; the pool: the member at seat 1; otherwise 0)
      table_offsets  (E + 1,) int64 numpy: table e's rows are table_offsets[e]:table_offsets[e + 1]
      dropped        (E,) int64 numpy: moves of table e that found its log full
    It can be handed to `BC.set_expert_data_loader` as it is (device obs / acts)."""

    def __init__(self, rows: th.Tensor, member: th.Tensor, table_offsets: np.ndarray, dropped: np.ndarray):
        from ..common.trajsaver import TurnBasedTransitions
        self.rows, self.member = rows, member
        self.obs, self.acts, self.flags = rows[:, :30], rows[:, 30:32], rows[:, 32]
        self.table_offsets, self.dropped = np.asarray(table_offsets, np.int64), np.asarray(dropped, np.int64)
        host = rows.cpu().numpy()
        self.transitions = TurnBasedTransitions(host[:, :30], host[:, 30:32], host[:, 32])

    def __len__(self) -> int:
        return int(self.rows.shape[0])


RECORD_SEATS = {None: -1, 0: 0, 1: 1}


def write_recording(env, file) -> "LiarRecording":
    """`--record FILE` of the device-resident CLIs: the tables' streams concatenated in table order, in the reference's .npy
    format (TurnBasedTransitions.write_transition); dropped moves are reported, not fatal"""
    rec = env.recorded()
    rec.transitions.write_transition(file)
    lost = int(rec.dropped.sum())
    if lost:
        print(f"WARNING: --record: {lost} moves of {int((rec.dropped > 0).sum())} tables did not fit the move log and were dropped")
    print(f"Recorded {len(rec)} moves of {env.E} tables to {file}")
    return rec


def export_recording(rows, counts, seat=None):
    """The export in plain numpy (what `ph_liar_record_export` does on the device): rows (E, cap, 33), counts (E,) rows logged per
    table; seat None / 0 / 1 selects every row / flag % 2 == seat.  -> (dense (N, 33), offsets (E + 1,) int64)"""
    rows, counts = np.asarray(rows), np.asarray(counts, np.int64)
    E, cap = rows.shape[0], rows.shape[1]
    counts = np.clip(counts, 0, cap)
    picked = []
    for e in range(E):
        r = rows[e, :counts[e]]
        picked.append(r if seat is None else r[r[:, 32].astype(np.int64) % 2 == int(seat)])
    offsets = np.zeros(E + 1, np.int64)
    offsets[1:] = np.cumsum([len(r) for r in picked])
    dense = np.concatenate(picked, axis=0) if E else np.zeros((0, rows.shape[2]), rows.dtype)
    return dense.reshape(-1, rows.shape[2]), offsets


class VecLiarStep:
    """What the three device-resident Liar's Dice drivers share -- VecLiarSelfPlay, VecLiarPartnerPool and (envs/crossplay.py)
    VecLiarCrossPlay.  One vectorised step is one protocol:

        seat-0 forward | after_ego | seat-1 forward (reply) | after_reply (ends of games, re-deal) | seat-1 forward (openers) |
        after_opening

    native=True runs it as ONE engine call per step; native=False walks it with the per-call entry points and torch masks -- the
    readable statement of the protocol, written once here (`_walk` and `_deal`), and the bit-exact cross-check of the native step.
    The base owns the game (`env`), `ego_first`, `obs_ego` / `obs_alt`, the constant masks, the native step's scratch and the part
    of its description every mode fills the same way.  A mode supplies
      * `_contexts()`: the engine contexts its calls run on;
      * `_counters(c)`: the Philox counters of step c's three forwards;
      * `_seat_act(seat, obs, mask, counter)`: who moves at a seat under a mask and a counter;
      * `_live()`: the tables that take part (None = all);
      * `_credit(reward, done, replied)` / `_acted(mask)`: seat 1's book (training);
      * `_on_deal(rm, c)`: what happens at a deal besides the dice;
      * `_game_end(reward, done)`: what the end of a game does -> the tables to deal again;
      * `_build_native()` / `_native_call()`: its description and entry point."""

    def _init_game(self, n_envs: int, ctx: nat.Context, dev, seed: int, probegostart: float, native: bool) -> None:
        self.E, self.dev, self.native = int(n_envs), dev, bool(native)
        self.env = VecLiarsDice(self.E, ctx, dev)
        self.seed, self.probegostart = int(seed), float(probegostart)
        u8 = lambda v=0: th.full((self.E,), v, dtype=th.uint8, device=dev)  # noqa: E731
        self.ego_first = u8()
        self.obs_ego = th.zeros((self.E, 30), dtype=th.float32, device=dev)
        self.obs_alt = th.zeros((self.E, 30), dtype=th.float32, device=dev)
        self.ones8, self.zeros8 = u8(1), u8(0)
        self.steps_done = 0
        self.recording = False
        self._ctxs = tuple(dict.fromkeys(self._contexts()))     # each engine context once: `_bind` runs in front of every step
        attach_adap_members(getattr(self, "members", ()), self.E)

    def _first_deal(self) -> None:
        """the constructor's deal: step 0's re-deal half for every table"""
        if self.native:
            self._build_native()
            self._done.fill_(1)
            self._native_call(0, deal_only=True)
        else:
            self._deal(self.ones8, 0)

    def _bind(self):
        stream = th.cuda.current_stream(self.dev).cuda_stream
        for ctx in self._ctxs:
            ctx.set_stream(stream)

    @staticmethod
    def _policy_of(agent):
        """the policy a pool / population member plays with (None: the scripted player)"""
        if isinstance(agent, VecLiarDefaultPartner):
            return None
        return agent.policy if isinstance(agent, (FrozenVecPartner, ClonedVecPartner)) else agent.model.policy

    # -- the engine-side step: what every description holds -------------------------------------------------------------------------
    def _fill_game(self, s, book: bool):
        """the native step's scratch, and the game block of its description `s` (the same-named fields of PhLiarSelfPlay /
        PhLiarPool / PhLiarXplay); `book`: seat 1 records, so the forwards need `can` / `es_alt`"""
        E, dev, env = self.E, self.dev, self.env
        f32 = lambda *shape: th.zeros(shape, dtype=th.float32, device=dev)  # noqa: E731
        u8 = lambda: th.zeros(E, dtype=th.uint8, device=dev)               # noqa: E731
        self._obs_next, self._rew1, self._rew2 = f32(E, 30), f32(E, 2), f32(E, 2)
        self._done1, self._done2, self._running = u8(), u8(), u8()
        self._alt_opens, self._ego_opens, self._done = u8(), u8(), u8()
        s.n, s.dice_seed, s.probegostart = E, self.seed, self.probegostart
        s.hands, s.history, s.nmoves, s.ego_first = (t.data_ptr() for t in (env.hands, env.history, env.nmoves, self.ego_first))
        s.obs_ego, s.obs_alt = self.obs_ego.data_ptr(), self.obs_alt.data_ptr()
        for name in ("obs_next", "rew1", "rew2", "done1", "done2", "running", "alt_opens", "ego_opens", "done"):
            setattr(s, name, getattr(self, "_" + name).data_ptr())
        if book:
            self._es_alt, self._can = f32(E), u8()
            s.es_alt, s.can = self._es_alt.data_ptr(), self._can.data_ptr()
        return s

    def _member_array(self, members):
        """the PhPoolMember array of a pool / population (kept alive with the learners' buffer records in `_member_rbc`)"""
        self._member_rbc = []
        arr = (nat.PhPoolMember * len(members))()
        for c, m in zip(arr, members):
            learner = isinstance(m, RaggedVecOnPolicyAgent)
            c.kind = nat.PH_POOL_LEARNER if learner else m.kind
            p = self._policy_of(m)
            if p is None:
                continue
            c.params, c.seed = p.params.data_ptr(), p._seed       # (a clone: its ph_bc_layout vector and key, nothing else)
            if isinstance(m, AdapFrozenVecPartner):
                c.seed = m.seed                                   # (its own key where two ADAP members loaded one file)
            if learner:
                rbc = m.model.rollout_buffer.c_struct()
                self._member_rbc.append(rbc)
                c.rb = C.pointer(rbc)
                c.pos, c.boundary, c.term, c.open = (t.data_ptr() for t in (m.pos, m.boundary, m.term, m.open))
                c.values, c.log_probs = m.values.data_ptr(), m.log_probs.data_ptr()
        self._member_arr = arr
        return arr

    def _member_arrays(self, members, towers: bool, adaps: bool, ego=None):
        """everything the one native call of a pool / population hands over beside its description: the member array (returned,
        and kept in `_member_arr`), `_member_arch_arr` where `towers`, `_member_adap_arr` where `adaps`, and `_ego_arch`, the
        ph_arch of a tower ego (the pool's `ego`; cross-play has none).  What is not asked for is None: the step is handed NULL
        there and keeps every member on the 64-wide kernels, which is what the narrow entry points forward (csrc/ph_abi.hip)."""
        arr = self._member_array(members)
        self._ego_arch = seat_arch(ego) if towers and ego is not None else None
        self._member_arch_arr = self._member_adap_arr = None
        if towers:
            self._member_archs(members)          # (stores `_member_arch_arr`)
        if adaps:
            self._member_adaps(members)          # (stores `_member_adap_arr` and `_member_adap_keep`)
        return arr

    def _member_archs(self, members):
        """the `member_archs` array of the `_arch` steps beside `_member_array`'s: entry k points at member k's ph_arch where it
        plays a tower, else NULL (the policies keep the archs alive)"""
        archs = (C.POINTER(nat.PhArch) * len(members))()
        for k, m in enumerate(members):
            p = self._policy_of(m)
            if p is not None and is_tower(p):
                archs[k] = C.pointer(p.arch)
        self._member_arch_arr = archs
        return archs

    def _member_adaps(self, members):
        """the `member_adaps` array of the `_adap` steps: entry k points at member k's ph_pool_adap where it is an
        AdapFrozenVecPartner, else NULL (`_member_adap_keep` keeps the structs alive)"""
        adaps = (C.POINTER(nat.PhPoolAdap) * len(members))()
        self._member_adap_keep = []
        for k, m in enumerate(members):
            if isinstance(m, AdapFrozenVecPartner):
                self._member_adap_keep.append(m.adap_struct())
                adaps[k] = C.pointer(self._member_adap_keep[-1])
        self._member_adap_arr = adaps
        return adaps

    # -- the move log (csrc/ph_record.h): TurnBasedRecorder's rows of every table, filled inside the step ----------------------------
    def start_recording(self, max_moves_per_table: int) -> None:
        """Log every move from the next step on, at most `max_moves_per_table` rows per table (a step logs up to three moves per
        table; later moves of a full table are dropped and counted).  native=True: the log lives on the device and the engine's
        step fills it (`ph_liar_record_attach` on the game's context) with no host work; native=False: the walk appends to
        per-table host lists at the same three points.  The constructors' `record=` starts it in front of the first deal, so a
        table's log begins with that game's opening, as the reference recorder's does."""
        cap = int(max_moves_per_table)
        if cap < 1:
            raise nat.NativeError(f"{type(self).__name__}.start_recording: max_moves_per_table must be at least 1, not {cap}")
        if self.recording:
            raise nat.NativeError(f"{type(self).__name__}.start_recording: already recording (stop_recording first)")
        E, dev = self.E, self.dev
        self._rec_cap = cap
        if self.native:
            i32 = lambda shape, v=0: th.full(shape, v, dtype=th.int32, device=dev)  # noqa: E731
            self._rec_rows, self._rec_member = self._record_alloc(cap)
            self._rec_count, self._rec_count_alt, self._rec_dropped, self._rec_pending = i32((E,)), i32((E,)), i32((E,)), i32((E,), -1)
            self._rec_desc = self._record_desc()
            self._bind()
            ctx = self.env.ctx
            # the context keeps the log's addresses: one recording environment per context, detached before its log is freed
            owner = getattr(ctx, "_liar_recorder", None)
            if owner is not None and owner() is not None and owner() is not self and owner().recording:
                raise nat.NativeError(f"{type(self).__name__}.start_recording: another environment records on this engine context")
            nat.check(ctx.lib.ph_liar_record_attach(ctx.handle, C.byref(self._rec_desc)))
            ctx._liar_recorder = weakref.ref(self)
        else:
            self._rec_lists = [[] for _ in range(E)]             # per table: (row (33,), member)
            self._rec_lost = np.zeros(E, np.int64)
        self.recording = True

    def _record_alloc(self, cap: int):
        """the log's storage: rows (E, cap, 33) float32 and member (E, cap) int32, zeroed"""
        return (th.zeros((self.E, cap, nat.RECORD_ROW), dtype=th.float32, device=self.dev),
                th.zeros((self.E, cap), dtype=th.int32, device=self.dev))

    def _record_desc(self) -> "nat.PhLiarRecord":
        r = nat.PhLiarRecord()
        r.n, r.cap = self.E, self._rec_cap
        r.rows, r.member = self._rec_rows.data_ptr(), self._rec_member.data_ptr()
        r.count, r.count_alt = self._rec_count.data_ptr(), self._rec_count_alt.data_ptr()
        r.dropped, r.pending = self._rec_dropped.data_ptr(), self._rec_pending.data_ptr()
        return r

    def stop_recording(self) -> None:
        """stop logging; what was logged stays readable through `recorded`"""
        if not self.recording:
            return
        if self.native:
            self._bind()
            ctx = self.env.ctx
            nat.check(ctx.lib.ph_liar_record_attach(ctx.handle, None))
        self.recording = False

    def __del__(self):  # pragma: no cover
        try:                                  # the engine context may outlive this object: it must not keep the log's addresses
            if getattr(self, "recording", False) and getattr(self, "native", False):
                self.stop_recording()
        except Exception:  # noqa: BLE001
            pass

    def recorded(self, seat=None) -> LiarRecording:
        """the log so far: every row (seat=None), seat 0's (0) or seat 1's (1) -- see LiarRecording (synchronises)"""
        if seat not in RECORD_SEATS:
            raise nat.NativeError(f"{type(self).__name__}.recorded: seat must be None, 0 or 1, not {seat!r}")
        if not hasattr(self, "_rec_cap"):
            raise nat.NativeError(f"{type(self).__name__}.recorded: nothing was recorded (start_recording first)")
        E, dev = self.E, self.dev
        if not self.native:
            picked = [[(r, m) for r, m in t if seat is None or int(r[32]) % 2 == seat] for t in self._rec_lists]
            offsets = np.zeros(E + 1, np.int64)
            offsets[1:] = np.cumsum([len(t) for t in picked])
            flat = [rm for t in picked for rm in t]
            rows = np.stack([r for r, _ in flat]).astype(np.float32) if flat else np.zeros((0, nat.RECORD_ROW), np.float32)
            member = np.asarray([m for _, m in flat], np.int32)
            return LiarRecording(th.as_tensor(rows).to(dev), th.as_tensor(member).to(dev), offsets, self._rec_lost.copy())
        self._bind()
        ctx, desc = self.env.ctx, C.byref(self._rec_desc)
        offsets = th.zeros(E + 1, dtype=th.int64, device=dev)
        nat.check(ctx.lib.ph_liar_record_export(ctx.handle, desc, RECORD_SEATS[seat], offsets.data_ptr(), None, None, 0))
        n = int(offsets[-1].item())
        rows = th.zeros((n, nat.RECORD_ROW), dtype=th.float32, device=dev)
        member = th.zeros(n, dtype=th.int32, device=dev)
        if n:
            nat.check(ctx.lib.ph_liar_record_export(ctx.handle, desc, RECORD_SEATS[seat], offsets.data_ptr(), rows.data_ptr(),
                                                    member.data_ptr(), n))
        return LiarRecording(rows, member, offsets.cpu().numpy(), self._rec_dropped.cpu().numpy())

    def _seat_member(self, seat: int):
        """the walk's member column: who sits at `seat` of every table (None: member 0)"""
        return None

    def _log_moves(self, mask, obs: th.Tensor, actions: th.Tensor, flags, seat: int) -> None:
        """the walk's recorder: one row [obs | action | flag] for every table in `mask` (None = all), appended to that table's
        host list -- or dropped and counted where the list is full"""
        E = self.E
        on = np.ones(E, bool) if mask is None else mask.bool().cpu().numpy()
        obs_h, act_h = obs.cpu().numpy(), actions.cpu().numpy().reshape(E, 2)
        flag_h = np.broadcast_to(flags.cpu().numpy() if isinstance(flags, th.Tensor) else np.asarray(flags), (E,))
        who = self._seat_member(seat)
        who_h = np.zeros(E, np.int32) if who is None else who.cpu().numpy()
        for e in np.nonzero(on)[0]:
            if len(self._rec_lists[e]) >= self._rec_cap:
                self._rec_lost[e] += 1
                continue
            row = np.concatenate([obs_h[e], act_h[e], [flag_h[e]]]).astype(np.float32)
            self._rec_lists[e].append((row, int(who_h[e])))

    # -- the walk: the per-call entry points with torch masks ------------------------------------------------------------------------
    def _members_act(self, which, ids: th.Tensor, obs: th.Tensor, mask: th.Tensor, counter: int, out: th.Tensor) -> th.Tensor:
        """the forward of every member in `which` with Philox counter `counter`; member k's move lands in the tables of `mask`
        where ids == k"""
        for k in which:
            m = self.members[k]
            mk = (mask.bool() & (ids == k)).to(th.uint8)
            if isinstance(m, VecLiarDefaultPartner):
                m.get_action(obs, mk, out, self.env.ctx)
                continue
            self._policy_of(m)._counter = counter - 1
            a = m.get_action(obs, mk)
            out.copy_(th.where(mk.bool()[:, None], a, out))
        return out

    def _live(self):
        return None

    def _credit(self, reward: th.Tensor, done: th.Tensor, replied) -> None:
        return None

    def _acted(self, mask: th.Tensor) -> None:
        return None

    def _on_deal(self, rm: th.Tensor, c: int) -> None:
        return None

    def _deal(self, reset_mask: th.Tensor, c: int) -> None:
        """deal the tables in reset_mask; where seat 1 opens, it moves once; seat 0's observation of every fresh table"""
        env, lib, h = self.env, self.env.ctx.lib, self.env.ctx.handle
        game = (env.hands.data_ptr(), env.history.data_ptr(), env.nmoves.data_ptr())
        self._bind()
        nat.check(lib.ph_liar_reset(h, *game, reset_mask.data_ptr(), self.ego_first.data_ptr(), self.seed, int(c), self.probegostart,
                                    self.E))
        rm = reset_mask.bool()
        self._on_deal(rm, c)
        for m in getattr(self, "members", ()):                      # a sampling ADAP member: a fresh context in every table dealt
            if isinstance(m, AdapFrozenVecPartner):
                m.redraw(reset_mask, c)
        alt_opens = (rm & ~self.ego_first.bool()).to(th.uint8)
        nat.check(lib.ph_liar_obs(h, *game, self.zeros8.data_ptr(), alt_opens.data_ptr(), self.obs_alt.data_ptr(), self.E))
        a_alt = self._seat_act(1, self.obs_alt, alt_opens, self._counters(c)[2])
        if self.recording:                                          # an opening never ends a game: ALT_NOT_DONE
            self._log_moves(alt_opens, self.obs_alt, a_alt, 1, 1)
        self._acted(alt_opens)
        env.player_step(a_alt, self.zeros8, alt_opens)              # obs_next = seat 0's observation in those tables
        self.obs_ego.copy_(th.where(alt_opens.bool()[:, None], env.obs_next, self.obs_ego))
        ego_opens = (rm & self.ego_first.bool()).to(th.uint8)
        nat.check(lib.ph_liar_obs(h, *game, self.ones8.data_ptr(), ego_opens.data_ptr(), self.obs_ego.data_ptr(), self.E))

    def _walk(self, c: int) -> th.Tensor:
        """one MultiAgentEnv.step of every live table -> (E,) bool: tables whose game ended in this step"""
        env = self.env
        self._bind()
        k = self._counters(c)
        live = self._live()
        a_ego = self._seat_act(0, self.obs_ego, live, k[0])                    # every live table is at seat 0's turn
        obs_alt, rew1, done1 = env.player_step(a_ego, self.ones8, live)
        rew1, done1 = rew1.clone(), done1.bool() if live is None else done1.bool() & live.bool()
        running = ~done1 if live is None else live.bool() & ~done1
        running8 = running.to(th.uint8)
        if self.recording:                                                     # EGO_NOT_DONE / EGO_DONE
            self._log_moves(live, self.obs_ego, a_ego, 2 * done1.to(th.int32), 0)
            obs_alt = obs_alt.clone()                                          # the reply's step writes the same buffer
        # a seat 1 that already acted this game is credited this transition (multiagentenv.py:163-170)
        self._credit(rew1[:, 1].contiguous(), done1.to(th.uint8), None)
        a_alt = self._seat_act(1, obs_alt, running8, k[1])                     # seat 1 replies where the game goes on
        self._acted(running8)
        obs_ego, rew2, done2 = env.player_step(a_alt, self.zeros8, running8)
        rew2 = th.where(running[:, None], rew2, th.zeros_like(rew2))
        done2 = done2.bool() & running
        if self.recording:                                                     # ALT_NOT_DONE / ALT_DONE
            self._log_moves(running8, obs_alt, a_alt, 1 + 2 * done2.to(th.int32), 1)
        self._credit(rew2[:, 1].contiguous(), done2.to(th.uint8), running8)
        done = done1 | done2
        self.obs_ego.copy_(th.where((running & ~done2)[:, None], obs_ego, self.obs_ego))
        # seat 0 collects both transitions of the step; the last done wins (agents.py:44-47, multiagentenv.py:201-202)
        self._deal(self._game_end((rew1[:, 0] + rew2[:, 0]).contiguous(), done), c)
        return done


class VecLiarTraining(VecLiarStep):
    """The training modes: a rectangular PPO ego (VecOnPolicyAgent) at seat 0 of every table, a book at seat 1 (`alt_acted`: seat 1
    has moved in the table's current game -- the partner's should_update), and the end of a game adds to the ego's reward row,
    flags its next episode start and counts `episodes`.  RNG counters of step c: ego forward c, seat-1 forwards 2c and 2c + 1,
    dice c."""

    def _init_training(self, n_envs: int, ego: VecOnPolicyAgent, seed: int, probegostart: float, native: bool) -> None:
        self.ego = ego
        pol = ego.model.policy
        self._init_game(n_envs, pol.ctx, pol.device, seed, probegostart, native)
        self.alt_acted = th.zeros(self.E, dtype=th.uint8, device=self.dev)
        self._episodes_dev = th.zeros(1, dtype=th.int64, device=self.dev)
        self.row0_counter = 1      # the step counter of row 0 of the ego's buffer: what EpisodeStats replays the pool's resamples from

    @property
    def episodes(self) -> int:
        return int(self._episodes_dev.item())

    def _counters(self, c: int):
        return c, 2 * c, 2 * c + 1

    def _fill_training(self, s):
        """the game and ego blocks of a PhLiarSelfPlay / PhLiarPool"""
        ego, pe = self.ego, self.ego.model.policy
        self._fill_game(s, book=True)
        ego._last_episode_starts = ego._last_episode_starts.clone()    # updated in place by the step from here on
        self._ego_rbc = ego.model.rollout_buffer.c_struct()
        s.spec, s.ego_params, s.ego_rb, s.ego_seed = C.pointer(pe.spec), pe.params.data_ptr(), C.pointer(self._ego_rbc), pe._seed
        s.ego_actions, s.ego_values, s.ego_log_probs = ego.actions.data_ptr(), ego.values.data_ptr(), ego.log_probs.data_ptr()
        s.ego_episode_start, s.alt_acted = ego._last_episode_starts.data_ptr(), self.alt_acted.data_ptr()
        s.episodes = self._episodes_dev.data_ptr()
        return s

    def _ego_act(self, counter: int) -> th.Tensor:
        self.ego.model.policy._counter = counter - 1
        return self.ego.get_action(self.obs_ego)

    def _acted(self, mask: th.Tensor) -> None:
        self.alt_acted.copy_((self.alt_acted.bool() | mask.bool()).to(th.uint8))

    def _on_deal(self, rm: th.Tensor, c: int) -> None:
        self.alt_acted.copy_(th.where(rm, self.zeros8, self.alt_acted))

    def _game_end(self, reward: th.Tensor, done: th.Tensor) -> th.Tensor:
        self.ego.update(reward, done.to(th.float32))
        self.ego.flush_rewards()
        done8 = done.to(th.uint8)
        self._episodes_dev += done8.sum()
        return done8

    # -- one vectorised MultiAgentEnv.step ---------------------------------------------------------------------------------
    def step(self):
        """-> (E,) uint8 device tensor: tables whose game ended in this step"""
        ego = self.ego
        self.steps_done += 1
        c = self.steps_done
        model, rb = ego.model, ego.model.rollout_buffer
        row0 = rb.pos == 0 or ego.n_steps >= model.n_steps       # this step fills row 0 (behind the roll-over, where one is due)
        if not self.native:
            done = self._walk(c).to(th.uint8)
            if row0:
                self.row0_counter = c
            return done
        if ego.n_steps >= model.n_steps:
            ego.learn_from_buffer()
        if row0:
            self.row0_counter = c                                # behind the roll-over: its scan replayed the rollout before
        self._native_call(c)
        rb.pos += 1
        rb.full = rb.pos == rb.buffer_size
        ego.n_steps += 1
        ego.num_timesteps += self.E
        for m in self.learners:
            m.num_timesteps += self.E
        return self._done


class VecLiarSelfPlay(VecLiarTraining):
    """`trainer.py LiarsDice-v0 PPO PPO` (BASELINE config 2) with n_envs tables resident on the device.

    One vectorised step is one `MultiAgentEnv.step` of every table from the ego's point of view (multiagentenv.py:
    172-215): the ego moves, the partner replies in the tables that are still running, finished tables are re-dealt and --
    where the partner opens the new game -- the partner moves once more, so every table is back at the ego's turn.
    The ego is a rectangular VecOnPolicyAgent (one row per table per step); the partner is ragged.

    native=True (default): the whole step is ONE engine call (`ph_liar_selfplay_step`: the three policy forwards and ONE
    book-keeping launch after each -- a table's state is touched by its own lane only -- every mask stays on the device, no host
    synchronisation).  native=False walks the same step with the per-call entry points and torch masks (VecLiarStep)."""

    def __init__(self, n_envs: int, ego: VecOnPolicyAgent, alt: RaggedVecOnPolicyAgent, seed: int = 0,
                 probegostart: float = 0.5, native: bool = True, record: int = 0):
        self.alt, self.learners, self.counter = alt, [alt], 0
        self._init_training(n_envs, ego, seed, probegostart, native)
        import os
        self.persistent = self.native and os.environ.get("LIAR_PERSISTENT", "1") != "0"   # whole rollouts as one launch
        self._archs = (seat_arch(ego), seat_arch(alt))        # a tower in either seat: the `_arch` step, launch by launch
        self.towers = any(a is not None for a in self._archs)
        if self.towers:
            self.persistent = False                           # ph_liar_selfplay_rollout is built around the 64-wide blocks
        # an ADAP learner in either seat: the `_adap` step, launch by launch (rows built and contexts redrawn inside it)
        self._adap = (adap_seat(ego), adap_seat(alt))
        self.adap = any(a is not None for a in self._adap)
        if self.adap:
            self.persistent = False
            if self.towers:
                raise nat.NativeError("VecLiarSelfPlay: an ADAP seat plays against PPO's 64-64 MlpPolicy or another ADAP learner, "
                                      "not against a net_arch tower")
            if record:
                raise nat.NativeError("VecLiarSelfPlay: the move log is not kept with an ADAP seat (record=0)")
        if record:
            self.start_recording(record)                      # in front of the first deal: its openings are the logs' first rows
        self._first_deal()

    @property
    def persistent(self) -> bool:
        """whole rollouts as one launch -- never while recording: the one-launch rollout does not fill the move log"""
        return self._persistent and not self.recording

    @persistent.setter
    def persistent(self, value) -> None:
        self._persistent = bool(value)

    def _contexts(self):
        return self.env.ctx, self.ego.model.policy.ctx, self.alt.model.policy.ctx

    def _build_native(self) -> None:
        alt, pa = self.alt, self.alt.model.policy
        s = self._fill_training(nat.PhLiarSelfPlay())
        self._alt_rbc = alt.model.rollout_buffer.c_struct()
        s.alt_params, s.alt_rb, s.alt_actions, s.alt_seed = pa.params.data_ptr(), C.pointer(self._alt_rbc), alt.actions.data_ptr(), pa._seed
        s.alt_values, s.alt_log_probs, s.alt_pos = alt.values.data_ptr(), alt.log_probs.data_ptr(), alt.pos.data_ptr()
        s.alt_boundary, s.alt_term, s.alt_open = alt.boundary.data_ptr(), alt.term.data_ptr(), alt.open.data_ptr()
        s.zeros8, s.ones8 = self.zeros8.data_ptr(), self.ones8.data_ptr()
        if self._adap[0] is not None and self._adap[1] is None:
            s.spec = C.pointer(pa.spec)                       # the description's spec is the one of the seat(s) without a spec of their own
        self._desc = s

    def _native_call(self, counter: int, deal_only: bool = False, ego_pos: int = -1) -> None:
        self._bind()
        ctx, rb = self.env.ctx, self.ego.model.rollout_buffer
        pos = int(rb.pos if ego_pos < 0 else ego_pos)
        if self.adap:
            nat.check(ctx.lib.ph_liar_selfplay_step_adap(ctx.handle, C.byref(self._desc), self._adap[0], self._adap[1], pos,
                                                         int(counter), int(deal_only)))
            return
        # two forms because the signatures differ (seats / archs); no tower in either seat: (None, None), the plain step
        nat.check(ctx.lib.ph_liar_selfplay_step_arch(ctx.handle, C.byref(self._desc), self._archs[0], self._archs[1], pos,
                                                     int(counter), int(deal_only)))

    def rollout_persistent(self, n_steps: int, first_counter: int, ego_pos: int = 0) -> None:
        """n_steps vectorised steps as ONE persistent launch (`ph_liar_selfplay_rollout`: one workgroup owns 16 tables for the
        whole rollout; bitwise the result of n_steps `_native_call`s with counters first_counter, first_counter + 1, ...)"""
        if self.towers:
            raise nat.NativeError("VecLiarSelfPlay.rollout_persistent: a net_arch tower policy does not run on the fused MLP kernels "
                                  "of the persistent rollout; use step()")
        if self.adap:
            raise nat.NativeError("VecLiarSelfPlay.rollout_persistent: an ADAP seat's rows and contexts are not part of the "
                                  "persistent rollout; use step()")
        self._bind()
        ctx = self.env.ctx
        nat.check(ctx.lib.ph_liar_selfplay_rollout(ctx.handle, C.byref(self._desc), int(ego_pos), int(n_steps),
                                                   int(first_counter)))

    # -- the walk's hooks -------------------------------------------------------------------------------------------------------------
    def _walk(self, c: int) -> th.Tensor:
        for agent in (self.ego, self.alt):
            if isinstance(agent, AdapSeat):
                agent.draw_counter = c                        # an ADAP seat redraws at the step's counter, as the dice are dealt
        return super()._walk(c)

    def _seat_act(self, seat: int, obs: th.Tensor, mask, counter: int) -> th.Tensor:
        if seat == 0:
            return self._ego_act(counter)
        self.alt.model.policy._counter = counter - 1
        return self.alt.get_action(obs, mask)

    def _credit(self, reward: th.Tensor, done: th.Tensor, replied) -> None:
        self.alt.update(reward, done, self.alt_acted if replied is None else replied)

    def rollout_and_learn(self, n_steps: int) -> None:
        """n_steps vectorised steps, the ego's update, and the partner's whenever all its columns are full"""
        ego, rb = self.ego, self.ego.model.rollout_buffer
        if self.native and self.persistent and rb.pos == 0 and n_steps == rb.buffer_size and ego.n_steps == 0:
            self.rollout_persistent(n_steps, self.steps_done + 1, 0)
            self.steps_done += n_steps
            rb.pos, rb.full = n_steps, True
            ego.n_steps += n_steps
            ego.num_timesteps += n_steps * self.E
            self.alt.num_timesteps += n_steps * self.E
        else:
            for _ in range(n_steps):
                self.step()
        self.ego.learn_from_buffer()
        if self.alt.full():
            self.alt.learn_from_buffer()


class VecLiarPartnerPool(VecLiarTraining):
    """`trainer.py LiarsDice-v0 PPO <alt>+ --n-envs E`: n_envs Liar's Dice tables resident on the device, seat 1 of every table
    held by one of K <= 8 pool members -- learners (RaggedVecOnPolicyAgent), frozen policies (FrozenVecPartner), behavioural
    clones (ClonedVecPartner) or the scripted player (VecLiarDefaultPartner).  `partnerid[e]` names table e's member; it is resampled at that table's own re-deal
    (`pool_resample`), the first deal included.

    Per table the callbacks are VecLiarSelfPlay's, with every partner-side mask ANDed with `partnerid == k`: credit goes to the
    member that has acted in this game (`alt_acted`, cleared at the deal), the member that opens a new game is the newly sampled
    one, and a member's `boundary` flag of a table survives the games it sits out, so its next recorded row there starts an
    episode.  RNG counters of step c: ego forward c, member forwards 2c and 2c + 1 (each member under its own seed), dice c,
    resample c.  `rollout_and_learn` trains the ego, then every learner whose `full()` holds; a learner's `min_full` becomes
    max(1, E // K) unless the caller lowered it already.

    native=True: one `ph_liar_pool_step` per vectorised step -- a bucket pass and ONE grouped forward per partner move whatever
    K is, no host synchronisation.  native=False: the readable walk (VecLiarStep) -- per-member get_action / update calls with
    torch masks (K full forwards per partner move), the per-call entry points only, the same counters; bitwise the native step."""
    # what the member check takes beside the plain kinds -- and so which arrays the native call is handed beside the member array
    accepts_towers = False      # net_arch towers as ego / members (TowerVecLiarPartnerPool)
    accepts_adaps = False       # AdapFrozenVecPartner members (AdapVecLiarPartnerPool)

    def __init__(self, n_envs: int, ego: VecOnPolicyAgent, members, seed: int = 0, probegostart: float = 0.5,
                 resample: str = "robin", native: bool = True, record: int = 0):
        members = list(members)
        if not 1 <= len(members) <= nat.PH_MAX_POOL:
            raise nat.NativeError(f"VecLiarPartnerPool: the pool holds 1..{nat.PH_MAX_POOL} members, not {len(members)}")
        if resample not in nat.POOL_RESAMPLE:
            raise nat.NativeError(f"VecLiarPartnerPool: resample must be one of {sorted(nat.POOL_RESAMPLE)}, not {resample!r}")
        self.members, self.resample, self.K = members, resample, len(members)
        for who in [ego] + members:
            p = self._policy_of(who)
            if p is None:
                continue
            if isinstance(p, FeedForward32Policy) and not isinstance(who, ClonedVecPartner):
                raise nat.NativeError("VecLiarPartnerPool: a FeedForward32Policy is seated as ClonedVecPartner(policy)")
            self._check_member(p, who)
        self.learners = [m for m in members if isinstance(m, RaggedVecOnPolicyAgent)]
        for m in self.learners:
            if m.E != n_envs:
                raise nat.NativeError("VecLiarPartnerPool: a learner's rollout buffer must have n_envs columns")
            if m.min_full >= m.E:
                m.min_full = max(1, n_envs // self.K)
        self._init_training(n_envs, ego, seed, probegostart, native)
        self.pool_seed = (self.seed ^ POOL_SEED_SALT) & 0x7FFFFFFFFFFFFFFF
        self.partnerid = th.zeros(self.E, dtype=th.int32, device=self.dev)
        self.alt_actions = th.zeros((self.E, 2), dtype=th.int32, device=self.dev)
        self._rows = np.arange(self.E)
        if record:
            self.start_recording(record)
        self._first_deal()

    def _check_member(self, policy, seat=None) -> None:
        check_liar_member_policy(policy, type(self).__name__, towers=self.accepts_towers,
                                 adap=self.accepts_adaps and isinstance(seat, AdapFrozenVecPartner))

    def _contexts(self):
        return [self.env.ctx] + [p.ctx for p in map(self._policy_of, [self.ego] + self.members) if p is not None]

    def _build_native(self) -> None:
        s = self._fill_training(nat.PhLiarPool())
        s.members = self._member_arrays(self.members, self.accepts_towers, self.accepts_adaps, ego=self.ego)
        s.n_members, s.partnerid = self.K, self.partnerid.data_ptr()
        s.resample, s.pool_seed = nat.POOL_RESAMPLE[self.resample], self.pool_seed
        s.alt_actions = self.alt_actions.data_ptr()
        self._desc = s

    def _native_call(self, counter: int, deal_only: bool = False, ego_pos: int = -1) -> None:
        self._bind()
        ctx, rb = self.env.ctx, self.ego.model.rollout_buffer
        # the widest entry point; what the class does not accept is None (`_member_arrays`): the narrow entry points' own forward
        nat.check(ctx.lib.ph_liar_pool_step_adap(ctx.handle, C.byref(self._desc), self._ego_arch, self._member_arch_arr,
                                                 self._member_adap_arr, int(rb.pos if ego_pos < 0 else ego_pos), int(counter),
                                                 int(deal_only)))

    # -- the walk's hooks -------------------------------------------------------------------------------------------------------------
    def _seat_act(self, seat: int, obs: th.Tensor, mask, counter: int) -> th.Tensor:
        if seat == 0:
            return self._ego_act(counter)
        return self._members_act(range(self.K), self.partnerid, obs, mask, counter, self.alt_actions)

    def _credit(self, reward: th.Tensor, done: th.Tensor, replied) -> None:
        mask = self.alt_acted if replied is None else replied
        for k, m in enumerate(self.members):
            if isinstance(m, RaggedVecOnPolicyAgent):
                mine = self.partnerid == k
                m.update(reward, (done.bool() & mine).to(th.uint8), (mask.bool() & mine).to(th.uint8))

    def _seat_member(self, seat: int):
        return self.partnerid if seat == 1 else None

    def _resampled(self, c: int) -> th.Tensor:
        if self.resample == "robin":
            return (self.partnerid + 1) % self.K
        words = philox_word0(self.pool_seed, c, self._rows, POOL_RESAMPLE_BLOCK).astype(np.uint64)
        ids = (words * np.uint64(self.K)) >> np.uint64(32)
        return th.as_tensor(ids.astype(np.int32)).to(self.dev)

    def _on_deal(self, rm: th.Tensor, c: int) -> None:
        super()._on_deal(rm, c)
        self.partnerid.copy_(th.where(rm, self._resampled(c).to(th.int32), self.partnerid))   # the member that sits at the new game

    def rollout_and_learn(self, n_steps: int) -> None:
        """n_steps vectorised steps, the ego's update, then the update of every learner whose full() holds"""
        for _ in range(n_steps):
            self.step()
        self.ego.learn_from_buffer()
        for m in self.learners:
            if m.full():
                m.learn_from_buffer()


class TowerVecLiarPartnerPool(VecLiarPartnerPool):
    """VecLiarPartnerPool whose ego and members may play `policy_kwargs=dict(net_arch=...)` towers: the ego a TowerVecOnPolicyAgent,
    learners TowerRaggedVecOnPolicyAgent, frozen members TowerFrozenVecPartner, beside every member the plain class takes.  It differs
    from the plain class in what its member check accepts, and so in the archs the step is handed beside the member array (tower
    tiles of the grouped forward run in pool_tower_kernel).  The walk is the plain class's: the member classes' own get_action /
    update."""
    accepts_towers = True


class AdapVecLiarPartnerPool(TowerVecLiarPartnerPool):
    """TowerVecLiarPartnerPool whose members may also be frozen ADAP checkpoints (AdapFrozenVecPartner, stated or sampled latent).
    It differs in what its member check accepts, and so in the ADAP descriptions the step is handed beside the member array (ADAP
    tiles of the grouped forward run in pool_adap_kernel, a sampling member's contexts are redrawn behind the pass that ends
    games).  The walk is the plain class's, with the members' own redraw at every deal."""
    accepts_adaps = True


def liar_pool_for(n_envs: int, ego, members, **kwargs) -> VecLiarPartnerPool:
    """the pool class that runs `ego` and `members`: the plain one when nobody plays a tower or a frozen ADAP checkpoint"""
    members = list(members)
    if any(isinstance(m, AdapFrozenVecPartner) for m in members):
        return AdapVecLiarPartnerPool(n_envs, ego, members, **kwargs)
    pols = [VecLiarStep._policy_of(m) for m in [ego] + members]
    towers = any(p is not None and is_tower(p) for p in pols)
    return (TowerVecLiarPartnerPool if towers else VecLiarPartnerPool)(n_envs, ego, members, **kwargs)


class LiarIterationGraph:
    """One whole iteration of the device-resident Liar's Dice self-play with everything a replay must vary resident on the device:
    every random stream is keyed (RNG epoch word, counter) with the step-local counter baked in, and ONE epoch word -- shared by
    the forwards, the dice and the minibatch permutations of both learners -- is advanced once per iteration.

    Persistent mode (default): the rollout is ONE launch (`ph_liar_selfplay_rollout`); then the ego's GAE pass + PPO update replay
    from a hipGraph on this object's stream while -- whenever all its columns are full, the one host decision of the loop -- the
    partner's update runs beside it on a second stream (the general gradient kernel holds one workgroup per CU at this batch
    size, so two learners' launches fill the CUs instead of taking turns); the epoch word is advanced after both joined.
    LIAR_PERSISTENT=0: n_steps x 6 launches + the ego's update as one graph, the partner's update after it (round 1).
    `capture=False` runs the same body launch by launch (the graph's cross-check)."""

    def __init__(self, sp: VecLiarSelfPlay, n_steps: int, capture: bool = True, warmup: int = 2):
        assert sp.native, "the graph replays the engine-side step"
        if getattr(sp, "adap", False):
            raise nat.NativeError("LiarIterationGraph: an iteration with an ADAP seat is not captured (ADAP.train and the seat's "
                                  "contexts under an RNG epoch word have no replay story yet); use rollout_and_learn")
        self.sp, self.T = sp, int(n_steps)
        ego, alt = sp.ego, sp.alt
        assert self.T == ego.model.n_steps and ego.model.rollout_buffer.pos == 0
        self.stream = th.cuda.Stream(device=sp.dev)
        self.side = th.cuda.Stream(device=sp.dev)
        self._fork, self._join = th.cuda.Event(), th.cuda.Event()
        self.epoch_word = th.zeros(1, dtype=th.int64, device=sp.dev)
        for agent in (ego, alt):
            ctx = agent.model.policy.ctx
            nat.check(ctx.lib.ph_ctx_set_rng_epoch(ctx.handle, self.epoch_word.data_ptr()))
            agent.model.device_permutations = True
        self.graph_id = None
        self._recording = bool(sp.recording)      # a captured step holds the record launches of the recorder attached at capture
        self.split = bool(sp.persistent)          # rollout launch | ego-update graph || partner update | epoch advance
        th.cuda.synchronize(sp.dev)
        with th.cuda.stream(self.stream):
            self._perm_seed = ego.model.permutation_seed + 1
            for _ in range(warmup):          # outside capture: sizes the workspaces, allocates the statistics buffers
                self._iteration(eager=True)
            self.stream.synchronize()
            if capture:
                ctx = sp.env.ctx
                sp._bind()
                nat.check(ctx.lib.ph_graph_begin(ctx.handle))
                try:
                    self._update_body() if self.split else self._body()
                finally:
                    gid = C.c_int(-1)
                    nat.check(ctx.lib.ph_graph_end(ctx.handle, C.byref(gid)))
                self.graph_id = gid.value

    def _update_body(self) -> None:
        ego = self.sp.ego
        ego.compute_returns()
        ego.model.permutation_seed = self._perm_seed - 1     # train() pre-increments: the same baked seed in every replay
        ego.model.train(sync_stats=False)

    def _body(self) -> None:
        sp = self.sp
        for t in range(self.T):
            sp._native_call(t + 1, ego_pos=t)
        self._update_body()
        ctx = sp.env.ctx
        nat.check(ctx.lib.ph_rng_epoch_advance(ctx.handle))

    def _iteration_split(self, eager: bool) -> None:
        sp, ego, alt = self.sp, self.sp.ego, self.sp.alt
        main = th.cuda.current_stream(sp.dev)
        sp.rollout_persistent(self.T, 1, 0)                   # the T steps as ONE launch (counters 1..T)
        train_alt = alt.full()                                # host decision (synchronises on the rollout)
        if train_alt:
            self._fork.record(main)
            self.side.wait_event(self._fork)
            with th.cuda.stream(self.side):
                alt.learn_from_buffer()                       # beside the ego's update
                self._join.record(self.side)
        sp._bind()
        ctx = sp.env.ctx
        if eager:
            self._update_body()
        else:
            nat.check(ctx.lib.ph_graph_launch(ctx.handle, self.graph_id))
        if train_alt:
            main.wait_event(self._join)
        sp._bind()
        nat.check(ctx.lib.ph_rng_epoch_advance(ctx.handle))    # after BOTH learners drew their minibatch orders
        ego.finish_update()
        sp.steps_done += self.T
        ego.num_timesteps += self.T * sp.E
        alt.num_timesteps += self.T * sp.E

    def _iteration(self, eager: bool) -> None:
        if self.split:
            self._iteration_split(eager)
            return
        sp, ego, alt = self.sp, self.sp.ego, self.sp.alt
        if eager:
            self._body()
        else:
            sp._bind()
            ctx = sp.env.ctx
            nat.check(ctx.lib.ph_graph_launch(ctx.handle, self.graph_id))
        ego.finish_update()
        sp.steps_done += self.T
        ego.num_timesteps += self.T * sp.E
        alt.num_timesteps += self.T * sp.E
        if alt.full():
            alt.learn_from_buffer()

    def launch(self) -> None:
        if self.graph_id is not None and bool(self.sp.recording) != self._recording:
            raise nat.NativeError("LiarIterationGraph: the environment's recorder was attached or detached after capture: the graph "
                                  "replays the launches it was captured with (start_recording before building the graph)")
        with th.cuda.stream(self.stream):
            self._iteration(eager=self.graph_id is None)


class VecBlockWorld:
    """n_envs tables of BlockEnv-v0 (variant 0) or BlockEnv-v1 (variant 1) resident on the device, stepped by the per-call entry
    points `ph_block_reset` / `ph_block_step` / `ph_block_obs`.  The planner (ego) and the constructor (partner) have different
    spaces, so the class carries two pairs."""
    GAMES = {0: "BlockEnv-v0", 1: "BlockEnv-v1"}

    def __init__(self, variant: int, n_envs: int, ctx: nat.Context, device):
        from .blockworld import BlockEnv, SimpleBlockEnv
        game = (SimpleBlockEnv, BlockEnv)[int(variant)]
        self.variant, self.E, self.ctx, self.device = int(variant), n_envs, ctx, device
        self.observation_space, self.action_space = game.observation_space, game.action_space
        self.partner_observation_space, self.partner_action_space = game.partner_observation_space, game.partner_action_space
        self.D_ego, self.D_alt = len(self.observation_space.nvec), len(self.partner_observation_space.nvec)
        self.state = th.zeros((n_envs, nat.PH_BLOCK_STATE_WORDS), dtype=th.int32, device=device)
        self.obs_next_alt = th.zeros((n_envs, self.D_alt), dtype=th.float32, device=device)
        self.obs_next_ego = th.zeros((n_envs, self.D_ego), dtype=th.float32, device=device)
        self.rewards = th.zeros((n_envs, 2), dtype=th.float32, device=device)
        self.done = th.zeros(n_envs, dtype=th.uint8, device=device)

    @classmethod
    def seat_spaces(cls, variant: int):
        """-> (planner, constructor): two space carriers a PPO model can be built from"""
        from .blockworld import BlockEnv, SimpleBlockEnv
        game = (SimpleBlockEnv, BlockEnv)[int(variant)]
        carrier = lambda o, a: type("Spaces", (), dict(observation_space=o, action_space=a, _is_dummy_space_env=True))()  # noqa: E731
        return (carrier(game.observation_space, game.action_space),
                carrier(game.partner_observation_space, game.partner_action_space))

    def _bind(self):
        self.ctx.set_stream(th.cuda.current_stream(self.device).cuda_stream)

    def reset(self, seed: int, counter: int, reset_mask: th.Tensor = None) -> None:
        self._bind()
        nat.check(self.ctx.lib.ph_block_reset(self.ctx.handle, self.variant, self.state.data_ptr(), nat.ptr(reset_mask), int(seed),
                                              int(counter), self.E))

    def load(self, state: np.ndarray) -> None:
        """packed tables (E, 12) int32, e.g. from envs.blockworld.pack_state"""
        self.state.copy_(th.as_tensor(np.ascontiguousarray(state, np.int32)))

    def player_step(self, actions: th.Tensor, is_ego: bool, active: th.Tensor = None):
        """the planner's tokens (E) or the constructor's moves (E, A) int32 -> (the OTHER seat's observation, rewards (E, 2), done)"""
        self._bind()
        out = self.obs_next_alt if is_ego else self.obs_next_ego
        nat.check(self.ctx.lib.ph_block_step(self.ctx.handle, self.variant, self.state.data_ptr(), actions.data_ptr(), int(is_ego),
                                             nat.ptr(active), out.data_ptr(), self.rewards.data_ptr(), self.done.data_ptr(), self.E))
        return out, self.rewards, self.done

    def observe(self, is_ego: bool, out: th.Tensor, active: th.Tensor = None) -> th.Tensor:
        self._bind()
        nat.check(self.ctx.lib.ph_block_obs(self.ctx.handle, self.variant, self.state.data_ptr(), int(is_ego), nat.ptr(active),
                                            out.data_ptr(), self.E))
        return out


class VecBlockScriptedPartner:
    """A scripted constructor for E tables, integer-exact (`ph_block_scripted_actions`): variant 1 with rule "DEFAULT" is
    DefaultConstructorAgent, variant 0 with "DEFAULT" SBWDefaultAgent and with "EASY" SBWEasyPartner (envs/blockworld.py).  Where
    SBWEasyPartner answers a negative block index the rule gives it modulo 5 -- the block the host game colours."""
    kind = nat.PH_POOL_SCRIPTED

    def __init__(self, variant: int, rule="DEFAULT"):
        self.variant = int(variant)
        if self.variant not in (0, 1):
            raise nat.NativeError("VecBlockScriptedPartner: variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)")
        if isinstance(rule, str):
            if rule not in nat.BLOCK_RULES:
                raise nat.NativeError(f"VecBlockScriptedPartner: unknown rule {rule!r} (DEFAULT or EASY)")
            rule = nat.BLOCK_RULES[rule]
        self.rule = int(rule)
        if self.rule not in (nat.PH_BLOCK_RULE_DEFAULT, nat.PH_BLOCK_RULE_EASY):
            raise nat.NativeError(f"VecBlockScriptedPartner: unknown rule {rule!r} (DEFAULT or EASY)")
        if self.rule == nat.PH_BLOCK_RULE_EASY and self.variant != 0:
            raise nat.NativeError("VecBlockScriptedPartner: EASY (SBWEasyPartner) exists for BlockEnv-v0 only, not BlockEnv-v1")

    def get_action(self, obs: th.Tensor, rec_mask: th.Tensor, out: th.Tensor, ctx: nat.Context) -> th.Tensor:
        """writes the rule's move into `out` (E, 3 | 2) int32 where rec_mask is set (None: everywhere); the other rows keep what
        they hold"""
        nat.check(ctx.lib.ph_block_scripted_actions(ctx.handle, self.variant, self.rule, obs.data_ptr(), nat.ptr(rec_mask),
                                                    out.data_ptr(), int(obs.shape[0])))
        return out

    def update(self, reward, done, mask=None) -> None:
        return None


class VecBlockSelfPlay:
    """`trainer.py BlockEnv-v0|v1 PPO PPO` with n_envs tables resident on the device.

    One vectorised step is one `MultiAgentEnv.step` of every table: the planner speaks; where that was not its last token the
    constructor moves; a finished table gets its next world at once, so every table is back at the planner's turn.  The planner
    is a rectangular VecOnPolicyAgent, the constructor a RaggedVecOnPolicyAgent: it is not asked to act in a table whose game
    the planner just ended (but is paid there, if it moved in that game).

    native=True: the step is ONE engine call (`ph_block_selfplay_step`: two forwards and one book-keeping launch after each,
    every mask on the device, no host synchronisation).  native=False walks the same step with the per-call entry points and
    torch masks -- the readable statement and the bitwise cross-check (same RNG counters: step c -> both forwards and the
    worlds of the games that start in it draw with counter c; the first worlds with counter 0)."""

    def __init__(self, variant: int, n_envs: int, ego: VecOnPolicyAgent, alt: RaggedVecOnPolicyAgent, seed: int = 0,
                 native: bool = True):
        self.variant, self.E, self.ego, self.alt, self.native = int(variant), n_envs, ego, alt, bool(native)
        pol = ego.model.policy
        self.dev = pol.device
        self.env = VecBlockWorld(variant, n_envs, pol.ctx, self.dev)
        self.seed = int(seed)
        E, dev = n_envs, self.dev
        u8 = lambda v=0: th.full((E,), v, dtype=th.uint8, device=dev)  # noqa: E731
        self.obs_ego = th.zeros((E, self.env.D_ego), dtype=th.float32, device=dev)
        self.obs_alt = th.zeros((E, self.env.D_alt), dtype=th.float32, device=dev)
        self.alt_acted = u8()
        self._done, self._running, self._can = u8(), u8(), u8()
        self._es_alt = th.zeros(E, dtype=th.float32, device=dev)
        self._episodes_dev = th.zeros(1, dtype=th.int64, device=dev)
        self.steps_done = 0
        self._archs = (seat_arch(ego), seat_arch(alt))        # a tower in either seat: the `_arch` step
        self.towers = any(a is not None for a in self._archs)
        self._bind()
        self.env.reset(self.seed, 0)
        self.env.observe(True, self.obs_ego)
        if self.native:
            self._build_native()

    @property
    def episodes(self) -> int:
        return int(self._episodes_dev.item())

    def _bind(self):
        stream = th.cuda.current_stream(self.dev).cuda_stream
        self.env.ctx.set_stream(stream)
        for agent in (self.ego, self.alt):
            agent.model.policy.ctx.set_stream(stream)

    def _build_native(self) -> None:
        ego, alt = self.ego, self.alt
        ego._last_episode_starts = ego._last_episode_starts.clone()    # updated in place by the step from here on
        s = nat.PhBlockSelfPlay()
        pe, pa = ego.model.policy, alt.model.policy
        s.n, s.variant = self.E, self.variant
        s.ego_spec, s.alt_spec = C.pointer(pe.spec), C.pointer(pa.spec)
        s.state, s.world_seed = self.env.state.data_ptr(), self.seed
        self._ego_rbc, self._alt_rbc = ego.model.rollout_buffer.c_struct(), alt.model.rollout_buffer.c_struct()
        s.ego_params, s.ego_rb, s.ego_actions = pe.params.data_ptr(), C.pointer(self._ego_rbc), ego.actions.data_ptr()
        s.ego_values, s.ego_log_probs = ego.values.data_ptr(), ego.log_probs.data_ptr()
        s.ego_episode_start, s.ego_seed = ego._last_episode_starts.data_ptr(), pe._seed
        s.alt_params, s.alt_rb, s.alt_actions = pa.params.data_ptr(), C.pointer(self._alt_rbc), alt.actions.data_ptr()
        s.alt_values, s.alt_log_probs, s.alt_pos = alt.values.data_ptr(), alt.log_probs.data_ptr(), alt.pos.data_ptr()
        s.alt_boundary, s.alt_term, s.alt_open = alt.boundary.data_ptr(), alt.term.data_ptr(), alt.open.data_ptr()
        s.alt_acted, s.alt_seed = self.alt_acted.data_ptr(), pa._seed
        s.obs_ego, s.obs_alt, s.episodes = self.obs_ego.data_ptr(), self.obs_alt.data_ptr(), self._episodes_dev.data_ptr()
        s.es_alt, s.running, s.can, s.done = (t.data_ptr() for t in (self._es_alt, self._running, self._can, self._done))
        self._desc = s

    def _native_call(self, counter: int, ego_pos: int = -1) -> None:
        self._bind()
        ctx, rb = self.env.ctx, self.ego.model.rollout_buffer
        pos = int(rb.pos if ego_pos < 0 else ego_pos)
        # no tower in either seat: (None, None), the plain step
        nat.check(ctx.lib.ph_block_selfplay_step_arch(ctx.handle, C.byref(self._desc), self._archs[0], self._archs[1], pos,
                                                      int(counter)))

    def step(self):
        """-> (E,) uint8 device tensor: tables whose game ended in this step"""
        ego, alt, env = self.ego, self.alt, self.env
        self.steps_done += 1
        c = self.steps_done
        if self.native:
            model, rb = ego.model, ego.model.rollout_buffer
            if ego.n_steps >= model.n_steps:
                ego.learn_from_buffer()
            self._native_call(c)
            rb.pos += 1
            rb.full = rb.pos == rb.buffer_size
            ego.n_steps += 1
            ego.num_timesteps += self.E
            alt.num_timesteps += self.E
            return self._done
        self._bind()
        ego.model.policy._counter = c - 1
        tokens = ego.get_action(self.obs_ego)                                  # every table is at the planner's turn
        obs_alt, rew, done = env.player_step(tokens, True)
        done8 = done.clone()
        d = done8.bool()
        # a partner that already moved in this game is credited this transition (multiagentenv.py:167-173)
        alt.update(rew[:, 1].contiguous(), done8, self.alt_acted)
        ego.update(rew[:, 0].contiguous(), done8.to(th.float32))
        ego.flush_rewards()
        self._episodes_dev += done8.sum()
        running = (~d).to(th.uint8)
        self.obs_alt.copy_(th.where(~d[:, None], obs_alt, self.obs_alt))
        # finished tables: the next world, nobody has acted in it, the planner's first observation
        env.reset(self.seed, c, done8)
        self.alt_acted.copy_(th.where(d, th.zeros_like(self.alt_acted), self.alt_acted))
        env.observe(True, self.obs_ego, done8)
        # the constructor moves where the game goes on
        alt.model.policy._counter = c - 1
        moves = alt.get_action(self.obs_alt, running)
        self.alt_acted.copy_((self.alt_acted.bool() | ~d).to(th.uint8))
        obs_ego, _, _ = env.player_step(moves, False, running)
        self.obs_ego.copy_(th.where(~d[:, None], obs_ego, self.obs_ego))
        return done8

    def rollout_and_learn(self, n_steps: int) -> None:
        """n_steps vectorised steps, the planner's update, and the constructor's whenever all its columns are full"""
        for _ in range(n_steps):
            self.step()
        self.ego.learn_from_buffer()
        if self.alt.full():
            self.alt.learn_from_buffer()


def check_block_pool_seat(agent, variant: int, seat: int, who: str) -> None:
    """the ego (seat 0: a VecOnPolicyAgent on the planner spaces) or a member (seat 1: RaggedVecOnPolicyAgent, FrozenVecPartner or
    VecBlockScriptedPartner on the constructor spaces) of the block worlds' partner pool runs on the pool step's kernels: the 64-64
    MlpPolicy on the variant's spaces, or the variant's scripted rule.  Everything else is refused by name, before a device is
    touched."""
    from ..adap import AdapPolicy
    from ..spaces import make_spec
    game = VecBlockWorld.GAMES[int(variant)]
    if isinstance(agent, VecBlockScriptedPartner):
        if seat == 0:
            raise nat.NativeError(f"{who}: a scripted constructor does not sit at the planner's seat")
        if agent.variant != int(variant):
            raise nat.NativeError(f"{who}: the scripted constructor is {VecBlockWorld.GAMES[agent.variant]}'s, not {game}'s")
        return
    if isinstance(agent, VecLiarDefaultPartner):
        raise nat.NativeError(f"{who}: VecLiarDefaultPartner is the Liar's Dice player; a block world's scripted constructor is "
                              "VecBlockScriptedPartner(variant, rule)")
    if isinstance(agent, ClonedVecPartner):
        raise nat.NativeError(f"{who}: a BC clone (ClonedVecPartner, FeedForward32Policy) does not sit in the block worlds' partner pool")
    if isinstance(agent, (AdapFrozenVecPartner, AdapSeat)):
        raise nat.NativeError(f"{who}: ADAP (a learner, an ego or an AdapFrozenVecPartner checkpoint) does not sit in the block worlds' "
                              "partner pool")
    if seat == 0:
        if not isinstance(agent, VecOnPolicyAgent):
            raise nat.NativeError(f"{who}: the ego is a VecOnPolicyAgent on {game}'s planner spaces, not {type(agent).__name__}")
        policy = agent.model.policy
    elif isinstance(agent, RaggedVecOnPolicyAgent):
        policy = agent.model.policy
    elif isinstance(agent, FrozenVecPartner):
        policy = agent.policy
    else:
        raise nat.NativeError(f"{who}: members are RaggedVecOnPolicyAgent (a learner), FrozenVecPartner or VecBlockScriptedPartner, "
                              f"not {type(agent).__name__}")
    if isinstance(policy, AdapPolicy) or is_adap(policy):
        raise nat.NativeError(f"{who}: ADAP (an AdapPolicy) does not sit in the block worlds' partner pool")
    if is_tower(policy):
        raise nat.NativeError(f"{who}: a net_arch tower (ArchActorCriticPolicy) does not sit in the block worlds' partner pool")
    if isinstance(policy, FeedForward32Policy):
        raise nat.NativeError(f"{who}: a FeedForward32Policy (a BC clone) does not sit in the block worlds' partner pool")
    if policy.spec.act.kind == nat.PH_SPACE_BOX:
        raise nat.NativeError(f"{who}: a policy with Box actions does not play a block world")
    require_mlp_kernels(policy, who)
    spaces = VecBlockWorld.seat_spaces(variant)[seat]
    want = nat.layout_of(make_spec(spaces.observation_space, spaces.action_space))
    lay = policy.layout
    if (lay.D, lay.F, lay.A, lay.L) != (want.D, want.F, want.A, want.L):
        raise nat.NativeError(f"{who}: the policy does not play on {game}'s {('planner', 'constructor')[seat]} spaces")


class VecBlockPartnerPool:
    """`trainer.py BlockEnv-v0|v1 PPO <alt>+ --partner-pool --n-envs E`: n_envs block-world tables resident on the device, the
    constructor's seat of every table held by one of K <= 8 pool members -- learners (RaggedVecOnPolicyAgent), frozen policies
    (FrozenVecPartner) or scripted constructors (VecBlockScriptedPartner).  `partnerid[e]` names table e's member; it is resampled
    where the table's game ends (`pool_resample`), the first world included: under "robin" every table starts at 1 % K.

    Per table the callbacks are VecBlockSelfPlay's, with every partner-side mask ANDed with `partnerid == k`: credit goes to the
    member that has acted in this game (`alt_acted`, cleared with the next world), and a member's `boundary` flag of a table
    survives the games it sits out.  RNG counters of step c: the ego's forward c, a member's forward c under its own seed, the
    worlds of the games that start in it c, the resample c (the first worlds and the first resample: 0) -- VecBlockSelfPlay's, so
    a pool of one learner is that class bit for bit.  `rollout_and_learn` trains the ego, then every learner whose `full()`
    holds; a learner's `min_full` becomes max(1, E // K) unless the caller lowered it already.  It carries what EpisodeStats
    reads of a pool (`partnerid`, `K`, `resample`, `pool_seed`, `row0_counter`, `steps_done`).

    native=True: one `ph_block_pool_step` per vectorised step -- five launches, six with a scripted member, whatever K is, no
    host synchronisation.  native=False: the readable walk -- K per-member get_action / update calls with torch masks, the
    per-call entry points only, the same counters; bitwise the native step."""

    def __init__(self, variant: int, n_envs: int, ego: VecOnPolicyAgent, members, seed: int = 0, resample: str = "robin",
                 native: bool = True):
        self.variant = int(variant)
        if self.variant not in (0, 1):
            raise nat.NativeError("VecBlockPartnerPool: variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)")
        members = list(members)
        if not 1 <= len(members) <= nat.PH_MAX_POOL:
            raise nat.NativeError(f"VecBlockPartnerPool: the pool holds 1..{nat.PH_MAX_POOL} members, not {len(members)}")
        if resample not in nat.POOL_RESAMPLE:
            raise nat.NativeError(f"VecBlockPartnerPool: resample must be one of {sorted(nat.POOL_RESAMPLE)}, not {resample!r}")
        check_block_pool_seat(ego, self.variant, 0, "VecBlockPartnerPool: the ego")
        for k, m in enumerate(members):
            check_block_pool_seat(m, self.variant, 1, f"VecBlockPartnerPool: member {k}")
        self.E, self.ego, self.members, self.native = int(n_envs), ego, members, bool(native)
        self.resample, self.K = resample, len(members)
        self.learners = [m for m in members if isinstance(m, RaggedVecOnPolicyAgent)]
        if ego.E != self.E:
            raise nat.NativeError("VecBlockPartnerPool: the ego's rollout buffer must have n_envs columns")
        for m in self.learners:
            if m.E != self.E:
                raise nat.NativeError("VecBlockPartnerPool: a learner's rollout buffer must have n_envs columns")
            if m.min_full >= m.E:
                m.min_full = max(1, self.E // self.K)
        pol = ego.model.policy
        self.dev = pol.device
        self.env = VecBlockWorld(self.variant, self.E, pol.ctx, self.dev)
        self.seed = int(seed)
        self.pool_seed = (self.seed ^ POOL_SEED_SALT) & 0x7FFFFFFFFFFFFFFF
        E, dev = self.E, self.dev
        u8 = lambda v=0: th.full((E,), v, dtype=th.uint8, device=dev)  # noqa: E731
        A = len(self.env.partner_action_space.nvec)
        self.obs_ego = th.zeros((E, self.env.D_ego), dtype=th.float32, device=dev)
        self.obs_alt = th.zeros((E, self.env.D_alt), dtype=th.float32, device=dev)
        self.partnerid = th.zeros(E, dtype=th.int32, device=dev)
        self.alt_actions = th.zeros((E, A), dtype=th.int32, device=dev)
        self.alt_acted = u8()
        self._done, self._running, self._can = u8(), u8(), u8()
        self._es_alt = th.zeros(E, dtype=th.float32, device=dev)
        self._episodes_dev = th.zeros(1, dtype=th.int64, device=dev)
        self._rows = np.arange(E)
        self.steps_done = 0
        self.row0_counter = 1      # the step counter of row 0 of the ego's buffer: what EpisodeStats replays the resamples from
        self._ctxs = tuple(dict.fromkeys([self.env.ctx] + [p.ctx for p in map(self._policy_of, [ego] + members) if p is not None]))
        self._bind()
        if self.native:
            self._build_native()
            self._native_call(0, first=True)
        else:
            self.env.reset(self.seed, 0)
            self.partnerid.copy_(self._resampled(0).to(th.int32))
            self.env.observe(True, self.obs_ego)

    @staticmethod
    def _policy_of(agent):
        """the policy a seat plays with (None: a scripted constructor)"""
        if isinstance(agent, VecBlockScriptedPartner):
            return None
        return agent.policy if isinstance(agent, FrozenVecPartner) else agent.model.policy

    @property
    def episodes(self) -> int:
        return int(self._episodes_dev.item())

    def _bind(self):
        stream = th.cuda.current_stream(self.dev).cuda_stream
        for ctx in self._ctxs:
            ctx.set_stream(stream)

    # -- the engine-side step ------------------------------------------------------------------------------------------------------
    def _member_array(self):
        """the PhPoolMember array (kept alive with the learners' buffer records); a scripted member's `seed` holds its rule"""
        self._member_rbc = []
        arr = (nat.PhPoolMember * self.K)()
        for c, m in zip(arr, self.members):
            learner = isinstance(m, RaggedVecOnPolicyAgent)
            c.kind = nat.PH_POOL_LEARNER if learner else m.kind
            if isinstance(m, VecBlockScriptedPartner):
                c.seed = m.rule
                continue
            p = self._policy_of(m)
            c.params, c.seed = p.params.data_ptr(), p._seed
            if learner:
                rbc = m.model.rollout_buffer.c_struct()
                self._member_rbc.append(rbc)
                c.rb = C.pointer(rbc)
                c.pos, c.boundary, c.term, c.open = (t.data_ptr() for t in (m.pos, m.boundary, m.term, m.open))
                c.values, c.log_probs = m.values.data_ptr(), m.log_probs.data_ptr()
        self._member_arr = arr
        return arr

    def _build_native(self) -> None:
        from ..spaces import make_spec
        ego, pe = self.ego, self.ego.model.policy
        ego._last_episode_starts = ego._last_episode_starts.clone()    # updated in place by the step from here on
        alt_spaces = VecBlockWorld.seat_spaces(self.variant)[1]
        self._alt_spec = make_spec(alt_spaces.observation_space, alt_spaces.action_space)
        s = nat.PhBlockPool()
        s.n, s.variant = self.E, self.variant
        s.ego_spec, s.alt_spec = C.pointer(pe.spec), C.pointer(self._alt_spec)
        s.state, s.world_seed = self.env.state.data_ptr(), self.seed
        self._ego_rbc = ego.model.rollout_buffer.c_struct()
        s.ego_params, s.ego_rb, s.ego_actions = pe.params.data_ptr(), C.pointer(self._ego_rbc), ego.actions.data_ptr()
        s.ego_values, s.ego_log_probs = ego.values.data_ptr(), ego.log_probs.data_ptr()
        s.ego_episode_start, s.ego_seed = ego._last_episode_starts.data_ptr(), pe._seed
        s.members, s.n_members, s.partnerid = self._member_array(), self.K, self.partnerid.data_ptr()
        s.resample, s.pool_seed = nat.POOL_RESAMPLE[self.resample], self.pool_seed
        s.alt_actions, s.alt_acted = self.alt_actions.data_ptr(), self.alt_acted.data_ptr()
        s.obs_ego, s.obs_alt, s.episodes = self.obs_ego.data_ptr(), self.obs_alt.data_ptr(), self._episodes_dev.data_ptr()
        s.es_alt, s.running, s.can, s.done = (t.data_ptr() for t in (self._es_alt, self._running, self._can, self._done))
        self._desc = s

    def _native_call(self, counter: int, ego_pos: int = -1, first: bool = False) -> None:
        self._bind()
        ctx, rb = self.env.ctx, self.ego.model.rollout_buffer
        pos = int(rb.pos if ego_pos < 0 else ego_pos)
        nat.check(ctx.lib.ph_block_pool_step(ctx.handle, C.byref(self._desc), pos, int(counter), int(first)))

    # -- the walk: the per-call entry points with torch masks ------------------------------------------------------------------------
    def _resampled(self, c: int) -> th.Tensor:
        if self.resample == "robin":
            return (self.partnerid + 1) % self.K
        words = philox_word0(self.pool_seed, c, self._rows, POOL_RESAMPLE_BLOCK).astype(np.uint64)
        ids = (words * np.uint64(self.K)) >> np.uint64(32)
        return th.as_tensor(ids.astype(np.int32)).to(self.dev)

    def _credit(self, reward: th.Tensor, done: th.Tensor, mask: th.Tensor) -> None:
        for k, m in enumerate(self.members):
            if isinstance(m, RaggedVecOnPolicyAgent):
                mine = self.partnerid == k
                m.update(reward, (done.bool() & mine).to(th.uint8), (mask.bool() & mine).to(th.uint8))

    def _members_act(self, obs: th.Tensor, mask: th.Tensor, counter: int) -> th.Tensor:
        """the forward of every member over all rows with Philox counter `counter`; member k's move lands in the tables of `mask`
        where partnerid == k"""
        out = self.alt_actions
        for k, m in enumerate(self.members):
            mk = (mask.bool() & (self.partnerid == k)).to(th.uint8)
            if isinstance(m, VecBlockScriptedPartner):
                m.get_action(obs, mk, out, self.env.ctx)
                continue
            self._policy_of(m)._counter = counter - 1
            a = m.get_action(obs, mk)
            out.copy_(th.where(mk.bool()[:, None], a, out))
        return out

    def _walk(self, c: int) -> th.Tensor:
        ego, env = self.ego, self.env
        self._bind()
        ego.model.policy._counter = c - 1
        tokens = ego.get_action(self.obs_ego)                                  # every table is at the planner's turn
        obs_alt, rew, done = env.player_step(tokens, True)
        done8 = done.clone()
        d = done8.bool()
        # the member that already moved in this game is credited this transition (multiagentenv.py:167-173)
        self._credit(rew[:, 1].contiguous(), done8, self.alt_acted)
        ego.update(rew[:, 0].contiguous(), done8.to(th.float32))
        ego.flush_rewards()
        self._episodes_dev += done8.sum()
        running = (~d).to(th.uint8)
        self.obs_alt.copy_(th.where(~d[:, None], obs_alt, self.obs_alt))
        # finished tables: the next world, nobody has acted in it, the member that sits at it, the planner's first observation
        env.reset(self.seed, c, done8)
        self.alt_acted.copy_(th.where(d, th.zeros_like(self.alt_acted), self.alt_acted))
        self.partnerid.copy_(th.where(d, self._resampled(c).to(th.int32), self.partnerid))
        env.observe(True, self.obs_ego, done8)
        # every running table's member moves
        moves = self._members_act(self.obs_alt, running, c)
        self.alt_acted.copy_((self.alt_acted.bool() | ~d).to(th.uint8))
        obs_ego, _, _ = env.player_step(moves, False, running)
        self.obs_ego.copy_(th.where(~d[:, None], obs_ego, self.obs_ego))
        return done8

    # -- one vectorised MultiAgentEnv.step -------------------------------------------------------------------------------------
    def step(self):
        """-> (E,) uint8 device tensor: tables whose game ended in this step"""
        ego = self.ego
        self.steps_done += 1
        c = self.steps_done
        model, rb = ego.model, ego.model.rollout_buffer
        row0 = rb.pos == 0 or ego.n_steps >= model.n_steps       # this step fills row 0 (behind the roll-over, where one is due)
        if not self.native:
            done = self._walk(c)
            if row0:
                self.row0_counter = c
            return done
        if ego.n_steps >= model.n_steps:
            ego.learn_from_buffer()
        if row0:
            self.row0_counter = c                                # behind the roll-over: its scan replayed the rollout before
        self._native_call(c)
        rb.pos += 1
        rb.full = rb.pos == rb.buffer_size
        ego.n_steps += 1
        ego.num_timesteps += self.E
        for m in self.learners:
            m.num_timesteps += self.E
        return self._done

    def rollout_and_learn(self, n_steps: int) -> None:
        """n_steps vectorised steps, the planner's update, then the update of every learner whose full() holds"""
        for _ in range(n_steps):
            self.step()
        self.ego.learn_from_buffer()
        for m in self.learners:
            if m.full():
                m.learn_from_buffer()
