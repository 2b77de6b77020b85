"""the workload of profiles/pool_tower_kernel_stats_k4.txt: two rollout_and_learn(128) calls of a native K = 4 partner pool with two
`policy_kwargs net_arch` towers -- E = 256, ego n_steps 128 (64-64), members [learner tower (32,) (n_steps 32), frozen tower
(128, 128), learner 64-64 (n_steps 32), scripted] -- to be run under `rocprofv3 --kernel-trace --stats` (no counters).  A partner
move is a bucket pass, the grouped forward and the tower-tile kernel.
`--empty`: instead, 64 grouped forwards of the same member table over no active table (`ph_pool_forward_arch`): every workgroup of
the three kernels returns at the tile count -- the time of a launch with no tile to run."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd import _native as nat  # noqa: E402
from pantheonrl_amd.envs.vec import (TowerFrozenVecPartner, VecLiarDefaultPartner, VecLiarsDice, liar_pool_for,  # noqa: E402
                                     ragged_agent_for)
from pantheonrl_amd.vec import vec_agent_for  # noqa: E402

E, T = 256, 128
spaces = type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                            _is_dummy_space_env=True))()


def model(seed, n_steps=T, widths=None):
    kw = dict(policy_kwargs=dict(net_arch=[dict(pi=list(widths), vf=list(widths))])) if widths else {}
    m = PPO("MlpPolicy", spaces, n_steps=n_steps, n_envs=E, batch_size=E * n_steps // 4, n_epochs=10, seed=seed, **kw)
    m.device_permutations = True
    return m


ego = vec_agent_for(model(0))
members = [ragged_agent_for(model(1, T // 4, (32,))), TowerFrozenVecPartner(model(2, 2, (128, 128)).policy),
           ragged_agent_for(model(3, T // 4)), VecLiarDefaultPartner()]
sp = liar_pool_for(E, ego, members, seed=3, native=True)
if "--empty" in sys.argv:
    sp._bind()
    ctx = sp.env.ctx
    for c in range(64):
        nat.check(ctx.lib.ph_pool_forward_arch(ctx.handle, C.byref(ego.model.policy.spec), sp._member_arr, sp.K, sp.obs_alt.data_ptr(),
                                               sp.partnerid.data_ptr(), sp.zeros8.data_ptr(), 1000 + c, sp.alt_actions.data_ptr(),
                                               sp._es_alt.data_ptr(), E, sp._member_arch_arr))
    th.cuda.synchronize()
    print("64 grouped forwards over no active table (after the first deal's one)")
    sys.exit(0)
for _ in range(2):
    sp.rollout_and_learn(T)
th.cuda.synchronize()
print(f"steps {sp.steps_done} episodes {sp.episodes} learner updates {[m.iteration for m in sp.learners]}")
