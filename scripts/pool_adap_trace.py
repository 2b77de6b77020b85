"""the workload of profiles/adap_members_speed_liar.txt's kernel trace: two rollout_and_learn(128) calls of a native K = 4 partner
pool with two frozen ADAP members -- E = 256, ego n_steps 128 (64-64), members [ADAP under a stated latent, frozen 64-64, ADAP under
sampled latents, scripted] -- to be run under `rocprofv3 --kernel-trace --stats` (no counters).  A partner move is a bucket pass,
the grouped forward (pool_fwd16h_kernel) and the ADAP-tile kernel (pool_adap_kernel); a step adds one context redraw."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd.adap import ADAP, AdapPolicy  # noqa: E402
from pantheonrl_amd.envs.vec import (AdapFrozenVecPartner, FrozenVecPartner, VecLiarDefaultPartner, VecLiarsDice,  # noqa: E402
                                     liar_pool_for)
from pantheonrl_amd.vec import vec_agent_for  # noqa: E402

E, T = 256, 128
spaces = type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                            _is_dummy_space_env=True))()


def model(seed, n_steps=T):
    m = PPO("MlpPolicy", spaces, n_steps=n_steps, n_envs=E, batch_size=E * n_steps // 4, n_epochs=10, seed=seed)
    m.device_permutations = True
    return m


def adap(seed):
    return ADAP(AdapPolicy, spaces, context_size=3, n_steps=2, n_envs=4, batch_size=4, n_epochs=1, seed=seed).policy


ego = vec_agent_for(model(0))
members = [AdapFrozenVecPartner(adap(1), np.asarray([1.0, 0.0, 0.0], np.float32)), FrozenVecPartner(model(2, 2).policy),
           AdapFrozenVecPartner(adap(3), "sample"), VecLiarDefaultPartner()]
sp = liar_pool_for(E, ego, members, seed=3, native=True)
for _ in range(2):
    sp.rollout_and_learn(T)
th.cuda.synchronize()
print(f"steps {sp.steps_done} episodes {sp.episodes}")
