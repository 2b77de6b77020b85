"""the workload of profiles/pool_clone_kernel_stats_k4.txt: two rollout_and_learn(128) calls of a native K = 4 partner pool with two
behavioural clones -- E = 256, ego n_steps 128, members [learner (n_steps 32), clone, learner (n_steps 32), clone] -- to be run under
`rocprofv3 --kernel-trace --stats` (no counters).  A partner move is a bucket pass, the grouped forward and the clone-tile kernel."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd.bc import FeedForward32Policy  # noqa: E402
from pantheonrl_amd.envs.vec import ClonedVecPartner, RaggedVecOnPolicyAgent, VecLiarPartnerPool, VecLiarsDice  # noqa: E402
from pantheonrl_amd.vec import VecOnPolicyAgent  # noqa: E402

E, T = 256, 128
spaces = type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                            _is_dummy_space_env=True))()


def model(seed, n_steps=T):
    m = PPO("MlpPolicy", spaces, n_steps=n_steps, n_envs=E, batch_size=E * n_steps // 4, n_epochs=10, seed=seed)
    m.device_permutations = True
    return m


def clone(seed):
    pol = FeedForward32Policy(spaces.observation_space, spaces.action_space, seed=seed)
    pol.set_flat_params(0.4 * np.random.default_rng(seed).standard_normal(pol.layout.P).astype(np.float32))
    return ClonedVecPartner(pol)


ego = VecOnPolicyAgent(model(0))
members = [RaggedVecOnPolicyAgent(model(1, T // 4)), clone(2), RaggedVecOnPolicyAgent(model(3, T // 4)), clone(4)]
sp = VecLiarPartnerPool(E, ego, members, seed=3, native=True)
for _ in range(2):
    sp.rollout_and_learn(T)
th.cuda.synchronize()
print(f"steps {sp.steps_done} episodes {sp.episodes} learner updates {[m.iteration for m in sp.learners]}")
