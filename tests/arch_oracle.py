"""The checker for `policy_kwargs net_arch`: MlpPolicyOracle (oracle/sb3_oracle.py, 64-wide) rebuilt for a tower width list, and
the device-side analogues of tests/helpers.py for ArchActorCriticPolicy.  The extractor is SB3's loop as the reference keeps it in
pantheonrl/algos/adap/policies.py:152-200: Linear then Tanh for every listed width, the same list for both towers."""
from __future__ import annotations

import numpy as np
import torch as th
from torch import nn

from oracle.sb3_oracle import MlpPolicyOracle
from tests import helpers as H

# name them once, use them everywhere
ARCHES = [(32,), (128, 128), (256, 256), (64, 64, 64), (256, 128), (96, 160, 32), (256, 256, 256), (64, 64)]
SPECS = ["rps", "overcooked", "liar", "wide", "quad16", "onehot32", "discrete20"]


def arch_id(a) -> str:
    return "x".join(str(w) for w in a)


def param_count(F: int, L: int, widths) -> int:
    """P = 2 * sum_l (in_l * w_l + w_l) + w_n * L + L + w_n + 1"""
    tower, fin = 0, F
    for w in widths:
        tower += fin * w + w
        fin = w
    return 2 * tower + widths[-1] * L + L + widths[-1] + 1


class ArchPolicyOracle(MlpPolicyOracle):
    """MlpPolicyOracle with towers of `widths`; parameter vector: policy tower W1 b1 .. Wn bn, value tower the same,
    act_W[w_n][L], act_b, val_W[w_n], val_b (weights input-major)."""

    def __init__(self, obs_space, act_space, widths, lr: float = 3e-4, ortho_init: bool = True):
        super().__init__(obs_space, act_space, lr=lr, ortho_init=False)
        self.widths = tuple(int(w) for w in widths)
        Fdim, L = obs_space.flat_len, act_space.flat_len

        def tower():
            layers, fin = [], Fdim
            for w in self.widths:
                layers += [nn.Linear(fin, w), nn.Tanh()]
                fin = w
            return nn.Sequential(*layers)
        self.policy_net, self.value_net_mlp = tower(), tower()
        self.action_net = nn.Linear(self.widths[-1], L)
        self.value_net = nn.Linear(self.widths[-1], 1)
        if ortho_init:  # gains and module order: modular/policies.py:229-241
            for mod, gain in ((self.policy_net, np.sqrt(2)), (self.value_net_mlp, np.sqrt(2)), (self.action_net, 0.01),
                              (self.value_net, 1.0)):
                for m in mod.modules():
                    if isinstance(m, nn.Linear):
                        nn.init.orthogonal_(m.weight, gain=gain)
                        m.bias.data.fill_(0.0)
        self.optimizer = th.optim.Adam(self.parameters(), lr=lr, eps=1e-5)

    def _linears(self):
        return ([m for m in self.policy_net if isinstance(m, nn.Linear)] + [m for m in self.value_net_mlp if isinstance(m, nn.Linear)]
                + [self.action_net, self.value_net])

    def flat_params(self) -> np.ndarray:
        out = []
        for lin in self._linears():
            out += [lin.weight.detach().t().contiguous().reshape(-1), lin.bias.detach()]
        return th.cat(out).numpy().astype(np.float32).copy()

    def load_flat_params(self, flat: np.ndarray) -> None:
        flat = th.as_tensor(np.asarray(flat, np.float32))
        o = 0
        with th.no_grad():
            for lin in self._linears():
                n = lin.weight.numel()
                lin.weight.copy_(flat[o:o + n].reshape(lin.in_features, lin.out_features).t())
                o += n
                lin.bias.copy_(flat[o:o + lin.bias.numel()])
                o += lin.bias.numel()
        assert o == flat.numel()

    def flat_grads(self) -> np.ndarray:
        out = []
        for lin in self._linears():
            out += [lin.weight.grad.t().contiguous().reshape(-1), lin.bias.grad]
        return th.cat(out).numpy().astype(np.float32).copy()


def oracle_policy(name: str, widths, seed: int = 0, perturb: float = 0.3) -> ArchPolicyOracle:
    """seeded checker; biases and the 0.01-gain action head perturbed as helpers.oracle_policy does"""
    th.manual_seed(seed)
    obs_s, act_s = H.CONFIGS[name]
    pol = ArchPolicyOracle(obs_s, act_s, widths)
    g = th.Generator().manual_seed(seed + 1)
    with th.no_grad():
        for p in pol.parameters():
            if p.ndim == 1:
                p.add_(perturb * th.randn(p.shape, generator=g))
        pol.action_net.weight.add_(perturb * th.randn(pol.action_net.weight.shape, generator=g))
    return pol


def device_policy(name: str, oracle: ArchPolicyOracle):
    from pantheonrl_amd.ppo import ArchActorCriticPolicy
    obs_s, act_s = H.CONFIGS[name]
    pol = ArchActorCriticPolicy(H.to_space(obs_s), H.to_space(act_s, "act"), net_arch=oracle.widths, device="cuda", seed=0)
    pol.set_flat_params(oracle.flat_params())
    return pol


def space_env(name: str):
    obs_s, act_s = H.CONFIGS[name]
    return type("E", (), dict(observation_space=H.to_space(obs_s), action_space=H.to_space(act_s, "act"), _is_dummy_space_env=True))()


def kwargs_of(widths) -> dict:
    return {"net_arch": [dict(pi=list(widths), vf=list(widths))]}


# the checker's Adam state in ArchPolicyOracle.flat_params()'s order: helpers' functions read the layout off flat_params() itself
flat_adam_state = H.flat_adam_state
load_flat_adam_state = H.load_flat_adam_state
