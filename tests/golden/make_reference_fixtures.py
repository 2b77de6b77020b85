"""Pins the host-side rows of the hot path AND the update loops (a7, a8, f4: ADAP.train = SB3's
PPO.train loop, ModularAlgorithm.train, BC.train, with their policies' text) to the REFERENCE's own Python text.
Build container only: `/root/reference` never travels, the fixtures this script writes do.

    python tests/golden/make_reference_fixtures.py            # regenerate in memory, compare byte for byte with the committed files
    python tests/golden/make_reference_fixtures.py --write    # (re)write tests/golden/ref_*.json, ref_transitions.npz, ref_adap_context.npz,
                                                              # ref_ppo_train.npz, ref_modular.npz, ref_bc.npz and
                                                              # ref_fixtures_sha256.json (their digests, checked by the not-gpu test)

What runs is the reference's source, imported from where it lies (nothing is copied into this repository):

    pantheonrl/common/multiagentenv.py   MultiAgentEnv.step/reset/_get_actions/_update_players, resampling, TurnBasedEnv, SimultaneousEnv
    pantheonrl/common/agents.py          OnPolicyAgent.__init__/get_action/update (:92-203)
    pantheonrl/common/observation.py     Observation, extract_obs, extract_partial_obs
    pantheonrl/common/util.py            action_from_policy, clip_actions, resample_noise, get_space_size, calculate_space, get_default_obs
    pantheonrl/common/wrappers.py        HistoryQueue, the frame-stack wrappers, the recorders
    pantheonrl/common/trajsaver.py       TransitionsMinimal / TurnBasedTransitions / SimultaneousTransitions (.npy wire format)
    pantheonrl/algos/adap/util.py        SAMPLERS, kl_divergence, get_context_kl_loss
    pantheonrl/algos/adap/adap_learn.py  ADAP.train (:229-371) -- the in-tree text of SB3's PPO.train() loop (+ the context term): SURVEY.md
                                         section 8 row a8's arithmetic and row f4's ADAP variant
    pantheonrl/algos/adap/policies.py    AdapPolicy.__init__/set_context/get_context/_get_latent/evaluate_actions (:20-135)
    pantheonrl/algos/modular/policies.py ModularPolicy: constructor defaults, _build, do_init_weights, evaluate_actions, _get_action_dist_from_latent
                                         (mask offset), get_action_logits_from_obs (:57-395)
    pantheonrl/algos/modular/learn.py    ModularAlgorithm.train (:221-351)
    trainer.py (as __main__)             argument parser, preset, input_check, latent_check; generate_env / generate_ego / gen_partner /
                                         generate_partners and the learn / record / save tail on recording doubles (:41-432)
    pantheonrl/envs/pettingzoo.py        PettingZooAECWrapper.__init__ / n_reset / n_step (:27-127): the action the environment is stepped with
                                         when the sample is illegal under the mask (`gymnasium` = five space class NAMES; a scripted AEC env)
    pantheonrl/algos/bc.py               BC.__init__ (optimizer construction), set_expert_data_loader, _calculate_loss, train,
                                         EpochOrBatchIteratorWithProgress (:67-365); common/util.py FeedForward32Policy (:114-123);
                                         common/trajsaver.py TransitionsMinimal.__getitem__ / transitions_collate_fn under torch's DataLoader

`pantheonrl/__init__.py` (which registers gym environments) is bypassed by pre-seating an empty package object whose __path__ is the
reference's directory.  Those files import `gym` and `stable_baselines3`, absent here; they are satisfied by INERT stand-ins for
exactly the names imported.  For the host-side rows (fixtures ref_*.json, ref_transitions.npz, ref_adap_context.npz) none of them
contributes a rule or arithmetic to what is recorded:

    gym.Env                                   empty base class
    gym.spaces.{Space,Box,Discrete,MultiBinary,MultiDiscrete}   holders of .low/.high/.shape/.dtype/.n/.nvec (constructor arguments kept)
    stable_baselines3.common.utils.configure_logger             returns None (the recording model installs its own recorder)
    stable_baselines3.common.utils.safe_mean                    returns {"safe_mean_of": <the list it was handed>}: the arithmetic is NOT done
                                                                here; the test applies SB3's published definition to the recorded list
    stable_baselines3.common.utils.obs_as_tensor                th.as_tensor(obs).to(device)   (SB3's behaviour for an ndarray)
    stable_baselines3.common.utils.should_collect_more_steps    never called on this path
    stable_baselines3.common.{policies,base_class,on_policy_algorithm,off_policy_algorithm}    class NAMES only (type annotations / bases)
    stable_baselines3.common.distributions.{Distribution,CategoricalDistribution,MultiCategoricalDistribution}
                                              holders of `.distribution` (torch.distributions.Categorical objects built by the TEST's model)
    stable_baselines3.common.buffers.RolloutBufferSamples       the namedtuple of that name (fields as SB3 1.7.0 publishes them)

For ADAP.train / AdapPolicy (fixture ref_ppo_train.npz) additionally -- names for imports, annotations and base classes, plus exactly
four pieces of behaviour, each SB3 1.7.0's published definition restated in one line and listed here because it is NOT the reference's text:

    stable_baselines3.common.{type_aliases,vec_env,callbacks,torch_layers,preprocessing,logger}, stable_baselines3.PPO, gym.Space,
    buffers.RolloutBuffer, utils.{get_schedule_fn,is_vectorized_observation}, distributions.{DiagGaussian,Bernoulli,StateDependentNoise}Distribution
                                              NAMES only (imports, annotations, isinstance checks that are false here; never called)
    stable_baselines3.common.policies.ActorCriticPolicy        base class whose __init__ only KEEPS the arguments the subclass's text hands up;
                                              the network (MlpExtractor 64-64 tanh, action_net, value_net, Adam(eps=1e-5)) is the TEST's
                                              torch module (oracle.MlpPolicyOracle), attached by the test's subclass
    stable_baselines3.common.utils.explained_variance          returns {"explained_variance_of": shapes}: logged only, arithmetic NOT done here
    CategoricalDistribution.log_prob / .entropy                 self.distribution.log_prob(actions) / self.distribution.entropy()
    MultiCategoricalDistribution.log_prob / .entropy            stack over the components (actions unbound along dim 1), summed along dim 1
    algo._update_learning_rate(optimizer)                       sets every param group's lr to the constant the case names (SB3 with a constant schedule)
    algo.rollout_buffer.get(batch_size)                         env-major flattening + slicing of the per-epoch index orders the TEST provides
                                              (np.random.permutation teacher-forced), yielding RolloutBufferSamples of torch tensors

For ModularPolicy (fixture ref_modular.npz), which BUILDS its network from SB3 classes, those classes are restated (SB3 1.7.0's definitions):

    policies.BasePolicy                       nn.Module keeping the spaces / optimizer class + kwargs; init_weights = orthogonal_(weight, gain) and
                                              bias 0 for Linear layers; extract_features = features_extractor(obs.float()); device = cpu
    torch_layers.FlattenExtractor             features_dim = prod(shape), nn.Flatten
    torch_layers.MlpExtractor                 net_arch [dict(pi=[..], vf=[..])] -> two separate Linear + activation towers, latent_dim_pi / _vf
    distributions.make_proba_distribution     Discrete(n) -> CategoricalDistribution(n); .proba_distribution_net = nn.Linear(latent, n);
                                              .proba_distribution(action_logits) = torch Categorical(logits=...)
    optimizer.zero_grad()                     forwarded as zero_grad(set_to_none=False): the default of the torch the reference pins (setup.py:15)

For BC (fixture ref_bc.npz): utils.get_device -> cpu; the module-level `log` (utils.configure_logger's result) is replaced by a recorder;
the policy class handed to BC is the TEST's subclass of the reference's FeedForward32Policy over oracle.FeedForward32Oracle (SB3's
`net_arch=[32, 32]` = a shared 32-32 tanh trunk: the constructor argument the reference's text passes up is recorded and checked).

The scenarios themselves (scripted games, recording partners, the recording model) are tests/refdrive.py -- shared with the tests
that replay them through pantheonrl_amd.common.
"""
from __future__ import annotations

import hashlib
import importlib
import io
import json
import os
import sys
import types
from collections import deque, namedtuple
from itertools import combinations

import numpy as np
import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
REFERENCE = os.environ.get("PANTHEON_REFERENCE", "/root/reference")
os.environ.setdefault("TQDM_DISABLE", "1")      # bc.py's progress bars (read when tqdm is first imported)

from tests import refdrive as rd  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------------
# stand-ins + loader
# ---------------------------------------------------------------------------------------------------------------------------
def inert_spaces() -> types.ModuleType:
    sp = types.ModuleType("gym.spaces")

    class Space:
        shape, dtype = (), None

    class Box(Space):
        def __init__(self, low, high, shape=None, dtype=np.float32):
            self.shape = tuple(np.shape(low) if shape is None else shape)
            self.dtype = np.dtype(dtype)
            self.low = np.broadcast_to(np.asarray(low, dtype), self.shape).copy()
            self.high = np.broadcast_to(np.asarray(high, dtype), self.shape).copy()

    class Discrete(Space):
        def __init__(self, n):
            self.n, self.shape, self.dtype = int(n), (), np.dtype(np.int64)

    class MultiBinary(Space):
        def __init__(self, n):
            self.n, self.shape, self.dtype = int(n), (int(n),), np.dtype(np.int8)

    class MultiDiscrete(Space):
        def __init__(self, nvec):
            self.nvec = np.asarray(nvec, np.int64)
            self.shape, self.dtype = (len(self.nvec),), np.dtype(np.int64)

    for c in (Space, Box, Discrete, MultiBinary, MultiDiscrete):
        setattr(sp, c.__name__, c)
    return sp


def _stand_ins() -> dict:
    mods = {}

    def mod(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        mods[name] = m
        return m

    spaces = inert_spaces()
    mods["gym.spaces"] = spaces
    mod("gym", Env=type("Env", (), {}), spaces=spaces, Space=spaces.Space)

    def name_only(n):
        return type(n, (), {})

    class Distribution:
        def __init__(self, distribution=None):
            self.distribution = distribution

    class CategoricalDistribution(Distribution):              # SB3 1.7.0 distributions.py: log_prob / entropy delegate to torch's Categorical
        def log_prob(self, actions):
            return self.distribution.log_prob(actions)

        def entropy(self):
            return self.distribution.entropy()

    class MultiCategoricalDistribution(Distribution):         # ... and the MultiCategorical sums its components' along dim 1
        def log_prob(self, actions):
            return th.stack([d.log_prob(a) for d, a in zip(self.distribution, th.unbind(actions, dim=1))], dim=1).sum(dim=1)

        def entropy(self):
            return th.stack([d.entropy() for d in self.distribution], dim=1).sum(dim=1)

    class ActorCriticPolicy:                                  # base of AdapPolicy / FeedForward32Policy: takes its constructor's arguments
        def __init__(self, *args, **kwargs):                  # and only KEEPS them (what the subclass's text handed up is checked by tests)
            self.init_args, self.init_kwargs = args, kwargs

    # -- ModularPolicy (modular/policies.py) BUILDS its network from SB3 classes: each restated below in its SB3 1.7.0 definition --
    def _categorical_init(self, arg=None):                    # CategoricalDistribution(action_dim) | the holder form used above
        if isinstance(arg, (int, np.integer)):
            self.action_dim, self.distribution = int(arg), None
        else:
            self.distribution = arg
    CategoricalDistribution.__init__ = _categorical_init
    CategoricalDistribution.proba_distribution_net = lambda self, latent_dim: th.nn.Linear(latent_dim, self.action_dim)

    def _proba_distribution(self, action_logits):
        self.distribution = th.distributions.Categorical(logits=action_logits)
        return self
    CategoricalDistribution.proba_distribution = _proba_distribution

    def make_proba_distribution(action_space, use_sde=False, dist_kwargs=None):
        assert isinstance(action_space, spaces.Discrete) and not use_sde
        return CategoricalDistribution(action_space.n)

    class BasePolicy(th.nn.Module):
        def __init__(self, observation_space, action_space, features_extractor_class=None, features_extractor_kwargs=None,
                     features_extractor=None, normalize_images=True, optimizer_class=th.optim.Adam, optimizer_kwargs=None,
                     squash_output=False):
            super().__init__()
            self.observation_space, self.action_space = observation_space, action_space
            self.features_extractor_class, self.features_extractor_kwargs = features_extractor_class, features_extractor_kwargs or {}
            self.optimizer_class, self.optimizer_kwargs, self.optimizer = optimizer_class, optimizer_kwargs or {}, None

        device = property(lambda self: th.device("cpu"))

        @staticmethod
        def init_weights(module, gain=1):                     # SB3 BasePolicy.init_weights
            if isinstance(module, (th.nn.Linear, th.nn.Conv2d)):
                th.nn.init.orthogonal_(module.weight, gain=gain)
                if module.bias is not None:
                    module.bias.data.fill_(0.0)

        def extract_features(self, obs):                      # preprocess_obs of a Box observation (obs.float()), then the extractor
            return self.features_extractor(obs.float())

    class FlattenExtractor(th.nn.Module):
        def __init__(self, observation_space):
            super().__init__()
            self.features_dim, self.flatten = int(np.prod(observation_space.shape)), th.nn.Flatten()

        def forward(self, observations):
            return self.flatten(observations)

    class MlpExtractor(th.nn.Module):                         # net_arch [dict(pi=[..], vf=[..])]: two separate towers, nothing shared
        def __init__(self, feature_dim, net_arch, activation_fn, device="auto"):
            super().__init__()
            assert len(net_arch) == 1 and isinstance(net_arch[0], dict)

            def tower(widths):
                layers, d = [], feature_dim
                for w in widths:
                    layers += [th.nn.Linear(d, w), activation_fn()]
                    d = w
                return th.nn.Sequential(*layers), d
            self.policy_net, self.latent_dim_pi = tower(net_arch[0]["pi"])
            self.value_net, self.latent_dim_vf = tower(net_arch[0]["vf"])

        def forward(self, features):
            return self.policy_net(features), self.value_net(features)

    utils = mod("stable_baselines3.common.utils",
                configure_logger=lambda *a, **k: None,
                safe_mean=lambda arr: {"safe_mean_of": rd.plain(list(arr))},
                obs_as_tensor=lambda obs, device: th.as_tensor(obs).to(device),
                should_collect_more_steps=None, get_schedule_fn=None, get_device=lambda device="auto": th.device("cpu"),
                is_vectorized_observation=None,
                explained_variance=lambda y_pred, y_true: {"explained_variance_of": [list(np.shape(y_pred)), list(np.shape(y_true))]})
    policies = mod("stable_baselines3.common.policies", ActorCriticPolicy=ActorCriticPolicy, BasePolicy=BasePolicy)
    onp = mod("stable_baselines3.common.on_policy_algorithm", OnPolicyAlgorithm=name_only("OnPolicyAlgorithm"))
    offp = mod("stable_baselines3.common.off_policy_algorithm", OffPolicyAlgorithm=name_only("OffPolicyAlgorithm"))
    base = mod("stable_baselines3.common.base_class", BaseAlgorithm=name_only("BaseAlgorithm"))
    dist = mod("stable_baselines3.common.distributions", Distribution=Distribution,
               CategoricalDistribution=CategoricalDistribution, MultiCategoricalDistribution=MultiCategoricalDistribution,
               make_proba_distribution=make_proba_distribution, DiagGaussianDistribution=name_only("DiagGaussianDistribution"),
               BernoulliDistribution=name_only("BernoulliDistribution"),
               StateDependentNoiseDistribution=name_only("StateDependentNoiseDistribution"))
    bufs = mod("stable_baselines3.common.buffers", RolloutBuffer=name_only("RolloutBuffer"), RolloutBufferSamples=namedtuple(
        "RolloutBufferSamples", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns"]))
    aliases = mod("stable_baselines3.common.type_aliases", GymEnv=name_only("GymEnv"), MaybeCallback=name_only("MaybeCallback"),
                  Schedule=name_only("Schedule"))
    vec_env = mod("stable_baselines3.common.vec_env", VecEnv=name_only("VecEnv"), VecTransposeImage=name_only("VecTransposeImage"))
    sb3_logger = mod("stable_baselines3.common.logger")
    callbacks = mod("stable_baselines3.common.callbacks", BaseCallback=name_only("BaseCallback"))
    layers = mod("stable_baselines3.common.torch_layers", BaseFeaturesExtractor=name_only("BaseFeaturesExtractor"),
                 FlattenExtractor=FlattenExtractor, MlpExtractor=MlpExtractor, create_mlp=None, NatureCNN=name_only("NatureCNN"))
    prep = mod("stable_baselines3.common.preprocessing", preprocess_obs=None, is_image_space=None, get_action_dim=None)
    common = mod("stable_baselines3.common", utils=utils, policies=policies, on_policy_algorithm=onp, off_policy_algorithm=offp,
                 base_class=base, distributions=dist, buffers=bufs, type_aliases=aliases, vec_env=vec_env, callbacks=callbacks,
                 torch_layers=layers, preprocessing=prep, logger=sb3_logger)
    mod("stable_baselines3", common=common, PPO=name_only("PPO"))
    pkg = types.ModuleType("pantheonrl")
    pkg.__path__ = [os.path.join(REFERENCE, "pantheonrl")]        # the reference's files, in place; its __init__.py is not run
    mods["pantheonrl"] = pkg
    return mods


class ReferenceModules:
    """context manager: the reference's modules importable under `pantheonrl.*`, sys.modules restored afterwards"""

    NAMES = ("common.observation", "common.util", "common.trajsaver", "common.agents", "common.multiagentenv", "common.wrappers",
             "algos.adap.util", "algos.adap.policies", "algos.adap.adap_learn", "algos.modular.policies", "algos.modular.learn",
             "algos.bc")

    def __enter__(self):
        self._stand = _stand_ins()
        self._saved = {k: sys.modules.get(k) for k in self._stand}
        self._before = set(sys.modules)
        sys.modules.update(self._stand)
        self.m = {n: importlib.import_module("pantheonrl." + n) for n in self.NAMES}
        for n, m in self.m.items():
            assert os.path.abspath(m.__file__).startswith(os.path.abspath(REFERENCE)), (n, m.__file__)
        return self

    def __exit__(self, *exc):
        for k in set(sys.modules) - self._before:
            if k.startswith(("pantheonrl", "gym", "stable_baselines3")):
                sys.modules.pop(k, None)
        for k, v in self._saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v

    def framework(self) -> types.SimpleNamespace:
        fw = types.SimpleNamespace()
        for m in self.m.values():
            for k, v in vars(m).items():
                if not k.startswith("_") and getattr(v, "__module__", None) == m.__name__:
                    setattr(fw, k, v)
        return fw

    @property
    def spaces(self):
        return self._stand["gym.spaces"]


# ---------------------------------------------------------------------------------------------------------------------------
# (v) ADAP: samplers and get_context_kl_loss of the reference, run on a model the TEST provides
# ---------------------------------------------------------------------------------------------------------------------------
ADAP_CASES = {"discrete6": dict(F=5, nvec=(6,), ctx=3, B=24, n_ctx=5, n_states=8, sampler="l2", seed=11),
              "multi_7_12": dict(F=4, nvec=(7, 12), ctx=4, B=40, n_ctx=4, n_states=64, sampler="unit_square", seed=12),
              "two_contexts": dict(F=6, nvec=(5,), ctx=2, B=16, n_ctx=2, n_states=16, sampler="positive_square", seed=13)}


def adap_case_inputs(c: dict):
    """(flat parameters in the oracle's layout, minibatch observations features ++ context) -- seeded test inputs"""
    from oracle import sb3_oracle as orc
    th.manual_seed(c["seed"])
    act = orc.SpaceSpec("discrete", nvec=c["nvec"]) if len(c["nvec"]) == 1 else orc.SpaceSpec("multidiscrete", nvec=c["nvec"])
    net = orc.MlpPolicyOracle(orc.SpaceSpec("box", dim=c["F"] + c["ctx"]), act)
    rng = np.random.default_rng(c["seed"])
    flat = net.flat_params() + 0.2 * rng.standard_normal(net.flat_params().shape).astype(np.float32)
    net.load_flat_params(flat)
    obs = rng.standard_normal((c["B"], c["F"] + c["ctx"])).astype(np.float32)
    obs[:, 0] = np.arange(c["B"])            # rows identifiable: lets the recorder recover th.randperm's draw
    return net, flat.astype(np.float32), obs


def adap_reference_run(util_mod, dist_mod, c: dict) -> dict:
    net, flat, obs = adap_case_inputs(c)
    seen = {"contexts": [], "states": None}

    class Model:                                         # the surface get_context_kl_loss touches (adap/util.py:108-127)
        context = th.zeros(1, c["ctx"])

        def get_context(self):
            return self.context

        def set_context(self, ctxt):
            self.context = ctxt

        def _get_latent(self, states):                   # AdapPolicy._get_latent: features ++ context (adap/policies.py:104-119)
            if seen["states"] is None:
                seen["states"] = states.detach().numpy().copy()
            seen["contexts"].append(self.context.detach().numpy().copy())
            feats = th.cat((states, self.context.reshape(1, -1).repeat(states.shape[0], 1)), dim=1)
            return net._latents(feats)[0], None, None

        def _get_action_dist_from_latent(self, latent_pi, latent_sde=None):
            logits = net.action_net(latent_pi)
            if len(c["nvec"]) == 1:
                return dist_mod.CategoricalDistribution(th.distributions.Categorical(logits=logits))
            return dist_mod.MultiCategoricalDistribution([th.distributions.Categorical(logits=z) for z in net._split(logits)])

    algo = types.SimpleNamespace(context_size=c["ctx"], num_context_samples=c["n_ctx"], num_state_samples=c["n_states"],
                                 context_sampler=c["sampler"])
    batch = sys.modules["stable_baselines3.common.buffers"].RolloutBufferSamples(th.as_tensor(obs), None, None, None, None, None)
    model = Model()
    keep = model.context
    th.manual_seed(100 + c["seed"])
    loss = util_mod.get_context_kl_loss(algo, model, batch)
    assert model.context is keep                          # util.py:127: the rollout's context is restored
    for p in net.parameters():                            # the value tower takes no gradient from this term: explicit zeros
        p.grad = th.zeros_like(p)
    loss.backward()
    state_idx = seen["states"][:, 0].astype(np.int64)
    return {"params": flat, "observations": obs, "state_idx": state_idx, "contexts": np.concatenate(seen["contexts"], 0),
            "loss": np.float32(loss.item()), "grad": net.flat_grads().astype(np.float32)}


def adap_sampler_run(util_mod) -> dict:
    """every SAMPLERS entry, torch and numpy flavour, under a fixed seed; `uniforms` = what th.rand yields for the same seed and
    shape (the float samplers are deterministic functions of it, util.py:42-67)"""
    out = {}
    for name, fn in util_mod.SAMPLERS.items():
        for ctx, num in ((3, 4), (1, 5)):
            key = f"{name}_{ctx}x{num}"
            th.manual_seed(7)
            out[key + "_torch"] = np.asarray(fn(ctx_size=ctx, num=num, torch=True).numpy())
            np.random.seed(7)
            out[key + "_numpy"] = np.asarray(fn(ctx_size=ctx, num=num, torch=False))
            th.manual_seed(7)
            out[key + "_uniforms"] = th.rand(num, ctx).numpy()
    return out



# ---------------------------------------------------------------------------------------------------------------------------
# (vi) the reference's ADAP.train TEXT (adap_learn.py:229-371 = SB3's PPO.train loop + the context term) and AdapPolicy's
#      evaluate_actions / _get_latent TEXT (adap/policies.py:97-135), run on a network, a buffer and index orders the TEST provides
# ---------------------------------------------------------------------------------------------------------------------------
TRAIN_CASES = {
    # context_loss_coeff = 0: the loss is PPO's (policy + ent_coef * entropy + vf_coef * value; the term's gradient is exactly 0) -- what
    # pantheonrl_amd.PPO.train computes on a Box(F + ctx) observation
    "ppo_discrete6": dict(F=9, ctx=3, nvec=(6,), T=16, E=4, batch=16, epochs=3, lr=3e-4, clip=0.2, clip_vf=None, ent=0.01, vf=0.5,
                          max_norm=0.5, target_kl=None, coef=0.0, n_ctx=5, n_states=32, sampler="l2", seed=21),
    # value clipping, a learning rate that moves the ratio out of the clip range, and the KL early stop at the second minibatch of epoch 2 (approx_kl 0.0845 > 1.5 x 0.052 after 0.0737 passed)
    "ppo_clipvf_klstop": dict(F=17, ctx=3, nvec=(5,), T=12, E=8, batch=32, epochs=4, lr=3e-3, clip=0.1, clip_vf=0.2, ent=0.0, vf=0.5,
                              max_norm=0.5, target_kl=0.052, coef=0.0, n_ctx=2, n_states=4, sampler="l2", seed=22),
    # ADAP as the reference constructs it (adap_learn.py:111-116 defaults), a ragged last minibatch (96 = 40 + 40 + 16)
    "adap_discrete6": dict(F=9, ctx=3, nvec=(6,), T=16, E=6, batch=40, epochs=3, lr=3e-4, clip=0.2, clip_vf=None, ent=0.0, vf=0.5,
                           max_norm=0.5, target_kl=None, coef=0.1, n_ctx=5, n_states=32, sampler="l2", seed=23),
    "adap_multi_7_12": dict(F=12, ctx=4, nvec=(7, 12), T=10, E=6, batch=30, epochs=2, lr=1e-3, clip=0.2, clip_vf=None, ent=0.01, vf=0.5,
                            max_norm=0.5, target_kl=None, coef=1.0, n_ctx=4, n_states=16, sampler="unit_square", seed=24),
}


def train_case_inputs(c: dict):
    """-> (network, its flat parameters, a full RolloutBufferOracle as the data holder, per-epoch index orders).  Seeded test inputs:
    rollout rows are N(0, 1) features ++ the environment's current context (resampled at episode starts, adap_learn.py:448-458), actions /
    values / log-probs are the network's own on those rows, rewards N(0, 1); advantages / returns by the buffer's GAE."""
    from oracle import sb3_oracle as orc
    th.manual_seed(c["seed"])
    D, A = c["F"] + c["ctx"], len(c["nvec"])
    act = orc.SpaceSpec("discrete", nvec=c["nvec"]) if A == 1 else orc.SpaceSpec("multidiscrete", nvec=c["nvec"])
    net = orc.MlpPolicyOracle(orc.SpaceSpec("box", dim=D), act, lr=c["lr"])
    rng = np.random.default_rng(c["seed"])
    flat = (net.flat_params() + 0.2 * rng.standard_normal(net.flat_params().shape)).astype(np.float32)
    net.load_flat_params(flat)
    T, E = c["T"], c["E"]
    buf = orc.RolloutBufferOracle(T, E, D, A)
    starts = np.ones(E, np.float32)
    ctx = np.zeros((E, c["ctx"]), np.float32)
    values = None
    for _ in range(T):
        for e in np.nonzero(starts)[0]:
            ctx[e] = orc.adap_sample_contexts(c["sampler"], c["ctx"], 1, rng.random((1, c["ctx"])))[0]
        obs = np.concatenate([rng.standard_normal((E, c["F"])).astype(np.float32), ctx], axis=1)
        with th.no_grad():
            actions, values, logp = net.forward(th.as_tensor(obs), uniforms=th.as_tensor(rng.random((E, A)).astype(np.float32)))
        buf.add(obs, actions.numpy(), rng.standard_normal(E).astype(np.float32), starts, values, logp)
        starts = (rng.random(E) < 0.1).astype(np.float32)
    buf.compute_returns_and_advantage(values, starts)
    perms = np.stack([rng.permutation(T * E) for _ in range(c["epochs"])]).astype(np.int64)
    return net, flat, buf, perms


def train_reference_run(ref: "ReferenceModules", c: dict) -> dict:
    learn_mod, pol_mod = ref.m["algos.adap.adap_learn"], ref.m["algos.adap.policies"]
    dist_mod = sys.modules["stable_baselines3.common.distributions"]
    Samples = sys.modules["stable_baselines3.common.buffers"].RolloutBufferSamples
    net, flat, buf, perms = train_case_inputs(c)
    cs, A = c["ctx"], len(c["nvec"])
    cur = {"features": None, "calls": 0}
    seen = {"state_idx": [], "contexts": []}

    class Policy(pol_mod.AdapPolicy):
        """the reference's AdapPolicy TEXT (set_context / get_context / _get_latent / evaluate_actions) over the test's network"""

        def __init__(self):
            pol_mod.AdapPolicy.__init__(self, None, None, None, context_size=cs)       # reference text: keeps context_size, calls the base
            self.sde_features_extractor = None
            self.value_net = net.value_net
            self.context = th.zeros(1, cs)                                             # the rollout's context (restored by util.py:127)

        def extract_features(self, obs):                   # FlattenExtractor on a flat Box observation: the identity
            if cur["calls"] > 0:                            # call 0 of a minibatch is evaluate_actions; 1.. are get_context_kl_loss's
                feats = obs.detach().numpy()
                if cur["calls"] == 1:
                    rows = [int(np.nonzero((cur["features"] == f).all(axis=1))[0][0]) for f in feats]
                    seen["state_idx"][-1][:len(rows)] = rows
                seen["contexts"][-1].append(self.context.detach().numpy().reshape(-1).copy())
            cur["calls"] += 1
            return obs

        def mlp_extractor(self, features):                  # SB3's default MlpExtractor: two 64-64 tanh towers
            return net.policy_net(features), net.value_net_mlp(features)

        def _get_action_dist_from_latent(self, latent_pi, latent_sde=None):
            logits = net.action_net(latent_pi)
            if A == 1:
                return dist_mod.CategoricalDistribution(th.distributions.Categorical(logits=logits))
            return dist_mod.MultiCategoricalDistribution([th.distributions.Categorical(logits=z) for z in net._split(logits)])

        def parameters(self):
            return net.parameters()

    steps = {"params": [], "grads": []}

    class OptimizerTap:                                     # torch.optim.Adam(eps=1e-5) of the network, every step recorded
        param_groups = net.optimizer.param_groups

        def zero_grad(self):
            net.optimizer.zero_grad()

        def step(self):
            steps["grads"].append(net.flat_grads())         # after clip_grad_norm_
            net.optimizer.step()
            steps["params"].append(net.flat_params())

    class Buffer:                                           # sampling only: env-major flattening, the test's index orders, slicing
        values, returns = buf.values, buf.returns

        def __init__(self):
            self.epoch = 0

        def get(self, batch_size):
            order = perms[self.epoch]
            self.epoch += 1
            for mb in buf.get(batch_size, order):
                cur["features"], cur["calls"] = mb["observations"].numpy()[:, :-cs], 0
                seen["state_idx"].append(np.full(c["n_states"], -1, np.int32))
                seen["contexts"].append([])
                yield Samples(mb["observations"], mb["actions"], mb["old_values"], mb["old_log_prob"], mb["advantages"], mb["returns"])

    class Logger:
        def __init__(self):
            self.kv = {}

        def record(self, key, value, exclude=None):
            self.kv[key] = value

    policy = Policy()
    policy.optimizer = OptimizerTap()

    def set_lr(optimizer):
        for g in optimizer.param_groups:
            g["lr"] = c["lr"]

    space = ref.spaces.Discrete(c["nvec"][0]) if A == 1 else ref.spaces.MultiDiscrete(list(c["nvec"]))
    algo = types.SimpleNamespace(
        policy=policy, rollout_buffer=Buffer(), n_epochs=c["epochs"], batch_size=c["batch"], action_space=space, use_sde=False,
        ent_coef=c["ent"], vf_coef=c["vf"], context_loss_coeff=c["coef"], target_kl=c["target_kl"], verbose=0, max_grad_norm=c["max_norm"],
        _n_updates=0, logger=Logger(), clip_range=lambda progress: c["clip"],
        clip_range_vf=None if c["clip_vf"] is None else (lambda progress: c["clip_vf"]), _current_progress_remaining=1.0,
        _update_learning_rate=set_lr, context_size=cs, num_context_samples=c["n_ctx"], num_state_samples=c["n_states"],
        context_sampler=c["sampler"])
    th.manual_seed(1000 + c["seed"])
    learn_mod.ADAP.train(algo)                              # <- the reference's text
    n_steps, n_mb_seen = len(steps["params"]), len(seen["state_idx"])
    assert n_steps >= 2 and algo._n_updates == c["epochs"]
    flatbuf = buf.flat()
    out = {"params0": flat, "perms": perms, "n_steps": np.int64(n_steps), "n_minibatches_seen": np.int64(n_mb_seen),
           "observations": buf.observations, "actions": buf.actions, "values": buf.values, "log_probs": buf.log_probs,
           "advantages": buf.advantages, "returns": buf.returns, "rewards": buf.rewards, "episode_starts": buf.episode_starts,
           "params_step1": steps["params"][0], "grads_step1": steps["grads"][0], "params_final": steps["params"][-1],
           "state_idx": np.stack(seen["state_idx"]),
           "contexts": np.stack([np.stack(x) for x in seen["contexts"]]).astype(np.float32)}
    assert out["contexts"].shape == (n_mb_seen, c["n_ctx"], cs) and flatbuf["observations"].shape[0] == c["T"] * c["E"]
    for k, v in algo.logger.kv.items():
        if isinstance(v, dict):                             # explained_variance's marker: nothing to keep
            continue
        out["log." + k] = np.float64(v)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# (vii) the reference's ModularPolicy TEXT (modular/policies.py:57-395: constructor defaults, _build, do_init_weights' gains,
#       evaluate_actions, the mask offset of _get_action_dist_from_latent, get_action_logits_from_obs) and ModularAlgorithm.train
#       TEXT (modular/learn.py:221-351: the PPO terms per partner + the marginal regulariser, the per-epoch KL rule)
# ---------------------------------------------------------------------------------------------------------------------------
MODULAR_CASES = {
    "two_partners": dict(D=20, n_act=6, K=2, T=8, E=8, batch=16, epochs=2, lr=3e-4, clip=0.2, clip_vf=None, ent=0.01, vf=0.5,
                         max_norm=0.5, target_kl=None, coef=0.5, kw={}, seed=31),
    # lr moves the policy fast: partner 0's second epoch exceeds 1.5 x target_kl and ends ITS epochs; partners 1, 2 start afresh
    "three_partners_klstop": dict(D=12, n_act=5, K=3, T=8, E=6, batch=24, epochs=4, lr=3e-3, clip=0.2, clip_vf=0.3, ent=0.0, vf=0.5,
                                  max_norm=0.5, target_kl=0.02, coef=0.0, kw={}, seed=32),
    "nomain": dict(D=9, n_act=4, K=2, T=8, E=4, batch=32, epochs=2, lr=1e-3, clip=0.2, clip_vf=None, ent=0.01, vf=0.5,
                   max_norm=0.5, target_kl=None, coef=0.4, kw={"nomain": True}, seed=33),
}


def modular_flat(pol, grads: bool = False) -> np.ndarray:
    """parameters of a REFERENCE ModularPolicy in the product's order: main network [pi_W1 pi_b1 pi_W2 pi_b2 vf_W1 vf_b1 vf_W2 vf_b2
    act_W act_b val_W val_b], then the same twelve blocks per partner module; weights input-major"""
    def vec(t, transpose):
        x = t.grad if grads else t.detach()
        x = th.zeros_like(t) if x is None else x
        return (x.t() if transpose else x).contiguous().reshape(-1)

    def module(ext, act, val):
        out = []
        for seq in (ext.policy_net, ext.value_net):
            for i in (0, 2):
                out += [vec(seq[i].weight, True), vec(seq[i].bias, False)]
        return out + [vec(act.weight, True), vec(act.bias, False), vec(val.weight, False), vec(val.bias, False)]
    out = module(pol.mlp_extractor, pol.action_net, pol.value_net)
    for k in range(pol.num_partners):
        out += module(pol.partner_mlp_extractor[k], pol.partner_action_net[k], pol.partner_value_net[k])
    return th.cat(out).numpy().astype(np.float32).copy()


def load_modular_oracle(c: dict, flat: np.ndarray):
    """an oracle.ModularPolicyOracle holding `flat` (modular_flat's order)"""
    from oracle import sb3_oracle as orc
    net = orc.ModularPolicyOracle(orc.SpaceSpec("box", dim=c["D"]), orc.SpaceSpec("discrete", nvec=(c["n_act"],)), num_partners=c["K"],
                                  lr=c["lr"], **c["kw"])
    t, o = th.as_tensor(flat), 0

    def take(p, transpose):
        nonlocal o
        n = p.numel()
        v = t[o:o + n]
        o += n
        with th.no_grad():
            p.copy_(v.reshape(p.shape[1], p.shape[0]).t() if transpose else v.reshape(p.shape))

    def module(pi, vf, act, val):
        for seq in (pi, vf):
            for i in (0, 2):
                take(seq[i].weight, True)
                take(seq[i].bias, False)
        take(act.weight, True)
        take(act.bias, False)
        take(val.weight, False)
        take(val.bias, False)
    module(net.policy_net, net.value_net_mlp, net.action_net, net.value_net)
    for pm in net.partners:
        module(pm["pi"], pm["vf"], pm["act"], pm["val"])
    assert o == t.numel()
    return net


def modular_reference_run(ref: "ReferenceModules", c: dict) -> dict:
    import contextlib
    from oracle import sb3_oracle as orc
    pol_mod, learn_mod = ref.m["algos.modular.policies"], ref.m["algos.modular.learn"]
    Samples = sys.modules["stable_baselines3.common.buffers"].RolloutBufferSamples
    spaces = ref.spaces
    K, D, T, E = c["K"], c["D"], c["T"], c["E"]
    th.manual_seed(c["seed"])
    with contextlib.redirect_stdout(io.StringIO()):            # (the constructor prints "CUDA: ...")
        pol = pol_mod.ModularPolicy(spaces.Box(-np.inf, np.inf, (D,)), spaces.Discrete(c["n_act"]), lambda progress: c["lr"],
                                    num_partners=K, **c["kw"])  # <- the reference's text: defaults, _build, do_init_weights
    # what _build + do_init_weights left (policies.py:221-267): per Linear layer, in modular_flat's module order, the extreme singular
    # values of its weight (an orthogonal init with gain g has all of them = g) and the largest |bias|; Adam's eps (:84-88)
    lins = []
    for ext, act, val in [(pol.mlp_extractor, pol.action_net, pol.value_net)] + [
            (pol.partner_mlp_extractor[k], pol.partner_action_net[k], pol.partner_value_net[k]) for k in range(K)]:
        lins += [ext.policy_net[0], ext.policy_net[2], ext.value_net[0], ext.value_net[2], act, val]
    sv = [th.linalg.svdvals(m.weight.detach().double()).numpy() for m in lins]
    out = {"init.sv_min": np.asarray([x.min() for x in sv]), "init.sv_max": np.asarray([x.max() for x in sv]),
           "init.bias_max": np.asarray([float(m.bias.detach().abs().max()) for m in lins]),
           "init.shapes": np.asarray([list(m.weight.shape) for m in lins], np.int64),
           "adam_eps": np.float64(pol.optimizer.defaults["eps"])}
    g = th.Generator().manual_seed(c["seed"] + 1)
    with th.no_grad():                                          # biases and the 0.01-gain heads perturbed: logits / values not ~0
        for p in pol.parameters():
            if p.ndim == 1:
                p.add_(0.3 * th.randn(p.shape, generator=g))
        for head in [pol.action_net] + list(pol.partner_action_net):
            head.weight.add_(0.3 * th.randn(head.weight.shape, generator=g))
    out["params0"] = modular_flat(pol)

    # forward family: evaluate_actions with and without a mask, get_action_logits_from_obs, on rows the test draws
    rng = np.random.default_rng(c["seed"])
    n = 37
    obs = rng.standard_normal((n, D)).astype(np.float32)
    acts = rng.integers(0, c["n_act"], n)
    mask = rng.random((n, c["n_act"])) < 0.7
    mask[np.arange(n), acts] = True
    out.update({"fwd.obs": obs, "fwd.actions": acts.astype(np.int64), "fwd.mask": mask})
    with th.no_grad():
        for k in range(K):
            v, lp, ent = pol.evaluate_actions(th.as_tensor(obs), th.as_tensor(acts), partner_idx=k)
            vm, lpm, entm = pol.evaluate_actions(th.as_tensor(obs), th.as_tensor(acts), partner_idx=k, action_mask=th.as_tensor(mask))
            zm, zp = pol.get_action_logits_from_obs(th.as_tensor(obs), partner_idx=k)
            for key, val in (("values", v), ("log_prob", lp), ("entropy", ent), ("masked_log_prob", lpm), ("masked_entropy", entm),
                             ("main_logits", zm), ("partner_logits", zp)):
                out[f"fwd.{key}.{k}"] = val.numpy().astype(np.float32)
            assert np.array_equal(v.numpy(), vm.numpy())

    # one rollout buffer per partner (learn.py:134-144), filled by the policy's own forward on seeded rows
    bufs = []
    for k in range(K):
        buf = orc.RolloutBufferOracle(T, E, D, 1)
        starts = np.ones(E, np.float32)
        for _ in range(T):
            o_t = rng.standard_normal((E, D)).astype(np.float32)
            a_t = rng.integers(0, c["n_act"], E)
            with th.no_grad():
                v, lp, _ = pol.evaluate_actions(th.as_tensor(o_t), th.as_tensor(a_t), partner_idx=k)
            buf.add(o_t, a_t.astype(np.float32), rng.standard_normal(E).astype(np.float32), starts, v.flatten(), lp)
            starts = (rng.random(E) < 0.1).astype(np.float32)
        buf.compute_returns_and_advantage(rng.standard_normal(E).astype(np.float32), starts)
        bufs.append(buf)
    perms = np.stack([np.stack([rng.permutation(T * E) for _ in range(c["epochs"])]) for _ in range(K)]).astype(np.int64)

    steps = {"params": [], "partner": []}
    current = {"partner": -1}
    adam = pol.optimizer

    class OptimizerTap:
        param_groups = adam.param_groups

        def zero_grad(self):                                   # the reference pins torch==1.13.1 (setup.py:15): set_to_none defaults to False
            adam.zero_grad(set_to_none=False)

        def step(self):
            adam.step()
            steps["params"].append(modular_flat(pol))
            steps["partner"].append(current["partner"])

    class Buffer:
        def __init__(self, k):
            self.k, self.epoch = k, 0

        def get(self, batch_size):
            current["partner"] = self.k
            order = perms[self.k][self.epoch]
            self.epoch += 1
            for mb in bufs[self.k].get(batch_size, order):
                yield Samples(mb["observations"], mb["actions"], mb["old_values"], mb["old_log_prob"], mb["advantages"], mb["returns"])

    class Logger:
        def __init__(self):
            self.kv = {}

        def record(self, key, value, exclude=None):
            self.kv[key] = value

    def set_lr(optimizer):
        for grp in optimizer.param_groups:
            grp["lr"] = c["lr"]

    pol.optimizer = OptimizerTap()
    buffers = [Buffer(k) for k in range(K)]
    algo = types.SimpleNamespace(
        policy=pol, rollout_buffer=buffers, n_epochs=c["epochs"], batch_size=c["batch"], action_space=spaces.Discrete(c["n_act"]),
        use_sde=False, ent_coef=c["ent"], vf_coef=c["vf"], marginal_reg_coef=c["coef"], target_kl=c["target_kl"], max_grad_norm=c["max_norm"],
        _n_updates=0, logger=Logger(), clip_range=lambda progress: c["clip"],
        clip_range_vf=None if c["clip_vf"] is None else (lambda progress: c["clip_vf"]), _current_progress_remaining=1.0,
        _update_learning_rate=set_lr)
    with contextlib.redirect_stdout(io.StringIO()):            # ("Early stopping at step ..." goes to stdout)
        learn_mod.ModularAlgorithm.train(algo)                  # <- the reference's text
    n_steps = len(steps["params"])
    assert n_steps >= 2 and algo._n_updates == c["epochs"]
    out.update({"perms": perms, "n_steps": np.int64(n_steps), "step_partner": np.asarray(steps["partner"], np.int64),
                "epochs_run": np.asarray([b.epoch for b in buffers], np.int64),
                "params_final": steps["params"][-1]})
    for k, buf in enumerate(bufs):
        for name in ("observations", "actions", "values", "log_probs", "advantages", "returns", "rewards", "episode_starts"):
            out[f"buf{k}.{name}"] = getattr(buf, name)
    for key, val in algo.logger.kv.items():
        out["log." + key] = np.float64(val)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# (viii) the reference's BC TEXT (pantheonrl/algos/bc.py): constructor (Adam with torch's defaults), the DataLoader over its
#        TransitionsMinimal, _calculate_loss, train -- on a network the TEST provides
# ---------------------------------------------------------------------------------------------------------------------------
BC_CASES = {"discrete6": dict(D=20, nvec=(6,), N=100, epochs=3, ent=1e-3, l2=0.0, seed=41),
            "l2_ragged": dict(D=9, nvec=(5,), N=77, epochs=2, ent=1e-2, l2=1e-3, seed=42)}


def bc_case_inputs(c: dict):
    from oracle import sb3_oracle as orc
    th.manual_seed(c["seed"])
    net = orc.FeedForward32Oracle(orc.SpaceSpec("box", dim=c["D"]), orc.SpaceSpec("discrete", nvec=c["nvec"]))
    g = th.Generator().manual_seed(c["seed"] + 1)
    with th.no_grad():
        for p in net.parameters():
            p.add_(0.2 * th.randn(p.shape, generator=g) * (1.0 if p.ndim == 1 else 0.3))
    rng = np.random.default_rng(c["seed"])
    obs = rng.standard_normal((c["N"], c["D"])).astype(np.float32)
    acts = rng.integers(0, c["nvec"][0], c["N"]).astype(np.float32)
    return net, net.flat_params(), obs, acts


def bc_reference_run(ref: "ReferenceModules", c: dict) -> dict:
    bc_mod, util_mod, traj_mod = ref.m["algos.bc"], ref.m["common.util"], ref.m["common.trajsaver"]
    net, flat, obs, acts = bc_case_inputs(c)
    seen = {"batches": []}

    class Policy(util_mod.FeedForward32Policy):             # the reference's class text; the layers are the test's
        def to(self, device):
            return self

        def parameters(self):
            return net.parameters()

        def evaluate_actions(self, o, a):
            rows = [int(np.nonzero((obs == r).all(axis=1))[0][0]) for r in o.numpy()]
            assert np.array_equal(acts[rows], a.numpy().reshape(-1))
            seen["batches"].append(rows)
            return net.evaluate_actions(o, a)

    class Recorder:
        def __init__(self):
            self.kv, self.dumps = {}, []

        def record(self, k, v):
            self.kv[k] = v

        def dump(self, step):
            self.dumps.append((step, dict(self.kv)))
            self.kv = {}

    bc_mod.log = Recorder()
    spaces = ref.spaces
    th.manual_seed(2000 + c["seed"])                          # the DataLoader's shuffles
    clone = bc_mod.BC(spaces.Box(-np.inf, np.inf, (c["D"],)), spaces.Discrete(c["nvec"][0]), policy_class=Policy,
                      expert_data=traj_mod.TransitionsMinimal(obs.copy(), acts.copy()), ent_weight=c["ent"], l2_weight=c["l2"])
    assert isinstance(clone.expert_data_loader, th.utils.data.DataLoader) and clone.expert_data_loader.batch_size == 32
    import contextlib
    with contextlib.redirect_stderr(io.StringIO()):           # (tqdm's progress bars)
        clone.train(n_epochs=c["epochs"], log_interval=1)    # <- the reference's text
    n_b = -(-c["N"] // 32)
    assert len(seen["batches"]) == c["epochs"] * n_b == len(bc_mod.log.dumps)
    orders = np.asarray([sum(seen["batches"][e * n_b:(e + 1) * n_b], []) for e in range(c["epochs"])], np.int64)
    assert all(sorted(o.tolist()) == list(range(c["N"])) for o in orders)
    keys = ("neglogp", "entropy", "ent_loss", "prob_true_act", "l2_norm", "l2_loss", "loss")
    stats = np.asarray([[d[k] for k in keys] for _, d in bc_mod.log.dumps], np.float64)
    progress = np.asarray([[d["epoch_num"], d["batch_num"], d["samples_so_far"]] for _, d in bc_mod.log.dumps], np.int64)
    dflt = clone.optimizer.defaults
    return {"params0": flat, "obs": obs, "acts": acts, "orders": orders, "stats": stats, "progress": progress,
            "params_final": net.flat_params(), "adam": np.asarray([dflt["lr"], dflt["betas"][0], dflt["betas"][1], dflt["eps"],
                                                                    dflt["weight_decay"]], np.float64),
            "net_arch": np.asarray(clone.policy.init_kwargs["net_arch"], np.int64)}


# ---------------------------------------------------------------------------------------------------------------------------
# (ix) the reference's trainer.py TEXT as a script: the argument parser, preset, input_check, latent_check (trainer.py:41-89,231-405)
#      -- run as __main__ on an argv list, stopped where it would build the environment (gym.make is a stand-in that stops the run)
# ---------------------------------------------------------------------------------------------------------------------------
TRAINER_ARGVS = {
    "rps_ppo_ppo": ["RPS-v0", "PPO", "PPO"],
    "rps_seed_steps": ["RPS-v0", "PPO", "PPO", "-s", "7", "-t", "10000"],
    "preset1": ["RPS-v0", "PPO", "PPO", "--preset", "1", "--seed", "0", "-t", "10000"],
    "preset1_keeps_given_names": ["LiarsDice-v0", "PPO", "DEFAULT", "--preset", "1", "--seed", "3", "--ego-save", "mine", "--tensorboard-log", "tb",
                                  "--tensorboard-name", "run"],
    "liar_default_partner": ["LiarsDice-v0", "PPO", "DEFAULT", "--env-config", '{"probegostart": 0.3}'],
    "rps_default_with_config": ["RPS-v0", "PPO", "DEFAULT", "--alt-config", '{"r": 2, "p": 1, "s": 1}'],
    "two_partners_one_flag": ["RPS-v0", "ModularAlgorithm", "PPO", "PPO", "--alt-config", '{"n_steps": 64}', '{"n_steps": 32}',
                              "--ego-config", '{"n_steps": 64, "marginal_reg_coef": 0.5}'],
    "three_kinds_of_partner": ["RPS-v0", "PPO", "PPO", "DEFAULT", "FIXED", "--alt-config", "{}", '{"r": 1}',
                               '{"type": "PPO", "location": "models/old"}'],
    "adap_shared_latent_short_flag": ["RPS-v0", "ADAP", "ADAP", "-l"],
    "adap_mult_shared_latent_configs": ["RPS-v0", "ADAP_MULT", "ADAP", "ADAP_MULT", "--share-latent", "--ego-config",
                                        '{"context_size": 4, "context_sampler": "unit_square"}', "--alt-config", "{}", '{"context_size": 4}'],
    "adap_not_shared": ["LiarsDice-v0", "ADAP", "PPO"],
    "load_ego": ["RPS-v0", "LOAD", "PPO", "--ego-config", '{"type": "PPO", "location": "models/ego"}'],
    "framestack_record": ["LiarsDice-v0", "PPO", "PPO", "-f", "3", "-r", "trajs/x"],
    "tensorboard_both_verbose_partner": ["RPS-v0", "PPO", "PPO", "--tensorboard-log", "logs", "--tensorboard-name", "n", "--verbose-partner"],
    "ego_verbose_given": ["RPS-v0", "PPO", "PPO", "--ego-config", '{"verbose": 0}', "-d", "cuda"],
    "saves": ["RPS-v0", "PPO", "PPO", "--ego-save", "m/e", "--alt-save", "m/a"],
    # rejected
    "bad_tensorboard_log_only": ["RPS-v0", "PPO", "PPO", "--tensorboard-log", "logs"],
    "bad_tensorboard_name_only": ["RPS-v0", "PPO", "PPO", "--tensorboard-name", "n"],
    "bad_config_count": ["RPS-v0", "PPO", "PPO", "--alt-config", "{}", "{}"],
    "bad_share_latent_ppo_partner": ["RPS-v0", "ADAP", "PPO", "-l"],
    "bad_share_latent_ppo_ego": ["RPS-v0", "PPO", "ADAP", "--share-latent"],
    "bad_share_latent_context_size": ["RPS-v0", "ADAP", "ADAP", "-l", "--alt-config", '{"context_size": 2}'],
    "bad_share_latent_sampler": ["RPS-v0", "ADAP", "ADAP", "-l", "--alt-config", '{"context_sampler": "categorical"}'],
    "bad_ego_choice": ["RPS-v0", "SAC", "PPO"],
    "bad_partner_choice": ["RPS-v0", "PPO", "LOAD"],
    "bad_env_choice": ["Pong-v0", "PPO", "PPO"],
    "bad_overcooked_without_layout": ["OvercookedMultiEnv-v0", "PPO", "PPO"],
    "bad_overcooked_layout": ["OvercookedMultiEnv-v0", "PPO", "PPO", "--env-config", '{"layout_name": "nowhere"}'],
}


def trainer_cli_reference_run() -> dict:
    """{case: {"args": vars(args) where the script would call gym.make} | {"rejected": exception class name}}"""
    import contextlib
    path = os.path.join(REFERENCE, "trainer.py")
    with open(path) as fh:
        code = compile(fh.read(), path, "exec")             # executed from where it lies; nothing of it is kept

    class StopBeforeTheEnvironment(Exception):
        pass

    def stop(*a, **k):
        raise StopBeforeTheEnvironment()

    def names(modname, *ns, **attrs):
        m = types.ModuleType(modname)
        for n in ns:
            setattr(m, n, type(n, (), {}))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    extra = {
        "stable_baselines3.common.monitor": names("stable_baselines3.common.monitor", "Monitor"),
        "pantheonrl.envs": names("pantheonrl.envs"),
        "pantheonrl.envs.rpsgym": names("pantheonrl.envs.rpsgym"),
        "pantheonrl.envs.rpsgym.rps": names("pantheonrl.envs.rpsgym.rps", "RPSEnv", "RPSWeightedAgent"),
        "pantheonrl.envs.liargym": names("pantheonrl.envs.liargym"),
        "pantheonrl.envs.liargym.liar": names("pantheonrl.envs.liargym.liar", "LiarEnv", "LiarDefaultAgent"),
        "pantheonrl.envs.blockworldgym": names("pantheonrl.envs.blockworldgym", simpleblockworld=names("simpleblockworld"),
                                               blockworld=names("blockworld")),
        "overcookedgym": names("overcookedgym", __path__=[os.path.join(REFERENCE, "overcookedgym")]),   # its __init__ is not run:
    }                                                                                                  # overcooked_utils.py is plain lists
    out = {}
    with ReferenceModules() as ref:
        saved = {k: sys.modules.get(k) for k in extra}
        sys.modules.update(extra)
        sys.modules["stable_baselines3.common.vec_env"].DummyVecEnv = type("DummyVecEnv", (), {})
        sys.modules["gym"].make = stop
        argv0 = sys.argv
        try:
            for case, argv in TRAINER_ARGVS.items():
                ns = {"__name__": "__main__", "__file__": path}
                sys.argv = ["trainer.py"] + list(argv)
                try:
                    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                        exec(code, ns)
                    raise AssertionError("the script ran past gym.make")
                except StopBeforeTheEnvironment:
                    out[case] = {"args": rd.plain(vars(ns["args"]))}
                except SystemExit as e:                                   # argparse: a value outside `choices`
                    out[case] = {"rejected": "SystemExit", "code": int(e.code)}
                except Exception as e:  # noqa: BLE001
                    assert type(e).__name__ == "EnvException", (case, repr(e))
                    out[case] = {"rejected": "EnvException"}
        finally:
            sys.argv = argv0
            for k, v in saved.items():
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
            for k in [k for k in sys.modules if k.startswith("overcookedgym")]:
                sys.modules.pop(k, None)
    return out


# (ix, continued) the same script run to its END on recording doubles (tests/refdrive.TrainerDoubles): which environments, wrappers,
# learners and agents a command line constructs with which arguments, who is registered as whose partner, learn / record / save calls
TRAINER_GRAPH_ARGVS = {k: TRAINER_ARGVS[k] for k in (
    "rps_ppo_ppo", "rps_seed_steps", "preset1", "liar_default_partner", "rps_default_with_config", "two_partners_one_flag",
    "adap_shared_latent_short_flag", "adap_mult_shared_latent_configs", "adap_not_shared", "load_ego", "framestack_record",
    "tensorboard_both_verbose_partner", "saves")}
TRAINER_GRAPH_ARGVS.update({
    "fixed_partners": ["RPS-v0", "PPO", "FIXED", "FIXED", "--alt-config", '{"type": "PPO", "location": "models/old"}',
                       '{"type": "ADAP", "location": "models/adap", "latent_val": [0.5, -0.5, 0.25]}', "--alt-save", "m/a"],
    "load_modular_ego_three_partners": ["LiarsDice-v0", "LOAD", "PPO", "PPO", "DEFAULT", "--ego-config",
                                        '{"type": "ModularAlgorithm", "location": "models/mod"}', "--seed", "5", "--ego-save", "m/e",
                                        "--alt-save", "m/a"],
})
# (not in the matrix: `LiarsDice-v0 PPO DEFAULT -f 2` -- the reference's gen_default tests isinstance(altenv, LiarEnv) on the frame-stack
# WRAPPER and raises "No default policy available", trainer.py:165-179; the product unwraps down to the game first)


def trainer_graph_reference_run() -> dict:
    import contextlib
    path = os.path.join(REFERENCE, "trainer.py")
    with open(path) as fh:
        code = compile(fh.read(), path, "exec")

    def module(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    out = {}
    argv0 = sys.argv
    for case, argv in TRAINER_GRAPH_ARGVS.items():
        d = rd.TrainerDoubles()

        class Monitor:
            def __init__(self, env):
                self.label = f"monitor({env.label})"

        class DummyVecEnv:
            def __init__(self, fns):
                self.label = f"vec({fns[0]().label})"

        class BCShell:
            def __init__(self, policy):
                self.policy = policy
        mods = dict(_stand_ins())
        mods.pop("pantheonrl")
        overlay = {
            "gym": module("gym", make=d.make, spaces=mods["gym.spaces"]),
            "stable_baselines3": module("stable_baselines3", PPO=d.PPO),
            "stable_baselines3.common": module("stable_baselines3.common"),
            "stable_baselines3.common.vec_env": module("stable_baselines3.common.vec_env", DummyVecEnv=DummyVecEnv),
            "stable_baselines3.common.monitor": module("stable_baselines3.common.monitor", Monitor=Monitor),
            "pantheonrl": module("pantheonrl"), "pantheonrl.common": module("pantheonrl.common"),
            "pantheonrl.common.wrappers": module("pantheonrl.common.wrappers", frame_wrap=d.frame_wrap, recorder_wrap=d.recorder_wrap),
            "pantheonrl.common.agents": module("pantheonrl.common.agents", OnPolicyAgent=d.OnPolicyAgent, StaticPolicyAgent=d.StaticPolicyAgent),
            "pantheonrl.algos": module("pantheonrl.algos"), "pantheonrl.algos.adap": module("pantheonrl.algos.adap"),
            "pantheonrl.algos.adap.adap_learn": module("pantheonrl.algos.adap.adap_learn", ADAP=d.ADAP),
            "pantheonrl.algos.adap.policies": module("pantheonrl.algos.adap.policies", AdapPolicyMult=d.AdapPolicyMult, AdapPolicy=d.AdapPolicy),
            "pantheonrl.algos.adap.agent": module("pantheonrl.algos.adap.agent", AdapAgent=d.AdapAgent),
            "pantheonrl.algos.modular": module("pantheonrl.algos.modular"),
            "pantheonrl.algos.modular.learn": module("pantheonrl.algos.modular.learn", ModularAlgorithm=d.ModularAlgorithm),
            "pantheonrl.algos.modular.policies": module("pantheonrl.algos.modular.policies", ModularPolicy=d.ModularPolicy),
            "pantheonrl.algos.bc": module("pantheonrl.algos.bc", BCShell=BCShell, reconstruct_policy=None),
            "pantheonrl.envs": module("pantheonrl.envs"), "pantheonrl.envs.rpsgym": module("pantheonrl.envs.rpsgym"),
            "pantheonrl.envs.rpsgym.rps": module("pantheonrl.envs.rpsgym.rps", RPSEnv=d.RPSEnv, RPSWeightedAgent=d.RPSWeightedAgent),
            "pantheonrl.envs.liargym": module("pantheonrl.envs.liargym"),
            "pantheonrl.envs.liargym.liar": module("pantheonrl.envs.liargym.liar", LiarEnv=d.LiarEnv, LiarDefaultAgent=d.LiarDefaultAgent),
            "pantheonrl.envs.blockworldgym": module("pantheonrl.envs.blockworldgym",
                                                    simpleblockworld=module("simpleblockworld", PartnerEnv=object()),
                                                    blockworld=module("blockworld", PartnerEnv=object())),
            "overcookedgym": module("overcookedgym", __path__=[os.path.join(REFERENCE, "overcookedgym")]),
        }
        saved = {k: sys.modules.get(k) for k in overlay}
        sys.modules.update(overlay)
        sys.argv = ["trainer.py"] + list(argv)
        try:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                exec(code, {"__name__": "__main__", "__file__": path})      # <- the reference's text, to its last line
        finally:
            sys.argv = argv0
            for k, v in saved.items():
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
            for k in [k for k in sys.modules if k.startswith("overcookedgym")]:
                sys.modules.pop(k, None)
        out[case] = rd.plain(d.events)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# (x) the integer action-mask rule, from the reference's PettingZooAECWrapper TEXT (pantheonrl/envs/pettingzoo.py:27-127): what the
#     base environment is stepped with when the acting agent's sample is illegal under the mask it was shown
# ---------------------------------------------------------------------------------------------------------------------------
MASK_CASES = {"mpe8_L5": dict(L=5, n=600, p_legal=0.8, n_players=8, seed=51), "wide_L20": dict(L=20, n=400, p_legal=0.3, n_players=3, seed=52)}


def action_mask_reference_run(c: dict) -> dict:
    """a scripted AEC environment behind the reference's wrapper: per step a Bernoulli(p_legal) mask with at least one legal action for
    the agent that moves next, a uniformly random sample as that agent's action -> the action base_env.step received"""
    def names(modname, *ns):
        m = types.ModuleType(modname)
        for n in ns:
            setattr(m, n, type(n, (), {"__init__": lambda self, **kw: self.__dict__.update(kw)}))
        return m
    gymn = types.ModuleType("gymnasium")
    gymn.spaces = types.ModuleType("gymnasium.spaces")
    for sub, cls in (("box", "Box"), ("discrete", "Discrete"), ("multi_discrete", "MultiDiscrete"), ("multi_binary", "MultiBinary"), ("dict", "Dict")):
        m = names("gymnasium.spaces." + sub, cls)
        setattr(gymn.spaces, sub, m)
    gymn.spaces.Space = type("Space", (), {})
    rng = np.random.default_rng(c["seed"])
    L, P = c["L"], c["n_players"]

    class Base:                                                           # the AEC surface the wrapper touches
        possible_agents = [f"agent_{i}" for i in range(P)]
        max_num_agents = P

        def __init__(self):
            self.received, self.masks, self.t = [], [], 0
            self.rewards = {a: 0.0 for a in self.possible_agents}
            self.terminations = {a: False for a in self.possible_agents}
            self.truncations = {a: False for a in self.possible_agents}
            self.infos = {a: {} for a in self.possible_agents}

        def action_space(self, agent):
            return gymn.spaces.discrete.Discrete(n=L)

        def observation_space(self, agent):
            box = gymn.spaces.box.Box(low=np.zeros(4, np.float32), high=np.ones(4, np.float32), dtype=np.float32)
            return gymn.spaces.dict.Dict(spaces={"observation": box})

        def reset(self):
            self.agent_selection = self.possible_agents[0]

        def observe(self, agent):
            mask = (rng.random(L) < c["p_legal"]).astype(np.int8)
            if not mask.any():
                mask[rng.integers(0, L)] = 1
            self.masks.append(mask.copy())
            return {"observation": rng.random(4).astype(np.float32), "action_mask": mask}

        def step(self, act):
            self.received.append(int(act))
            self.t += 1
            self.agent_selection = self.possible_agents[self.t % P]
    with ReferenceModules() as ref:
        saved = {k: sys.modules.get(k) for k in ("gymnasium", "pantheonrl.envs")}
        sys.modules["gymnasium"] = gymn
        envs_pkg = types.ModuleType("pantheonrl.envs")                       # its __init__.py (gym registrations) is not run
        envs_pkg.__path__ = [os.path.join(REFERENCE, "pantheonrl", "envs")]
        sys.modules["pantheonrl.envs"] = envs_pkg
        try:
            pz = importlib.import_module("pantheonrl.envs.pettingzoo")
            assert os.path.abspath(pz.__file__).startswith(os.path.abspath(REFERENCE))
            base = Base()
            env = pz.PettingZooAECWrapper(base, ego_ind=0)                   # <- the reference's text
            assert env.action_space.n == L and tuple(env.observation_space.shape) == (4,)
            env.n_reset()
            sampled = rng.integers(0, L, c["n"])
            for a in sampled:
                env.n_step([np.int64(a)])
        finally:
            for k, v in saved.items():
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
    masks = np.stack(base.masks[:c["n"]]).astype(np.uint8)                   # mask i is what the agent acting at step i was shown
    return {"masks": masks, "sampled": sampled.astype(np.int32), "stepped_with": np.asarray(base.received, np.int32)}


# ---------------------------------------------------------------------------------------------------------------------------
# (xi) the hand-made DEFAULT partners of trainer.py (gen_default, :165-179): LiarDefaultAgent (liargym/liar.py:29-42) and
#      RPSWeightedAgent (rpsgym/rps.py:14-30), run from the reference's files (loader of tests/golden/check_against_reference.py)
# ---------------------------------------------------------------------------------------------------------------------------
def default_agents_reference_run() -> dict:
    from tests.golden.check_against_reference import load_reference_games
    liar_ns, rps_ns = load_reference_games(REFERENCE)
    rng = np.random.default_rng(61)
    agent = liar_ns["LiarDefaultAgent"]()
    obs_rows, acts = [], []
    for _ in range(400):
        dice = rng.integers(0, 6, 6)
        hand = [int((dice == f).sum()) for f in range(6)]
        n_moves = int(rng.integers(0, 5))
        hist = []
        for _m in range(n_moves):
            hist += [int(rng.integers(0, 6)), int(rng.integers(1, 13))]
        hist += [6, 0] * (12 - n_moves)
        o = np.asarray(hand + hist, np.int64)
        obs_rows.append([int(v) for v in o])
        acts.append([int(v) for v in np.asarray(agent.get_action(types.SimpleNamespace(obs=o))).reshape(-1)])
        agent.update(0.0, False)

    class Rolls:
        def __init__(self, rolls):
            self.rolls = list(rolls)

        def rand(self):
            return self.rolls.pop(0)
    rps = []
    rolls = [float(v) for v in np.round(rng.random(40), 6)] + [0.0, 1.0 / 3, 2.0 / 3, 0.25, 0.5, 0.75]
    for r, p_, s_ in ((1, 1, 1), (2, 1, 1), (1, 0, 0), (0, 0, 0), (0, 3, 1), (5, 0, 5)):
        a = rps_ns["RPSWeightedAgent"](r=r, p=p_, s=s_, np_random=Rolls(rolls))
        rps.append({"weights": [r, p_, s_], "actions": [int(a.get_action(None)) for _ in rolls]})
    return {"liar_obs": obs_rows, "liar_actions": acts, "rps_rolls": rolls, "rps": rps}


# ---------------------------------------------------------------------------------------------------------------------------
# (xii) the ego's loop on recording doubles (tests/refdrive.LoopDoubles): ModularAlgorithm.learn + collect_rollouts TEXT
#       (modular/learn.py:157-219,353-403) and ADAP.collect_rollouts TEXT (adap_learn.py:377-473 = SB3's collect_rollouts + context lines)
# ---------------------------------------------------------------------------------------------------------------------------
LOOP_CASES = {"modular_two_partners": dict(kind="modular", K=2, n_steps=5, total=23, seed=71),
              "modular_one_partner": dict(kind="modular", K=1, n_steps=4, total=9, seed=72),
              "ppo_collect": dict(kind="adap", ctx=0, n_steps=7, rollouts=3, seed=73),
              "adap_collect": dict(kind="adap", ctx=3, n_steps=6, rollouts=3, seed=74)}
LOOP_D, LOOP_ACTIONS = 3, 4


def loop_reference_run(ref: "ReferenceModules", c: dict) -> list:
    import time
    d = rd.LoopDoubles(c["seed"], LOOP_D, LOOP_ACTIONS, K=c.get("K", 1), ctx=c.get("ctx", 0))
    algo = types.SimpleNamespace(policy=d.policy, env=d.env, n_steps=c["n_steps"], use_sde=False, sde_sample_freq=-1, device="cpu",
                                 action_space=ref.spaces.Discrete(LOOP_ACTIONS), num_timesteps=0, _last_obs=None, logger=d.logger,
                                 ep_info_buffer=deque(maxlen=100), train=d.train, start_time=time.time())

    def update_info_buffer(infos, dones=None):                 # SB3's _update_info_buffer: the finished episodes' statistics
        for info in infos:
            if info.get("episode") is not None:
                algo.ep_info_buffer.extend([info["episode"]])
    algo._update_info_buffer = update_info_buffer
    if c["kind"] == "modular":
        cls = ref.m["algos.modular.learn"].ModularAlgorithm
        algo.rollout_buffer = d.buffers
        algo.collect_rollouts = types.MethodType(cls.collect_rollouts, algo)

        def setup_learn(total_timesteps, eval_env, callback, *rest):       # SB3's _setup_learn: counters, clock, the first observation
            algo.num_timesteps, algo.start_time, algo._last_obs = 0, time.time(), algo.env.reset()
            return total_timesteps, callback
        algo._setup_learn = setup_learn
        algo._update_current_progress_remaining = lambda n, t: None
        cls.learn(algo, total_timesteps=c["total"], callback=d.callback)   # <- the reference's text (learn and, through it, collect_rollouts)
    else:
        cls = ref.m["algos.adap.adap_learn"].ADAP
        algo.context_size, algo.context_sampler, algo.full_obs_shape = c["ctx"], "l2", None
        algo._last_obs, algo._last_episode_starts = algo.env.reset(), np.ones((1,), dtype=bool)
        th.manual_seed(c["seed"])
        for _ in range(c["rollouts"]):
            assert cls.collect_rollouts(algo, algo.env, d.callback, d.buffers[0], n_rollout_steps=c["n_steps"]) is True   # <- the reference's text
    return rd.plain(d.events)

# ---------------------------------------------------------------------------------------------------------------------------
def generate() -> dict:
    """-> {file name: bytes} of every reference-generated fixture"""
    files = {}
    with ReferenceModules() as ref:
        fw, spaces = ref.framework(), ref.spaces
        logs = {"simultaneous": rd.drive_simultaneous(fw), "turnbased": rd.drive_turnbased(fw), "three_player": rd.drive_three_player(fw),
                "observation": rd.drive_observation(fw)}
        files["ref_multiagent.json"] = logs
        files["ref_onpolicy_agent.json"] = {"verbose": rd.drive_onpolicy_agent(fw, spaces, verbose=1),
                                            "quiet": rd.drive_onpolicy_agent(fw, spaces, seed=8, n_steps=4, n_calls=19, verbose=0),
                                            "recorded_only": rd.drive_onpolicy_agent(fw, spaces, **rd.RECORDED_ONLY),
                                            "static_and_wrapper": rd.drive_static_and_wrapper(fw, spaces)}
        # (pantheonrl/algos/adap/agent.py's AdapAgent is NOT here: as written its get_action reshapes the observation ++ context row
        # (D + context_size elements) to (1,) + policy.observation_space.shape = (1, D) and raises for every recorded call,
        # agent.py:115-123 with util.py:75 fixing policy.observation_space to the environment's; the product stores the row the text
        # evidently means -- tests/test_gpu_adap.py::test_adap_agent_partner_side against the oracle)
        files["ref_framestack.json"] = {"history_queue": rd.drive_history_queue(fw), "wrappers": rd.drive_framestack(fw, spaces)}
        rec = rd.drive_recorders(fw, spaces)
        files["ref_recorders.json"] = rec["views"]
        npy = {k: np.frombuffer(v, np.uint8) for k, v in rec["files"].items()}
        util_mod, dist_mod = ref.m["algos.adap.util"], sys.modules["stable_baselines3.common.distributions"]
        adap = {}
        for name, c in ADAP_CASES.items():
            for k, v in adap_reference_run(util_mod, dist_mod, c).items():
                adap[f"{name}.{k}"] = v
        for k, v in adap_sampler_run(util_mod).items():
            adap["sampler." + k] = v
        train = {}
        for name, c in TRAIN_CASES.items():
            for k, v in train_reference_run(ref, c).items():
                train[f"{name}.{k}"] = np.asarray(v)
        modular = {}
        for name, c in MODULAR_CASES.items():
            for k, v in modular_reference_run(ref, c).items():
                modular[f"{name}.{k}"] = np.asarray(v)
        bc = {}
        for name, c in BC_CASES.items():
            for k, v in bc_reference_run(ref, c).items():
                bc[f"{name}.{k}"] = np.asarray(v)
    masks = {}
    for name, c in MASK_CASES.items():
        for k, v in action_mask_reference_run(c).items():
            masks[f"{name}.{k}"] = v
    files["ref_default_agents.json"] = default_agents_reference_run()
    with ReferenceModules() as ref:
        files["ref_ego_loop.json"] = {name: loop_reference_run(ref, c) for name, c in LOOP_CASES.items()}
    files["ref_trainer_cli.json"] = trainer_cli_reference_run()
    files["ref_trainer_graph.json"] = trainer_graph_reference_run()
    out = {}
    for name, obj in files.items():
        out[name] = (json.dumps(obj, indent=None, separators=(",", ":"), sort_keys=True) + "\n").encode()
    for name, arrays in (("ref_transitions.npz", npy), ("ref_adap_context.npz", adap), ("ref_ppo_train.npz", train),
                         # the ModularPolicy cases' final parameters in a file of their own: each file stays under 1 MiB
                         ("ref_modular.npz", {k: v for k, v in modular.items() if not k.endswith(".params_final")}),
                         ("ref_modular_final.npz", {k: v for k, v in modular.items() if k.endswith(".params_final")}),
                         ("ref_bc.npz", bc),
                         ("ref_action_mask.npz", masks)):
        f = io.BytesIO()
        np.savez(f, **{k: arrays[k] for k in sorted(arrays)})       # uncompressed + sorted: byte-reproducible
        out[name] = f.getvalue()
    return out


MANIFEST = "ref_fixtures_sha256.json"


def manifest(made: dict) -> bytes:
    """SHA-256 of every generated fixture's bytes: what the not-gpu test checks the committed files against"""
    digests = {name: hashlib.sha256(data).hexdigest() for name, data in made.items()}
    return (json.dumps(digests, indent=1, sort_keys=True) + "\n").encode()


def main() -> int:
    if not os.path.isdir(REFERENCE):
        print(f"{REFERENCE} not present: this script runs in the build container only")
        return 0
    made = generate()
    write = "--write" in sys.argv
    bad = []
    for name, data in {**made, MANIFEST: manifest(made)}.items():
        path = os.path.join(HERE, name)
        if write:
            with open(path, "wb") as fh:
                fh.write(data)
        elif not os.path.exists(path) or open(path, "rb").read() != data:
            bad.append(name)
    if bad:
        print("fixtures differ from what the reference produces now:", bad)
        return 1
    print(("wrote " if write else "reference reproduces ") + ", ".join(f"{n} ({len(d)} B)" for n, d in made.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
