"""Writes tests/golden/blockworld_ref.npz from the REFERENCE's own block-world code (build container only).

    python tests/golden/make_block_fixtures.py            # write the fixture
    python tests/golden/make_block_fixtures.py --check    # regenerate in memory and compare with the committed file

What runs is the reference's text, loaded from where it lies (`pantheonrl/envs/blockworldgym/{gridutils,blockworld,
simpleblockworld}.py`); nothing of it is copied here and only arrays are committed.  The two game files import `gym` and two
PantheonRL modules that need `gym` / `stable_baselines3` (absent here); the rules use nothing of them beyond the base-class names
and module-level space constants, so the files are executed with inert stand-ins for exactly those names (as
check_against_reference.py does for Liar's Dice).  No game rule comes from a stand-in.

Content, per variant (v0 = SimpleBlockEnv, v1 = BlockEnv):
  * 256 tables, each from `multi_reset(True)` under np.random.seed(2025);
  * 24 rounds of moves per table from default_rng(2025): the planner's token is the terminal one with probability 0.25, else
    uniform over the others; the constructor's action is uniform (v0: with probability 0.5 its colour is the block's true colour);
    every round is played whether or not a game ended (the reference has no guard);
  * per round: the constructor's observation, both rewards and done after ego_step, the planner's observation after alt_step;
  * for every token, 64 random constructor observations and the action of each scripted partner.

(The file is not called ref_*: those names belong to make_reference_fixtures.py's manifest, which lists exactly its own files.)
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("PANTHEON_REFERENCE", "/root/reference")
PATH = os.path.join(HERE, "blockworld_ref.npz")
N_TABLES, N_ROUNDS, N_OBS, SEED = 256, 24, 64, 2025


def load_reference_blockworld(root: str = REFERENCE):
    """-> (gridutils, blockworld, simpleblockworld) namespaces, executed from the reference's files"""
    class _Space:
        def __init__(self, *a, **k):
            self.args, self.kwargs = a, k

    class _Base:
        def __init__(self, *a, **k):
            pass

    def module(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    def run(rel):
        path = os.path.join(root, rel)
        ns = {"__name__": "reference_" + os.path.basename(rel)[:-3], "__file__": path}
        with open(path) as fh:
            exec(compile(fh.read(), path, "exec"), ns)     # the reference's text, run in place
        return ns

    spaces = module("gym.spaces", **{n: type(n, (_Space,), {}) for n in ("MultiDiscrete", "Discrete", "Box", "MultiBinary")})
    stand_ins = {"gym": module("gym", spaces=spaces, Env=object), "gym.spaces": spaces,
                 "pantheonrl": module("pantheonrl"), "pantheonrl.common": module("pantheonrl.common"),
                 "pantheonrl.common.agents": module("pantheonrl.common.agents", Agent=_Base),
                 "pantheonrl.common.multiagentenv": module("pantheonrl.common.multiagentenv", TurnBasedEnv=_Base, DummyEnv=_Base),
                 "pantheonrl.envs": module("pantheonrl.envs"),
                 "pantheonrl.envs.blockworldgym": module("pantheonrl.envs.blockworldgym")}
    saved = {k: sys.modules.get(k) for k in list(stand_ins) + ["pantheonrl.envs.blockworldgym.gridutils"]}
    sys.modules.update(stand_ins)
    try:
        grid = run("pantheonrl/envs/blockworldgym/gridutils.py")
        sys.modules["pantheonrl.envs.blockworldgym.gridutils"] = module("pantheonrl.envs.blockworldgym.gridutils", **{
            k: v for k, v in grid.items() if not k.startswith("__")})
        return grid, run("pantheonrl/envs/blockworldgym/blockworld.py"), run("pantheonrl/envs/blockworldgym/simpleblockworld.py")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def play(variant: int, env_cls, grid_ns) -> dict:
    """tables, moves and the reference's answers for one variant"""
    np.random.seed(SEED)
    tables = []
    for _ in range(N_TABLES):
        t = env_cls()
        t.multi_reset(True)
        tables.append(t)
    world = np.array([t.gridworld for t in tables]).astype(np.int8)          # (N, 7, 7) | (N, 5, 4)
    rng = np.random.default_rng(SEED)
    n_tok, A = (30, 3) if variant else (16, 2)
    De, Da = (98, 50) if variant else (40, 21)
    tokens = np.zeros((N_TABLES, N_ROUNDS), np.int8)
    acts = np.zeros((N_TABLES, N_ROUNDS, A), np.int8)
    alt_obs = np.zeros((N_TABLES, N_ROUNDS, Da), np.int8)
    ego_obs = np.zeros((N_TABLES, N_ROUNDS, De), np.int8)
    rew = np.zeros((N_TABLES, N_ROUNDS, 2), np.float32)
    done = np.zeros((N_TABLES, N_ROUNDS), np.uint8)
    noop = np.zeros((N_TABLES, N_ROUNDS), np.uint8)       # v1: 1 = horizontal at x = 6, 2 = blocked column
    for e, t in enumerate(tables):
        for r in range(N_ROUNDS):
            token = n_tok - 1 if rng.random() < 0.25 else int(rng.integers(0, n_tok - 1))
            if variant:
                act = [int(rng.integers(0, 7)), int(rng.integers(0, 2)), int(rng.integers(0, 2))]
            else:
                act = [int(rng.integers(0, 5)), int(rng.integers(0, 3))]
                if rng.random() < 0.5:
                    act[1] = int(t.gridworld[act[0]][3])
            tokens[e, r], acts[e, r] = token, act
            o, rw, d, _ = t.ego_step(token)
            alt_obs[e, r], rew[e, r], done[e, r] = np.asarray(o), np.asarray(rw, np.float64).astype(np.float32), bool(d)
            if variant:
                if act[1] == grid_ns["HORIZONTAL"] and act[0] == 6:
                    noop[e, r] = 1
                elif grid_ns["gravity"](t.constructor_obs, act[1], act[0]) == -1:
                    noop[e, r] = 2
            o, rw, d, _ = t.alt_step(np.asarray(act))
            assert list(rw) == [0, 0] and not d
            ego_obs[e, r] = np.asarray(o)
    k = f"v{variant}_"
    return {k + "world": world, k + "tokens": tokens, k + "acts": acts, k + "alt_obs": alt_obs, k + "ego_obs": ego_obs,
            k + "rew": rew, k + "done": done, k + "noop": noop}


def partner_tables(block_ns, simple_ns) -> dict:
    """for every token, N_OBS random constructor observations -> what each scripted partner of the reference answers"""
    rng = np.random.default_rng(SEED + 1)
    np.random.seed(SEED + 1)
    easy, default, ctor = simple_ns["SBWEasyPartner"](), simple_ns["SBWDefaultAgent"](), block_ns["DefaultConstructorAgent"]()
    sbw_obs = np.zeros((16, N_OBS, 21), np.int8)
    sbw_easy, sbw_default = np.zeros((16, N_OBS, 2), np.int8), np.zeros((16, N_OBS, 2), np.int8)
    for token in range(16):
        for i in range(N_OBS):
            blocks = simple_ns["generate_grid_world"]()
            view = [v for b in blocks for v in (b[0], b[1], b[2], int(rng.integers(0, 3)))]
            sbw_obs[token, i] = [token] + view
            obs = types.SimpleNamespace(obs=np.array([token] + view))
            sbw_easy[token, i] = [int(v) for v in easy.get_action(obs)]
            sbw_default[token, i] = [int(v) for v in default.get_action(obs)]
    ctor_obs = np.zeros((30, N_OBS, 50), np.int8)
    ctor_act = np.zeros((30, N_OBS, 3), np.int8)
    for token in range(30):
        for i in range(N_OBS):
            ctor_obs[token, i] = [token] + [int(v) for v in rng.integers(0, 3, 49)]
            ctor_act[token, i] = [int(v) for v in ctor.get_action(types.SimpleNamespace(obs=ctor_obs[token, i].astype(np.int64)))]
    return dict(sbw_obs=sbw_obs, sbw_easy=sbw_easy, sbw_default=sbw_default, ctor_obs=ctor_obs, ctor_act=ctor_act)


def check_coverage(z) -> dict:
    """the conditions the fixture must meet (asserted here and again by tests/test_blockworld.py)"""
    ends = z["v1_done"].astype(bool)
    values = z["v1_rew"][..., 0][ends]
    noop = z["v1_noop"]
    out = dict(v1_evaluations=int(ends.sum()), v1_values=int(len(np.unique(values))), v1_max=float(values.max()),
               v1_noop_share=float((noop > 0).mean()), v1_refused_x6=int((noop == 1).sum()), v1_refused_blocked=int((noop == 2).sum()),
               v0_counts=[int((z["v0_rew"][..., 0][z["v0_done"].astype(bool)] == 20.0 * k).sum()) for k in range(6)])
    assert out["v1_evaluations"] >= 1000 and out["v1_values"] >= 40 and out["v1_max"] >= 0.5, out
    assert 0.15 <= out["v1_noop_share"] <= 0.5 and out["v1_refused_x6"] > 0 and out["v1_refused_blocked"] > 0, out
    assert min(out["v0_counts"]) >= 50, out
    return out


def generate() -> dict:
    grid_ns, block_ns, simple_ns = load_reference_blockworld()
    z = {}
    z.update(play(0, simple_ns["SimpleBlockEnv"], grid_ns))
    z.update(play(1, block_ns["BlockEnv"], grid_ns))
    z.update(partner_tables(block_ns, simple_ns))
    return z


def main() -> int:
    if not os.path.isdir(REFERENCE):
        print(f"{REFERENCE} not present: this generator runs in the build container only")
        return 0
    import warnings
    warnings.simplefilter("ignore", RuntimeWarning)     # the reference's match count divides 0 by 0 on purpose
    z = generate()
    print("coverage:", check_coverage(z))
    if "--check" in sys.argv:
        committed = np.load(PATH)
        assert sorted(committed.files) == sorted(z)
        for k, v in z.items():
            assert v.dtype == committed[k].dtype and np.array_equal(v, committed[k]), f"blockworld_ref.npz[{k}] differs from the reference"
        print("blockworld_ref.npz matches the reference's output")
        return 0
    np.savez_compressed(PATH, **z)
    print(f"{PATH} written ({os.path.getsize(PATH)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
