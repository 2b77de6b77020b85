"""not-gpu: frozen ADAP checkpoints as members of the device-resident Liar's Dice pool and cross-play -- what can be pinned without a
device: the command lines' plans and refusals, and, through ph_adap_vec_host (the text the kernels run), the rows and the sampled
contexts a member sees against the numpy statement of tests/adap_vec_ref.py."""
import numpy as np
import pytest

from pantheonrl_amd import _native as nat
from pantheonrl_amd import crossplay, trainer
from pantheonrl_amd.trainer import EnvException
from tests import adap_vec_ref as A

LIAR_NVEC = [7] * 6 + [7, 12] * 12


def _plan(*alt_configs, alts=("FIXED",), extra=()):
    argv = ["LiarsDice-v0", "PPO", *alts, "--n-envs", "8", "--alt-config", *alt_configs, *extra]
    return trainer.pool_plan(trainer.parse_cli(argv))


# ---- the trainer's plan ------------------------------------------------------------------------------------------------------------
def test_pool_plan_accepts_a_stated_and_a_sampled_adap_member_and_keeps_them():
    stated = '{"type": "ADAP", "location": "m", "latent_val": [1, 0, 0.5]}'
    sampled = '{"type": "ADAP", "location": "m", "latent_val": "sample"}'
    plan = _plan(stated, sampled, "{}", alts=("FIXED", "FIXED", "DEFAULT"))
    assert [k for k, _ in plan["members"]] == ["FIXED", "FIXED", "DEFAULT"]
    assert plan["members"][0][1] == {"type": "ADAP", "location": "m", "latent_val": [1.0, 0.0, 0.5]}
    assert plan["members"][1][1] == {"type": "ADAP", "location": "m", "latent_val": "sample"}
    # beside a learner and a PPO checkpoint
    plan = _plan("{}", stated, '{"type": "PPO", "location": "p"}', alts=("PPO", "FIXED", "FIXED"))
    assert [c.get("type") for _, c in plan["members"]] == [None, "ADAP", "PPO"]


@pytest.mark.parametrize("config, words", [
    ('{"type": "ADAP", "location": "m"}', "PPO checkpoint"),                    # no latent_val: the pinned sentence, extended
    ('{"type": "ADAP", "location": "m"}', "latent_val"),
    ('{"type": "ADAP", "location": "m", "latent_val": "draw"}', '"sample"'),
    ('{"type": "ADAP", "location": "m", "latent_val": []}', "context_size"),
    ('{"type": "ADAP", "location": "m", "latent_val": [1, "x"]}', "context_size"),
    ('{"type": "ADAP", "location": "m", "latent_val": 3}', "context_size"),
    ('{"type": "ADAP", "location": "m", "latent_val": %s}' % ([0.5] * 65), "1..64"),
    ('{"type": "ADAP_MULT", "location": "m", "latent_val": [1]}', "PPO checkpoint"),
])
def test_pool_plan_refusals_before_a_device_is_touched(config, words):
    with pytest.raises(EnvException, match=words):
        _plan(config)


def test_adap_learner_members_and_the_tester_stay_refused():
    with pytest.raises(EnvException, match="pool of"):
        trainer.pool_plan(trainer.parse_cli(["LiarsDice-v0", "PPO", "PPO", "ADAP", "--n-envs", "8"]))
    with pytest.raises(EnvException, match="pool of"):
        trainer.pool_plan(trainer.parse_cli(["LiarsDice-v0", "ADAP", "FIXED", "DEFAULT", "--n-envs", "8", "--alt-config",
                                             '{"type": "ADAP", "location": "m", "latent_val": "sample"}', "{}"]))


# ---- crossplay --agents --------------------------------------------------------------------------------------------------------------
def test_parse_agent_forms():
    assert crossplay.parse_agent("ADAP:models/a@1,0,0") == ("ADAP", ("models/a", [1.0, 0.0, 0.0]))
    assert crossplay.parse_agent("ADAP:models/a@-0.25") == ("ADAP", ("models/a", [-0.25]))
    assert crossplay.parse_agent("ADAP:models/a@sample") == ("ADAP", ("models/a", "sample"))
    assert crossplay.parse_agent("ADAP:run@3/a@sample") == ("ADAP", ("run@3/a", "sample"))        # the last @ splits
    # the forms that were there stay what they were
    assert crossplay.parse_agent("DEFAULT") == ("DEFAULT", None)
    assert crossplay.parse_agent("BC:c.pt") == ("BC", "c.pt")
    assert crossplay.parse_agent("models/a") == ("PPO", "models/a")


@pytest.mark.parametrize("agent", ["ADAP:models/a", "ADAP:", "ADAP:@1,0", "ADAP:models/a@", "ADAP:models/a@one", "ADAP:m@1,,2"])
def test_parse_agent_refusals_name_the_form(agent):
    with pytest.raises(EnvException, match="ADAP:<path>@"):
        crossplay.parse_agent(agent)


def test_crossplay_plan_checks_adap_agents_before_a_device_is_touched():
    args = crossplay.build_parser().parse_args(["LiarsDice-v0", "--agents", "ADAP:m@1,0,0", "ADAP:m@sample", "DEFAULT", "--n-envs", "9"])
    assert crossplay.plan(args)["n_pairs"] == 9
    args = crossplay.build_parser().parse_args(["LiarsDice-v0", "--agents", "ADAP:m", "DEFAULT", "--n-envs", "9"])
    with pytest.raises(EnvException, match="ADAP:<path>@"):
        crossplay.plan(args)


# ---- what a member sees: rows and sampled contexts against numpy -----------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["l2", "categorical"])
@pytest.mark.parametrize("cs", [1, 3, 52])
def test_member_rows_and_sampled_contexts_are_the_numpy_statement(cs, sampler):
    n, seed = 37, 0x1234567 + cs
    rng = np.random.default_rng(cs)
    env_space = nat.make_space(nat.PH_SPACE_DISCRETE, 30, LIAR_NVEC)
    obs = (rng.random((n, 30)) * np.asarray(LIAR_NVEC)).astype(np.int64).astype(np.float32)
    obs[0, 7], obs[n - 1, 0], obs[5, 29] = 99.0, -3.0, 12.0                         # clamped components
    # the first deal draws every table at counter 0; a later step redraws the dealt tables only
    ctx0, _ = nat.adap_vec_host(cs, n, sampler=sampler, seed=seed, counter=0)
    assert np.array_equal(ctx0.view(np.uint32), A.draw_contexts(sampler, cs, seed, 0, np.arange(n)).view(np.uint32))
    dealt = (rng.random(n) < 0.4).astype(np.uint8)
    ctx1, rows = nat.adap_vec_host(cs, n, sampler=sampler, seed=seed, counter=11, redraw=dealt, contexts=ctx0, env_space=env_space,
                                   obs=obs)
    want = ctx0.copy()
    want[dealt != 0] = A.draw_contexts(sampler, cs, seed, 11, np.nonzero(dealt)[0])
    assert np.array_equal(ctx1.view(np.uint32), want.view(np.uint32))
    assert dealt.any() and not dealt.all()
    if cs > 1 or sampler == "l2":                                                    # (categorical over one category is constant)
        assert not np.array_equal(ctx1, ctx0)
    assert rows.shape == (n, 270 + cs)
    assert np.array_equal(rows.view(np.uint32), A.rows(LIAR_NVEC, obs, want).view(np.uint32))
    assert (rows[:, :270].sum(axis=1) == 30).all()
    # a stated member: every table's row ends in the latent
    latent = rng.standard_normal(cs).astype(np.float32)
    _, rows = nat.adap_vec_host(cs, n, contexts=np.tile(latent, (n, 1)), env_space=env_space, obs=obs)
    assert np.array_equal(rows.view(np.uint32), A.rows(LIAR_NVEC, obs, np.tile(latent, (n, 1))).view(np.uint32))
    # two members that loaded one file draw under different seeds: different streams
    other = A.draw_contexts(sampler, cs, seed + 1, 0, np.arange(n))
    if cs > 1 or sampler == "l2":                                                    # (categorical over one category is constant)
        assert not np.array_equal(other, ctx0)


def test_native_bindings_exist():
    assert ("spec", "context_size", "sampler", "contexts", "draw") == tuple(f[0] for f in nat.PhPoolAdap._fields_)
    for name in ("ph_pool_forward_adap", "ph_liar_pool_step_adap", "ph_liar_xplay_step_adap"):
        assert name in nat.SIGNATURES
        assert len(nat.SIGNATURES[name]) == len(nat.SIGNATURES[name.replace("_adap", "_arch")]) + 1
