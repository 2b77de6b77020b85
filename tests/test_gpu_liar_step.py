"""gpu: the one Liar's Dice step behind self-play, the partner pool and cross-play -- each driver's native step against the shared
walk after every step at a table count that leaves partial 16-row tiles, and the null check of the self-play entry points."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from tests import liar_cases as LC

pytestmark = pytest.mark.gpu


def _liar_selfplay(E, T_ego, T_alt, seed=0, native=True):
    """64-wide PPO in both seats, the buffers' default GAE mode"""
    ego, alt = LC.ppo(E, T_ego, seed, gae_mode=None), LC.ppo(E, T_alt, seed + 1, gae_mode=None)
    return LC.selfplay(E, ego, alt, seed=seed, native=native)


def _driver(mode, native):
    """-> (driver, state function); both forms of a mode from the same seeds"""
    E = 50
    if mode == "selfplay":
        sp, ego, alt = _liar_selfplay(E, 4, 4, seed=3, native=native)
        return sp, lambda: LC.train_state(sp, ego)
    if mode == "pool":
        sp, ego, members = LC.pool(E, 4, 4, ["learner", "frozen", "scripted"], seed=3, native=native, resample="random")
        return sp, lambda: LC.train_state(sp, ego)                   # (with the pool's partnerid and alt_actions)
    xp = LC.xplay(E, ["frozen", "scripted", "frozen"], 2, native=native)
    return xp, lambda: LC.xstate(xp)


@pytest.mark.parametrize("mode", ["selfplay", "pool", "crossplay"])
def test_each_native_step_is_bitwise_the_shared_walk_after_every_step(mode):
    (a, state_a), (b, state_b) = (_driver(mode, native) for native in (True, False))
    assert a.native and not b.native and a.E == 50
    moved = False
    for step in range(4):                      # the constructor's deal, then three steps
        sa, sb = state_a(), state_b()
        assert set(sa) == set(sb)
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (mode, step, key)
        moved |= step > 0 and bool((sb["nmoves"] > 0).any())
        if step < 3:
            a.step()
            b.step()
    assert moved and a.steps_done == b.steps_done == 3
    if mode != "crossplay":
        assert sb["episodes"] > 0 and sb["pos0"].max() >= 1 and np.abs(sb["e_rewards"][:3]).sum() > 0      # nothing vacuous


def test_selfplay_entry_points_report_a_null_game_pointer():
    """Host validation only: nothing is launched with a bad pointer, so the same object steps afterwards."""
    sp, ego, alt = _liar_selfplay(16, 4, 4, seed=1)
    sp._bind()
    ctx, d = sp.env.ctx, sp._desc
    lib, h = ctx.lib, ctx.handle
    for field in ("hands", "obs_next", "done"):
        good = getattr(d, field)
        setattr(d, field, None)
        assert lib.ph_liar_selfplay_step(h, C.byref(d), 0, 1, 0) != 0 and b"incomplete" in lib.ph_last_error(), field
        assert lib.ph_last_error().startswith(b"ph_liar_selfplay_step:")
        assert lib.ph_liar_selfplay_rollout(h, C.byref(d), 0, 4, 1) != 0 and b"incomplete" in lib.ph_last_error(), field
        assert lib.ph_last_error().startswith(b"ph_liar_selfplay_rollout:")
        setattr(d, field, good)
    sp.step()
    th.cuda.synchronize()
    host = ego.model.rollout_buffer.host()
    assert all(np.isfinite(host[k][0]).all() for k in ("observations", "actions", "rewards", "values", "log_probs"))
