"""gpu: the one Liar's Dice step behind self-play, the partner pool and cross-play -- each driver's native step against the shared
walk after every step at a table count that leaves partial 16-row tiles, and the null check of the self-play entry points."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from tests.test_gpu_crossplay import _state as _xplay_state
from tests.test_gpu_crossplay import _xplay
from tests.test_gpu_parity import _liar_selfplay
from tests.test_gpu_pool import RB_KEYS, _pool

pytestmark = pytest.mark.gpu

BASE = ("ego_first", "obs_ego", "obs_alt")          # what VecLiarStep owns, besides the game (env.hands / history / nmoves)


def _learner_state(prefix, m):
    """a learner's cursor, flags, value cache and the recorded rows of its ragged buffer"""
    pos = m.pos.cpu().numpy()
    out = {prefix + "pos": pos, prefix + "flags": np.stack([t.cpu().numpy() for t in (m.boundary, m.term, m.open)]),
           prefix + "values": m.values.cpu().numpy()}
    for k, v in m.model.rollout_buffer.host().items():
        if k in RB_KEYS:
            out[prefix + k] = v[np.arange(v.shape[0])[:, None] < pos[None, :]]
    return out


def _training_state(sp, ego, learners):
    th.cuda.synchronize()
    out = {k: getattr(sp, k).cpu().numpy().copy() for k in BASE + ("alt_acted",)}
    out.update(hands=sp.env.hands.cpu().numpy(), history=sp.env.history.cpu().numpy(), nmoves=sp.env.nmoves.cpu().numpy(),
               episodes=sp.episodes, es=ego._last_episode_starts.cpu().numpy().copy())
    out.update({"e_" + k: v for k, v in ego.model.rollout_buffer.host().items() if k in RB_KEYS})
    for i, m in enumerate(learners):
        out.update(_learner_state(f"a{i}_", m))
    return out


def _driver(mode, native):
    """-> (driver, state function); both forms of a mode from the same seeds"""
    E = 50
    if mode == "selfplay":
        sp, ego, alt, _ = _liar_selfplay(E, 4, 4, seed=3, native=native)
        return sp, lambda: _training_state(sp, ego, [alt])
    if mode == "pool":
        sp, ego, members = _pool(E, 4, 4, ["learner", "frozen", "scripted"], seed=3, native=native, resample="random")
        return sp, lambda: dict(_training_state(sp, ego, sp.learners), partnerid=sp.partnerid.cpu().numpy().copy(),
                                alt_actions=sp.alt_actions.cpu().numpy().copy())
    xp = _xplay(E, ["frozen", "scripted", "frozen"], 2, native=native)
    return xp, lambda: _xplay_state(xp)


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
        assert sb["episodes"] > 0 and sb["a0_pos"].max() >= 1 and np.abs(sb["e_rewards"][:3]).sum() > 0      # nothing vacuous


def test_selfplay_entry_points_report_a_null_game_pointer():
    """Host validation only: nothing is launched with a bad pointer, so the same object steps afterwards."""
    sp, ego, alt, _ = _liar_selfplay(16, 4, 4, seed=1)
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
