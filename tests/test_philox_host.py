"""not-gpu: tests/philox_ref.py, the host statement of the project's random stream -- the published Philox4x32-10 known answers,
agreement with the product's own host statement of word 0 (envs/vec.py::philox_word0), and the written map of who draws what,
with its disjointness asserted from the project's constants.  tests/test_gpu_sampler_streams.py holds every device draw to this
statement."""
import numpy as np
import pytest

from pantheonrl_amd import _native as nat
from pantheonrl_amd.envs import liar as liar_game
from pantheonrl_amd.envs import vec as V
from tests import philox_ref as R
from tests import sampler_cases as S


# ---- known answers -------------------------------------------------------------------------------------------------------------------
# Random123's kat_vectors, philox4x32 with 10 rounds: (counter words, key words, expected words)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_published_known_answers_all_four_words(ctr, key, want):
    got = R.philox4x32_10_words(*ctr, *key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [int(w) for w in got] == list(want), [hex(int(w)) for w in got]
    # the same vector through the project's call: (key, counter, row, block) with the counter words (row, block, lo, hi)
    got2 = R.philox4x32_10(key[0] | key[1] << 32, ctr[2] | ctr[3] << 32, ctr[0], ctr[1])
    assert np.array_equal(got2, got)
    # the product's host statement asserts word 0 of the first two (tests/test_pool_host.py): the same numbers
    assert int(V.philox_word0(key[0] | key[1] << 32, ctr[2] | ctr[3] << 32, np.array([ctr[0]]), ctr[1])[0]) == want[0]


def test_word0_agrees_with_the_products_host_statement_on_random_coordinates():
    rng = np.random.default_rng(0)
    rows = rng.integers(0, 1 << 32, size=512, dtype=np.uint64)
    for _ in range(8):                                                     # 8 x 512 coordinates, high words in use
        key, ctr = int(rng.integers(0, 1 << 63)) * 2 + 1, int(rng.integers(0, 1 << 63)) * 2 + 1
        assert key >> 32 and ctr >> 32
        block = int(rng.integers(0, 1 << 32))
        mine = R.philox4x32_10(key, ctr, rows, block)
        assert mine.shape == (512, 4)
        assert np.array_equal(mine[:, 0], V.philox_word0(key, ctr, rows, block))
    for key, ctr, block in ((5, 0, 0), (5, 9, 100), (2 ** 40 + 3, 2 ** 33 + 1, 101), (7, 2 ** 32 + 5, 2)):
        assert np.array_equal(R.philox4x32_10(key, ctr, np.arange(300), block)[:, 0], V.philox_word0(key, ctr, np.arange(300), block))
    # every coordinate matters, high words included
    base = R.philox4x32_10(11, 5, np.arange(64), 3)
    for other in (R.philox4x32_10(11 + (1 << 32), 5, np.arange(64), 3), R.philox4x32_10(11, 5 + (1 << 32), np.arange(64), 3),
                  R.philox4x32_10(11, 5, np.arange(64) + 1, 3), R.philox4x32_10(11, 5, np.arange(64), 4)):
        assert (base != other).all(axis=1).mean() > 0.9


def test_uniforms_are_the_top_24_bits_exactly():
    w = np.array([0, 0xFF, 0x100, 0xFFFFFFFF, 0x80000000], np.uint32)
    u = R.to_uniform(w)
    assert u.dtype == np.float32
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5]
    rows = np.arange(1000)
    u4 = R.uniform4(3, 2 ** 35 + 1, rows, 2)
    assert u4.dtype == np.float32 and u4.shape == (1000, 4) and (u4 >= 0).all() and (u4 < 1).all()
    assert np.array_equal(R.uniform(3, 2 ** 35 + 1, rows, 2), u4[:, 0])
    assert np.array_equal(u4.astype(np.float64) * 2 ** 24, (R.philox4x32_10(3, 2 ** 35 + 1, rows, 2) >> 8).astype(np.float64))


def test_epoch_key_is_the_splitmix_finaliser():
    # splitmix64's published first outputs for the state 0: the finaliser of 1 * golden, 2 * golden
    assert R.epoch_key(0, 0) == 0xE220A8397B1DCDAF
    assert R.epoch_key(0, 1) == 0x6E789E6AA1B965F4
    assert R.epoch_key(0x9E3779B97F4A7C15, 0) == R.epoch_key(0, 1)            # seed and epoch enter through one sum
    assert R.epoch_key(2 ** 64 - 1, 0) == R.epoch_key(-1 & R.MASK64, 0) < 2 ** 64
    assert len({R.epoch_key(s, e) for s in range(8) for e in range(8)}) == 64


# ---- the map of the stream --------------------------------------------------------------------------------------------------------------
# who draws what: (stream, key, the blocks / components it can reach, the counters it uses).  Rows of one key must never reach the same
# (block or component, counter); streams under different keys are separated by the key.  The row slot is the table (dice, first mover,
# pool), the global row of the launch (actions) or the context index (ADAP).
ADAP_SALT = R.ADAP_SALT
GAUSS_SECOND = 128                             # csrc/ph_rowtail.h: the Gaussian head's second uniform sits at component c + 128
ADAP_MAX_CTX = 64                              # a context is part of a Box observation row; far below any other user of its key


def stream_map():
    n_dice_blocks = -(-2 * liar_game.N_DICE // 4)
    A = nat.PH_MAX_LOGITS                      # action components: c < A <= L <= PH_MAX_LOGITS
    return [
        dict(stream="dice", key="dice", blocks=range(0, n_dice_blocks), counter="step c"),
        dict(stream="first mover", key="dice", blocks=range(R.FIRST_MOVER_BLOCK, R.FIRST_MOVER_BLOCK + 1), counter="step c"),
        dict(stream="pool resample", key="dice ^ POOL_SEED_SALT", blocks=range(V.POOL_RESAMPLE_BLOCK, V.POOL_RESAMPLE_BLOCK + 1),
             counter="as the pool sets it"),
        dict(stream="action component c", key="policy", blocks=range(0, A), counter="as the forward passes it"),
        dict(stream="Gaussian second uniform", key="policy", blocks=range(GAUSS_SECOND, GAUSS_SECOND + A),
             counter="as the forward passes it"),
        dict(stream="ADAP contexts", key="epoch_key((seed ^ ADAP_SALT) + epoch, minibatch)", blocks=range(0, ADAP_MAX_CTX), counter="1"),
        dict(stream="Liar training, ego", key="ego policy", blocks=range(0, A), counter="c"),
        dict(stream="Liar training, seat 1", key="seat-1 policy", blocks=range(0, A), counter="2c, 2c + 1"),
    ]


def test_stream_map_consumers_under_one_key_are_disjoint():
    rows = stream_map()
    assert len({r["stream"] for r in rows}) == len(rows) == 8
    by_key = {}
    for r in rows:
        by_key.setdefault(r["key"], []).append(r)
    for key, users in by_key.items():
        for i, a in enumerate(users):
            for b in users[i + 1:]:
                assert not set(a["blocks"]) & set(b["blocks"]), (key, a["stream"], b["stream"])
    # the constants behind it, read from the project; the two that only the kernels' text holds are checked against that text
    import os
    csrc = os.path.join(os.path.dirname(os.path.abspath(nat.__file__)), "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("ph_rowtail.h", "ph_adap.hip", "ph_adapmult.hip", "ph_liar.h", "ph_pool.h")}
    assert "(uint32_t)(c + %d)" % GAUSS_SECOND in text["ph_rowtail.h"]
    assert all("a.seed ^ 0x%Xull" % ADAP_SALT in text[f] for f in ("ph_adap.hip", "ph_adapmult.hip"))
    assert "(uint32_t)e, %du)" % R.FIRST_MOVER_BLOCK in text["ph_liar.h"] and "%du," % V.POOL_RESAMPLE_BLOCK in text["ph_pool.h"]
    assert nat.PH_MAX_LOGITS <= GAUSS_SECOND                                   # component c and c + 128 never overlap
    assert 2 * liar_game.N_DICE == 2 * R.LIAR_DICE == 12 and liar_game.N_SIDES == R.LIAR_SIDES
    dice = set(by_key["dice"][0]["blocks"])
    assert dice == {0, 1, 2} and R.FIRST_MOVER_BLOCK == 100 and V.POOL_RESAMPLE_BLOCK == 101
    assert len({R.FIRST_MOVER_BLOCK, V.POOL_RESAMPLE_BLOCK} | dice) == 5        # disjoint even if the salt were dropped
    assert V.POOL_SEED_SALT & 0x7FFFFFFFFFFFFFFF != 0                          # the pool's key is another key than the dice's
    for seed in (0, 5, 2 ** 40 + 3):
        assert (seed ^ V.POOL_SEED_SALT) & 0x7FFFFFFFFFFFFFFF != seed
    # Liar training: step c uses the ego's counter c and seat 1's counters 2c (reply) and 2c + 1 (opening): no two steps share one
    counters = [V.VecLiarTraining._counters(None, c) for c in range(0, 200)]
    assert all(k == (c, 2 * c, 2 * c + 1) for c, k in enumerate(counters))
    seat1 = [x for _, r, o in counters for x in (r, o)]
    assert len(set(seat1)) == len(seat1) and len({e for e, _, _ in counters}) == len(counters)
    # ADAP's key moves with the epoch word and the minibatch, and is not the permutation's key of the same seed
    keys = {R.epoch_key((7 ^ ADAP_SALT) + e, mb) for e in range(4) for mb in range(4)}
    assert len(keys) == 16 and not keys & {R.epoch_key(7 + e, mb) for e in range(4) for mb in range(4)}


def test_host_deal_is_a_deal():
    """the host statement of the Liar's Dice deal: six dice a player, tables differ, the two hands of a table differ, the first mover
    follows probegostart"""
    tables = np.arange(300)
    for key, ctr in ((5, 0), (5, 9), (2 ** 40 + 3, 2 ** 33 + 1)):
        h = R.liar_deal(key, ctr, tables)
        assert h.shape == (300, 12) and (h[:, :6].sum(1) == 6).all() and (h[:, 6:].sum(1) == 6).all()
        assert len({tuple(r) for r in h.tolist()}) > 290
        assert (h[:, :6] != h[:, 6:]).any(1).mean() > 0.9
        assert not np.array_equal(h, R.liar_deal(key, ctr + 1, tables))
        assert not np.array_equal(h, R.liar_deal(key, ctr + 2 ** 32, tables))
        f = R.liar_ego_first(key, ctr, tables, 0.25)
        assert 0.15 < f.mean() < 0.35 and (R.liar_ego_first(key, ctr, tables, 0.5) >= f).all()


# ---- the GPU test's inputs decide: checked on the checker alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in S.CASES])
def test_sampler_cases_meet_the_caps_and_the_negative_control_on_the_checker(cid):
    """tests/test_gpu_sampler_streams.py leaves out rows whose uniform lies within helpers.EDGE_MARGIN of a CDF edge of the checker:
    for the key, counters and observation seeds it uses there is no such row at n <= 65 and at most 3 % at n >= 257, and a shifted
    row, component, counter (low or high word) or key high word moves the predicted action in at least 20 % of the rows"""
    case = S.BY_ID[cid]
    assert S.KEY >> 32 and S.KEY & 0xFFFFFFFF and any(c >> 32 for c in S.COUNTERS)
    for n in case.rows:
        obs, mask = S.inputs(case, n)
        probs = S.probabilities64(case, obs, mask)
        assert all(p.dtype == np.float64 and np.abs(p.sum(1) - 1).max() < 1e-12 for p in probs)
        for c in S.COUNTERS:
            acts, near = S.predict(probs, S.uniforms(n, len(probs), S.KEY, c))
            ctl = S.control(probs, n, S.KEY, c)
            print(cid, "n", n, "counter", c, "near", int(near.sum()), "control", {k: round(v, 3) for k, v in ctl.items()})
            S.assert_caps_and_control(cid, n, near, ctl, c)
            assert (acts >= 0).all() and (acts < np.asarray(S.spaces(case)[1].nvec)).all()
            if mask is not None:                                   # a masked entry has probability e^-30: never drawn
                lo = np.concatenate([[0], np.cumsum(S.spaces(case)[1].nvec)[:-1]])
                assert mask[np.arange(n)[:, None], lo[None, :] + acts].all()


@pytest.mark.parametrize("E,T", S.ROLLOUT_SHAPES)
def test_rollout_cases_meet_the_caps_and_the_control_on_the_checker(E, T):
    obs = S.rollout_data(E, T).obs.numpy()
    assert obs.shape == (T, E, 62)
    for c0, epoch in S.ROLLOUT_RUNS:
        acts, near, ctl = S.rollout_prediction(obs, S.KEY, c0, epoch)
        print((E, T), "counter", c0, "epoch", epoch, "near", int(near.sum()), "control", {k: round(v, 3) for k, v in ctl.items()})
        S.assert_rollout_caps((E, T, c0, epoch), near, ctl)
        assert acts.shape == (T, E)
        assert T == 1 or (acts[0] != acts[1]).any()
    # the epoch word is a coordinate: the same rollout under another word is another rollout
    a0 = S.rollout_prediction(obs, S.KEY, 7, 0)[0]
    assert (a0 != S.rollout_prediction(obs, S.KEY, 7, 1)[0]).mean() >= S.CONTROL_MIN


def test_pool_case_meets_the_caps_and_the_control_on_the_checker():
    obs, pid, active = S.pool_inputs()
    assert len({tuple(r) for r in obs.tolist()}) == S.POOL_N and set(pid.tolist()) == {0, 1} and 0 < (active == 0).sum() < 10
    for c in S.COUNTERS:
        acts, near, ctl = S.pool_prediction(obs, pid, c)
        S.assert_rollout_caps(("pool", c), near, ctl)
        assert len(np.unique(acts, axis=0)) > 10
