"""not-gpu: the device-resident move log of the vectorised Liar's Dice step -- the new symbols and struct of the C ABI, the host
statement of the export (scan + seat filter) on hand-made logs, and what the command lines accept and refuse before a device is
touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pantheonrl_amd import _native as nat
from pantheonrl_amd import tester, trainer
from pantheonrl_amd.common.trajsaver import TurnBasedTransitions
from pantheonrl_amd.common.wrappers import ALT_DONE, ALT_NOT_DONE, EGO_DONE, EGO_NOT_DONE
from pantheonrl_amd.envs.vec import RECORD_SEATS, export_recording
from pantheonrl_amd.trainer import EnvException

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "pantheon_hip.h")).read()


# ---- 1. symbols and the struct -------------------------------------------------------------------------------------------------
def test_record_symbols_are_declared_and_exported():
    lib = nat.load()
    for name in ("ph_liar_record_attach", "ph_liar_record_export"):
        assert re.search(r"^int\s+" + name + r"\s*\(", HEADER, flags=re.M), name
        assert hasattr(lib, name) and name in nat.SIGNATURES
    assert lib.ph_abi_version() == 7                                   # additive: the version stays
    assert int(re.search(r"#define PH_ABI_VERSION (\d+)", HEADER).group(1)) == 7
    body = re.search(r"typedef struct ph_liar_record \{(.*?)\} ph_liar_record;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip(" *") for n in re.sub(r"^(?:const\s+)?(?:unsigned\s+)?(?:long\s+long|[a-z_]+)\s", "", decl).split(",")]
    assert [n for n, _ in nat.PhLiarRecord._fields_] == names == ["n", "cap", "rows", "member", "count", "count_alt", "dropped", "pending"]
    assert C.sizeof(nat.PhLiarRecord) == 8 + 6 * 8                      # two ints share a slot, six pointers
    assert nat.RECORD_ROW == 33 and (EGO_NOT_DONE, ALT_NOT_DONE, EGO_DONE, ALT_DONE) == (0, 1, 2, 3)
    # the structs the new entry points sit beside keep their pinned sizes
    assert C.sizeof(nat.PhPoolMember) == 80


def test_null_context_is_an_error_text_not_a_crash():
    lib = nat.load()
    rec = nat.PhLiarRecord()
    assert lib.ph_liar_record_attach(None, None) != 0 and b"null" in lib.ph_last_error()
    assert lib.ph_liar_record_attach(None, C.byref(rec)) != 0 and b"null" in lib.ph_last_error()
    assert lib.ph_liar_record_export(None, C.byref(rec), -1, None, None, None, 0) != 0 and b"null" in lib.ph_last_error()


# ---- 2. the export's host statement --------------------------------------------------------------------------------------------
def _log(flags_per_table, cap):
    """a hand-made log: table e holds len(flags) rows whose every component names (table, row), flag as given; rows past the
    count are poisoned"""
    E = len(flags_per_table)
    rows = np.full((E, cap, 33), -77.0, np.float32)
    counts = np.zeros(E, np.int64)
    for e, flags in enumerate(flags_per_table):
        counts[e] = len(flags)
        for r, f in enumerate(flags):
            rows[e, r, :32] = 100 * e + r
            rows[e, r, 32] = f
    return rows, counts


def test_export_is_a_scan_of_the_counts_and_a_seat_filter():
    # an empty table in front, in the middle and at the end; a full table (cap rows); every flag
    tables = [[], [1, 0, 1, 2], [], [0, 3, 1, 0, 1, 0], [3], []]
    cap = 6
    rows, counts = _log(tables, cap)
    dense, offsets = export_recording(rows, counts)
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 0, 4, 4, 10, 11, 11]
    assert dense.shape == (11, 33) and not (dense == -77.0).any()
    assert dense[:, 0].tolist() == [100, 101, 102, 103, 300, 301, 302, 303, 304, 305, 400]     # table-major, each table in order
    assert dense[:, 32].tolist() == [1, 0, 1, 2, 0, 3, 1, 0, 1, 0, 3]
    full = TurnBasedTransitions(dense[:, :30], dense[:, 30:32], dense[:, 32])
    for seat, side in ((0, full.get_ego_transitions()), (1, full.get_alt_transitions())):
        part, off = export_recording(rows, counts, seat)
        want = [sum(1 for f in t if f % 2 == seat) for t in tables]
        assert off.tolist() == [0] + np.cumsum(want).tolist()
        assert np.array_equal(part, dense[dense[:, 32].astype(int) % 2 == seat])                # the host's selection, in order
        assert np.array_equal(part[:, :30], side.obs) and np.array_equal(part[:, 30:32], side.acts)
    assert export_recording(rows, counts, 0)[1][-1] + export_recording(rows, counts, 1)[1][-1] == 11
    # a cursor past the table is clamped: nothing is read past rows[e]
    over = counts.copy()
    over[3] = 9
    assert np.array_equal(export_recording(rows, over)[0], dense)
    # N = 0: no table holds a row; one seat holds none
    none, off = export_recording(*_log([[], [], []], 4))
    assert none.shape == (0, 33) and off.tolist() == [0, 0, 0, 0]
    ego_only, off = export_recording(*_log([[0, 2], [0]], 2), seat=1)
    assert ego_only.shape == (0, 33) and off.tolist() == [0, 0, 0]
    assert RECORD_SEATS == {None: -1, 0: 0, 1: 1}


# ---- 3. the command lines, before a device is touched --------------------------------------------------------------------------
def _trainer_args(argv):
    return trainer.parse_cli(argv)


@pytest.mark.parametrize("alts", [["PPO"], ["PPO", "DEFAULT"]])
def test_trainer_accepts_record_with_n_envs_for_liars_dice(alts):
    args = _trainer_args(["LiarsDice-v0", "PPO"] + alts + ["--n-envs", "32", "--record", "f.npy"])
    trainer.vectorised_record_check(args)                              # no exception
    assert args.record == "f.npy"
    plan = trainer.pool_plan(args)
    assert (plan is None) == (alts == ["PPO"])
    # sized from the run: at most 3 moves per step plus the first opening
    assert trainer.record_capacity(4, 16) == 3 * 4 * 16 + 1


@pytest.mark.parametrize("env", ["RPS-v0", "BlockEnv-v0", "BlockEnv-v1"])
def test_trainer_refuses_record_with_n_envs_for_the_other_games(env, monkeypatch):
    monkeypatch.setattr(nat, "Context", None)            # touching a device would be a TypeError, not an EnvException
    with pytest.raises(EnvException, match="recorder exists for LiarsDice-v0"):
        trainer.run([env, "PPO", "PPO", "--n-envs", "8", "--record", "f.npy"])
    trainer.vectorised_record_check(_trainer_args([env, "PPO", "PPO", "--n-envs", "8"]))     # without --record: as before


@pytest.mark.parametrize("env", ["LiarsDice-v0", "RPS-v0"])
def test_trainer_still_refuses_framestack_with_n_envs(env, monkeypatch):
    monkeypatch.setattr(nat, "Context", None)
    with pytest.raises(EnvException, match="--framestack"):
        trainer.run([env, "PPO", "PPO", "--n-envs", "8", "--framestack", "2", "--record", "f.npy"])
    with pytest.raises(EnvException, match="--framestack"):
        trainer.run([env, "PPO", "PPO", "--n-envs", "8", "-f", "3"])


@pytest.mark.parametrize("env", ["RPS-v0", "BlockEnv-v0", "BlockEnv-v1"])
def test_tester_refuses_the_other_games_and_framestack_with_n_envs(env, monkeypatch):
    monkeypatch.setattr(nat, "Context", None)
    monkeypatch.setattr(tester, "gen_load", None)
    with pytest.raises(EnvException, match="LiarsDice-v0, not " + env):
        tester.run([env, "PPO", "DEFAULT", "--ego-load", "m", "--n-envs", "8", "--record", "f.npy"])
    with pytest.raises(EnvException, match="--framestack"):
        tester.run(["LiarsDice-v0", "PPO", "DEFAULT", "--ego-load", "m", "--n-envs", "8", "--framestack", "2", "--record", "f.npy"])


def test_crossplay_cli_takes_record():
    from pantheonrl_amd import crossplay as xcli
    args = xcli.build_parser().parse_args(["LiarsDice-v0", "--agents", "a", "DEFAULT", "--n-envs", "16", "-t", "8", "--record", "g.npy"])
    assert args.record == "g.npy" and xcli.plan(args) == dict(n_members=2, n_pairs=4, episodes_per_table=2)
    assert xcli.build_parser().parse_args(["LiarsDice-v0", "--agents", "a"]).record is None
