"""The clone, its reset and the train-path assertion of the BC shape tests (tests/test_gpu_bc_shapes.py), shared with the
sharp-policy tests."""
import os

import numpy as np

from tests import helpers as H


VALU_ONLY = os.environ.get("PH_BC_MFMA", "1").startswith("0")


def _clone(case, obs, acts, batch_size=128, **opt):
    from pantheonrl_amd.bc import BC
    from pantheonrl_amd.common import TransitionsMinimal
    return BC(H.to_space(case.obs), H.to_space(case.act), expert_data=TransitionsMinimal(obs, acts),
              optimizer_kwargs=dict(betas=(0.0, 0.999), **opt), batch_size=batch_size)


def _reset(clone, p0, ent_weight, l2_weight):
    clone.policy.set_flat_params(p0)
    H.load_device_adam_state(clone, np.zeros_like(p0), np.zeros_like(p0), 0)
    clone.ent_weight, clone.l2_weight = float(ent_weight), float(l2_weight)


def _assert_path(case, clone):
    from pantheonrl_amd import _native as nat
    want = min(case.path, 1) if VALU_ONLY else case.path
    assert nat.bc_train_path(clone.policy.spec) == want, (case.id, nat.bc_train_path(clone.policy.spec), want)
    return want
