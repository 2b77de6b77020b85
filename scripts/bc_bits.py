#!/usr/bin/env python
"""The bits of behavioural-cloning training, one sha256 per case: what a change to csrc/ph_bc.hip that is meant to leave the
arithmetic alone is compared on, before and after.  A digest covers (params, adam_m, adam_v, opt_step, stats) after BC.train.

Every trainable shape class of tests/bc_cases.py on the checker's data, N = 77 rows, two epochs of teacher-forced orders under
torch's default betas (non-zero moments and the running bias corrections take part), (ent_weight, l2_weight) = (0.5, 0.25),
batch 32 (a 13-row last minibatch) and batch 50 (two tiles per minibatch), as one launch and as one launch per minibatch
(on_batch_end).  The run is made twice: in this process under the environment as it is, and in a fresh process with PH_BC_MFMA=0
(bc_train_kernel on every shape; the switch is read once per process).

The digests belong to a compiler version as much as to the source: compare two builds by the same compiler, nothing else.

    python scripts/bc_bits.py > bits.txt"""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import bc_cases as B  # noqa: E402
from tests import helpers as H  # noqa: E402

N, EPOCHS, ENT_WEIGHT, L2_WEIGHT = 77, 2, 0.5, 0.25
BATCHES = (32, 50)


def digest(case, batch, per_batch):
    from pantheonrl_amd.bc import BC
    from pantheonrl_amd.common import TransitionsMinimal
    orac, obs, acts = B.checker(case, N)
    clone = BC(H.to_space(case.obs), H.to_space(case.act), expert_data=TransitionsMinimal(obs, acts), ent_weight=ENT_WEIGHT,
               l2_weight=L2_WEIGHT, batch_size=batch)
    clone.policy.set_flat_params(orac.flat_params())
    orders = np.stack([B.permutation(N, seed=ep) for ep in range(EPOCHS)])
    stats = clone.train(n_epochs=EPOCHS, orders=orders, on_batch_end=(lambda: None) if per_batch else None)
    h = hashlib.sha256()
    for part in (clone.policy.get_flat_params(), clone.adam_m.cpu().numpy(), clone.adam_v.cpu().numpy(), clone.opt_step.cpu().numpy(),
                 stats):
        h.update(np.ascontiguousarray(part).tobytes())
    return h.hexdigest()


def run():
    from pantheonrl_amd import _native as nat
    env = "PH_BC_MFMA=" + os.environ.get("PH_BC_MFMA", "default")
    for case in B.TRAINABLE:
        path = nat.bc_train_path(B.native_spec(case))
        for batch in BATCHES:
            for per_batch in (False, True):
                print(f"{env} path={path} {case.id} batch={batch} {'on_batch_end' if per_batch else 'one_launch'} "
                      f"{digest(case, batch, per_batch)}", flush=True)


if __name__ == "__main__":
    run()
    if "--no-child" not in sys.argv:
        sys.stdout.flush()
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "--no-child"], cwd=ROOT,
                                env={**os.environ, "PH_BC_MFMA": "0"}, timeout=900).returncode)
