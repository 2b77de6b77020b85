"""-m gpu: the refusals of the forward entry points of the C ABI -- ph_policy_forward / ph_arch_forward, their ragged forms and the
two scripted rollouts.  Every case returns from the host before any launch, so each asserts three things: NativeError is raised,
its message names the entry point that was called (ph_arch_forward never reports as ph_policy_forward), and after a context sync
the sentinel-filled outputs and rollout-buffer rows are untouched.

Shapes are the smallest there are: E = 2, T = 2, the RPS spec (Discrete(1) -> Discrete(3)) on the 64-wide side and with
net_arch (32,) on the tower side."""
import ctypes as C

import pytest
import torch as th

from pantheonrl_amd import _native as nat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, T = 2, 2
SENTINEL = -777.0
RB_KEYS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")


def _spec(obs, act):
    s = nat.PhSpec()
    s.obs, s.act = obs, act
    return s


def _discrete(*nvec):
    return nat.make_space(nat.PH_SPACE_DISCRETE, len(nvec), nvec)


class _World:
    """one context, one buffer and one set of argument tensors for every case"""

    def __init__(self):
        self.ctx = nat.Context(0)
        self.ctx.set_stream(th.cuda.current_stream(th.device(DEV)).cuda_stream)
        self.lib, self.h = self.ctx.lib, self.ctx.handle
        self.rps = _spec(_discrete(1), _discrete(3))
        self.two = _spec(_discrete(1), _discrete(3, 3))                      # two action components: not the 16-row shape class
        self.gauss = _spec(_discrete(1), nat.make_space(nat.PH_SPACE_BOX, 1))
        self.arch = nat.make_arch((32,))
        P = max(nat.layout_of(self.rps).P, nat.layout_of(self.two).P, nat.layout_of(self.gauss).P,
                nat.arch_layout_of(self.rps, self.arch).P)
        f = lambda *s: th.zeros(*s, dtype=th.float32, device=DEV)  # noqa: E731
        self.params = f(P + 4)                                               # room for the view one float further on
        self.obs = f(T + 1, E, 1)                                            # a forward's rows, or a scripted sequence
        self.rew, self.done, self.es, self.pending = f(T + 1, E), f(T + 1, E), f(E), f(E)
        self.mask = th.ones((E, 1), dtype=th.uint8, device=DEV)
        self.pos_env = th.zeros(E, dtype=th.int32, device=DEV)
        self.rec = th.ones(E, dtype=th.uint8, device=DEV)
        self.acts = th.empty((E, 2), dtype=th.int32, device=DEV)
        self.vals, self.lps = f(E), f(E)
        self.rb_arrays = {k: f(T, E, 2 if k == "actions" else 1) for k in RB_KEYS}
        self.rb = nat.PhRollout()
        self.rb.T, self.rb.E = T, E
        for k, t in self.rb_arrays.items():
            setattr(self.rb, k, t.data_ptr())

    def outputs(self):
        return [self.acts, self.vals, self.lps] + list(self.rb_arrays.values())

    def fill(self):
        for t in self.outputs():
            t.fill_(int(SENTINEL) if t.dtype == th.int32 else SENTINEL)

    def untouched(self):
        self.ctx.sync()
        th.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.outputs())


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.ctx.close()


# ---- the calls: keyword overrides on a call that would succeed --------------------------------------------------------------------
def _forward(w, tower, *, spec=None, params="ok", n=E, mask=None, rb=True, pos=0, es=True, pending=False):
    p = {"ok": w.params.data_ptr(), "null": None, "off": w.params.data_ptr() + 4}[params]
    head = (w.h, C.byref(spec or w.rps)) + ((C.byref(w.arch),) if tower else ())
    fn = w.lib.ph_arch_forward if tower else w.lib.ph_policy_forward
    return fn(*head, p, w.obs.data_ptr(), n, nat.ptr(mask), None, None, 5, 1, 0, w.acts.data_ptr(), None, w.vals.data_ptr(),
              w.lps.data_ptr(), None, None, C.byref(w.rb) if rb else None, pos, w.es.data_ptr() if es else None,
              w.pending.data_ptr() if pending else None, 0)


def _ragged(w, tower, *, params="ok", pos_env=True, es=True):
    p = {"ok": w.params.data_ptr(), "null": None, "off": w.params.data_ptr() + 4}[params]
    head = (w.h, C.byref(w.rps)) + ((C.byref(w.arch),) if tower else ())
    fn = w.lib.ph_arch_forward_ragged if tower else w.lib.ph_policy_forward_ragged
    return fn(*head, p, w.obs.data_ptr(), None, 5, 1, 0, w.acts.data_ptr(), w.vals.data_ptr(), w.lps.data_ptr(), C.byref(w.rb),
              w.pos_env.data_ptr() if pos_env else None, w.rec.data_ptr(), w.es.data_ptr() if es else None,
              *((0,) if tower else ()))


def _scripted(w, tower, *, spec=None, params="ok", n=E, n_steps=1, pos0=0, es=True):
    p = {"ok": w.params.data_ptr(), "null": None, "off": w.params.data_ptr() + 4}[params]
    head = (w.h, C.byref(spec or w.rps)) + ((C.byref(w.arch),) if tower else ())
    fn = w.lib.ph_arch_scripted_rollout if tower else w.lib.ph_scripted_rollout
    return fn(*head, p, w.obs.data_ptr(), w.rew.data_ptr(), w.done.data_ptr(), n, n_steps, w.es.data_ptr() if es else None, 5, 1,
              w.acts.data_ptr(), w.vals.data_ptr(), w.lps.data_ptr(), C.byref(w.rb), pos0, 0)


NAMES = {_forward: ("ph_policy_forward", "ph_arch_forward"), _ragged: ("ph_policy_forward_ragged", "ph_arch_forward_ragged"),
         _scripted: ("ph_scripted_rollout", "ph_arch_scripted_rollout")}

# (case, call, overrides, text the message contains) -- run for both twins of the pair
BOTH = [
    ("null_params", _forward, dict(params="null"), "null params/obs"),
    ("null_params", _ragged, dict(params="null"), "null argument"),
    ("null_params", _scripted, dict(params="null"), "null argument"),
    ("misaligned_params", _forward, dict(params="off"), "params must be 16-byte aligned"),
    ("misaligned_params", _ragged, dict(params="off"), "params must be 16-byte aligned"),
    ("misaligned_params", _scripted, dict(params="off"), "params must be 16-byte aligned"),
    ("n_zero", _forward, dict(n=0), "n must be positive"),
    ("n_zero", _scripted, dict(n=0), "n and n_steps must be positive"),
    ("n_not_E", _forward, dict(n=1), "fused add needs n == rollout E"),
    ("n_not_E", _scripted, dict(n=1), "n must equal the rollout buffer's E"),
    ("pos_T", _forward, dict(pos=T), "pos out of range"),
    ("pos_T", _scripted, dict(pos0=T), "must lie in the buffer"),
    ("no_episode_start", _forward, dict(es=False), "fused add needs episode_start_in"),
    ("no_episode_start", _ragged, dict(es=False), "null argument"),
    ("no_episode_start", _scripted, dict(es=False), "null argument"),
    ("pending_without_buffer", _forward, dict(rb=False, pending=True), "pending_reward needs the fused rollout-buffer write"),
    ("pending_at_pos_0", _forward, dict(pos=0, pending=True), "pending_reward needs pos >= 1"),
    ("null_pos_env", _ragged, dict(pos_env=False), "null argument"),
    ("n_steps_zero", _scripted, dict(n_steps=0), "n and n_steps must be positive"),
    ("one_row_past_the_end", _scripted, dict(pos0=1, n_steps=T), "must lie in the buffer"),
]
CASES = [(f"{NAMES[call][tower]}-{case}", call, tower, kw, text) for case, call, kw, text in BOTH for tower in (0, 1)]


def _refused(w, call, tower, kw, text):
    w.fill()
    with pytest.raises(nat.NativeError) as err:
        nat.check(call(w, tower, **kw))
    msg = str(err.value)
    assert msg.startswith(NAMES[call][tower] + ":"), msg
    assert text in msg, msg
    assert w.untouched()


@pytest.mark.parametrize("call,tower,kw,text", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_refusal_names_its_entry_point_and_writes_nothing(world, call, tower, kw, text):
    _refused(world, call, tower, kw, text)


def test_scripted_rollout_refuses_a_spec_outside_the_16_row_shape_class(world):
    _refused(world, _scripted, 0, dict(spec=world.two), "16-row forward")


def test_policy_forward_refuses_a_mask_on_a_gaussian_head(world):
    _refused(world, _forward, 0, dict(spec=world.gauss, mask=world.mask), "categorical heads")
