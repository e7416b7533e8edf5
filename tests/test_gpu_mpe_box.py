"""GPU tests (`-m gpu`) of the Box-action step kernels tsm_mpe_spread_step_box / tsm_mpe_tag_step_box (csrc/mpe.hip, csrc/mpe_tag.hip,
mpe_box_action_force in csrc/mpe_dev.h) behind `continuous_actions=True` of both device envs.  Shapes: n_env 17 (a full 16-env
workgroup and a ragged one of 1) and 1; spread N in {1, 3, 8}; tag at its smallest and its largest."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

import mpe_box_ref as ref  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.env.mpe_tag import DeviceSimpleTagVectorEnv

SHAPES = [(k, s, E) for k, s in (("spread", (1,)), ("spread", (3,)), ("spread", (8,)), ("tag", (1, 1, 0)), ("tag", (4, 4, 4))) for E in (17, 1)]
IDS = [f"{k}{'x'.join(map(str, s))}-E{E}" for k, s, E in SHAPES]
OUTS = ("obs_next", "rew", "terminated", "truncated", "done_env", "obs_cur", "agent_pos", "agent_vel", "landmark_pos", "steps", "episode_ctr", "rng_tick")


def _env(kind, sizes, E, box, max_cycles=3, auto_reset=True):
    kw = dict(max_cycles=max_cycles, device=DEV, seed=7, auto_reset=auto_reset, continuous_actions=box)
    return DeviceSimpleSpreadVectorEnv(E, sizes[0], **kw) if kind == "spread" else DeviceSimpleTagVectorEnv(E, sizes[1], sizes[0], sizes[2], **kw)


@pytest.mark.parametrize("kind,sizes,E", SHAPES, ids=IDS)
def test_one_hot_actions_give_the_discrete_step_bit_for_bit(kind, sizes, E):
    d, c = _env(kind, sizes, E, False), _env(kind, sizes, E, True)
    assert torch.equal(d.reset_device(), c.reset_device()) and c.act_dim == 5 and c.action_space[0].shape == (5,)
    rng = np.random.default_rng(0)
    for t in range(2 * 3 + 1):   # max_cycles 3, auto_reset: the reset path is crossed twice
        a = torch.from_numpy(rng.integers(0, 5, (E, d.n_agent)).astype(np.int32)).to(DEV)
        d.step_device(a, rng_tick_inc=3)
        c.step_device(torch.nn.functional.one_hot(a.long(), 5).float().contiguous(), rng_tick_inc=3)
        for name in OUTS:
            assert torch.equal(getattr(d, name), getattr(c, name)), (t, name)
    assert int(d.episode_ctr.min()) == 3


@pytest.mark.parametrize("actions", ["uniform", "unclamped"])
@pytest.mark.parametrize("kind,sizes,E", SHAPES, ids=IDS)
def test_general_actions_match_float64(kind, sizes, E, actions):
    """Each of five steps against mpe_box_ref.step_box from the device's own pre-step state at the single-step bar of the discrete
    kernels against the same oracles (rtol = atol = 2e-5: test_gpu_pipeline.py:82-83, test_gpu_tag.py:444; tag rewards atol 2e-4:
    test_gpu_tag.py:451; rewards of envs with a contact decision within CLEAR = 1e-5 of its threshold left out: env_cases.py:52), and
    the trajectory chained on the float64 side at the chained bar (2e-3: test_gpu_pipeline.py:47).  "unclamped" puts components at
    -0.5 and 1.7: a kernel that clamped to the Box would miss the velocity by 1.2 accel dt >= 0.36."""
    env = _env(kind, sizes, E, True, max_cycles=50, auto_reset=False)
    env.reset_device()
    NL, rng = (sizes[0] if kind == "spread" else sizes[2]), np.random.default_rng(1)
    chain = [ref.make_world(kind, sizes, 50) for _ in range(E)]
    for t in range(5):
        state = [x.cpu().numpy().astype(np.float64) for x in (env.agent_pos, env.agent_vel, env.landmark_pos[:, :NL])]
        a = rng.uniform(0, 1, (E, env.n_agent, 5)).astype(np.float32)
        if actions == "unclamped":
            a[..., 1 + 2 * (t % 2)], a[..., 2 + 2 * (t % 2)] = -0.5, 1.7
        obs_next, rew, _, trunc, _ = (x.cpu().numpy() for x in env.step_device(torch.from_numpy(a).to(DEV)))
        assert not trunc.any()
        for e, wc in enumerate(chain):
            w = ref.make_world(kind, sizes, 50)
            w.set_state(*(x[e] for x in state), steps=t)
            if t == 0:
                wc.set_state(*(x[e] for x in state))
            o, r, _, _ = ref.step_box(w, a[e])
            np.testing.assert_allclose(obs_next[e], o, rtol=2e-5, atol=2e-5, err_msg=f"step {t} env {e}")
            if ref.decision_margin(w) > 1e-5:
                np.testing.assert_allclose(rew[e], r, rtol=2e-5, atol=2e-5 if kind == "spread" else 2e-4, err_msg=f"step {t} env {e}")
            np.testing.assert_allclose(obs_next[e], ref.step_box(wc, a[e])[0], rtol=2e-3, atol=2e-3, err_msg=f"chained, step {t} env {e}")


@pytest.mark.parametrize("kind,sizes", [("spread", (3,)), ("tag", (3, 1, 2))])
def test_argument_checks(kind, sizes):
    box, disc = _env(kind, sizes, 4, True), _env(kind, sizes, 4, False)
    N = box.n_agent
    with pytest.raises(ValueError, match="continuous_actions=True"):
        box.step_device(torch.zeros(4, N, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="must be int32"):
        disc.step_device(torch.zeros(4, N, 5, device=DEV))
    with pytest.raises(ValueError, match=r"\[4, %d, 5\]" % N):
        box.step_device(torch.zeros(4, N, 4, device=DEV))
    box.reset_device()
    assert torch.isfinite(box.step_device(torch.rand(4 * N, 5, device=DEV))[0]).all()   # [n_env * N, 5] is the same call
    entry, cfg = ("tsm_mpe_spread_step_box", box._cfg) if kind == "spread" else ("tsm_mpe_tag_step_box", box._tag_cfg)
    with pytest.raises(ValueError, match=entry + ": null pointer"):   # act is checked for null on the host
        _abi.call(entry, C.byref(cfg), 0, 1, None, *([1] * 10), 1, None, 0, None)
