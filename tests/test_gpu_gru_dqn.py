"""GPU tests (`-m gpu`) of the GRU net under the learner: acting step by step with the hidden state kept in HBM, its reset, the host
`forward(batch, state)`, and one `DQN.update` on a `stack_num = L` buffer.  Reference and bar as in tests/test_gpu_gru_shapes.py."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

from test_gpu_gru_shapes import _bars, _d, _n, _t64, ref_net  # noqa: E402
from test_gpu_recurrent_dqn import _Discrete, _filled  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd.algorithm.dqn import DQN, DiscreteQLearningPolicy
    from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory
    from tianshou_marl_amd.data.batch import Batch
    from tianshou_marl_amd.data.buffer import VectorReplayBuffer
    from tianshou_marl_amd.utils.net import Recurrent


@pytest.mark.parametrize("layers,H,L", [(1, 128, 3), (2, 32, 4)])
def test_acting_steps_equal_one_stacked_forward_and_reset_restarts_env_rows(layers, H, L):
    E, N, D = 9, 2, 6   # 18 rows: a full tile and a partial one
    net = Recurrent(layer_num=layers, state_shape=D, action_shape=4, hidden_layer_size=H, device=DEV, seed=3, cell="gru")
    pol = DiscreteQLearningPolicy(model=net, action_space=_Discrete(4))
    obs = np.random.RandomState(4).standard_normal((E * N, L, D)).astype(np.float32)
    state = net.zero_state(E * N)
    for t in range(L):  # the same steps three times: the policy's kept state, a state of the caller's in place, the host call
        res = pol.act_device(_d(obs[:, t]).view(E, N, D))
        q, new = net(_d(obs[:, t]), state, save=False, state_out=state)
        out = pol(Batch(obs=obs[:, t], info=Batch()), None if t == 0 else out.state)
    assert len(pol._act_state) == 1 and new[0].data_ptr() == state[0].data_ptr()
    assert set(out.state.get_keys()) == {"hidden"} and tuple(out.state.hidden.shape) == (E * N, layers, H)
    rq, rh = (t.detach().numpy() for t in ref_net(net)(_t64(obs)))
    full, (fh,) = net(_d(obs), save=False)
    _bars(f"gru acting layers={layers} H={H} L={L}", [(_n(res["q"]), rq), (_n(pol._act_state[0]), rh), (_n(q), rq), (_n(state[0]), rh),
                                                      (_n(full), rq), (_n(fh), rh), (_n(out.logits), rq), (_n(out.state.hidden), rh)])
    assert np.array_equal(res["act"].cpu().numpy(), _n(res["q"]).argmax(1))
    done = torch.tensor([0, 1, 0, 0, 0, 0, 0, 1, 0], dtype=torch.uint8, device=DEV)   # exactly the rows of envs 1 and 7 restart
    before = pol._act_state[0].clone()
    pol.reset_state_device(done)
    keep, hid = (done == 0).repeat_interleave(N), pol._act_state[0]
    assert torch.equal(hid[keep], before[keep]) and not hid[~keep].any() and before[~keep].any() and (~keep).sum() == 2 * N


def test_dqn_update_on_a_stacking_buffer_moves_every_parameter():
    E, N, D, A, L = 4, 2, 6, 4, 3
    buf = VectorReplayBuffer(E * 8, E, device=DEV, stack_num=L)
    _filled(buf, Batch, E, N, D, A, 7, 21)
    net = Recurrent(layer_num=2, state_shape=D, action_shape=A, hidden_layer_size=32, device=DEV, seed=13, cell="gru")
    algo = DQN(policy=DiscreteQLearningPolicy(model=net, action_space=_Discrete(4)), optim=AdamOptimizerFactory(lr=1e-3), gamma=0.97,
               n_step_return_horizon=2, target_update_freq=1)
    assert algo.model_old.cell == "gru" and algo.model_old.flat.numel() == net.flat.numel()
    before = net.flat.data.clone()
    algo.is_within_training_step = True
    stats = algo.update(buf, 16, agent=1)
    assert np.isfinite(stats.loss) and torch.isfinite(net.flat.data).all()
    assert all((a != b).any() for (_, a), (_, b) in zip(net.reference_named_views(), net.reference_named_views(before)))
