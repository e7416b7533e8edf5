"""CPU: the host side of the learned global states -- argument checks of the ops wrappers and the nets (every limit of
include/tsmarl.h's TSM_GSTATE_*, adjacency validation, the shapes `GlobalStateConstructor` keeps refusing with
NotImplementedError), the vector layout under the reference's keys against tests/golden/gstate.npz, and the pooling coefficients
of an adjacency against float64."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gstate_restatement as R  # noqa: E402
from tianshou_marl_amd import _abi, _build, ops  # noqa: E402

_build.build()
from tianshou_marl_amd.algorithm.multiagent.ctde import CentralizedCritic, CTDEPolicy, DecentralizedActor, GlobalStateConstructor  # noqa: E402
from tianshou_marl_amd.utils.net import AttentionStateNet, FlatAdam, GraphStateNet, agent_pool_coefficients, lagged_copy  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "gstate.npz"))


def test_limits_are_the_headers():
    assert (_abi.GSTATE_MAX_AGENTS, _abi.GSTATE_HEADS, _abi.GSTATE_MAX_DIM) == (8, 4, 256)
    assert _abi.GSTATE_MAX_AGENTS == _abi.QMIX_MAX_AGENTS == _abi.MADDPG_MAX_AGENTS
    assert _abi.GSTATE_ROWS_PER_BLOCK >= 1
    for name in ("tsm_gstate_check", "tsm_attn_pool_forward", "tsm_attn_pool_backward", "tsm_agent_pool_forward",
                 "tsm_agent_pool_backward"):
        assert name in _abi.SIGNATURES


@pytest.mark.parametrize("N,D,word", [(0, 8, "agents"), (9, 8, "agents"), (3, 0, "obs_dim"), (3, 6, "obs_dim"), (3, 2, "obs_dim"),
                                      (3, 260, "obs_dim"), (3, 257, "obs_dim")])
def test_gstate_check_names_the_limit(N, D, word):
    with pytest.raises(ValueError, match=word):
        ops.gstate_check(N, D)
    with pytest.raises(ValueError, match="tsm_gstate_check"):   # the library's own check agrees
        ops.call("tsm_gstate_check", N, D)


def test_gstate_check_accepts_the_corners():
    for N, D in ((1, 4), (8, 256), (8, 48), (3, 8)):
        ops.gstate_check(N, D)
        ops.call("tsm_gstate_check", N, D)


def test_wrappers_reject_bad_arguments_before_any_launch():
    f = lambda *s: torch.zeros(*s)  # noqa: E731
    with pytest.raises(ValueError, match="float32"):
        ops.attn_pool_forward(f(2, 3, 24).double(), 3)
    with pytest.raises(ValueError, match="contiguous"):
        ops.attn_pool_forward(f(2, 3, 48)[:, :, ::2], 3)
    with pytest.raises(ValueError, match="obs_dim"):
        ops.attn_pool_forward(f(2, 3, 18), 3)            # D = 6
    with pytest.raises(ValueError, match="agents"):
        ops.attn_pool_forward(f(2, 9, 24), 9)
    with pytest.raises(ValueError, match="n_agents"):
        ops.attn_pool_forward(f(2, 3, 24), 2)
    with pytest.raises(ValueError, match="non-empty"):
        ops.attn_pool_forward(f(0, 3, 24), 3)
    with pytest.raises(RuntimeError, match="device"):
        ops.attn_pool_forward(f(2, 3, 24), 3)
    with pytest.raises(ValueError, match="P must be"):
        ops.attn_pool_backward(f(2, 8), f(2, 3, 24), f(2, 3, 3, 3))
    with pytest.raises(ValueError, match="d_ctx"):
        ops.attn_pool_backward(f(3, 8), f(2, 3, 24), f(2, 4, 3, 3))
    with pytest.raises(ValueError, match="qkv must be"):
        ops.attn_pool_backward(f(2, 8), f(2, 3, 12), f(2, 4, 3, 3))
    with pytest.raises(RuntimeError, match="device"):
        ops.attn_pool_backward(f(2, 8), f(2, 3, 24), f(2, 4, 3, 3))
    with pytest.raises(ValueError, match="agents"):
        ops.agent_pool_forward(f(2, 9, 5), f(9))
    with pytest.raises(ValueError, match="c must be"):
        ops.agent_pool_forward(f(2, 3, 5), f(4))
    with pytest.raises(ValueError, match="at least 1"):
        ops.agent_pool_forward(f(2, 3, 0), f(3))
    with pytest.raises(ValueError, match="float32"):
        ops.agent_pool_forward(f(2, 3, 5), f(3).double())
    with pytest.raises(RuntimeError, match="device"):
        ops.agent_pool_forward(f(2, 3, 5), f(3))
    with pytest.raises(ValueError, match="agents"):
        ops.agent_pool_backward(f(2, 5), f(9), 9)
    with pytest.raises(ValueError, match="h_relu"):
        ops.agent_pool_backward(f(2, 5), f(3), 3, h_relu=f(2, 3, 4))
    with pytest.raises(RuntimeError, match="device"):
        ops.agent_pool_backward(f(2, 5), f(3), 3)


@pytest.mark.parametrize("kw,word", [(dict(obs_dim=6, n_agents=3), "obs_dim = 6"), (dict(obs_dim=8), "needs obs_dim and n_agents"),
                                     (dict(n_agents=3), "needs obs_dim and n_agents"), (dict(obs_dim=260, n_agents=3), "256"),
                                     (dict(obs_dim=8, n_agents=9), "1 to 8 agents")])
def test_constructor_keeps_refusing_what_the_kernels_do_not_serve(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        GlobalStateConstructor("attention", **kw)


def test_graph_constructor_limits_and_adjacency():
    with pytest.raises(NotImplementedError, match="1 to 8 agents"):
        GlobalStateConstructor("graph", obs_dim=5, n_agents=9)
    with pytest.raises(NotImplementedError, match="needs obs_dim"):
        GlobalStateConstructor("graph", n_agents=3)
    ok = np.eye(3) + 0.5
    for bad, word in ((np.ones((3, 2)), r"\[3, 3\]"), (np.ones((4, 4)), r"\[3, 3\]"), (ok * -1, "non-negative"),
                      (np.where(np.eye(3) > 0, np.nan, ok), "finite"), (np.where(np.eye(3) > 0, np.inf, ok), "finite"),
                      (ok * np.array([[1.0], [0.0], [1.0]]), "row sum")):
        with pytest.raises(ValueError, match=word):
            GlobalStateConstructor("graph", obs_dim=5, n_agents=3, adjacency_matrix=torch.as_tensor(bad), device="cpu")
    gsc = GlobalStateConstructor("graph", obs_dim=5, n_agents=3, adjacency_matrix=torch.as_tensor(ok), device="cpu", seed=0)
    assert isinstance(gsc.net, GraphStateNet) and list(gsc.state_dict()) == list(R.GRAPH_KEYS)


def test_pooling_coefficients_against_float64():
    for p in ("gr1_", "gr2_", "gr4_"):
        A = G[p + "adjacency"]
        N = A.shape[0]
        c = agent_pool_coefficients(N, torch.as_tensor(A))
        want = (A.astype(np.float64) / A.astype(np.float64).sum(1, keepdims=True)).sum(0) / N
        assert c.dtype == np.float64 and np.abs(c - want).max() <= 1e-15 and abs(c.sum() - 1) <= 1e-15
        np.testing.assert_array_equal(c, R.pool_coefficients(N, A))
        assert np.ptp(c) > 0.01   # not the plain mean
        net = GraphStateNet(int(G[p + "dims"][1]), N, int(G[p + "dims"][2]), A, device="cpu", seed=0)
        np.testing.assert_array_equal(net.c.numpy(), want.astype(np.float32))
    np.testing.assert_array_equal(agent_pool_coefficients(4), np.full(4, 0.25))


@pytest.mark.parametrize("p", ["at0_", "at1_", "at2_", "gr1_", "gr3_"])
def test_reference_named_views_keys_shapes_and_order(p):
    N, D, H, _ = (int(x) for x in G[p + "dims"])
    net = AttentionStateNet(D, N, H, device="cpu", seed=1) if p.startswith("at") else GraphStateNet(D, N, H, device="cpu", seed=1)
    views = net.reference_named_views()
    assert [k for k, _ in views] == [str(k) for k in G[p + "keys"]]
    assert [",".join(str(d) for d in v.shape) for _, v in views] == [str(s) for s in G[p + "shapes"]]
    # the views tile the vector in this order: what FlatAdam splits its moments by
    o = 0
    for _, v in views:
        assert v.data_ptr() == net.flat.data_ptr() + 4 * o and v.is_contiguous()
        o += v.numel()
    assert o == net.flat.numel() and net.param_shapes() == [tuple(v.shape) for _, v in views]
    # a checkpoint round trip through the reference's keys, and a lagged twin
    sd = {str(k): G[f"{p}w_{k}"] for k in G[p + "keys"]}
    net.load_reference_state_dict(sd)
    for k, v in net.to_reference_state_dict().items():
        np.testing.assert_array_equal(v.numpy(), sd[k])
    twin = lagged_copy(net)
    assert type(twin) is type(net) and torch.equal(twin.flat.data, net.flat.data) and twin.flat.data_ptr() != net.flat.data_ptr()
    assert twin.head.flat.data_ptr() == twin.flat.data_ptr()


def test_attention_init_is_torchs_and_seeded():
    a, b, c = (AttentionStateNet(8, 3, 16, device="cpu", seed=s) for s in (3, 3, 4))
    assert torch.equal(a.flat.data, b.flat.data) and not torch.equal(a.flat.data, c.flat.data)
    v = dict(a.reference_named_views())
    assert float(v["attention.in_proj_bias"].abs().max()) == 0.0 and float(v["attention.out_proj.bias"].abs().max()) == 0.0
    assert float(v["attention.in_proj_weight"].abs().max()) <= np.sqrt(6.0 / (8 + 24))
    assert float(v["attention.in_proj_weight"].abs().max()) > 1.0 / np.sqrt(8)   # xavier's bound, wider than nn.Linear's
    assert 0 < float(v["output_proj.bias"].abs().max()) <= 1.0 / np.sqrt(8)
    state = torch.get_rng_state()
    AttentionStateNet(8, 3, 16, device="cpu", seed=5)
    GraphStateNet(8, 3, 16, device="cpu", seed=5)
    assert torch.equal(state, torch.get_rng_state())   # a seeded init leaves the global generator alone


def test_ctde_policy_checks_its_constructor():
    actor, critic = DecentralizedActor(8, 5, 16, device="cpu", seed=0), CentralizedCritic(16, 3, 16, device="cpu", seed=1)
    gsc = GlobalStateConstructor("attention", obs_dim=8, n_agents=3, hidden_dim=16, device="cpu", seed=2)
    pol = CTDEPolicy(actor=actor, critic=critic, state_constructor=gsc)
    assert isinstance(pol.optim_state, FlatAdam) and pol.optim_state.param.data_ptr() == gsc.net.flat.data_ptr()
    assert list(pol.state_dict()) == [f"{n}.fc{i}.{p}" for n in ("actor", "critic") for i in (1, 2, 3) for p in ("weight", "bias")]
    with pytest.raises(TypeError, match="learned mode"):
        CTDEPolicy(actor=actor, critic=critic, state_constructor=GlobalStateConstructor("mean", obs_dim=8, n_agents=3))
    with pytest.raises(ValueError, match="hidden_dim"):
        CTDEPolicy(actor=actor, critic=CentralizedCritic(24, 3, 16, device="cpu", seed=1), state_constructor=gsc)
    with pytest.raises(ValueError, match="optim_state"):
        CTDEPolicy(actor=actor, critic=critic, optim_state=FlatAdam(gsc.net))
    with pytest.raises(RuntimeError, match="holds no network"):
        GlobalStateConstructor("mean").build_joint(torch.zeros(2, 3, 8))
