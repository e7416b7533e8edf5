"""CPU tests of the MADDPG port: the import surface, the reference signatures, the float64 restatement
(tests/maddpg_restatement.py) against the reference's own float64 run (tests/golden/maddpg.npz, maddpg_n8.npz) -- which is
also what proves the phase order --, phase order against the literal agent-by-agent loop, the fixtures' kink-redraw
shares, the constructor's refusals, and the argument checks of the tsm_maddpg_* / tsm_polyak / tsm_mlp_input_grad entry
points (which fail before touching a device)."""
import inspect
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from maddpg_restatement import MaddpgRestatement  # noqa: E402
from tianshou_marl_amd import _abi, ops  # noqa: E402
from tianshou_marl_amd.algorithm.multiagent.maddpg import MADDPGPolicy  # noqa: E402
from tianshou_marl_amd.utils.net import FlatMLP  # noqa: E402

VARIANTS = ("small", "n8", "odd")


def _g(name: str = "small"):
    return np.load(os.path.join(HERE, "golden", "maddpg_n8.npz" if name == "n8" else "maddpg.npz"))


def _restatement(g, name):
    N, D, Ad, H, B, rounds = (int(x) for x in g[f"{name}_dims"])
    R = MaddpgRestatement(g[f"{name}_init"], N, [D, H, H, Ad], [N * (D + Ad), H, H, 1], gamma=float(g["gamma"]),
                          tau=float(g["tau"]))
    return R, rounds


def _rows(g, name, k):
    return [g[f"{name}_r{k}_{f}"] for f in ("obs", "act", "rew", "obs_next", "term")]


def test_maddpg_importable_from_ctde_and_multiagent():
    from tianshou_marl_amd.algorithm.multiagent import MADDPGPolicy as P2
    from tianshou_marl_amd.algorithm.multiagent.ctde import MADDPGPolicy as P3

    assert MADDPGPolicy is P2 and MADDPGPolicy is P3


def _check_digest(g, key, x):
    scale = max(np.abs(x).max(), 1e-300)
    assert abs(x.sum() - float(g[f"{key}_dsum"])) <= 1e-12 * max(abs(float(g[f"{key}_dsum"])), scale * x.size ** 0.5), key
    assert abs((x * x).sum() - float(g[f"{key}_dsq"])) <= 1e-12 * float(g[f"{key}_dsq"]), key
    ref = g[f"{key}_dval"]
    got = x[g[f"{key}_didx"]]
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref) + 1e-12 * scale * 1e-3), key


@pytest.mark.parametrize("name", VARIANTS)
def test_restatement_reproduces_reference_f64(name):
    """The phase-ordered restatement at float64 reproduces the reference's float64 losses, first-call gradients, weights
    after every learn and targets after every update to 1e-12 relative (digests of the parameter arrays)."""
    g = _g(name)
    R, rounds = _restatement(g, name)
    keys = [str(k) for k in g[f"{name}_loss_keys"]]
    assert keys[-2:] == ["actor_loss", "critic_loss"] and len(keys) == 2 * R.N + 2
    for k in range(rounds):
        r = R.learn(*_rows(g, name, k))
        assert [kk for kk in r if kk.endswith("_loss")] == keys
        for kk, ref in zip(keys, g[f"{name}_r{k}_losses"][0]):
            assert r[kk] == pytest.approx(float(ref), rel=1e-12, abs=0), (k, kk)
        if k == 0:
            _check_digest(g, f"{name}_r0_grad", r["grads"])
        _check_digest(g, f"{name}_r{k}_weights", R.weights())
        R.update_targets()
        _check_digest(g, f"{name}_r{k}_targets", R.targets())


@pytest.mark.parametrize("name", VARIANTS)
def test_phase_order_equals_the_sequential_loop(name):
    g = _g(name)
    (Rp, rounds), (Rs, _) = _restatement(g, name), _restatement(g, name)
    for k in range(rounds):
        rp = Rp.learn(*_rows(g, name, k))
        rs = Rs.learn(*_rows(g, name, k), sequential=True)
        for kk in rp:
            if kk != "grads":
                assert rp[kk] == pytest.approx(rs[kk], rel=1e-12, abs=0), (k, kk)
        np.testing.assert_allclose(rp["grads"], rs["grads"], rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(Rp.weights(), Rs.weights(), rtol=1e-12, atol=1e-18)
        Rp.update_targets()
        Rs.update_targets()
        np.testing.assert_allclose(Rp.targets(), Rs.targets(), rtol=1e-12, atol=1e-18)


def test_fixture_redraw_share_within_bound_and_flags_differ_between_agents():
    for name in VARIANTS:
        g = _g(name)
        share = g[f"{name}_redraw_share"]
        assert share.size == int(g[f"{name}_dims"][5]) and (share <= 0.25).all(), (name, share)
        term = g[f"{name}_r0_term"]
        assert term.any(1).all() and any((term[0] != term[i]).any() for i in range(1, term.shape[0])), name


def test_signatures_cover_the_reference_and_state_dict_is_empty():
    """Every reference parameter is accepted under its own name, in its own position, with the same default."""
    import ast

    g = _g()

    def params(sig_text):
        inner = sig_text[sig_text.index("(") + 1:sig_text.rindex(")", 0, sig_text.rfind("->") if "->" in sig_text else None)]
        parts, depth, cur = [], 0, ""
        for ch in inner:
            depth += ch in "[("
            depth -= ch in "])"
            if ch == "," and depth == 0:
                parts.append(cur.strip())
                cur = ""
            else:
                cur += ch
        if cur.strip():
            parts.append(cur.strip())
        out = []
        for part in parts:
            head, _, default = part.partition("=")
            name = head.split(":")[0].strip()
            out.append((name.lstrip("*"), ast.literal_eval(default.strip()) if default else None, name.startswith("**")))
        return out

    for ours, key in ((MADDPGPolicy.__init__, "sig_policy"), (MADDPGPolicy.learn, "sig_learn"),
                      (MADDPGPolicy.forward, "sig_forward"), (MADDPGPolicy.update_target_networks, "sig_update_target_networks")):
        mine = list(inspect.signature(ours).parameters.values())
        ref = params(str(g[key]))
        assert len([p for p in ref if not p[2]]) >= 1
        for k, (name, default, var_kw) in enumerate(ref):
            if var_kw:
                assert any(q.kind == q.VAR_KEYWORD for q in mine), key
                continue
            assert mine[k].name == name, (key, k, name, mine[k].name)
            if default is not None:
                assert mine[k].default == default, (key, name)
    assert [p.name for p in inspect.signature(MADDPGPolicy.__init__).parameters.values()][1:10] == [
        "actors", "critics", "observation_space", "action_space", "n_agents", "optimizer_actors", "optimizer_critics",
        "discount_factor", "tau"]
    assert g["sd_keys"].size == 0  # the reference's state_dict() is empty (quirk Q13)


class _Box:
    def __init__(self, n, low=-1.0, high=1.0):
        self.shape, self.low, self.high = (n,), np.full(n, low, np.float32), np.full(n, high, np.float32)


class _Discrete:
    def __init__(self, n):
        self.n = n


def _nets(N, D, Ad, H=8, critic_out=1, critic_in=None):
    actors = [FlatMLP([D, H, Ad], device="cpu", seed=i) for i in range(N)]
    critics = [FlatMLP([critic_in or N * (D + Ad), H, critic_out], device="cpu", seed=10 + i) for i in range(N)]
    return actors, critics


def test_constructor_refuses_what_the_kernels_do_not_serve():
    N, D, Ad = 2, 5, 2
    with pytest.raises(NotImplementedError, match="Discrete"):
        MADDPGPolicy(*_nets(N, D, Ad), None, _Discrete(4), N)
    with pytest.raises(TypeError, match="Box"):
        MADDPGPolicy(*_nets(N, D, Ad), None, None, N)
    with pytest.raises(TypeError, match="FlatMLP"):
        MADDPGPolicy([torch.nn.Linear(D, Ad)] * N, _nets(N, D, Ad)[1], None, _Box(Ad), N)
    a, c = _nets(N, D, Ad)
    a[1] = FlatMLP([D + 1, 8, Ad], device="cpu", seed=3)
    with pytest.raises(ValueError, match="same observation width"):
        MADDPGPolicy(a, c, None, _Box(Ad), N)
    a, c = _nets(N, D, Ad)
    a[1] = FlatMLP([D, 8, Ad + 1], device="cpu", seed=3)
    with pytest.raises(ValueError, match="same action width"):
        MADDPGPolicy(a, c, None, _Box(Ad), N)
    with pytest.raises(ValueError, match="Box has shape"):
        MADDPGPolicy(*_nets(N, D, Ad), None, _Box(Ad + 1), N)
    with pytest.raises(ValueError, match="output width 3"):
        MADDPGPolicy(*_nets(N, D, Ad, critic_out=3), None, _Box(Ad), N)
    with pytest.raises(ValueError, match="joint row"):
        MADDPGPolicy(*_nets(N, D, Ad, critic_in=N * D), None, _Box(Ad), N)
    with pytest.raises(ValueError, match="1 to 8 agents"):
        MADDPGPolicy(*_nets(9, D, Ad), None, _Box(Ad), 9)
    with pytest.raises(ValueError, match="2 actors and 2 critics for n_agents = 3"):
        MADDPGPolicy(*_nets(N, D, Ad), None, _Box(Ad), 3)


def test_optimizer_lists_are_taken_over_or_refused():
    N, D, Ad = 2, 5, 2
    p = [torch.nn.Parameter(torch.zeros(1)) for _ in range(N)]
    kw = dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6)
    pol = MADDPGPolicy(*_nets(N, D, Ad), None, _Box(Ad), N, optimizer_actors=[torch.optim.Adam([q], **kw) for q in p],
                       optimizer_critics=None)
    oa, oc = pol.optimizer_actors, pol.optimizer_critics
    assert (oa.lr, oa.betas, oa.eps) == (3e-4, (0.8, 0.99), 1e-6) and (oc.lr, oc.betas, oc.eps) == (1e-3, (0.9, 0.999), 1e-8)
    assert oa.coef64 and oc.coef64
    assert oa.param.numel() == pol.n_actor_params and oa.param.numel() + oc.param.numel() == pol.flat.numel()
    assert (pol.discount_factor, pol.tau) == (0.99, 0.01)
    with pytest.raises(ValueError, match="differ in their hyper-parameters"):
        MADDPGPolicy(*_nets(N, D, Ad), None, _Box(Ad), N,
                     optimizer_critics=[torch.optim.Adam([p[0]], lr=1e-3), torch.optim.Adam([p[1]], lr=2e-3)])
    with pytest.raises(ValueError, match="amsgrad"):
        MADDPGPolicy(*_nets(N, D, Ad), None, _Box(Ad), N, optimizer_actors=[torch.optim.Adam([q], amsgrad=True) for q in p])
    with pytest.raises(ValueError, match="amsgrad / maximize"):
        MADDPGPolicy(*_nets(N, D, Ad), None, _Box(Ad), N, optimizer_actors=[torch.optim.Adam([q], maximize=True) for q in p])
    with pytest.raises(TypeError, match="torch.optim.Adam"):
        MADDPGPolicy(*_nets(N, D, Ad), None, _Box(Ad), N, optimizer_actors=[torch.optim.SGD([q], lr=0.1) for q in p])


def test_joint_vector_layout_targets_and_reference_state_dict():
    """[actors | critics] in one vector viewed by the nets; targets start as copies and draw nothing from the global RNG;
    state_dict() is empty and to_reference_state_dict() carries all four net lists under fc{k} keys."""
    N, D, Ad = 2, 5, 2
    actors, critics = _nets(N, D, Ad)
    before = torch.cat([m.flat.data.clone() for m in actors + critics])
    torch.manual_seed(123)
    pol = MADDPGPolicy(actors, critics, None, _Box(Ad), N)
    after = torch.rand(8)
    torch.manual_seed(123)
    assert torch.equal(after, torch.rand(8))
    assert torch.equal(pol.flat, before) and torch.equal(pol.target_flat, before)
    assert all(m.flat.data_ptr() == pol.flat.data_ptr() + 4 * o for m, o in zip(actors + critics, pol._offs))
    assert all(m.flat.data_ptr() == pol.target_flat.data_ptr() + 4 * o
               for m, o in zip(pol.target_actors + pol.target_critics, pol._offs))
    assert len(pol.state_dict()) == 0
    sd = pol.to_reference_state_dict()
    assert list(sd)[:4] == ["actors.0.fc1.weight", "actors.0.fc1.bias", "actors.0.fc2.weight", "actors.0.fc2.bias"]
    assert len(sd) == 4 * N * 4 and "target_critics.1.fc2.bias" in sd and tuple(sd["critics.0.fc1.weight"].shape) == (8, N * (D + Ad))
    pol2 = MADDPGPolicy(*_nets(N, D, Ad, H=8), None, _Box(Ad), N)
    pol2.flat.zero_()
    pol2.target_flat.fill_(1.0)
    pol2.load_reference_state_dict(sd)
    assert torch.equal(pol2.flat, pol.flat) and torch.equal(pol2.target_flat, pol.target_flat)


def test_entry_points_reject_bad_arguments_without_a_device():
    nul3 = (_abi.C.c_void_p * 8)()
    one = (_abi.C.c_void_p * 8)(*([16] * 8))
    # tsm_maddpg_joint_rows
    with pytest.raises(ValueError, match="n_agents = 9"):
        _abi.call("tsm_maddpg_joint_rows", one, one, None, 9, 4, 5, 2, 16, None)
    with pytest.raises(ValueError, match="n_agents = 0"):
        _abi.call("tsm_maddpg_joint_rows", one, one, None, 0, 4, 5, 2, 16, None)
    with pytest.raises(ValueError, match="B = 0"):
        _abi.call("tsm_maddpg_joint_rows", one, one, None, 3, 0, 5, 2, 16, None)
    with pytest.raises(ValueError, match="act_dim = 0"):
        _abi.call("tsm_maddpg_joint_rows", one, one, None, 3, 4, 5, 0, 16, None)
    with pytest.raises(ValueError, match="obs_dim = 0"):
        _abi.call("tsm_maddpg_joint_rows", one, one, None, 3, 4, 0, 2, 16, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_maddpg_joint_rows", one, one, None, 3, 4, 5, 2, None, None)
    with pytest.raises(ValueError, match="null pointer for agent 0"):
        _abi.call("tsm_maddpg_joint_rows", nul3, one, None, 3, 4, 5, 2, 16, None)
    with pytest.raises(ValueError, match="null replacement for agent 0"):
        _abi.call("tsm_maddpg_joint_rows", one, one, nul3, 3, 4, 5, 2, 16, None)
    # tsm_maddpg_td / partial_elems
    ag = _abi.tsm_maddpg_agents()
    with pytest.raises(ValueError, match="n_agents = 9"):
        _abi.call("tsm_maddpg_td", _abi.C.byref(ag), 9, 16, 0.99, 16, None)
    with pytest.raises(ValueError, match="B = 0"):
        _abi.call("tsm_maddpg_td", _abi.C.byref(ag), 3, 0, 0.99, 16, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_maddpg_td", _abi.C.byref(ag), 3, 16, 0.99, None, None)
    with pytest.raises(ValueError, match="null pointer for agent 0"):
        _abi.call("tsm_maddpg_td", _abi.C.byref(ag), 3, 16, 0.99, 16, None)
    assert _abi.call("tsm_maddpg_partial_elems", 0, 3) == -1 and _abi.call("tsm_maddpg_partial_elems", 16, 9) == -1
    assert _abi.call("tsm_maddpg_partial_elems", 257, 3) == 3 * 2 and ops.maddpg_partial_elems(256, 8) == 8
    # tsm_maddpg_finalize
    with pytest.raises(ValueError, match="n_agents = 9"):
        _abi.call("tsm_maddpg_finalize", 16, 1, one, 9, 16, 16, None)
    with pytest.raises(ValueError, match="B = -1"):
        _abi.call("tsm_maddpg_finalize", 16, 1, one, 3, -1, 16, None)
    with pytest.raises(ValueError, match="n_blocks = 0"):
        _abi.call("tsm_maddpg_finalize", 16, 0, one, 3, 16, 16, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_maddpg_finalize", None, 1, one, 3, 16, 16, None)
    with pytest.raises(ValueError, match="null pointer for agent 0"):
        _abi.call("tsm_maddpg_finalize", 16, 1, nul3, 3, 16, 16, None)
    # tsm_maddpg_act
    with pytest.raises(ValueError, match="n_agents = 9"):
        _abi.call("tsm_maddpg_act", one, 9, 4, 2, 16, 0, 0, None, None, None, 16, None)
    with pytest.raises(ValueError, match="act_dim = 0"):
        _abi.call("tsm_maddpg_act", one, 3, 4, 0, 16, 0, 0, None, None, None, 16, None)
    with pytest.raises(ValueError, match="E = -1"):
        _abi.call("tsm_maddpg_act", one, 3, -1, 2, 16, 0, 0, None, None, None, 16, None)
    with pytest.raises(ValueError, match="come together"):
        _abi.call("tsm_maddpg_act", one, 3, 4, 2, 16, 0, 0, None, 16, None, 16, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_maddpg_act", one, 3, 4, 2, None, 0, 0, None, None, None, 16, None)
    with pytest.raises(ValueError, match="null actor output for agent 0"):
        _abi.call("tsm_maddpg_act", nul3, 3, 4, 2, 16, 0, 0, None, None, None, 16, None)
    _abi.call("tsm_maddpg_act", None, 3, 0, 2, None, 0, 0, None, None, None, None, None)  # no envs: nothing to do
    # tsm_polyak
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_polyak", None, 16, 8, 0.01, None)
    with pytest.raises(ValueError, match="n = -1"):
        _abi.call("tsm_polyak", 16, 16, -1, 0.01, None)
    with pytest.raises(ValueError, match="tau = 1.5"):
        _abi.call("tsm_polyak", 16, 16, 8, 1.5, None)
    # tsm_adam_step_coef64: tsm_adam_step's checks under its own name
    with pytest.raises(ValueError, match="tsm_adam_step_coef64: bad sizes"):
        _abi.call("tsm_adam_step_coef64", 16, 16, 0, 8, 16, 16, 1, None, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0.0, None, None, None, None)
    with pytest.raises(ValueError, match="tsm_adam_step_coef64: null pointer"):
        _abi.call("tsm_adam_step_coef64", None, 16, 1, 8, 16, 16, 1, None, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0.0, None, None, None, None)
    with pytest.raises(ValueError, match="tsm_adam_step: bad sizes"):
        _abi.call("tsm_adam_step", 16, 16, 0, 8, 16, 16, 1, None, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 0.0, None, None, None, None)
    # tsm_mlp_input_grad
    d = ops.mlp_desc([60, 64, 64, 1])
    ref = _abi.C.byref(d)
    for col0, n_col in ((59, 2), (-1, 2), (0, 0), (0, 61)):
        with pytest.raises(ValueError, match="leave the input width 60"):
            _abi.call("tsm_mlp_input_grad", ref, 16, 16, 4, 16, 16, 16, col0, n_col, 16, max(n_col, 1), None)
    with pytest.raises(ValueError, match="batch must be >= 1"):
        _abi.call("tsm_mlp_input_grad", ref, 16, 16, 0, 16, 16, 16, 54, 2, 16, 2, None)
    with pytest.raises(ValueError, match="ldx = 1"):
        _abi.call("tsm_mlp_input_grad", ref, 16, 16, 4, 16, 16, 16, 54, 2, 16, 1, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_mlp_input_grad", ref, 16, 16, 4, 16, 16, 16, 54, 2, None, 2, None)
    with pytest.raises(ValueError, match="d_acts workspace"):
        _abi.call("tsm_mlp_input_grad", ref, 16, 16, 4, 16, 16, None, 54, 2, 16, 2, None)
    with pytest.raises(ValueError, match="null descriptor"):
        _abi.call("tsm_mlp_input_grad", None, 16, 16, 4, 16, 16, 16, 54, 2, 16, 2, None)
    # the Python wrappers name the limit before any pointer is taken
    with pytest.raises(ValueError, match="1 to 8 agents"):
        ops.maddpg_check(9)
    with pytest.raises(ValueError, match="leave the input width"):
        ops.mlp_input_grad(d, torch.zeros(1), torch.zeros(4, 60), torch.zeros(1), torch.zeros(4, 1), 59, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.polyak(torch.zeros(4), torch.zeros(4), 0.01)
