"""CPU tests of the QMIX port: the import surface, the float64 restatement (tests/qmix_restatement.py) against the
reference's own float64 run (tests/golden/qmix.npz), the fixture's kink-redraw share, the reference signatures, and the
argument checks of the tsm_qmix_* entry points (which fail before touching a device)."""
import inspect
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "qmix.npz")

from qmix_restatement import QmixRestatement  # noqa: E402


def _g(name: str = "small") -> dict:
    """The fixture arrays of a variant: qmix.npz, or for c3 qmix_c3.npz with its inputs from qmix_c3_rows.npz."""
    if name != "c3":
        return np.load(GOLD)
    d = dict(np.load(os.path.join(HERE, "golden", "qmix_c3.npz")))
    d.update(np.load(os.path.join(HERE, "golden", "qmix_c3_rows.npz")))
    return d


def test_qmix_importable_from_ctde_and_multiagent():
    from tianshou_marl_amd.algorithm.multiagent import QMIXMixer as M2, QMIXPolicy as P2
    from tianshou_marl_amd.algorithm.multiagent.ctde import QMIXMixer, QMIXPolicy

    assert QMIXPolicy is P2 and QMIXMixer is M2


def _rows(g, name, k):
    return {f: g[f"{name}_r{k}_{f}"] for f in ("obs", "obs_next", "act", "rew", "term")}


def _check_digest(g, key, x):
    scale = max(np.abs(x).max(), 1e-300)
    assert abs(x.sum() - float(g[f"{key}_dsum"])) <= 1e-12 * max(abs(float(g[f"{key}_dsum"])), scale * x.size ** 0.5), key
    assert abs((x * x).sum() - float(g[f"{key}_dsq"])) <= 1e-12 * float(g[f"{key}_dsq"]), key
    ref = g[f"{key}_dval"]
    got = x[g[f"{key}_didx"]]
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref) + 1e-12 * scale * 1e-3), key


@pytest.mark.parametrize("name", ["small", "nonmono", "c3"])
def test_restatement_reproduces_reference_f64(name):
    """The restatement at float64 reproduces the reference's float64 losses, q_values, first-call gradients, weights after
    every learn and targets after every update to 1e-12 relative (digests of the parameter arrays)."""
    g = _g(name)
    N, D, A, H, S, E, Hh, B, rounds, mono = (int(x) for x in g[f"{name}_dims"])
    R = QmixRestatement(g[f"{name}_init"], (N, D, A, H, S, E, Hh), monotonic=bool(mono), gamma=float(g["gamma"]))
    for k in range(rounds):
        rows = _rows(g, name, k)
        gs = rows["obs"].transpose(1, 0, 2).reshape(B, S)
        gsn = rows["obs_next"].transpose(1, 0, 2).reshape(B, S)
        r = R.learn(rows["obs"], rows["act"], rows["rew"], rows["obs_next"], rows["term"], gs, gsn)
        assert r["loss"] == pytest.approx(float(g[f"{name}_r{k}_loss"][0]), rel=1e-12, abs=0)
        assert r["q_values"] == pytest.approx(float(g[f"{name}_r{k}_q_values"][0]), rel=1e-12, abs=1e-15)
        if k == 0:
            _check_digest(g, f"{name}_r0_grad", r["grads"])
        _check_digest(g, f"{name}_r{k}_weights", R.weights())
        R.update_targets(float(g["tau"]))
        _check_digest(g, f"{name}_r{k}_targets", R.targets())


def test_fixture_redraw_share_within_bound():
    for name in ("small", "nonmono", "c3"):
        share = _g(name)[f"{name}_redraw_share"]
        assert share.size >= 1 and (share <= 0.25).all(), (name, share)


def test_signatures_cover_the_reference():
    """Every reference parameter is accepted under its own name, in its own position, with the same default."""
    from tianshou_marl_amd.algorithm.multiagent.qmix import QMIXMixer, QMIXPolicy

    g = _g()

    def params(sig_text):
        """[(name, default or None, is **kwargs)] of a signature's text (annotations dropped)."""
        import ast

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

    for ours, key in ((QMIXMixer.__init__, "sig_mixer"), (QMIXPolicy.__init__, "sig_policy"),
                      (QMIXPolicy.learn, "sig_learn"), (QMIXPolicy.forward, "sig_forward"),
                      (QMIXPolicy.update_target_networks, "sig_update_target_networks")):
        mine = list(inspect.signature(ours).parameters.values())
        for k, (name, default, var_kw) in enumerate(params(str(g[key]))):
            if var_kw:
                assert any(q.kind == q.VAR_KEYWORD for q in mine), key
                continue
            assert mine[k].name == name, (key, k, name, mine[k].name)
            if default is not None:
                assert mine[k].default == default, (key, name)

def test_entry_points_reject_bad_arguments_without_a_device():
    from tianshou_marl_amd import _abi, ops
    from tianshou_marl_amd.algorithm.multiagent.qmix import QMIXMixer

    ag = _abi.tsm_qmix_agents()
    nul = [None] * 9
    with pytest.raises(ValueError, match="n_agents = 9"):
        _abi.call("tsm_qmix_mix_td", _abi.C.byref(ag), 9, 5, 16, 32, *nul, 0.99, 1, None, None, None, None, None, None, None)
    with pytest.raises(ValueError, match="must be 32 or 64"):
        _abi.call("tsm_qmix_mix_td", _abi.C.byref(ag), 3, 5, 16, 48, *nul, 0.99, 1, None, None, None, None, None, None, None)
    with pytest.raises(ValueError, match="n_act = 65"):
        _abi.call("tsm_qmix_mix_td", _abi.C.byref(ag), 3, 65, 16, 32, *nul, 0.99, 1, None, None, None, None, None, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_qmix_mix_td", _abi.C.byref(ag), 3, 5, 16, 32, *nul, 0.99, 1, None, None, None, None, None, None, None)
    with pytest.raises(ValueError, match="n_agents = 0"):
        _abi.call("tsm_qmix_egreedy", None, 0, 4, 5, None, 0, 0, None, None, 1, None)
    with pytest.raises(ValueError, match="row stride"):
        _abi.call("tsm_qmix_egreedy", None, 3, 4, 5, None, 0, 0, None, None, 2, None)
    with pytest.raises(ValueError, match="bad sizes"):
        _abi.call("tsm_qmix_finalize", None, 0, 16, None, None)
    assert _abi.call("tsm_qmix_partial_elems", 16, 48) == -1
    assert _abi.call("tsm_qmix_partial_elems", 256, 32) == 2 * 8  # 32 rows per workgroup at E = 32
    with pytest.raises(ValueError, match="1 to 8 agents"):
        QMIXMixer(9, 16, device="cpu")
    with pytest.raises(ValueError, match=r"\(32, 64\)"):
        ops.qmix_check(3, 16)
