"""Generate tests/golden/gstate.npz by RUNNING THE REFERENCE's `GlobalStateConstructor` in its modes "attention" and "graph"
(algorithm/multiagent/ctde.py:230-343, imported through oracle/ref_shim.py) and its `CTDEPolicy.learn` behind them, in float64
(`.double()` modules on the float32 initial weights, float64 copies of the float32 inputs).  Every stored result is the float64
run's, rounded to float32 (losses stay float64).  Does nothing without /root/reference.

Sections (every array is data: initial weights, inputs, expected outputs):
  at{i}_*  attention, (N, D, hidden) = ATT_CASES[i]: weights under the state_dict keys, obs [B, N, D], `build` output, a fixed
           upstream d_state and, from autograd, every parameter gradient of sum(state * d_state); keys and shapes of the
           state_dict in its order.
  gr{i}_*  graph, GRAPH_CASES[i] = (N, D, hidden, adjacency or none); the adjacency is a ring with self-loops and unequal,
           non-symmetric weights.  The same arrays.
  la_* lg_*  ONE `CTDEPolicy.learn` step per mode (N = 3, D = 8, hidden = 16, B = 32): `batch.global_obs = gsc.build(obs_dict)`
           left attached to autograd and the constructor's parameters in `optim_critic`'s Adam; stored: both losses and the
           post-step weights of critic, actor and constructor.  The generator asserts that the constructor's weights moved.
           Adam runs at eps = LEARN_EPS, not torch's 1e-8: the in-projection's KEY bias has a gradient that is zero in exact
           arithmetic (a shift common to all keys leaves the softmax unchanged), and Adam's first step lr g / (|g| + eps) turns
           the float32 rounding noise of such an entry, 1e-10, into 1e-5 of movement at eps = 1e-8 -- in the reference's own
           float32 run as here (printed below as e_ref) -- which says nothing about the kernels.
The generator asserts that the restatement (tests/gstate_restatement.py) follows the reference's float64 run to 1e-10 in both
orders of operations, and that no gnn_layer1 pre-activation lies within DELTA of zero.
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import ref_shim  # noqa: E402

if not ref_shim.reference_available():
    print("make_gstate_fixtures: the reference is not on this machine; nothing written")
    sys.exit(0)
ref_shim.install()

import torch  # noqa: E402
from tianshou.algorithm.multiagent.ctde import (  # noqa: E402
    CentralizedCritic,
    CTDEPolicy,
    DecentralizedActor,
    GlobalStateConstructor,
)
from tianshou.data import Batch  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

import gstate_restatement as R  # noqa: E402

DELTA = 1e-5
LR, LEARN_EPS, GAMMA = 1e-3, 1e-5, 0.99
ATT_CASES = ((3, 8, 16), (8, 48, 64), (1, 4, 5))
ATT_ROWS = (7, 5, 6)


def ring(N: int) -> np.ndarray:
    """A ring with self-loops, unequal weights, not symmetric: agent n hears itself, n + 1 and (less) n - 1."""
    A = np.zeros((N, N), np.float32)
    for n in range(N):
        A[n, n] = 1.0 + 0.25 * n
        A[n, (n + 1) % N] += 0.5
        A[n, (n - 1) % N] += 0.125 * (n + 1)
    return A


GRAPH_CASES = ((3, 6, 16, False), (3, 6, 16, True), (8, 48, 64, True), (1, 5, 3, False), (5, 7, 9, True))
GRAPH_ROWS = (7, 7, 5, 6, 9)


def weights32(mod) -> dict:
    return {k: v.detach().numpy().astype(np.float32).copy() for k, v in mod.state_dict().items()}


def r32(x) -> np.ndarray:
    return np.asarray(x, np.float64).astype(np.float32)


def obs_dict(obs: np.ndarray) -> dict:
    """obs [B, N, D] -> {agent_n: float64 tensor [B, D]} in agent order."""
    return {f"agent_{n}": torch.as_tensor(obs[:, n].astype(np.float64)) for n in range(obs.shape[1])}


def close(a, b, what) -> None:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.abs(a - b).max() <= 1e-10 * max(np.abs(b).max(), 1e-300), (what, np.abs(a - b).max(), np.abs(b).max())


def case_section(res, prefix, mode, N, D, H, B, seed, adjacency=None):
    for s in range(seed, seed + 100):
        torch.manual_seed(s)
        rs = np.random.RandomState(s)
        kw = dict(adjacency_matrix=torch.as_tensor(adjacency.astype(np.float64))) if adjacency is not None else {}
        gsc = GlobalStateConstructor(mode=mode, obs_dim=D, n_agents=N, hidden_dim=H, **kw)
        w = weights32(gsc)
        obs = rs.standard_normal((B, N, D)).astype(np.float32)
        if mode != "graph" or R.relu_gap(w, obs) > DELTA:
            break
    else:
        raise AssertionError("no seed without a kink")
    d_state = rs.standard_normal((B, H)).astype(np.float32)
    gsc = gsc.double()
    state = gsc.build(obs_dict(obs))
    (state * torch.as_tensor(d_state.astype(np.float64))).sum().backward()
    grads = {k: p.grad.numpy() for k, p in gsc.named_parameters()}
    fwd, bwd = (R.attention_forward, R.attention_backward) if mode == "attention" else \
        (lambda w, o, pooled: R.graph_forward(w, o, adjacency, pooled), R.graph_backward)
    for pooled in (False, True):
        mine, cache = fwd(w, obs, pooled=pooled)
        close(mine, state.detach().numpy(), (prefix, "state", pooled))
    for k, g in bwd(w, cache, d_state).items():
        close(g, grads[k], (prefix, k))
    res[prefix + "keys"] = np.array(list(w.keys()))
    res[prefix + "shapes"] = np.array([",".join(str(d) for d in v.shape) for v in w.values()])
    res[prefix + "dims"] = np.array([N, D, H, B], np.int64)
    res.update({prefix + "obs": obs, prefix + "d_state": d_state, prefix + "state": r32(state.detach().numpy())})
    if adjacency is not None:
        res[prefix + "adjacency"] = adjacency
    for k, v in w.items():
        res[f"{prefix}w_{k}"] = v
        res[f"{prefix}g_{k}"] = r32(grads[k])
    print(prefix, mode, (N, D, H, B), "seed", s, "max |state|", float(np.abs(state.detach().numpy()).max()))


def learn_section(res, prefix, mode, seed, adjacency=None):
    N, D, H, B, A, hid = 3, 8, 16, 32, 5, 16
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    kw = dict(adjacency_matrix=torch.as_tensor(adjacency.astype(np.float64))) if adjacency is not None else {}
    gsc0 = GlobalStateConstructor(mode=mode, obs_dim=D, n_agents=N, hidden_dim=H, **kw)
    actor0, critic0 = DecentralizedActor(D, A, hidden_dim=hid), CentralizedCritic(H, N, hidden_dim=hid)
    init = {"gsc": weights32(gsc0), "actor": weights32(actor0), "critic": weights32(critic0)}
    obs, obs_next = (rs.standard_normal((B, N, D)).astype(np.float32) for _ in range(2))
    act, rew = rs.randint(0, A, B), rs.standard_normal(B).astype(np.float32)
    term = rs.rand(B) < 0.15
    if mode == "graph":
        assert min(R.relu_gap(init["gsc"], obs), R.relu_gap(init["gsc"], obs_next)) > DELTA
    out = {}
    for dbl, eps in ((True, LEARN_EPS), (False, LEARN_EPS), (True, 1e-8), (False, 1e-8)):
        dt, ndt = (torch.float64, np.float64) if dbl else (torch.float32, np.float32)
        gsc, actor, critic = (copy.deepcopy(m).to(dt) for m in (gsc0, actor0, critic0))
        if adjacency is not None:
            gsc.adjacency_matrix = torch.as_tensor(adjacency.astype(ndt))
        pol = CTDEPolicy(actor=actor, critic=critic,
                         optim_actor=torch.optim.Adam(actor.parameters(), lr=LR, eps=eps),
                         optim_critic=torch.optim.Adam(list(critic.parameters()) + list(gsc.parameters()), lr=LR, eps=eps),
                         observation_space=gym.spaces.Box(-np.inf, np.inf, (D,)), action_space=gym.spaces.Discrete(A),
                         discount_factor=GAMMA)
        od = {f"agent_{n}": torch.as_tensor(obs[:, n].astype(ndt)) for n in range(N)}
        nd = {f"agent_{n}": torch.as_tensor(obs_next[:, n].astype(ndt)) for n in range(N)}
        batch = Batch(obs=obs[:, 0].astype(ndt), act=act, rew=rew.astype(ndt), obs_next=obs_next[:, 0].astype(ndt), terminated=term)
        batch.global_obs = gsc.build(od)              # attached: critic_loss.backward() reaches the constructor
        batch.global_obs_next = gsc.build(nd)         # the target side is detached by the reference itself (ctde.py:172)
        losses = pol.learn(batch)
        out[dbl, eps] = dict(losses=np.array([losses["actor_loss"], losses["critic_loss"]], np.float64),
                             **{name: {k: v.detach().double().numpy() for k, v in m.state_dict().items()}
                                for name, m in (("gsc", gsc), ("actor", actor), ("critic", critic))})
    ref = out[True, LEARN_EPS]
    moved = max(np.abs(ref["gsc"][k] - init["gsc"][k]).max() for k in init["gsc"])
    assert moved > 0.5 * LR, moved   # the constructor's weights moved, by an Adam step
    for eps in (LEARN_EPS, 1e-8):    # the reference's own float32 error on the constructor's vector, relative to max |w|
        cat = lambda d: np.concatenate([v.reshape(-1) for v in d.values()])  # noqa: E731
        a, b = cat(out[True, eps]["gsc"]), cat(out[False, eps]["gsc"])
        print(f"{prefix} Adam eps {eps:g}: e_ref of the constructor's post-step vector = {np.abs(a - b).max() / np.abs(a).max():.3g}")
    res.update({prefix + "obs": obs, prefix + "obs_next": obs_next, prefix + "act": act.astype(np.int64), prefix + "rew": rew,
                prefix + "terminated": term, prefix + "losses": ref["losses"],
                prefix + "dims": np.array([N, D, H, B, A, hid], np.int64),
                prefix + "hyper": np.array([LR, LEARN_EPS, GAMMA], np.float64)})
    if adjacency is not None:
        res[prefix + "adjacency"] = adjacency
    for name in ("gsc", "actor", "critic"):
        for k, v in init[name].items():
            res[f"{prefix}{name}_w_{k}"] = v
            res[f"{prefix}{name}_after_{k}"] = r32(ref[name][k])
    print(prefix, mode, "losses", ref["losses"].tolist(), "moved", float(moved))


def main():
    torch.set_num_threads(4)
    res = {"delta": np.float64(DELTA), "att_cases": np.array(ATT_CASES, np.int64),
           "graph_cases": np.array([c[:3] + (int(c[3]),) for c in GRAPH_CASES], np.int64)}
    for i, ((N, D, H), B) in enumerate(zip(ATT_CASES, ATT_ROWS)):
        case_section(res, f"at{i}_", "attention", N, D, H, B, 100 + i)
    for i, ((N, D, H, adj), B) in enumerate(zip(GRAPH_CASES, GRAPH_ROWS)):
        case_section(res, f"gr{i}_", "graph", N, D, H, B, 200 + i, ring(N) if adj else None)
    learn_section(res, "la_", "attention", 301)
    learn_section(res, "lg_", "graph", 302, ring(3))
    path = os.path.join(HERE, "gstate.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 400 * 1024


if __name__ == "__main__":
    main()
