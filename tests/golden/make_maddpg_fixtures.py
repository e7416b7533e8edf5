"""Generate tests/golden/maddpg.npz and maddpg_n8.npz by RUNNING THE REFERENCE's MADDPGPolicy (ctde.py:728-955, imported
through oracle/ref_shim.py) in float32 and in float64 (`.double()` on every module, fresh Adams, float64 inputs).

Variants (actors D -> H -> H -> Ad as DecentralizedActor; critics N (D + Ad) -> H -> H -> 1, a module defined here since the
reference has no one-output critic class; discount 0.99, tau 0.01, Adam lr 1e-3):
  small    N 3, D 18, Ad 2, H 64, B 256: three rounds of learn + update_target_networks
  odd      N 2, D 17, Ad 3, H 32, B 67: one round (unaligned rows, partial tiles)
  n8       N 8, D 16, Ad 2, H 32, B 128: two rounds (maddpg_n8.npz)
  forward  the actions of MADDPGPolicy.forward on `small`'s initial actors
About 10 % of every agent's rows are terminated, the flags drawn per agent.
Stored: inputs and initial weights (f32, as the reference holds them); the losses of both runs; per parameter array
(first-call gradients, weights after every learn, targets after every update) the reference's own f32 error
e_ref = max |ref32 - ref64| and a digest of the f64 array (sum, sum of squares, 512 fixed entries) that pins the float64
restatement (tests/maddpg_restatement.py) to the reference; the GPU tests compare against the restatement's full arrays.
Every file stays <= 1 MiB.

Gradients are the ones each Adam steps on (recorded by the optimizer's own `step`): after `learn` returns, a critic's
`.grad` also carries what `actor_loss.backward()` added to it (:924; the critic's zero_grad runs only before its own
backward, :901).

Kinks: before every call each joint row is redrawn while any f64 ReLU pre-activation of any pass the call makes (actors,
target actors, critics on X and X', the stepped critics on X_i) lies within DELTA of zero (rows act independently); the
share redrawn in the first pass is recorded and must stay <= 25 %.
"""
from __future__ import annotations

import copy
import inspect
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import ref_shim  # noqa: E402

ref_shim.install()

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402
from tianshou.algorithm.multiagent.ctde import DecentralizedActor, MADDPGPolicy  # noqa: E402
from tianshou.data import Batch  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from maddpg_restatement import MaddpgRestatement  # noqa: E402

DELTA = 1e-5
N_DIGEST = 512


class JointCritic(nn.Module):
    """[obs_0 .. obs_{N-1} | act_0 .. act_{N-1}] -> one value."""

    def __init__(self, in_dim: int, hidden_dim: int) -> None:
        super().__init__()
        self.fc1 = nn.Linear(in_dim, hidden_dim)
        self.fc2 = nn.Linear(hidden_dim, hidden_dim)
        self.fc3 = nn.Linear(hidden_dim, 1)

    def forward(self, x):
        return self.fc3(F.relu(self.fc2(F.relu(self.fc1(x)))))


class RecordingAdam(torch.optim.Adam):
    """torch.optim.Adam that keeps a copy of the gradients it steps on."""

    def step(self, closure=None):
        self.stepped_on = [p.grad.detach().clone() for g in self.param_groups for p in g["params"]]
        return super().step(closure)


def flat_nets(nets) -> np.ndarray:
    return np.concatenate([p.detach().double().reshape(-1).numpy() for m in nets for p in m.parameters()])


def flat_grads(pol) -> np.ndarray:
    return np.concatenate([g.double().reshape(-1).numpy() for o in list(pol.optimizer_actors) + list(pol.optimizer_critics)
                           for g in o.stepped_on])


def digest(res: dict, key: str, x: np.ndarray) -> None:
    idx = np.random.RandomState(12345).choice(x.size, min(N_DIGEST, x.size), replace=False)
    idx.sort()
    res[f"{key}_dsum"] = np.float64(x.sum())
    res[f"{key}_dsq"] = np.float64((x * x).sum())
    res[f"{key}_didx"] = idx.astype(np.int32)
    res[f"{key}_dval"] = x[idx]


def draw_rows(rs, N, B, D, Ad):
    return dict(obs=rs.standard_normal((N, B, D)).astype(np.float32), obs_next=rs.standard_normal((N, B, D)).astype(np.float32),
                act=rs.uniform(-1, 1, (N, B, Ad)).astype(np.float32), rew=rs.standard_normal((N, B)).astype(np.float32),
                term=rs.rand(N, B) < 0.1)


def redraw(rs, rows, R, N, B, D, Ad):
    """Redraw kinked rows until none is left; -> share of rows redrawn in the first pass."""
    share = None
    for _ in range(50):
        bad = R.kink_rows(rows["obs"], rows["act"], rows["rew"], rows["obs_next"], rows["term"], DELTA)
        if share is None:
            share = float(bad.mean())
        if not bad.any():
            if share > 0.25:
                raise RuntimeError(f"{share:.3f} of the rows had to be redrawn (> 25 %)")
            return share
        fresh = draw_rows(rs, N, B, D, Ad)
        for k in rows:
            rows[k][:, bad] = fresh[k][:, bad]
    raise RuntimeError("kinked rows remain after 50 redraws")


def ref_batch(rows, N, dtype):
    b = Batch()
    for i in range(N):
        b[f"agent_{i}"] = Batch(obs=rows["obs"][i].astype(dtype), act=rows["act"][i].astype(dtype),
                                rew=rows["rew"][i].astype(dtype), obs_next=rows["obs_next"][i].astype(dtype),
                                terminated=rows["term"][i].copy())
    return b


def make_policy(actors, critics, N, D, Ad, double: bool):
    actors = [copy.deepcopy(a).double() if double else copy.deepcopy(a) for a in actors]
    critics = [copy.deepcopy(c).double() if double else copy.deepcopy(c) for c in critics]
    return MADDPGPolicy(actors, critics, gym.spaces.Box(-np.inf, np.inf, (D,)), gym.spaces.Box(-1.0, 1.0, (Ad,)), N,
                        optimizer_actors=[RecordingAdam(a.parameters()) for a in actors],
                        optimizer_critics=[RecordingAdam(c.parameters()) for c in critics])


def run_variant(res, name, N, D, Ad, H, B, rounds, seed):
    rs = np.random.RandomState(seed)
    torch.manual_seed(seed)
    actors = [DecentralizedActor(D, Ad, hidden_dim=H) for _ in range(N)]
    critics = [JointCritic(N * (D + Ad), H) for _ in range(N)]
    init32 = flat_nets(actors + critics).astype(np.float32)
    res[f"{name}_dims"] = np.array([N, D, Ad, H, B, rounds], np.int64)
    res[f"{name}_init"] = init32
    p32, p64 = make_policy(actors, critics, N, D, Ad, False), make_policy(actors, critics, N, D, Ad, True)
    R = MaddpgRestatement(init32, N, [D, H, H, Ad], [N * (D + Ad), H, H, 1], gamma=p64.discount_factor, tau=p64.tau)
    shares = []
    for k in range(rounds):
        rows = draw_rows(rs, N, B, D, Ad)
        shares.append(redraw(rs, rows, R, N, B, D, Ad))
        for kk, v in rows.items():
            res[f"{name}_r{k}_{kk}"] = v
        r32 = p32.learn(ref_batch(rows, N, np.float32))
        r64 = p64.learn(ref_batch(rows, N, np.float64))
        rr = R.learn(rows["obs"], rows["act"], rows["rew"], rows["obs_next"], rows["term"])
        keys = [k_ for k_ in r64 if k_.endswith("_loss")]
        res[f"{name}_loss_keys"] = np.array(keys)
        res[f"{name}_r{k}_losses"] = np.array([[float(r64[k_]) for k_ in keys], [float(r32[k_]) for k_ in keys]])
        arrays = {}
        if k == 0:
            arrays["grad"] = (flat_grads(p64), flat_grads(p32))
        arrays["weights"] = (flat_nets(p64.actors + p64.critics), flat_nets(p32.actors + p32.critics))
        p32.update_target_networks()
        p64.update_target_networks()
        R.update_targets()
        arrays["targets"] = (flat_nets(p64.target_actors + p64.target_critics), flat_nets(p32.target_actors + p32.target_critics))
        for an, (a64, a32) in arrays.items():
            key = f"{name}_r{k}_{an}"
            res[f"{key}_eref"] = np.float64(np.abs(a32 - a64).max())
            digest(res, key, a64)
        # the generator's own check that the restatement follows the reference (the CPU test repeats it from the file)
        for k_ in keys:
            assert abs(rr[k_] - float(r64[k_])) <= 1e-12 * abs(float(r64[k_])), (name, k, k_)
        assert np.allclose(R.weights(), arrays["weights"][0], rtol=1e-12, atol=1e-15), (name, k)
        assert np.allclose(R.targets(), arrays["targets"][0], rtol=1e-12, atol=1e-15), (name, k)
    res[f"{name}_redraw_share"] = np.array(shares)
    print(name, "params", init32.size, "redraw shares", shares, "critic_loss",
          [float(res[f"{name}_r{k}_losses"][0][-1]) for k in range(rounds)])
    return actors, critics


def forward_case(res, actors, critics, N, D, Ad, B=33, seed=7):
    rs = np.random.RandomState(seed)
    pol = make_policy(actors, critics, N, D, Ad, False)
    obs = rs.standard_normal((N, B, D)).astype(np.float32)
    out = pol.forward(Batch(**{f"agent_{i}": Batch(obs=obs[i]) for i in range(N)}))
    res["fwd_obs"] = obs
    res["fwd_act"] = np.stack([out[f"agent_{i}"].act.detach().numpy() for i in range(N)])


def signatures(res, actors, critics, N, D, Ad):
    res["sig_policy"] = np.array(str(inspect.signature(MADDPGPolicy.__init__)))
    for m in ("forward", "learn", "update_target_networks"):
        res[f"sig_{m}"] = np.array(str(inspect.signature(getattr(MADDPGPolicy, m))))
    res["sd_keys"] = np.array(list(make_policy(actors, critics, N, D, Ad, False).state_dict().keys()), dtype=str)


def save(name: str, arrays: dict) -> None:
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(arrays)} arrays, {size} bytes")
    assert size <= 1 << 20, f"{name} is larger than 1 MiB"


def main():
    torch.set_num_threads(4)
    common = {"gamma": np.float64(0.99), "tau": np.float64(0.01), "delta": np.float64(DELTA)}
    res = dict(common)
    actors, critics = run_variant(res, "small", 3, 18, 2, 64, 256, 3, seed=31)
    run_variant(res, "odd", 2, 17, 3, 32, 67, 1, seed=37)
    # (run_variant hands back the modules it built: the policies work on copies, so these still hold small's initial weights)
    forward_case(res, actors, critics, 3, 18, 2)
    signatures(res, actors, critics, 3, 18, 2)
    save("maddpg.npz", res)
    n8 = dict(common)
    run_variant(n8, "n8", 8, 16, 2, 32, 128, 2, seed=41)
    save("maddpg_n8.npz", n8)


if __name__ == "__main__":
    main()
