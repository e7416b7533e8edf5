"""Generate tests/golden/qmix.npz, qmix_c3.npz and qmix_c3_rows.npz by RUNNING THE REFERENCE's QMIXPolicy
(ctde.py:417-725, imported through oracle/ref_shim.py) in float32 and in float64 (`.double()` on every module, a fresh
Adam, float64 inputs).

Variants (actor Q-nets D -> H -> H -> A, mixer on the concatenated joint observation, mixing_embed_dim 32,
hypernet_embed_dim 64, discount 0.99, tau 0.005):
  small    N 3, D 18, A 5, H 64, B 256: three rounds of learn + update_target_networks, ~10 % terminated rows
  nonmono  the same nets and first batch with enforce_monotonic=False, one round
  c3       N 8, D 48, A 5, H 64, B 128: two rounds (qmix_c3.npz; its per-round inputs in qmix_c3_rows.npz)
  forward  greedy actions on both forward paths; epsilon = 1 and epsilon = 0.5 over 20 calls under fixed seeds
Stored: inputs and initial weights (f32, as the reference holds them); losses and q_values of both runs; per parameter
array (first-call gradients, weights after every learn, targets after every update) the reference's own f32 error
e_ref = max |ref32 - ref64| and a digest of the f64 array (sum, sum of squares, 512 fixed entries) that pins the
float64 restatement (tests/qmix_restatement.py) to the reference; the GPU tests compare against the restatement's full
arrays.  Why digests: fixtures added from this generator on are kept at most 1 MiB per file, so that the repository does not
grow by megabytes per feature (the older ctde_c3.npz / ppo_update_wide.npz predate that rule).  One f64 copy of c3's
153 641 parameters alone is 1.2 MB, and a variant needs five (c3) to seven (small) such arrays (small: 36 016 parameters, 2 MB in all).

Kinks: before every call each joint row is redrawn while any f64 ReLU pre-activation, w1raw / w2raw entry or greedy top-2
Q gap (online or target) lies within DELTA of its kink (rows act independently); the share redrawn is recorded and must
stay <= 25 %.
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
from tianshou.algorithm.multiagent.ctde import DecentralizedActor, QMIXMixer, QMIXPolicy  # noqa: E402
from tianshou.data import Batch  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from qmix_restatement import QmixRestatement  # noqa: E402

DELTA = 1e-5
TAU = 0.005
N_DIGEST = 512


def flat_params(actors, mixer, grad: bool = False) -> np.ndarray:
    ps = [p for a in actors for p in a.parameters()] + list(mixer.parameters())
    return np.concatenate([(p.grad if grad else p).detach().double().reshape(-1).numpy() for p in ps])


def digest(res: dict, key: str, x: np.ndarray) -> None:
    idx = np.random.RandomState(12345).choice(x.size, min(N_DIGEST, x.size), replace=False)
    idx.sort()
    res[f"{key}_dsum"] = np.float64(x.sum())
    res[f"{key}_dsq"] = np.float64((x * x).sum())
    res[f"{key}_didx"] = idx.astype(np.int32)
    res[f"{key}_dval"] = x[idx]


def draw_rows(rs, N, B, D, A):
    return dict(obs=rs.standard_normal((N, B, D)).astype(np.float32), obs_next=rs.standard_normal((N, B, D)).astype(np.float32),
                act=rs.randint(0, A, (N, B)).astype(np.int64), rew=rs.standard_normal((N, B)).astype(np.float32),
                term=rs.rand(B) < 0.1)


def redraw(rs, rows, R, N, B, D, A):
    """Redraw kinked rows until none is left; -> share of rows redrawn in the first pass."""
    share = None
    for _ in range(50):
        gs = rows["obs"].transpose(1, 0, 2).reshape(B, N * D)
        gsn = rows["obs_next"].transpose(1, 0, 2).reshape(B, N * D)
        bad = R.kink_rows(rows["obs"], rows["obs_next"], gs, gsn, DELTA)
        if share is None:
            share = float(bad.mean())
        if not bad.any():
            return share
        fresh = draw_rows(rs, N, B, D, A)
        for k in rows:
            if k == "term":
                rows[k][bad] = fresh[k][bad]
            else:
                rows[k][:, bad] = fresh[k][:, bad]
    raise RuntimeError("kinked rows remain after 50 redraws")


def ref_batch(rows, N, B, D, dtype):
    b = Batch()
    for i in range(N):
        b[f"agent_{i}"] = Batch(obs=rows["obs"][i].astype(dtype), act=rows["act"][i], rew=rows["rew"][i].astype(dtype),
                                obs_next=rows["obs_next"][i].astype(dtype), terminated=rows["term"].copy())
    b["global_obs"] = rows["obs"].transpose(1, 0, 2).reshape(B, N * D).astype(dtype)
    b["global_obs_next"] = rows["obs_next"].transpose(1, 0, 2).reshape(B, N * D).astype(dtype)
    return b


def make_policy(actors, mixer, N, D, A, double: bool):
    if double:
        actors = [copy.deepcopy(a).double() for a in actors]
        mixer = copy.deepcopy(mixer).double()
        params = [p for a in actors for p in a.parameters()] + list(mixer.parameters())
        opt = torch.optim.Adam(params)
    else:
        actors = [copy.deepcopy(a) for a in actors]
        mixer = copy.deepcopy(mixer)
        opt = None
    pol = QMIXPolicy(actors, mixer, gym.spaces.Box(-np.inf, np.inf, (D,)), gym.spaces.Discrete(A), N, optimizer=opt)
    return pol


def run_variant(res, name, N, D, A, H, B, rounds, mono, seed, init=None, first_rows=None):
    E, Hh = 32, 64
    rs = np.random.RandomState(seed)
    torch.manual_seed(seed)
    actors = [DecentralizedActor(D, A, hidden_dim=H) for _ in range(N)]
    mixer = QMIXMixer(N, N * D, mixing_embed_dim=E, hypernet_embed_dim=Hh, enforce_monotonic=mono)
    if init is not None:  # the same initial weights as another variant
        ps = [p for a in actors for p in a.parameters()] + list(mixer.parameters())
        o = 0
        with torch.no_grad():
            for p in ps:
                p.copy_(torch.as_tensor(init[o:o + p.numel()]).view_as(p))
                o += p.numel()
    init32 = flat_params(actors, mixer).astype(np.float32)
    res[f"{name}_dims"] = np.array([N, D, A, H, N * D, E, Hh, B, rounds, int(mono)], np.int64)
    res[f"{name}_init"] = init32
    p32, p64 = make_policy(actors, mixer, N, D, A, False), make_policy(actors, mixer, N, D, A, True)
    R = QmixRestatement(init32, (N, D, A, H, N * D, E, Hh), monotonic=mono)
    shares = []
    for k in range(rounds):
        rows = {kk: v.copy() for kk, v in first_rows.items()} if (first_rows is not None and k == 0) else draw_rows(rs, N, B, D, A)
        shares.append(redraw(rs, rows, R, N, B, D, A))
        for kk, v in rows.items():
            res[f"{name}_r{k}_{kk}"] = v
        r32 = p32.learn(ref_batch(rows, N, B, D, np.float32))
        r64 = p64.learn(ref_batch(rows, N, B, D, np.float64))
        gs = rows["obs"].transpose(1, 0, 2).reshape(B, N * D)
        gsn = rows["obs_next"].transpose(1, 0, 2).reshape(B, N * D)
        rr = R.learn(rows["obs"], rows["act"], rows["rew"], rows["obs_next"], rows["term"], gs, gsn)
        res[f"{name}_r{k}_loss"] = np.array([r64["loss"], r32["loss"]])
        res[f"{name}_r{k}_q_values"] = np.array([r64["q_values"], r32["q_values"]])
        arrays = {}
        if k == 0:
            arrays["grad"] = (flat_params(p64.actors, p64.mixer, grad=True), flat_params(p32.actors, p32.mixer, grad=True))
        arrays["weights"] = (flat_params(p64.actors, p64.mixer), flat_params(p32.actors, p32.mixer))
        p32.update_target_networks(TAU)
        p64.update_target_networks(TAU)
        R.update_targets(TAU)
        arrays["targets"] = (flat_params(p64.target_actors, p64.target_mixer), flat_params(p32.target_actors, p32.target_mixer))
        for an, (a64, a32) in arrays.items():
            key = f"{name}_r{k}_{an}"
            res[f"{key}_eref"] = np.float64(np.abs(a32 - a64).max())
            digest(res, key, a64)
        # the generator's own check that the restatement follows the reference (the CPU test repeats it from the file)
        assert abs(rr["loss"] - r64["loss"]) <= 1e-12 * abs(r64["loss"]), (name, k)
        assert np.allclose(R.weights(), arrays["weights"][0], rtol=1e-12, atol=1e-15), (name, k)
    res[f"{name}_redraw_share"] = np.array(shares)
    print(name, "redraw shares", shares, "losses", [float(res[f"{name}_r{k}_loss"][0]) for k in range(rounds)])
    return init32


def forward_cases(res, N=3, D=18, A=5, H=64, B=64, seed=7):
    rs = np.random.RandomState(seed)
    torch.manual_seed(seed)
    actors = [DecentralizedActor(D, A, hidden_dim=H) for _ in range(N)]
    mixer = QMIXMixer(N, N * D)
    res["fwd_dims"] = np.array([N, D, A, H, B], np.int64)
    res["fwd_init"] = flat_params(actors, mixer).astype(np.float32)
    pol = make_policy(actors, mixer, N, D, A, False)
    R = QmixRestatement(res["fwd_init"], (N, D, A, H, N * D, 32, 64))
    rows = draw_rows(rs, N, B, D, A)
    redraw(rs, rows, R, N, B, D, A)
    obs = rows["obs"]
    res["fwd_obs"] = obs
    single = Batch(obs=obs[0])
    multi = Batch(**{f"agent_{i}": Batch(obs=obs[i]) for i in range(N)})
    pol.epsilon = 0.0
    res["fwd_greedy_single"] = pol.forward(single).act.numpy()
    out = pol.forward(multi)
    res["fwd_greedy_multi"] = np.stack([out[f"agent_{i}"].act.numpy() for i in range(N)])
    for tag, eps in (("eps1", 1.0), ("eps05", 0.5)):
        pol.epsilon = eps
        np.random.seed(1000 + int(eps * 10))
        torch.manual_seed(2000 + int(eps * 10))
        seq = []
        for _ in range(20):
            out = pol.forward(multi)
            seq.append(np.stack([out[f"agent_{i}"].act.numpy() for i in range(N)]))
        res[f"fwd_{tag}"] = np.stack(seq)
        res[f"fwd_{tag}_seeds"] = np.array([1000 + int(eps * 10), 2000 + int(eps * 10)], np.int64)


def signatures(res):
    res["sig_mixer"] = np.array(str(inspect.signature(QMIXMixer.__init__)))
    res["sig_policy"] = np.array(str(inspect.signature(QMIXPolicy.__init__)))
    for m in ("forward", "learn", "update_target_networks"):
        res[f"sig_{m}"] = np.array(str(inspect.signature(getattr(QMIXPolicy, m))))
    torch.manual_seed(0)
    N, D, A = 3, 18, 5
    pol = make_policy([DecentralizedActor(D, A, 64) for _ in range(N)], QMIXMixer(N, N * D), N, D, A, False)
    sd = pol.state_dict()
    res["sd_keys"] = np.array(list(sd.keys()))
    res["sd_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])


def main():
    res = {"gamma": np.float64(0.99), "tau": np.float64(TAU), "delta": np.float64(DELTA)}
    torch.set_num_threads(4)
    init = run_variant(res, "small", 3, 18, 5, 64, 256, 3, True, seed=11)
    first = {k.split("_r0_")[1]: res[k] for k in list(res) if k.startswith("small_r0_")
             and k.split("_r0_")[1] in ("obs", "obs_next", "act", "rew", "term")}
    run_variant(res, "nonmono", 3, 18, 5, 64, 256, 1, False, seed=11, init=init, first_rows=first)
    forward_cases(res)
    signatures(res)
    save("qmix.npz", res)
    c3 = {"gamma": res["gamma"], "tau": res["tau"], "delta": res["delta"]}
    run_variant(c3, "c3", 8, 48, 5, 64, 128, 2, True, seed=23)
    rows = {k: c3.pop(k) for k in [k for k in c3 if k.endswith(("_obs", "_obs_next"))]}
    save("qmix_c3.npz", c3)
    save("qmix_c3_rows.npz", rows)


def save(name: str, arrays: dict) -> None:
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(arrays)} arrays, {size} bytes")
    assert size <= 1 << 20, f"{name} is larger than 1 MiB"


if __name__ == "__main__":
    main()
