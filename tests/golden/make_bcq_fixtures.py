"""Generate tests/golden/bcq.npz by RUNNING THE REFERENCE's BCQ, BCQPolicy, VAE and Perturbation (imitation/bcq.py,
utils/net/continuous.py:395-513, imported through oracle/ref_shim.py) in float64 and float32: per case two consecutive
`_update_with_batch` calls on a small hand-filled buffer, then `BCQPolicy.forward` on a few observations.  Every torch.randn /
torch.randn_like is replaced by arrays drawn here and recorded as data, so both runs and every test see the same draws.  The
encoder, decoder, perturbation and critic modules are defined here or in make_cac_fixtures.py (the reference's Net casts
observations to float32, which a float64 run cannot use); the VAE and Perturbation around them are the reference's.  In the
float64 run `Tensor.float()` keeps float64: bcq.py:237 rounds the target to float32 in any run, which a float64 yardstick must
not.

Sizes: obs 6, act 3, hidden 16-16 (VAE 8-8: the fixture stays below cql.npz), B 12, K 3, L 6, S 5, 4 acting observations,
buffer 4 x 16 with 13 steps.  Cases (`cases`): critic2=None, lmbda, phi, the log_std bias of the first L / 2 latents, max_action.  With phi = 0.5 the decoder's and
the perturbation net's last layers are scaled up so that a share of the perturbed actions clip at +-max_action
(`s{k}_clipped`); a log_std bias of -5 puts a share of the raw log_std below -4 (`s{k}_below`).  Per case `c{i}_`:
  init_{pert, critic, critic2, vae}          the initial flat vectors (float32 values; the VAE's in the package's layout:
                                             encoder with mean stacked over log_std as its last layer, then the decoder)
  s{k}_indices, z_vae, z_next, z_obs         the sampled rows and the three normal draws of call k
  s{k}_stats (float64 run), stats32, s{k}_target; `*_eref` = max |ref32 - ref64|
  s{k}_grad_{net}                            every gradient at its optimizer's step, with `_eref`
  s1_w_{net}                                 every network after the second call, with `_eref`
  act_obs, act_z, act, act_index, act_eref   acting after the second call
The generator asserts that no ReLU pre-activation, no q1-versus-q2 gap of a real twin, no raw log_std versus -4 and 15, no
normal versus +-0.5, no unclamped perturbed action versus +-max_action and no gap between the top two q of an acting group
lies within DELTA of zero, and that the restatement (tests/bcq_restatement.py) follows the float64 run to 1e-10.  It prints
the float32 run's distance from the float64 run per quantity.
"""
from __future__ import annotations

import copy
import inspect
import os

import numpy as np

import make_cac_fixtures as M  # noqa: E402  (installs the shim, through make_dqn_fixtures)
from make_cac_fixtures import AD, B, D, HID, LR, N_ENV, S, T, TAU, Critic, Kink, Noise, _MLP, emax, fill  # noqa: E402
from make_dqn_fixtures import DELTA, GAMMA  # noqa: E402

import torch  # noqa: E402
from tianshou.algorithm.imitation.bcq import BCQ, BCQPolicy  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net.common import MLP, Net  # noqa: E402
from tianshou.utils.net.continuous import VAE, ContinuousCritic, Perturbation  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from bcq_restatement import BcqRestatement  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
K, L, S_ACT, N_ACT, VHID = 3, 6, 5, 4, [8, 8]
STAT_KEYS = ("actor_loss", "critic1_loss", "critic2_loss", "vae_loss")
NETS = ["pert", "critic", "critic2", "vae", "pert_old", "critic_old", "critic2_old"]
#        critic2=None lmbda phi   ls_bias max_action
CASES = [(0, 0.75, 0.05, 0.0, 1.0), (1, 0.75, 0.05, 0.0, 1.0), (0, 1.0, 0.05, 0.0, 1.0), (0, 0.75, 0.5, 0.0, 1.0),
         (0, 0.75, 0.05, -5.0, 1.0), (0, 0.75, 0.05, 0.0, 2.0)]


def _cast(x, w):
    return x.to(w.dtype) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(w.dtype)


class Trunk(_MLP):
    """The reference's encoder `MLP(output_dim=0)`: every layer is followed by its ReLU."""

    def forward(self, x):
        return self.trunk(_cast(x, self.layers[0].weight), len(self.layers))


class Dec(_MLP):
    def forward(self, x):
        return self.layers[-1](self.trunk(_cast(x, self.layers[0].weight), len(self.layers) - 1))


class PNet(Dec):
    """Stands where Perturbation's `preprocess_net` (a `Net`) stands: -> (logits, state)."""

    def forward(self, x, state=None, info=None):
        return super().forward(x), state


def layers_flat(layers, grad=False):
    ps = [q.grad if grad else q for l in layers for q in (l.weight, l.bias)]
    return np.concatenate([p.detach().double().reshape(-1).numpy() for p in ps])


def vae_flat(v, grad=False):
    """The package's layout of the reference VAE: the encoder's layers, [mean.weight; log_std.weight], [mean.bias;
    log_std.bias], the decoder's layers."""
    f = (lambda q: q.grad) if grad else (lambda q: q)
    cat = lambda a, b: torch.cat([f(a), f(b)], 0).detach().double().reshape(-1).numpy()  # noqa: E731
    return np.concatenate([layers_flat(v.encoder.layers, grad), cat(v.mean.weight, v.log_std.weight), cat(v.mean.bias, v.log_std.bias),
                           layers_flat(v.decoder.layers, grad)])


def net_flat(algo, name, grad=False):
    m = {"pert": lambda: algo.policy.actor_perturbation, "critic": lambda: algo.policy.critic, "critic2": lambda: algo.critic2,
         "vae": lambda: algo.policy.vae, "pert_old": lambda: algo.actor_perturbation_target.module,
         "critic_old": lambda: algo.critic_target.module, "critic2_old": lambda: algo.critic2_target.module}[name]()
    if name == "vae":
        return vae_flat(m, grad)
    return layers_flat(m.preprocess_net.layers if name.startswith("pert") else m.layers, grad)


def record_grads(algo) -> dict:
    got = {}
    for name, opt in (("vae", algo.vae_optim), ("critic", algo.critic_optim), ("critic2", algo.critic2_optim),
                      ("pert", algo.actor_perturbation_optim)):
        inner = opt._optim.step

        def step(*a, _inner=inner, _name=name, **kw):
            got[_name] = net_flat(algo, _name, grad=True)
            return _inner(*a, **kw)

        opt._optim.step = step
    return got


def make_modules(seed, phi, ls_bias, max_action):
    torch.manual_seed(seed)
    enc, dec = Trunk([D + AD, *VHID]), Dec([D + L, *VHID, AD])
    vae = VAE(encoder=enc, decoder=dec, hidden_dim=VHID[-1], latent_dim=L, max_action=max_action)
    pert = Perturbation(preprocess_net=PNet([D + AD, *HID, AD]), max_action=max_action, phi=phi)
    c1, c2 = Critic([D + AD, *HID, 1]), Critic([D + AD, *HID, 1])
    with torch.no_grad():
        vae.log_std.bias[:L // 2].add_(ls_bias)
        if phi > 0.1:   # wide actions and wide perturbations: some of their sums leave +-max_action
            for p in list(dec.layers[-1].parameters()) + list(pert.preprocess_net.layers[-1].parameters()):
                p.mul_(4.0)
    return vae, pert, c1, c2


def run_case(ci, case, seed, draws):
    no_c2, lmbda, phi, ls_bias, max_action = case
    rs = np.random.RandomState(seed)
    mods = make_modules(seed, phi, ls_bias, max_action)
    space = gym.spaces.Box(low=-max_action, high=max_action, shape=(AD,), dtype=np.float32)
    opt = lambda: AdamOptimizerFactory(lr=LR)  # noqa: E731
    bufs, algos, caught = {}, {}, {}
    for dbl in (True, False):
        bufs[dbl], _ = fill(np.random.RandomState(seed + 1000), VectorReplayBuffer, np.float64 if dbl else np.float32)
        cp = lambda n: copy.deepcopy(n).double() if dbl else copy.deepcopy(n)  # noqa: E731
        vae, pert, c1, c2 = (cp(m) for m in mods)
        algos[dbl] = BCQ(policy=BCQPolicy(actor_perturbation=pert, action_space=space, critic=c1, vae=vae,
                                          forward_sampled_times=S_ACT), actor_perturbation_optim=opt(), critic_optim=opt(),
                         vae_optim=opt(), critic2=None if no_c2 else c2, gamma=GAMMA, tau=TAU, lmbda=lmbda, num_sampled_action=K)
        caught[dbl] = record_grads(algos[dbl])
    init = {n: net_flat(algos[False], n).astype(np.float32) for n in ("pert", "critic", "critic2", "vae")}
    if no_c2:
        init.pop("critic2")
    Rst = BcqRestatement(init, D, AD, L, [D + AD, *HID, AD], [D + AD, *HID, 1], [D + AD, *VHID, 2 * L], [D + L, *VHID, AD], TAU, GAMMA,
                         lr=LR, max_action=max_action, phi=phi, lmbda=lmbda, num_sampled_action=K, forward_sampled_times=S_ACT)
    allidx = bufs[True].sample_indices(0)
    pk = f"c{ci}_"
    new = {pk + "init_" + n: v for n, v in init.items()}
    dist, seen = {}, dict(clipped=0.0, below=0.0)

    def both(fn, zs):
        out = {}
        for dbl, algo in algos.items():
            draws.queue, draws.dtype = list(zs), torch.float64 if dbl else torch.float32
            caught[dbl].clear()
            real_float = torch.Tensor.float
            if dbl:
                torch.Tensor.float = lambda t: t.double()
            try:
                out[dbl] = fn(dbl, algo)
            finally:
                torch.Tensor.float = real_float
            assert not draws.queue, "a draw was not consumed"
        return out[True], out[False]

    for k in range(2):
        indices = rs.choice(allidx, B, replace=True).astype(np.int64)
        zs = [rs.standard_normal(shape).astype(np.float32) for shape in ((B, L), (B * K, L), (B, L))]

        def call(dbl, algo):
            st = algo._update_with_batch(bufs[dbl][indices])
            return dict(stats=np.array([float(getattr(st, q)) for q in STAT_KEYS]), g=dict(caught[dbl]),
                        w={n: net_flat(algo, n) for n in NETS})

        r64, r32 = both(call, zs)
        b32 = bufs[False][indices]
        r = Rst.update(b32.obs, b32.act, b32.rew, b32.done, b32.obs_next, *zs)
        if Rst.kink <= DELTA:
            raise Kink
        seen = dict(clipped=max(seen["clipped"], Rst.clipped), below=max(seen["below"], Rst.below))
        mine = np.array([r[q] for q in STAT_KEYS])
        assert np.allclose(mine, r64["stats"], rtol=1e-10, atol=1e-13), (case, k, mine, r64["stats"])
        assert set(r["grads"]) == set(r64["g"])
        for n, gv in r["grads"].items():
            assert np.allclose(gv, r64["g"][n], rtol=1e-10, atol=1e-15), (case, k, n, np.abs(gv - r64["g"][n]).max())
        for n in NETS:
            assert np.allclose(Rst.weights(n), r64["w"][n], rtol=1e-10, atol=1e-13), (case, k, n)
        sk = f"{pk}s{k}_"
        new.update({sk + "indices": indices, sk + "stats": r64["stats"], sk + "stats32": r32["stats"], sk + "z_vae": zs[0],
                    sk + "z_next": zs[1], sk + "z_obs": zs[2], sk + "target": r["target"],
                    sk + "clipped": np.float64(Rst.clipped), sk + "below": np.float64(Rst.below)})
        for n, gv in r64["g"].items():
            new.update({f"{sk}grad_{n}": gv, f"{sk}grad_{n}_eref": emax(gv, r32["g"][n])})
            dist[f"grad_{n}"] = max(dist.get(f"grad_{n}", 0.0), emax(gv, r32["g"][n]) / max(np.abs(gv).max(), 1e-300))
        dist["stats"] = max(dist.get("stats", 0.0), float(np.max(np.abs(r64["stats"] - r32["stats"]) / np.abs(r64["stats"]))))
        if k == 1:
            for n in NETS:
                new.update({f"{sk}w_{n}": r64["w"][n], f"{sk}w_{n}_eref": emax(r64["w"][n], r32["w"][n])})
                dist[f"w_{n}"] = max(dist.get(f"w_{n}", 0.0), emax(r64["w"][n], r32["w"][n]) / np.abs(r64["w"][n]).max())
    if (phi > 0.1 and not seen["clipped"] > 0.0) or (ls_bias < 0 and not seen["below"] > 0.0):
        raise Kink   # the case is there for the clamp: a seed without a clamped entry is not used
    # acting after the second call: S_ACT candidates for each of N_ACT observations, one torch.randn per observation
    obs = rs.standard_normal((N_ACT, D)).astype(np.float32)
    za = [rs.standard_normal((S_ACT, L)).astype(np.float32) for _ in range(N_ACT)]
    a64, a32 = both(lambda dbl, algo: np.asarray(algo.policy(Batch(obs=obs.astype(np.float64 if dbl else np.float32), info=Batch())).act,
                                                 np.float64), za)
    ra = Rst.act(obs, np.concatenate(za, 0))
    if Rst.kink <= DELTA:
        raise Kink
    assert np.allclose(ra["act"], a64, rtol=1e-10, atol=1e-13), (case, ra["act"], a64)
    new.update({pk + "act_obs": obs, pk + "act_z": np.concatenate(za, 0), pk + "act": a64, pk + "act_index": ra["index"],
                pk + "act_eref": emax(a64, a32)})
    dist["act"] = emax(a64, a32) / np.abs(a64).max()
    return new, dist


def signatures(res):
    for cls in (BCQ, BCQPolicy):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])


def state_dict_keys(res):
    """The key names and shapes of a reference BCQ around the reference's own network classes (offline_bcq.py's)."""
    space = gym.spaces.Box(low=-1.0, high=1.0, shape=(AD,), dtype=np.float32)
    crit = lambda: ContinuousCritic(preprocess_net=Net(state_shape=D, action_shape=AD, hidden_sizes=HID, concat=True))  # noqa: E731
    vae = VAE(encoder=MLP(input_dim=D + AD, hidden_sizes=VHID), decoder=MLP(input_dim=D + L, output_dim=AD, hidden_sizes=VHID),
              hidden_dim=VHID[-1], latent_dim=L, max_action=1.0)
    pert = Perturbation(preprocess_net=Net(state_shape=D + AD, action_shape=AD, hidden_sizes=HID), max_action=1.0, phi=0.05)
    opt = lambda: AdamOptimizerFactory(lr=LR)  # noqa: E731
    algo = BCQ(policy=BCQPolicy(actor_perturbation=pert, action_space=space, critic=crit(), vae=vae), actor_perturbation_optim=opt(),
               critic_optim=opt(), vae_optim=opt(), critic2=crit())
    sd = {k: v for k, v in algo.state_dict().items() if isinstance(v, torch.Tensor)}   # (the module entries: no optimizers)
    res["sd_keys"] = np.array(list(sd.keys()))
    res["sd_shapes"] = np.array(["x".join(str(s) for s in v.shape) for v in sd.values()])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    draws = Noise()
    torch.randn = draws.randn
    torch.randn_like = lambda t, **kw: draws.randn(tuple(t.shape), dtype=t.dtype)
    res = dict(delta=np.float64(DELTA), gamma=np.float64(GAMMA), tau=np.float64(TAU), lr=np.float64(LR),
               dims=np.array([D, AD, *HID, B, N_ENV, S, T, K, L, S_ACT, N_ACT, *VHID], np.int64), stat_keys=np.array(STAT_KEYS),
               nets=np.array(NETS), cases=np.array(["|".join(str(v) for v in c) for c in CASES]))
    worst = {}
    for ci, case in enumerate(CASES):
        base = 501 + 7 * ci
        for seed in range(base, base + 200):   # the first seed that keeps DELTA away from every kink
            try:
                new, dist = run_case(ci, case, seed, draws)
            except Kink:
                continue
            res.update(new)
            res[f"c{ci}_seed"] = np.int64(seed)
            for q, v in dist.items():
                worst[q] = max(worst.get(q, 0.0), float(v))
            print("case", case, "seed", seed, "stats", res[f"c{ci}_s1_stats"].round(6).tolist(), "clipped",
                  [float(res[f"c{ci}_s{k}_clipped"]) for k in range(2)], "below", [float(res[f"c{ci}_s{k}_below"]) for k in range(2)])
            break
        else:
            raise AssertionError(f"no seed for {case}")
    print("float32 reference's relative distance from the float64 reference (max over cases):",
          {k: f"{v:.2e}" for k, v in sorted(worst.items())})
    res["ref32_distance_keys"] = np.array(sorted(worst))
    res["ref32_distance"] = np.array([worst[k] for k in sorted(worst)])
    signatures(res)
    state_dict_keys(res)
    path = os.path.join(HERE, "bcq.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= os.path.getsize(os.path.join(HERE, "cql.npz"))


if __name__ == "__main__":
    main()
