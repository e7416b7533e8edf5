"""Generate tests/golden/rainbow.npz by RUNNING THE REFERENCE's RainbowDQN, NoisyLinear and dueling Net (rainbow.py,
utils/net/discrete.py, utils/net/common.py, imported through oracle/ref_shim.py) in float64 and float32, with
e_ref = max |ref32 - ref64| per array.

The noise is data: `NoisyLinear.sample` is replaced by a reader of stored eps arrays (float32 values, drawn here as
sign(x) sqrt(|x|) of numpy normals), and the tests load the same arrays with `RainbowNet.set_noise` / `RainbowDQN.noise_feed`.
`MLP.forward` is replaced by one that casts the observation to the module's own dtype (the reference casts to float32, which a
float64 run cannot multiply); nothing else of the reference is touched.  Every net is `Net(softmax=True, num_atoms=N,
linear_layer=NoisyLinear, dueling_param=(Q, V))` with NoisyLinear in every layer of trunk and streams.

Sections (every array is data: inputs, noise, indices, initial weights, expected outputs; large float64 arrays as digests):
  nl_*   one NoisyLinear 33 -> 7 (a non-dueling net without hidden layer, A = 1, N = 7), forward and backward from a given
         d_out, in training and eval mode.
  du_*   the dueling net 6-32, Q 32-32-255, V 32-32-51 (A = 5, N = 51), B = 37: the raw output (the softmax taken off: the
         combine's result) and the gradient from a given d_out, in both modes.
  up_*   three updates on dqn.npz's buffer script with that net, n_step 3, target_update_freq 2, lr 1e-3: updates 0 and 2 are
         copy calls (the lagged net ends with the ONLINE net's noise), update 1 is not.
  pr_*   two updates in front of the reference's PrioritizedVectorReplayBuffer.
  ma_*   two Rainbow agents (6/4-16 trunk, streams without hidden layers, 8 atoms) under MultiAgentOffPolicyAlgorithm on
         dqn.npz's hand-filled AEC buffer.
  sd_*   reference state_dict keys and shapes;  sig_*  constructor signatures.
The generator asserts that no ReLU pre-activation it keeps lies within RELU_DELTA of 0 (it takes the first seed for which that
holds) and that the restatement (tests/rainbow_restatement.py) follows the reference's float64 run to 1e-10.
"""
from __future__ import annotations

import inspect
import os

import numpy as np

from make_dqn_fixtures import DELTA, GAMMA, FakeEnv, digest, flat  # noqa: E402  (installs the shim)
from make_distq_fixtures import emax, loss_of, up_buffers  # noqa: E402

import torch  # noqa: E402
from tianshou.algorithm.modelfree.c51 import C51Policy  # noqa: E402
from tianshou.algorithm.modelfree.rainbow import RainbowDQN  # noqa: E402
from tianshou.algorithm.multiagent.marl import MultiAgentOffPolicyAlgorithm  # noqa: E402
from tianshou.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou.utils.net import common as ref_common  # noqa: E402
from tianshou.utils.net.common import Net  # noqa: E402
from tianshou.utils.net.discrete import NoisyLinear  # noqa: E402
import gymnasium as gym  # noqa: E402  (the shim's fake)

from dqn_restatement import nstep_walk  # noqa: E402
from rainbow_restatement import (RainbowNetRestatement, RainbowRestatement, layer_size, noisy_f, split_flat)  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
RELU_DELTA = DELTA
V_MIN, V_MAX = -10.0, 10.0
NOISY_STD = 0.5
FEED: list = []     # (eps_p, eps_q) per NoisyLinear.sample call, in call order


def _fed_sample(self) -> None:
    p, q = FEED.pop(0)
    with torch.no_grad():
        self.eps_p.copy_(torch.as_tensor(p).to(self.eps_p.dtype))
        self.eps_q.copy_(torch.as_tensor(q).to(self.eps_q.dtype))


def _mlp_forward(self, obs):
    p = next(self.parameters())
    obs = torch.as_tensor(obs, device=p.device, dtype=p.dtype)
    if self.flatten_input:
        obs = obs.flatten(1)
    return self.model(obs)


def noisy(x: int, y: int) -> NoisyLinear:
    return NoisyLinear(x, y, NOISY_STD)


def draw_init(rs, R: RainbowNetRestatement) -> np.ndarray:
    """NoisyLinear.reset and a first draw, as float32 values on the flat layout."""
    out = np.zeros(R.P)
    for (i, o, z), v in zip(R.layers, split_flat(out, R.layers)):
        b = 1.0 / np.sqrt(i)
        v["mu_W"][...], v["mu_bias"][...] = rs.uniform(-b, b, (o, i)), rs.uniform(-b, b, o)
        v["sigma_W"][...], v["sigma_bias"][...] = NOISY_STD / np.sqrt(i), NOISY_STD / np.sqrt(i)
        v["eps_p"][...], v["eps_q"][...] = noisy_f(rs.standard_normal(i)), noisy_f(rs.standard_normal(o))
    return out.astype(np.float32)


def draw_noise(rs, R: RainbowNetRestatement) -> np.ndarray:
    return noisy_f(rs.standard_normal(R.n_slots)).astype(np.float32)


def feed(R: RainbowNetRestatement, eps) -> None:
    """Queue one draw of a whole net: per noisy layer (eps_p, eps_q), in module order."""
    p = 0
    for i, o, z in R.layers:
        if z:
            FEED.append((eps[p:p + i].copy(), eps[p + i:p + i + o].copy()))
            p += i + o


def make_net(R: RainbowNetRestatement, init, double: bool, hidden, q_hidden, v_hidden, obs_dim):
    kw = dict(state_shape=(obs_dim,), action_shape=R.A, hidden_sizes=list(hidden), softmax=True, num_atoms=R.N, linear_layer=noisy)
    if R.dueling:
        kw["dueling_param"] = ({"hidden_sizes": list(q_hidden), "linear_layer": noisy}, {"hidden_sizes": list(v_hidden), "linear_layer": noisy})
    net = Net(**kw)
    ps = list(net.parameters())
    assert sum(q.numel() for q in ps) == R.P == sum(layer_size(*l) for l in R.layers)
    with torch.no_grad():
        o = 0
        for q in ps:
            q.copy_(torch.as_tensor(init[o:o + q.numel()]).reshape(q.shape))
            o += q.numel()
    return net.double() if double else net


def make_algo(net, A, N, double, **kw):
    pol = C51Policy(model=net, action_space=gym.spaces.Discrete(A), num_atoms=N, v_min=V_MIN, v_max=V_MAX)
    algo = RainbowDQN(policy=pol, optim=AdamOptimizerFactory(lr=1e-3), gamma=GAMMA, **kw)
    if double:
        pol.support.data = pol.support.data.double()
    # what `Algorithm.update` does around `_update_with_batch` (torch_train_mode): the lagged net, which Rainbow holds without its
    # eval-mode wrapper, follows the algorithm into training mode (the wrapper's constructor had put it into eval mode)
    algo.train()
    return algo


def raw_of(net, obs):
    """The net's output with the softmax taken off: the dueling combine's result, [R, A * N]."""
    net.softmax = False
    out = net(obs)[0]
    net.softmax = True
    return out.reshape(out.shape[0], -1)


def grads_of(net):
    return np.concatenate([(torch.zeros_like(q) if q.grad is None else q.grad).detach().double().reshape(-1).numpy()
                           for q in net.parameters()])


# ---- nl / du -----------------------------------------------------------------------------------------------------------
def net_section(res, tag, rs, obs_dim, hidden, A, N, q_hidden, v_hidden, dueling, B):
    R = RainbowNetRestatement(obs_dim, hidden, A, N, q_hidden, v_hidden, dueling, True)
    while True:
        init = draw_init(rs, R)
        x = rs.standard_normal((B, obs_dim)).astype(np.float32)
        if all(RainbowNetRestatement.min_relu_gap(R.forward(init, x, t)[1]) > RELU_DELTA for t in (True, False)):
            break
    d = (rs.standard_normal((B, A * N)) / B).astype(np.float32)
    res.update({f"{tag}_init": init, f"{tag}_x": x, f"{tag}_d": d,
                f"{tag}_dims": np.array([obs_dim, A, N, B, int(dueling), len(hidden), len(q_hidden), len(v_hidden), *hidden, *q_hidden,
                                         *v_hidden], np.int64)})
    for mode, training in (("train", True), ("eval", False)):
        out = {}
        for dbl in (True, False):
            net = make_net(R, init, dbl, hidden, q_hidden, v_hidden, obs_dim)
            net.train(training)
            y = raw_of(net, x)
            y.backward(torch.as_tensor(d).to(y.dtype))
            out[dbl] = (y.detach().double().numpy(), grads_of(net))
        y, cache = R.forward(init, x, training)
        g = R.backward(cache, d)
        assert np.allclose(y, out[True][0], rtol=1e-10, atol=1e-13) and np.allclose(g, out[True][1], rtol=1e-10, atol=1e-14), (tag, mode)
        if not training:   # eval mode: sigma takes no gradient
            assert not any(v[k].any() for v in split_flat(out[True][1], R.layers) for k in ("sigma_W", "sigma_bias"))
        assert not any(v[k].any() for v in split_flat(out[True][1], R.layers) for k in ("eps_p", "eps_q"))
        digest(res, f"{tag}_{mode}_out", out[True][0].reshape(-1))
        digest(res, f"{tag}_{mode}_grad", out[True][1])
        res.update({f"{tag}_{mode}_out_eref": emax(out[True][0], out[False][0]), f"{tag}_{mode}_grad_eref": emax(out[True][1], out[False][1])})
    print(tag, "P", R.P, "slots", R.n_slots)


# ---- up / pr -----------------------------------------------------------------------------------------------------------
UP = dict(obs_dim=6, hidden=(32,), A=5, N=51, q_hidden=(32,), v_hidden=(32,))


def up_restatement():
    return RainbowNetRestatement(UP["obs_dim"], UP["hidden"], UP["A"], UP["N"], UP["q_hidden"], UP["v_hidden"], True, True)


def up_algos(R, init, n_step, freq):
    return {dbl: make_algo(make_net(R, init, dbl, UP["hidden"], UP["q_hidden"], UP["v_hidden"], UP["obs_dim"]), R.A, R.N, dbl,
                           n_step_return_horizon=n_step, target_update_freq=freq) for dbl in (True, False)}


def update_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    B, n_env, S, n_step, freq, steps = d[4:10]
    R = up_restatement()

    class Kink(Exception):
        pass

    def attempt(seed):
        rs = np.random.RandomState(seed)
        init = draw_init(rs, R)
        eps = np.stack([[draw_noise(rs, R), draw_noise(rs, R)] for _ in range(steps)])      # [step][online, lagged][slot]
        res.update(up_init=init, up_eps=eps, up_dims=np.array([UP["obs_dim"], UP["A"], UP["N"], *UP["hidden"], *UP["q_hidden"],
                                                               *UP["v_hidden"]], np.int64))
        algos = up_algos(R, init, n_step, freq)
        bufs, RB = up_buffers(gd, VectorReplayBuffer)
        RS = RainbowRestatement(init, R, target_update_freq=freq, v_min=V_MIN, v_max=V_MAX)
        allidx = bufs[True].sample_indices(0)
        for k in range(steps):
            indices = rs.choice(allidx, B, replace=True).astype(np.int64)
            out = {}
            for dbl, algo in algos.items():
                buf = bufs[dbl]
                batch = algo._preprocess_batch(buf[indices], buf, indices)
                feed(R, eps[k, 0])
                feed(R, eps[k, 1])
                stats = algo._update_with_batch(batch)
                assert not FEED
                out[dbl] = (loss_of(stats), flat(algo.policy.model), flat(algo.model_old), batch.returns.double().numpy().reshape(-1),
                            grads_of(algo.policy.model))
            idx_n, mc, gpow, vmask = nstep_walk(RB, indices, n_step, GAMMA, 0)
            o, on = bufs[False][indices].obs, bufs[False][indices].obs_next      # c51.py:124: the one-step successors
            r = RS.update(o, bufs[False][indices].act, on, None, mc, gpow, vmask, eps_online=eps[k, 0], eps_target=eps[k, 1])
            if r["relu_gap"] <= RELU_DELTA:
                raise Kink
            assert abs(r["loss"] - out[True][0]) <= 1e-10 * abs(out[True][0]), (k, r["loss"], out[True][0])
            assert np.allclose(RS.weights(), out[True][1], rtol=1e-9, atol=1e-12) and np.allclose(RS.targets(), out[True][2], rtol=1e-9, atol=1e-12)
            assert np.allclose(r["grads"], out[True][4], rtol=1e-9, atol=1e-14)
            assert np.allclose(r["returns"].reshape(-1), out[True][3], rtol=1e-12, atol=1e-13)
            assert np.abs(np.abs(out[True][3]) - V_MAX).min() > DELTA
            # quirk: on a copy call the lagged net holds the online net's noise, else its own draw
            noise = lambda fl: np.concatenate([v[kk].reshape(-1) for v in split_flat(fl, R.layers) for kk in ("eps_p", "eps_q")])  # noqa: E731
            assert np.array_equal(noise(out[True][1]), eps[k, 0].astype(np.float64))
            assert np.array_equal(noise(out[True][2]), eps[k, 0 if k % freq == 0 else 1].astype(np.float64))
            pk = f"up_s{k}_"
            digest(res, pk + "weights", out[True][1])
            digest(res, pk + "targets", out[True][2])
            digest(res, pk + "returns", out[True][3])
            digest(res, pk + "grad", out[True][4])
            res.update({pk + "indices": indices, pk + "loss": np.array([out[True][0], out[False][0]]),
                        pk + "grad_eref": emax(out[True][4], out[False][4]), pk + "weights_eref": emax(out[True][1], out[False][1]),
                        pk + "returns_eref": emax(out[True][3], out[False][3])})
        print("update losses", [float(res[f"up_s{k}_loss"][0]) for k in range(steps)])

    for seed in range(41, 141):   # the first seed whose three updates keep RELU_DELTA away from every kink
        try:
            FEED.clear()
            attempt(seed)
            res["up_seed"] = np.int64(seed)
            break
        except Kink:
            continue
    else:
        raise AssertionError("no seed without a kink")


def prio_section(res, gd):
    d = [int(x) for x in gd["up_dims"]]
    B, n_env, S, n_step, freq = d[4:9]
    alpha, beta = 0.6, 0.4
    R = up_restatement()
    rs = np.random.RandomState(57)
    eps = np.stack([[draw_noise(rs, R), draw_noise(rs, R)] for _ in range(2)])
    res.update(pr_alpha=np.float64(alpha), pr_beta=np.float64(beta), pr_eps=eps)
    algos = up_algos(R, res["up_init"], n_step, freq)
    bufs, _ = up_buffers(gd, PrioritizedVectorReplayBuffer, alpha=alpha, beta=beta)
    bound = bufs[True].weight._bound
    np.random.seed(43)
    for k in range(2):
        indices = bufs[True].sample_indices(B).astype(np.int64)
        out = {}
        for dbl, algo in algos.items():
            buf = bufs[dbl]
            batch = buf[indices]
            w_in = np.asarray(batch.weight, np.float64).copy()
            batch = algo._preprocess_batch(batch, buf, indices)
            feed(R, eps[k, 0])
            feed(R, eps[k, 1])
            stats = algo._update_with_batch(batch)
            algo._postprocess_batch(batch, buf, indices)
            out[dbl] = (loss_of(stats), w_in, buf.weight._value[bound:bound + n_env * S].copy(),
                        np.array([float(buf._max_prio), float(buf._min_prio)]))
        pk = f"pr_s{k}_"
        res.update({pk + "indices": indices, pk + "loss": np.array([out[True][0], out[False][0]]), pk + "weight": out[True][1],
                    pk + "weight_eref": emax(out[True][1], out[False][1]), pk + "leaves": out[True][2],
                    pk + "leaves_eref": emax(out[True][2], out[False][2]), pk + "prio": out[True][3],
                    pk + "prio_eref": emax(out[True][3], out[False][3])})
    print("prioritized losses", [float(res[f"pr_s{k}_loss"][0]) for k in range(2)])


# ---- ma / sd / sig -----------------------------------------------------------------------------------------------------
def marl_section(res, gd):
    rs = np.random.RandomState(23)
    N_AG, n_env, S, D, A, n_step, T = (int(x) for x in gd["ma_dims"][:7])
    NA, H = 8, 16
    env = FakeEnv(N_AG)
    R = RainbowNetRestatement(D, (H,), A, NA, (), (), True, True)
    inits = np.stack([draw_init(rs, R) for _ in range(N_AG)])
    eps = np.stack([[draw_noise(rs, R), draw_noise(rs, R)] for _ in range(N_AG)])     # [agent][online, lagged][slot]
    res.update(ma_dims=np.array([D, H, A, NA], np.int64), ma_init=inits, ma_eps=eps)
    out = {}
    for dbl in (True, False):
        dt = np.float64 if dbl else np.float32
        buf = VectorReplayBuffer(n_env * S, n_env)
        for t in range(T):
            ids = np.array([env.agents[a] for a in gd["ma_turn"][t]], dtype=object)
            nxt = np.array([env.agents[(a + 1) % N_AG] for a in gd["ma_turn"][t]], dtype=object)
            buf.add(Batch(obs=Batch(agent_id=ids, obs=gd["ma_obs"][t].astype(dt), mask=gd["ma_mask"][t]), act=gd["ma_act"][t],
                          rew=gd["ma_rew"][t].astype(np.float64), terminated=gd["ma_term"][t], truncated=gd["ma_trunc"][t],
                          obs_next=Batch(agent_id=nxt, obs=gd["ma_obs_next"][t].astype(dt), mask=gd["ma_mask"][t])),
                    buffer_ids=np.arange(n_env))
        algos = [make_algo(make_net(R, inits[i], dbl, (H,), (), (), D), A, NA, dbl, n_step_return_horizon=n_step, target_update_freq=3)
                 for i in range(N_AG)]
        ma = MultiAgentOffPolicyAlgorithm(algorithms=algos, env=env)
        batch, indices = buf.sample(0)
        for i in range(N_AG):
            feed(R, eps[i, 0])
            feed(R, eps[i, 1])
        stats = ma._update_with_batch(ma._preprocess_batch(batch, buf, indices))
        assert not FEED
        out[dbl] = [loss_of(stats._agent_id_to_stats[a]) for a in env.agents]
    res["ma_loss"] = np.array([out[True], out[False]])
    print("marl losses", out[True])


def statedict_and_signatures(res):
    R = up_restatement()
    net = make_net(R, res["up_init"], False, UP["hidden"], UP["q_hidden"], UP["v_hidden"], UP["obs_dim"])
    algo = make_algo(net, R.A, R.N, False, target_update_freq=2)
    sd = {k: v for k, v in algo.state_dict().items() if isinstance(v, torch.Tensor) and v.dim() > 0}
    res["sd_keys"] = np.array(list(sd.keys()))
    res["sd_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    for cls in (C51Policy, RainbowDQN):
        ps = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        res[f"sig_{cls.__name__}"] = np.array([f"{q.name}={'<required>' if q.default is inspect.Parameter.empty else repr(q.default)}"
                                               for q in ps])


def main():
    import logging

    logging.disable(logging.WARNING)
    torch.set_num_threads(4)
    ref_common.MLP.forward = _mlp_forward
    gd = dict(np.load(os.path.join(HERE, "dqn.npz")))
    res = {"delta": np.float64(RELU_DELTA), "gamma": np.float64(GAMMA), "v_min": np.float64(V_MIN), "v_max": np.float64(V_MAX),
           "noisy_std": np.float64(NOISY_STD)}
    rs = np.random.RandomState(29)
    # nets are built with the reference's own sampler (its constructor draws); from here on the noise is read from FEED
    real_sample = NoisyLinear.sample
    try:
        NoisyLinear.sample = lambda self: _fed_sample(self) if FEED else real_sample(self)  # noqa: E731
        net_section(res, "nl", rs, 33, (), 1, 7, (), (), False, 37)
        net_section(res, "du", rs, 6, (32,), 5, 51, (32,), (32,), True, 37)
        update_section(res, gd)
        prio_section(res, gd)
        marl_section(res, gd)
        statedict_and_signatures(res)
    finally:
        NoisyLinear.sample = real_sample
    path = os.path.join(HERE, "rainbow.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print(f"wrote {path}: {len(res)} arrays, {size} bytes")
    assert size <= 1 << 20


if __name__ == "__main__":
    main()
