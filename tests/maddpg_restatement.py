"""Torch restatement of MADDPGPolicy.learn / update_target_networks (reference ctde.py:817-955) in any dtype and on any
device -- the yardstick of the MADDPG tests and of tools/bench_maddpg.py.  Pinned to the reference by
tests/test_host_maddpg.py (float64 against tests/golden/maddpg.npz and maddpg_n8.npz).

Parameters travel as ONE flat vector in the joint order of the HIP policy:
  [actor_0 (w0 b0 w1 b1 ...) ... actor_{N-1} | critic_0 ... critic_{N-1}],
each net with its own Adam, as upstream.  `learn` is written phase by phase over all agents (the order of the HIP
policy); `sequential=True` follows the reference's agent-by-agent loop literally.  Within a call the agents are independent
(iteration i reads the batch, the target actors, target critic i, critic i and actor i), so both give the same numbers."""
from __future__ import annotations

import copy

import numpy as np
import torch
import torch.nn.functional as F


def net_shapes(dims) -> list:
    out = []
    for k in range(len(dims) - 1):
        out += [(dims[k + 1], dims[k]), (dims[k + 1],)]
    return out


class MaddpgRestatement:
    def __init__(self, flat, N: int, actor_dims, critic_dims, dtype=torch.float64, device="cpu", lr: float = 1e-3,
                 gamma: float = 0.99, tau: float = 0.01) -> None:
        self.N, self.actor_dims, self.critic_dims = int(N), [int(d) for d in actor_dims], [int(d) for d in critic_dims]
        self.D, self.Ad = self.actor_dims[0], self.actor_dims[-1]
        assert self.critic_dims[0] == self.N * (self.D + self.Ad) and self.critic_dims[-1] == 1
        self.dtype, self.device, self.gamma, self.tau, self.lr = dtype, device, gamma, tau, lr
        # nets[k]: list of parameter tensors; k < N actors, then critics
        self.net_dims = [self.actor_dims] * self.N + [self.critic_dims] * self.N
        self.params = self._split(flat, True)
        self.target = self._split(flat, False)
        self.opts = [torch.optim.Adam(ps, lr=lr) for ps in self.params]

    def _split(self, flat, requires_grad: bool):
        flat = torch.as_tensor(np.asarray(flat, np.float64) if not isinstance(flat, torch.Tensor) else flat)
        flat = flat.to(self.device, self.dtype)
        nets, o = [], 0
        for dims in self.net_dims:
            ps = []
            for shp in net_shapes(dims):
                n = int(np.prod(shp))
                ps.append(flat[o:o + n].reshape(shp).clone().requires_grad_(requires_grad))
                o += n
            nets.append(ps)
        assert o == flat.numel()
        return nets

    @staticmethod
    def flat_of(ts) -> np.ndarray:
        return torch.cat([t.detach().reshape(-1).to("cpu", torch.float64) for t in ts]).numpy()

    @staticmethod
    def _mlp(ps, x, track=None):
        """ReLU between the layers, linear output.  track: list that receives, per hidden layer, min |pre-activation| of
        every row."""
        L = len(ps) // 2
        for k in range(L):
            x = F.linear(x, ps[2 * k], ps[2 * k + 1])
            if k + 1 < L:
                if track is not None:
                    track.append(x.detach().abs().min(dim=1).values)
                x = F.relu(x)
        return x

    def _t(self, x, dtype=None):
        return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(self.device, dtype or self.dtype)

    def _inputs(self, obs, act, rew, obs_next, term):
        N = self.N
        o = [self._t(obs[i]) for i in range(N)]
        a = [self._t(act[i]).reshape(o[i].shape[0], self.Ad) for i in range(N)]
        r = [self._t(rew[i]).reshape(-1) for i in range(N)]
        on = [self._t(obs_next[i]) for i in range(N)]
        t = [self._t(term[i], torch.bool).reshape(-1) for i in range(N)]
        return o, a, r, on, t

    def _step(self, k: int, loss) -> list:
        """Gradient of `loss` w.r.t. net k alone, then that net's Adam step; -> the gradients."""
        grads = torch.autograd.grad(loss, self.params[k])
        for p, g in zip(self.params[k], grads):
            p.grad = g
        self.opts[k].step()
        return grads

    def learn(self, obs, act, rew, obs_next, term, want_grads: bool = True, sequential: bool = False, track=None,
              track_stepped: bool = True) -> dict:
        """obs / obs_next [N][B][D], act [N][B][Ad], rew [N][B], term [N][B] (every agent its own flags) -> per-agent and
        aggregate losses, grads (flat f64: critic gradients before the critic step, actor gradients through the stepped
        critic), one Adam step per net.  want_grads=False (timing): no export, losses stay device scalars."""
        N = self.N
        o, a, r, on, t = self._inputs(obs, act, rew, obs_next, term)
        grads = [None] * (2 * N)
        la, lc = [None] * N, [None] * N
        if sequential:  # ctde.py:829-928, line by line
            for i in range(N):
                with torch.no_grad():
                    a_next = [self._mlp(self.target[j], on[j], track) for j in range(N)]
                all_obs, all_act = torch.cat(o, dim=-1), torch.cat(a, dim=-1)
                q = self._mlp(self.params[N + i], torch.cat([all_obs, all_act], dim=-1), track)
                with torch.no_grad():
                    qn = self._mlp(self.target[N + i], torch.cat([torch.cat(on, dim=-1), torch.cat(a_next, dim=-1)], dim=-1), track)
                    y = r[i] + self.gamma * qn.reshape(-1) * (~t[i]).to(self.dtype)
                lc[i] = F.mse_loss(q.reshape(-1), y)
                grads[N + i] = self._step(N + i, lc[i])
                a_i = self._mlp(self.params[i], o[i], track)
                for_actor = list(a)
                for_actor[i] = a_i
                la[i] = -self._mlp(self.params[N + i], torch.cat([all_obs, torch.cat(for_actor, dim=-1)], dim=-1), track).mean()
                grads[i] = self._step(i, la[i])
        else:
            with torch.no_grad():
                a_next = [self._mlp(self.target[j], on[j], track) for j in range(N)]                       # 1
                x = torch.cat(o + a, dim=-1)                                                               # 2
                x_next = torch.cat(on + a_next, dim=-1)
            q = [self._mlp(self.params[N + i], x, track).reshape(-1) for i in range(N)]                    # 3
            with torch.no_grad():
                qn = [self._mlp(self.target[N + i], x_next, track).reshape(-1) for i in range(N)]
                y = [r[i] + self.gamma * qn[i] * (~t[i]).to(self.dtype) for i in range(N)]                 # 4
            for i in range(N):                                                                             # 5
                lc[i] = F.mse_loss(q[i], y[i])
                grads[N + i] = self._step(N + i, lc[i])
            a_pi = [self._mlp(self.params[i], o[i], track) for i in range(N)]                              # 6
            for i in range(N):                                                                             # 7-9
                x_i = torch.cat(o + a[:i] + [a_pi[i]] + a[i + 1:], dim=-1)
                la[i] = -self._mlp(self.params[N + i], x_i, track if track_stepped else None).mean()
                grads[i] = self._step(i, la[i])
        if not want_grads:
            return {"actor_losses": [v.detach() for v in la], "critic_losses": [v.detach() for v in lc]}
        out = {}
        for i in range(N):
            out[f"agent_{i}_actor_loss"] = float(la[i].item())
            out[f"agent_{i}_critic_loss"] = float(lc[i].item())
        out["actor_loss"] = float(np.mean([v for k, v in out.items() if "actor_loss" in k]))
        out["critic_loss"] = float(np.mean([v for k, v in out.items() if "critic_loss" in k]))
        out["grads"] = self.flat_of([g for gs in grads for g in gs])
        return out

    def adam_cond(self) -> np.ndarray:
        """lr / (sqrt(v^) + eps) per parameter from the optimizers' own state: how far one Adam step moves a parameter per
        unit of gradient error (the `adamcond` allowance of the CTDE replays)."""
        out = []
        for ps, opt in zip(self.params, self.opts):
            for p in ps:
                st = opt.state[p]
                v_hat = st["exp_avg_sq"].detach().to("cpu", torch.float64) / (1.0 - 0.999 ** float(st["step"]))
                out.append((self.lr / (torch.sqrt(v_hat) + 1e-8)).reshape(-1))
        return torch.cat(out).numpy()

    @torch.no_grad()
    def update_targets(self) -> None:
        """ctde.py:936-955."""
        for ps, ts in zip(self.params, self.target):
            for p, t in zip(ps, ts):
                t.data.copy_(self.tau * p.data + (1 - self.tau) * t.data)

    def weights(self) -> np.ndarray:
        return self.flat_of([p for ps in self.params for p in ps])

    def targets(self) -> np.ndarray:
        return self.flat_of([p for ps in self.target for p in ps])

    def forward(self, obs) -> list:
        """Per agent actor_i(obs[i]) (ctde.py:803-813)."""
        with torch.no_grad():
            return [self._mlp(self.params[i], self._t(obs[i])).to("cpu", torch.float64).numpy() for i in range(self.N)]

    def kink_rows(self, obs, act, rew, obs_next, term, delta: float, stepped: bool = True) -> np.ndarray:
        """Rows [B] bool where any ReLU pre-activation of any pass that `learn` would make on these rows lies within `delta`
        of zero: actors on obs, target actors on obs_next, critics on X, target critics on X', and the STEPPED critics on
        the actor-side rows X_i.  Runs the call on a copy; this object is left as it was.  stepped=False leaves the last
        pass out: its weights depend on every row of the batch, so with it the rows no longer act independently."""
        track: list = []
        copy.deepcopy(self).learn(obs, act, rew, obs_next, term, want_grads=False, track=track, track_stepped=stepped)
        return (torch.stack(track).min(dim=0).values < delta).cpu().numpy()
