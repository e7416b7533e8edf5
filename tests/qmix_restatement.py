"""Torch restatement of QMIXPolicy.learn / update_target_networks (reference ctde.py:468-499, 618-725) in any dtype and on
any device -- the yardstick of the QMIX tests and of tools/bench_qmix.py.  Pinned to the reference by
tests/test_host_qmix.py (float64 against tests/golden/qmix.npz and qmix_c3.npz).

Parameters travel as ONE flat vector in the joint order of the HIP policy:
  [actor_0 (w0 b0 w1 b1 w2 b2) ... actor_{N-1} | hyper_w1 (0.w 0.b 2.w 2.b) | hyper_w2 | hyper_b1 (w b) | hyper_b2],
which is also the reference's optimizer order (the actors' parameters, then mixer.parameters())."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def layer_shapes(N: int, D: int, A: int, H: int, S: int, E: int, Hh: int):
    """[(name, shape)] of the joint vector."""
    out = []
    for i in range(N):
        dims = [D, H, H, A]
        for k in range(3):
            out += [(f"actor{i}.w{k}", (dims[k + 1], dims[k])), (f"actor{i}.b{k}", (dims[k + 1],))]
    mix = {"hyper_w1": [S, Hh, N * E], "hyper_w2": [S, Hh, E], "hyper_b1": [S, E], "hyper_b2": [S, E, 1]}
    for name, dims in mix.items():
        keys = [""] if len(dims) == 2 else ["0.", "2."]
        for k, pre in enumerate(keys):
            out += [(f"mixer.{name}.{pre}weight", (dims[k + 1], dims[k])), (f"mixer.{name}.{pre}bias", (dims[k + 1],))]
    return out


def mix(q, w1, b1, w2, b2, monotonic: bool):
    """QMIXMixer.forward after the hypernetworks (ctde.py:485-499): q [B, N], w1 [B, N, E], b1 [B, 1, E], w2 [B, E, 1],
    b2 [B, 1, 1] -> q_tot [B, 1]."""
    B = q.shape[0]
    if monotonic:
        w1, w2 = torch.abs(w1), torch.abs(w2)
    h = F.elu(torch.bmm(q.view(B, 1, -1), w1) + b1)
    return (torch.bmm(h, w2) + b2).view(B, 1)


def td_loss(q_tot, q_tot_next, rew_by_agent, term, gamma: float):
    """The TD target and loss of QMIXPolicy.learn (ctde.py:668-678): q_tot / q_tot_next [B, 1], rew_by_agent [N] of [B],
    term [B] bool -> the mse_loss scalar."""
    rewards = torch.stack(list(rew_by_agent), dim=-1).mean(dim=-1, keepdim=True)
    td_target = rewards + gamma * q_tot_next * (~term).to(q_tot.dtype).unsqueeze(-1)
    return F.mse_loss(q_tot, td_target)


class QmixRestatement:
    def __init__(self, flat, dims, monotonic: bool = True, dtype=torch.float64, device="cpu", lr: float = 1e-3,
                 gamma: float = 0.99) -> None:
        self.N, self.D, self.A, self.H, self.S, self.E, self.Hh = (int(x) for x in dims)
        self.shapes = layer_shapes(self.N, self.D, self.A, self.H, self.S, self.E, self.Hh)
        self.monotonic, self.dtype, self.device, self.gamma, self.lr = monotonic, dtype, device, gamma, lr
        self.params = self._split(flat, requires_grad=True)
        self.target = self._split(flat, requires_grad=False)
        self.opt = torch.optim.Adam(self.params, lr=lr)

    def _split(self, flat, requires_grad: bool):
        flat = torch.as_tensor(np.asarray(flat, np.float64) if not isinstance(flat, torch.Tensor) else flat)
        flat = flat.to(self.device, self.dtype)
        out, o = [], 0
        for _, shp in self.shapes:
            n = int(np.prod(shp))
            out.append(flat[o:o + n].reshape(shp).clone().requires_grad_(requires_grad))
            o += n
        return out

    @staticmethod
    def flat_of(ts) -> np.ndarray:
        return torch.cat([t.detach().reshape(-1).to("cpu", torch.float64) for t in ts]).numpy()

    def _actor(self, ps, i, x):
        w = ps[6 * i:6 * i + 6]
        x = F.relu(F.linear(x, w[0], w[1]))
        x = F.relu(F.linear(x, w[2], w[3]))
        return F.linear(x, w[4], w[5])

    def _hyper(self, ps, s):
        """The four hypernetworks on the states s [B, S] -> (w1raw [B, N, E], b1 [B, 1, E], w2raw [B, E, 1], b2 [B, 1, 1])."""
        m = ps[6 * self.N:]
        B = s.shape[0]
        w1 = F.linear(F.relu(F.linear(s, m[0], m[1])), m[2], m[3]).view(B, self.N, -1)
        w2 = F.linear(F.relu(F.linear(s, m[4], m[5])), m[6], m[7]).view(B, -1, 1)
        b1 = F.linear(s, m[8], m[9]).view(B, 1, -1)
        b2 = F.linear(F.relu(F.linear(s, m[10], m[11])), m[12], m[13]).view(B, 1, 1)
        return w1, b1, w2, b2

    def _mixer(self, ps, q, s):
        return mix(q, *self._hyper(ps, s), self.monotonic)

    def _t(self, x, dtype=None):
        return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).to(self.device, dtype or self.dtype)

    def learn(self, obs, act, rew, obs_next, term, gs, gsn, want_grads: bool = True) -> dict:
        """obs / obs_next [N][B][D], act / rew [N][B], term [B] (agent 0's), gs / gsn [B][S] -> loss, q_values,
        grads (flat f64), then one Adam step.  ctde.py:628-697, step by step.  want_grads=False (timing): no gradient
        export and no host synchronisation -- loss and q_values come back as device scalars."""
        qs, qn = [], []
        for i in range(self.N):
            q = self._actor(self.params, i, self._t(obs[i]))
            qs.append(q.gather(1, self._t(act[i], torch.int64).unsqueeze(-1)))
            with torch.no_grad():
                qn.append(self._actor(self.target, i, self._t(obs_next[i])).max(dim=-1, keepdim=True)[0])
        q_all, qn_all = torch.cat(qs, dim=-1), torch.cat(qn, dim=-1)
        q_total = self._mixer(self.params, q_all, self._t(gs))
        with torch.no_grad():
            q_total_next = self._mixer(self.target, qn_all, self._t(gsn))
        loss = td_loss(q_total, q_total_next, [self._t(rew[i]) for i in range(self.N)], self._t(term, torch.bool), self.gamma)
        self.opt.zero_grad()
        loss.backward()
        grads = self.flat_of([p.grad for p in self.params]) if want_grads else None
        self.opt.step()
        if not want_grads:
            return {"loss": loss.detach(), "q_values": q_total.detach().mean()}
        return {"loss": float(loss.item()), "q_values": float(q_total.mean().item()), "grads": grads}

    def adam_cond(self) -> np.ndarray:
        """lr / (sqrt(v^) + eps) per parameter from the optimizer's own state: how far one Adam step moves a parameter per
        unit of gradient error (the `adamcond` allowance of the CTDE replays, tests/golden/make_fixtures.py)."""
        out = []
        for p in self.params:
            st = self.opt.state[p]
            v_hat = st["exp_avg_sq"].detach().to("cpu", torch.float64) / (1.0 - 0.999 ** float(st["step"]))
            out.append((self.lr / (torch.sqrt(v_hat) + 1e-8)).reshape(-1))
        return torch.cat(out).numpy()

    @torch.no_grad()
    def update_targets(self, tau: float = 0.005) -> None:
        for p, t in zip(self.params, self.target):
            t.data.copy_(tau * p.data + (1 - tau) * t.data)

    def weights(self) -> np.ndarray:
        return self.flat_of(self.params)

    def targets(self) -> np.ndarray:
        return self.flat_of(self.target)

    @torch.no_grad()
    def kink_rows(self, obs, obs_next, gs, gsn, delta: float) -> np.ndarray:
        """Rows [B] bool where any ReLU pre-activation (Q-nets, hypernetworks), any w1raw / w2raw entry, or the greedy top-2
        gap of any Q row, online or target, lies within `delta` of its kink."""
        bad = None

        def near(x):
            return (x.abs() < delta).reshape(x.shape[0], -1).any(1)

        for ps, o, s in ((self.params, obs, gs), (self.target, obs_next, gsn)):
            for i in range(self.N):
                w = ps[6 * i:6 * i + 6]
                x = self._t(o[i])
                z1 = F.linear(x, w[0], w[1])
                z2 = F.linear(F.relu(z1), w[2], w[3])
                q = F.linear(F.relu(z2), w[4], w[5])
                top = torch.topk(q, 2, dim=1).values if q.shape[1] > 1 else None
                b = near(z1) | near(z2)
                if top is not None:
                    b = b | ((top[:, 0] - top[:, 1]).abs() < delta)
                bad = b if bad is None else bad | b
            m = ps[6 * self.N:]
            st = self._t(s)
            z = [F.linear(st, m[0], m[1]), F.linear(st, m[4], m[5]), F.linear(st, m[10], m[11])]
            w1 = F.linear(F.relu(z[0]), m[2], m[3])
            w2 = F.linear(F.relu(z[1]), m[6], m[7])
            for x in (*z, w1, w2):
                bad = bad | near(x)
        return bad.cpu().numpy()
