"""Float64 restatement of the DQN path (reference dqn.py:145-151, 277-285, 365-404; algorithm_base.py:773-806, 1155-1216;
manager.py:85-91, 334-358) -- the yardstick of the DQN tests.  Written from the reference's description of what it
computes, step by step; pinned to the reference by tests/test_host_dqn.py against tests/golden/dqn.npz.

  `RestatedBuffer`   the index state of a VectorReplayBuffer(total, buffer_num) under a script of adds, in numpy
  `nstep_walk`       idx_n, mc, gamma^m, value mask of compute_nstep_return
  `td_head`          DQN._target_q after its forwards, the n-step target, the loss and d loss / d q (torch, any dtype)
  `DqnRestatement`   a fully-connected Q-net on one flat vector, Adam, the lagged copy with the `_iter` rule
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


class RestatedBuffer:
    """B sub-buffers of S slots; flat index = env * S + slot."""

    def __init__(self, buffer_num: int, sub_size: int, rew_dim: int) -> None:
        self.B, self.S = buffer_num, sub_size
        n = buffer_num * sub_size
        self.done = np.zeros(n, bool)
        self.term = np.zeros(n, bool)
        self.rew = np.zeros((n, rew_dim))
        self.ins = np.zeros(buffer_num, np.int64)
        self.size = np.zeros(buffer_num, np.int64)
        self.last_index = np.arange(buffer_num, dtype=np.int64) * sub_size

    def add(self, env: int, rew, term: bool, trunc: bool) -> int:
        cur = int(self.ins[env]) + env * self.S
        self.rew[cur], self.term[cur], self.done[cur] = rew, term, term or trunc
        self.ins[env] = (self.ins[env] + 1) % self.S
        self.size[env] = min(self.size[env] + 1, self.S)
        self.last_index[env] = cur
        return cur

    def sample_indices_all(self) -> np.ndarray:
        out = []
        for e in range(self.B):
            sz, ins = int(self.size[e]), int(self.ins[e])
            out.append(np.concatenate([np.arange(ins, sz), np.arange(ins)]) + e * self.S)
        return np.concatenate(out).astype(np.int64)

    def unfinished_index(self) -> np.ndarray:
        out = []
        for e in range(self.B):
            if self.size[e] > 0:
                last = int((self.ins[e] - 1) % self.size[e]) + e * self.S
                if not self.done[last]:
                    out.append(last)
        return np.array(out, np.int64)

    def next(self, index: np.ndarray) -> np.ndarray:
        index = np.asarray(index, np.int64) % (self.B * self.S)
        env = index // self.S
        end = self.done[index] | (index == self.last_index[env])
        lens = np.maximum(self.size[env], 1)
        return (index + (1 - end) - env * self.S) % lens + env * self.S


def nstep_walk(buf: RestatedBuffer, indices, n_step: int, gamma: float, col: int):
    """-> (idx_n i64, mc f64, gpow f64, vmask bool): the backward loop of `_nstep_return`, as written there."""
    stack = [np.asarray(indices, np.int64) % (buf.B * buf.S)]
    for _ in range(n_step - 1):
        stack.append(buf.next(stack[-1]))
    end = buf.done.copy()
    end[buf.unfinished_index()] = True
    I = len(stack[0])
    gbuf = np.ones(n_step + 1)
    for i in range(1, n_step + 1):
        gbuf[i] = gbuf[i - 1] * gamma
    mc = np.zeros(I)
    m = np.full(I, n_step)
    for n in range(n_step - 1, -1, -1):
        now = stack[n]
        m[end[now]] = n + 1
        mc[end[now]] = 0.0
        mc = buf.rew[now, col] + gamma * mc
    return stack[-1], mc, gbuf[m], ~buf.term[stack[-1]]


def td_head(q, qn_on, qn_tg, mask_next, act, mc, gpow, vmask, weight, is_double: bool, huber_delta, dtype=torch.float64):
    """-> dict(returns, td_error, loss, dq) as numpy f64.  qn_tg None: no target network."""
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)  # noqa: E731
    q = t(q).clone().requires_grad_(True)
    on, tg = t(qn_on), (t(qn_on) if qn_tg is None else t(qn_tg))
    B = q.shape[0]
    rows = torch.arange(B)
    if is_double:
        sel = on
        if mask_next is not None:
            sel = on + (1 - t(np.asarray(mask_next, bool))) * (on.min() - on.max() - 1.0)
        target = tg[rows, sel.argmax(dim=1)]
    else:
        target = tg.max(dim=1)[0]
    returns = target * t(np.asarray(vmask, bool)) * t(gpow) + t(mc)
    qs = q[rows, torch.as_tensor(np.asarray(act, np.int64))]
    td = returns - qs
    if huber_delta is not None:
        loss = F.huber_loss(qs.reshape(-1, 1), returns.reshape(-1, 1), delta=huber_delta, reduction="mean")
    else:
        loss = (td.pow(2) * (1.0 if weight is None else t(weight))).mean()
    loss.backward()
    n = lambda x: x.detach().to(torch.float64).numpy()  # noqa: E731
    return dict(returns=n(returns), td_error=n(td), loss=float(loss.item()), dq=n(q.grad))


class DqnRestatement:
    """Q-net dims[0] -> ... -> dims[-1] (ReLU) on one flat vector in `parameters()` order (w0 b0 w1 b1 ...)."""

    def __init__(self, flat, dims, lr: float = 1e-3, target_update_freq: int = 0, is_double: bool = True,
                 huber_delta=None, dtype=torch.float64) -> None:
        self.dims, self.dtype, self.lr = [int(d) for d in dims], dtype, lr
        self.freq, self.is_double, self.huber_delta = int(target_update_freq), is_double, huber_delta
        self.params = self._split(flat, True)
        self.target = self._split(flat, False) if self.freq > 0 else None
        self.opt = torch.optim.Adam(self.params, lr=lr)
        self._iter = 0

    def _split(self, flat, grad: bool):
        flat = torch.as_tensor(np.asarray(flat, np.float64)).to(self.dtype)
        out, o = [], 0
        for i in range(len(self.dims) - 1):
            for shp in ((self.dims[i + 1], self.dims[i]), (self.dims[i + 1],)):
                n = int(np.prod(shp))
                out.append(flat[o:o + n].reshape(shp).clone().requires_grad_(grad))
                o += n
        return out

    def net(self, ps, x):
        x = torch.as_tensor(np.asarray(x)).to(self.dtype)
        L = len(self.dims) - 1
        for i in range(L):
            x = F.linear(x, ps[2 * i], ps[2 * i + 1])
            if i < L - 1:
                x = F.relu(x)
        return x

    @staticmethod
    def flat_of(ts) -> np.ndarray:
        return torch.cat([t.detach().reshape(-1).to(torch.float64) for t in ts]).numpy()

    def weights(self) -> np.ndarray:
        return self.flat_of(self.params)

    def targets(self) -> np.ndarray:
        return self.flat_of(self.target)

    def update(self, obs, act, obs_next, mask_next, mc, gpow, vmask, weight=None) -> dict:
        """One `_preprocess_batch` (after the walk) + `_update_with_batch`: the target values with the weights as they are,
        then the `_iter` rule's copy, then the loss, its gradient and one Adam step."""
        with torch.no_grad():
            on = self.net(self.params, obs_next)
            tg = self.net(self.target, obs_next) if self.freq > 0 else None
        if self.freq > 0 and self._iter % self.freq == 0:
            for p, t in zip(self.params, self.target):
                t.data.copy_(p.data)
        self._iter += 1
        q = self.net(self.params, obs)
        h = td_head(q.detach().numpy(), on.numpy(), None if tg is None else tg.numpy(), mask_next, act, mc, gpow, vmask, weight,
                    self.is_double, self.huber_delta, self.dtype)
        self.opt.zero_grad()
        q.backward(torch.as_tensor(h["dq"]).to(self.dtype))
        h["grads"] = self.flat_of([p.grad for p in self.params])
        self.opt.step()
        return h

    def adam_cond(self) -> np.ndarray:
        """lr / (sqrt(v^) + eps) per parameter: how far one Adam step moves a parameter per unit of gradient error."""
        out = []
        for p in self.params:
            st = self.opt.state[p]
            v_hat = st["exp_avg_sq"].detach().to(torch.float64) / (1.0 - 0.999 ** float(st["step"]))
            out.append((self.lr / (torch.sqrt(v_hat) + 1e-8)).reshape(-1))
        return torch.cat(out).numpy()

    def min_kink_gap(self, xs) -> float:
        """The smallest |ReLU pre-activation| and greedy top-2 gap over the rows `xs`, online and target nets."""
        gap = np.inf
        with torch.no_grad():
            for ps in [self.params] + ([self.target] if self.target is not None else []):
                x = torch.as_tensor(np.asarray(xs)).to(self.dtype)
                L = len(self.dims) - 1
                for i in range(L):
                    x = F.linear(x, ps[2 * i], ps[2 * i + 1])
                    if i < L - 1:
                        gap = min(gap, float(x.abs().min()))
                        x = F.relu(x)
                top = torch.topk(x, 2, dim=1).values
                gap = min(gap, float((top[:, 0] - top[:, 1]).abs().min()))
        return gap
