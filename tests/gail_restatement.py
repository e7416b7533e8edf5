"""Float64 restatement of the GAIL path (reference algorithm/imitation/gail.py:193-248) -- the yardstick of the GAIL tests.
Written from the reference's description of what it computes; pinned to the reference by tests/test_gail_restatement.py against
tests/golden/gail.npz.  Nothing here calls the library.

  `check`            the bounds of tsm_gail_check
  `draw`             the expert pair ids of one discriminator step, over tests/philox_restatement.py
  `rows`             [obs[p] | one_hot(act[p])]
  `reward`           softplus(logit) written over the rewards of the given pairs
  `head`             the discriminator loss, its two accuracies and d loss / d logits, with the per-workgroup partials
  `finalize`         {loss, acc_pi, acc_exp} from the partials
  `GailRestatement`  a ReLU MLP discriminator on one flat vector (`parameters()` order), torch autograd, Adam: one whole `update`
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from philox_restatement import M64, philox4
from sampling_restatement import counters, own

GAIL_KEY = 0x4741494C45585054        # csrc/gail.hip kGailKey
ROWS_PER_BLOCK = 256                 # TSM_GAIL_ROWS_PER_BLOCK


def check(obs_dim: int, n_act: int) -> None:
    if obs_dim < 1:
        raise ValueError(f"obs_dim = {obs_dim} below 1")
    if not 1 <= n_act <= 64:
        raise ValueError(f"n_act = {n_act} outside [1, 64]")


def draw(valid, n_valid: int, n_agent: int, R: int, seed: int, counter: int = 0, counter_dev=None):
    """Element i: word 0 at counter + *counter_dev + i under the key seed ^ GAIL_KEY; j = (w0 n_valid n_agent) >> 32;
    id = (valid[j // n_agent] or j // n_agent) * n_agent + j % n_agent.  -> (ids i64 [R], j, the words the call owns)."""
    n = int(n_valid) * int(n_agent)
    assert 1 <= n < 2 ** 32
    key = (int(seed) ^ GAIL_KEY) & M64
    ctr = counters(counter, counter_dev, np.arange(R))
    w0 = philox4(key, ctr, 0)[:, 0].astype(np.uint64)
    j = ((w0 * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    row, a = j // n_agent, j % n_agent
    if valid is not None:
        row = np.asarray(valid, np.int64)[row]
    return row * n_agent + a, j, own(key, ctr, 0, (0,))


def softplus(x):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def rows(obs, act, n_act: int, ids=None, R=None):
    """obs [P, D] (any leading shape), act [P]: -> [R, D + n_act] in obs's dtype; an action outside [0, n_act) gives zeros."""
    obs, act = np.asarray(obs), np.asarray(act).reshape(-1).astype(np.int64)
    obs = obs.reshape(act.size, -1)
    p = np.arange(act.size if R is None else R) if ids is None else np.asarray(ids, np.int64)
    out = np.zeros((p.size, obs.shape[1] + n_act), obs.dtype)
    out[:, :obs.shape[1]] = obs[p]
    a = act[p]
    ok = (a >= 0) & (a < n_act)
    out[np.nonzero(ok)[0], obs.shape[1] + a[ok]] = 1
    return out


def reward(logits, rew, ids=None):
    """A float64 copy of rew with softplus(logits[r]) written at ids[r] (or r)."""
    out = np.asarray(rew, np.float64).copy()
    flat = out.reshape(-1)
    lg = np.asarray(logits, np.float64).reshape(-1)
    flat[np.arange(lg.size) if ids is None else np.asarray(ids, np.int64)] = softplus(lg)
    return out


def head(logits, Rp: int) -> dict:
    """logits [Rp + Re], the policy rows first: loss = mean softplus(l_pi) + mean softplus(-l_exp), acc_pi = mean(l_pi < 0),
    acc_exp = mean(l_exp > 0), d_logits, and partial [blocks, 4] = per ROWS_PER_BLOCK rows {sum softplus(l_pi),
    sum softplus(-l_exp), count(l_pi < 0), count(l_exp > 0)}."""
    lg = np.asarray(logits, np.float64).reshape(-1)
    n, Rp = lg.size, int(Rp)
    Re = n - Rp
    is_pi = np.arange(n) < Rp
    v = np.stack([np.where(is_pi, softplus(lg), 0.0), np.where(is_pi, 0.0, softplus(-lg)),
                  np.where(is_pi & (lg < 0), 1.0, 0.0), np.where(~is_pi & (lg > 0), 1.0, 0.0)], 1)
    nb = -(-n // ROWS_PER_BLOCK)
    partial = np.stack([v[b * ROWS_PER_BLOCK:(b + 1) * ROWS_PER_BLOCK].sum(0) for b in range(nb)])
    d = np.where(is_pi, sigmoid(lg) / Rp, -sigmoid(-lg) / Re)   # sigmoid(l) - 1 = -sigmoid(-l), without the cancellation
    return dict(d_logits=d, partial=partial, **finalize(partial, Rp, Re))


def finalize(partial, Rp: int, Re: int) -> dict:
    s = np.asarray(partial, np.float64).reshape(-1, 4).sum(0)
    return dict(loss=s[0] / Rp + s[1] / Re, acc_pi=s[2] / Rp, acc_exp=s[3] / Re)


def chunks(R: int, disc_update_num: int) -> list:
    """`Batch.split(bsz, merge_last=True)` with bsz = R // disc_update_num: [(lo, hi)] of R // bsz chunks, the remainder in the last."""
    bsz = R // disc_update_num
    steps = R // bsz
    return [(k * bsz, R if k == steps - 1 else (k + 1) * bsz) for k in range(steps)]


class GailRestatement:
    """A ReLU MLP dims[0] -> .. -> 1 on one flat vector (w0 b0 w1 b1 ..), Adam.  `kink`: the smallest |logit| or |ReLU
    pre-activation| met so far."""

    def __init__(self, flat, dims, n_act: int, lr: float = 1e-3, dtype=torch.float64) -> None:
        self.dims, self.A, self.dtype = [int(d) for d in dims], int(n_act), dtype
        flat = torch.as_tensor(np.asarray(flat, np.float64)).to(dtype)
        self.params, o = [], 0
        for i in range(len(self.dims) - 1):
            for shp in ((self.dims[i + 1], self.dims[i]), (self.dims[i + 1],)):
                n = int(np.prod(shp))
                self.params.append(flat[o:o + n].reshape(shp).clone().requires_grad_(True))
                o += n
        assert o == flat.numel()
        self.opt = torch.optim.Adam(self.params, lr=lr)
        self.kink = np.inf

    def weights(self) -> np.ndarray:
        return torch.cat([p.detach().reshape(-1).to(torch.float64) for p in self.params]).numpy()

    def logits(self, obs, act):
        x = torch.as_tensor(rows(np.asarray(obs, np.float64), act, self.A)).to(self.dtype)
        L = len(self.dims) - 1
        for i in range(L):
            x = F.linear(x, self.params[2 * i], self.params[2 * i + 1])
            self.kink = min(self.kink, float(x.detach().abs().min()))
            if i < L - 1:
                x = F.relu(x)
        return x.reshape(-1)

    def update(self, obs, act, perm, exp_obs, exp_act, disc_update_num: int) -> dict:
        """One update's GAIL part.  obs [R, D], act [R]: the rollout's pairs in batch order; perm: the order they are cut in;
        exp_obs [steps, bsz, D], exp_act [steps, bsz]: the expert pairs of every step.
        -> rew [R] (the discriminator of BEFORE the steps), per step loss / acc_pi / acc_exp [steps], grads of the first step."""
        obs, act, perm = np.asarray(obs), np.asarray(act), np.asarray(perm, np.int64)
        with torch.no_grad():
            rew = softplus(self.logits(obs, act).to(torch.float64).numpy())
        out = dict(rew=rew, loss=[], acc_pi=[], acc_exp=[])
        for k, (lo, hi) in enumerate(chunks(len(act), disc_update_num)):
            p = perm[lo:hi]
            l_pi, l_exp = self.logits(obs[p], act[p]), self.logits(exp_obs[k], exp_act[k])
            loss = -F.logsigmoid(-l_pi).mean() - F.logsigmoid(l_exp).mean()
            self.opt.zero_grad()
            loss.backward()
            if k == 0:
                out["grads"] = torch.cat([q.grad.reshape(-1).to(torch.float64) for q in self.params]).numpy()
                out["logits0"] = torch.cat([l_pi, l_exp]).detach().to(torch.float64).numpy()
            self.opt.step()
            out["loss"].append(loss.item())
            out["acc_pi"].append((l_pi < 0).to(torch.float64).mean().item())
            out["acc_exp"].append((l_exp > 0).to(torch.float64).mean().item())
        return {k: np.asarray(v) for k, v in out.items()}
