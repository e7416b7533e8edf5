"""Float64 restatement of the FQF path (reference fqf.py:66-106, 178-256; utils/net/discrete.py:240-253, 289-315;
algorithm_base.py:796, 1213-1215) -- the yardstick of the FQF tests.  Written from the description of what the reference
computes, step by step; pinned to the reference by tests/test_host_fqf.py against tests/golden/fqf.npz.  The embedding, the
MLPs and the Adam bookkeeping are those of tests/iqn_restatement.py.

  `propose`          the linear layer, softmax, cumulative sum, midpoints and entropy; with `d_logits`, dWf and dbf
  `fqf_values`       the fraction-weighted sum and the first argmax under compute_q_value's whole-tensor mask offset
  `fqf_head`         both losses, the priorities, d loss / d out and d (fraction - ent_coef entropy loss) / d fraction logits
  `FqfRestatement`   `IqnRestatement`'s net with a fraction layer under an Adam of its own; the successor forwards BEFORE
                     the lagged copy, the lagged net at the ONLINE proposal's fractions
Layout here: out [B, N, A] (fraction-major); the reference's logits are its transpose [B, A, N].
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from iqn_restatement import IqnRestatement, _embed, _np, _t


def _fractions(x):
    """torch: fraction logits [R, N] -> (taus [R, N + 1], tau_hats [R, N], logp [R, N], entropies [R])."""
    logp = x - torch.logsumexp(x, dim=1, keepdim=True)
    p = torch.softmax(logp, dim=1)
    taus = F.pad(torch.cumsum(p, dim=1), (1, 0))
    return taus, (taus[:, :-1] + taus[:, 1:]).detach() / 2.0, logp, -(logp * p).sum(-1)


def fractions_of(x, dtype=torch.float64) -> dict:
    """Fraction logits [R, N] -> dict(taus, tau_hats, logp, entropies) as arrays."""
    return dict(zip(("taus", "tau_hats", "logp", "entropies"), (_np(v) for v in _fractions(_t(x, dtype)))))


def propose(f, Wf, bf, feature_act: bool = False, d_logits=None, dtype=torch.float64) -> dict:
    """f [R, H] -> dict(logits, taus, tau_hats, logp, entropies) and, given d_logits [R, N], dWf and dbf."""
    Wf, bf = (_t(x, dtype).clone().requires_grad_(True) for x in (Wf, bf))
    f = _t(f, dtype)
    x = F.linear(F.relu(f) if feature_act else f, Wf, bf)
    out = dict(zip(("taus", "tau_hats", "logp", "entropies"), (_np(v) for v in _fractions(x))), logits=_np(x))
    if d_logits is not None:
        x.backward(_t(d_logits, dtype))
        out.update(dWf=_np(Wf.grad), dbf=_np(bf.grad))
    return out


def fqf_values(out, taus, mask=None, dtype=torch.float64) -> dict:
    """out [R, N, A], taus [R, N + 1] -> dict(q [R, A], act [R] under `mask`)."""
    taus = _t(taus, dtype)
    q = ((taus[:, 1:] - taus[:, :-1]).unsqueeze(1) * _t(out, dtype).transpose(1, 2)).sum(2)
    sel = q
    if mask is not None:
        sel = q + (1 - _t(np.asarray(mask, bool), dtype)) * (q.min() - q.max() - 1.0)
    return dict(q=_np(q), act=sel.argmax(dim=1).numpy())


def fqf_head(out, out_tau, frac_logits, out_next_on, taus_next, out_next_tg, mask_next, act, mc, gpow, vmask, weight,
             ent_coef: float = 0.0, dtype=torch.float64) -> dict:
    """out [B, N, A] at the midpoints and out_tau [B, N - 1, A] at the interior fractions of the proposal `frac_logits` [B, N];
    out_next_on [B, N, A] with its proposal's taus_next [B, N + 1] chooses a*; out_next_tg [B, N, A] or None (then the online
    forward is the next distribution).  -> returns [B, N], prio [B], quantile_loss, fraction_loss, entropy_loss, loss, d_out
    [B, N, A], d_logits [B, N], a_star [B], q_taken [B], u [B, N, N], cmp_gap (the least distance of two compared quantiles)."""
    B, N = np.asarray(frac_logits).shape
    rows = torch.arange(B)
    a_star = torch.as_tensor(fqf_values(out_next_on, taus_next, mask_next, dtype)["act"])
    nxt = _t(out_next_on if out_next_tg is None else out_next_tg, dtype)[rows, :, a_star]            # [B, N]
    vm = _t(np.asarray(vmask, bool), dtype).reshape(-1, 1)
    returns = nxt * vm * _t(gpow, dtype).reshape(-1, 1) + _t(mc, dtype).reshape(-1, 1)
    x = _t(out, dtype).clone().requires_grad_(True)
    xf = _t(frac_logits, dtype).clone().requires_grad_(True)
    taus, tau_hats, _, entropies = _fractions(xf)
    a = torch.as_tensor(np.asarray(act, np.int64))
    curr = x[rows, :, a]                                                                             # [B, N]
    u = returns.unsqueeze(1) - curr.unsqueeze(2)                                                     # u[b][i][j]
    au = u.abs()
    h = torch.where(au < 1.0, 0.5 * u * u, au - 0.5)
    k = (tau_hats.unsqueeze(2) - (u.detach() <= 0).to(dtype)).abs()
    per_row = (h * k).sum(-1).mean(1)
    quantile_loss = (per_row * (1.0 if weight is None else _t(weight, dtype))).mean()
    with torch.no_grad():
        qh, qt = curr.detach(), _t(out_tau, dtype)[rows, :, a]                                       # [B, N], [B, N - 1]
        lo, hi = torch.cat([qh[:, :1], qt[:, :-1]], dim=1), torch.cat([qt[:, 1:], qh[:, -1:]], dim=1)
        v1, v2 = qt - qh[:, :-1], qt - qh[:, 1:]
        g = torch.where(qt > lo, v1, -v1) + torch.where(qt < hi, v2, -v2)
        cmp_gap = float(torch.minimum((qt - lo).abs(), (qt - hi).abs()).min())
    fraction_loss = (g * taus[:, 1:-1]).sum(1).mean()
    entropy_loss = entropies.mean()
    fe = fraction_loss - ent_coef * entropy_loss
    fe.backward(retain_graph=True)
    quantile_loss.backward()
    return dict(returns=_np(returns), prio=_np(h.abs().sum(-1).mean(1)), quantile_loss=float(quantile_loss.item()),
                fraction_loss=float(fraction_loss.item()), entropy_loss=float(entropy_loss.item()),
                loss=float(quantile_loss.item()) + float(fe.item()), d_out=_np(x.grad), d_logits=_np(xf.grad),
                a_star=a_star.numpy(), q_taken=_np(curr.mean(1)), u=_np(u), cmp_gap=cmp_gap)


class FqfRestatement(IqnRestatement):
    """`IqnRestatement`'s net plus the fraction layer [N, H] + [N] over the (detached) features, each under its own Adam."""

    def __init__(self, flat, frac_flat, pre_dims, last_dims, C: int, N: int, feature_act: bool = True, lr: float = 1e-3,
                 target_update_freq: int = 0, ent_coef: float = 0.0, dtype=torch.float64) -> None:
        super().__init__(flat, pre_dims, last_dims, C, feature_act, lr, target_update_freq, dtype)
        H = self.pre_dims[-1]
        ff = torch.as_tensor(np.asarray(frac_flat, np.float64)).to(dtype)
        assert ff.numel() == N * H + N
        self.frac = [ff[:N * H].reshape(N, H).clone().requires_grad_(True), ff[N * H:].clone().requires_grad_(True)]
        self.frac_opt = torch.optim.Adam(self.frac, lr=lr)
        self.N, self.ent_coef = int(N), float(ent_coef)

    def features(self, ps, x, kinks: list | None = None):
        """The preprocess net: -> (its last LINEAR output, what the rest of the net reads)."""
        x = _t(x, self.dtype)
        n_pre = len(self.pre_dims) - 1
        for i in range(n_pre):
            x = F.linear(x, ps[2 * i], ps[2 * i + 1])
            if (i < n_pre - 1 or self.feature_act) and kinks is not None:
                kinks.append(x)
            if i < n_pre - 1:
                x = F.relu(x)
        return x

    def quantiles(self, ps, f, taus, kinks: list | None = None):
        """The embedding at `taus` and `last`: -> out [B, S, A]."""
        n_pre, n_last = len(self.pre_dims) - 1, len(self.last_dims) - 1
        x, pre = _embed(f, taus, ps[-2], ps[-1], self.feature_act)
        if kinks is not None:
            kinks.append(pre)
        for i in range(n_last):
            x = F.linear(x, ps[2 * (n_pre + i)], ps[2 * (n_pre + i) + 1])
            if i < n_last - 1:
                if kinks is not None:
                    kinks.append(x)
                x = F.relu(x)
        return x

    def frac_logits(self, f):
        f = f.detach()
        return F.linear(F.relu(f) if self.feature_act else f, self.frac[0], self.frac[1])

    def frac_weights(self) -> np.ndarray:
        return self.flat_of(self.frac)

    def update(self, obs, act, obs_next, mask_next, mc, gpow, vmask, weight=None) -> dict:
        """The successor forwards (online at its own proposal, lagged at those fractions), the `_iter` rule's copy, both
        losses, both gradients, the fraction model's Adam step, then the quantile model's."""
        kinks: list = []
        with torch.no_grad():
            f_n = self.features(self.params, obs_next, kinks)
            taus_n, hats_n, _, _ = _fractions(self.frac_logits(f_n))
            on = self.quantiles(self.params, f_n, hats_n, kinks).numpy()
            tg = None
            if self.freq > 0:
                tg = self.quantiles(self.target, self.features(self.target, obs_next, kinks), hats_n, kinks).numpy()
        if self.freq > 0 and self._iter % self.freq == 0:
            for p, t in zip(self.params, self.target):
                t.data.copy_(p.data)
        self._iter += 1
        f = self.features(self.params, obs, kinks)
        xf = self.frac_logits(f)
        taus, hats, _, _ = _fractions(xf)
        out = self.quantiles(self.params, f, hats, kinks)
        with torch.no_grad():
            out_tau = self.quantiles(self.params, f, taus[:, 1:-1], kinks)
        h = fqf_head(out.detach().numpy(), out_tau.numpy(), xf.detach().numpy(), on, taus_n.numpy(), tg, mask_next, act, mc,
                     gpow, vmask, weight, self.ent_coef, self.dtype)
        self.opt.zero_grad()
        self.frac_opt.zero_grad()
        xf.backward(torch.as_tensor(h["d_logits"]).to(self.dtype))
        out.backward(torch.as_tensor(h["d_out"]).to(self.dtype))
        h["grads"] = self.flat_of([p.grad for p in self.params])
        h["frac_grads"] = self.flat_of([p.grad for p in self.frac])
        self.frac_opt.step()
        self.opt.step()
        q = fqf_values(on, taus_n.numpy())["q"]
        top = np.sort(q, axis=1)
        # the distance to the nearest point of non-smoothness: of the ReLUs (pre-activations at 0), and of the head (top-2 gaps
        # of q, u at 0, |u| at 1, the two sides of every s1 / s2 comparison)
        h["relu_gap"] = min(float(k.detach().abs().min()) for k in kinks)
        h["head_gap"] = min(float((top[:, -1] - top[:, -2]).min()), float(np.abs(h["u"]).min()),
                            float(np.abs(np.abs(h["u"]) - 1.0).min()), h["cmp_gap"])
        return h

    def frac_adam_cond(self) -> np.ndarray:
        """`adam_cond` of the fraction model's Adam."""
        out = []
        for p in self.frac:
            st = self.frac_opt.state[p]
            v_hat = st["exp_avg_sq"].detach().to(torch.float64) / (1.0 - 0.999 ** float(st["step"]))
            out.append((self.lr / (torch.sqrt(v_hat) + 1e-8)).reshape(-1))
        return torch.cat(out).numpy()
