"""Float64 restatement of the ICM path (reference utils/net/discrete.py:378-429, algorithm/modelbased/icm.py:77-109) -- the
yardstick of the ICM tests.  Written from the reference's description of what it computes; pinned to the reference by
tests/test_icm_restatement.py against tests/golden/icm.npz.

  `head`             mse, cross entropy, the three gradients and the three losses from the networks' outputs (numpy, explicit)
  `join_grad`        the feature net's d_out [2R, F] from the two input gradients and d_phi2_fwd (any float dtype, written order)
  `IcmRestatement`   feature net + forward model + inverse model on one flat vector (`parameters()` order), torch autograd, Adam
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def head(phi2_hat, phi2, act_hat, act, forward_loss_weight: float, lr_scale: float) -> dict:
    """-> mse [R], ce [R], d_phi2_hat, d_phi2_fwd [R, F], d_act_hat [R, A], forward_loss, inverse_loss, loss (f64)."""
    ph, p2, x = (np.asarray(v, np.float64) for v in (phi2_hat, phi2, act_hat))
    act = np.asarray(act, np.int64)
    R, A = x.shape
    w, s = float(forward_loss_weight), float(lr_scale)
    d = ph - p2
    mse = 0.5 * (d * d).sum(1)
    t = x - x.max(1, keepdims=True)
    e = np.exp(t)
    se = e.sum(1, keepdims=True)
    onehot = np.zeros((R, A))
    onehot[np.arange(R), act] = 1.0
    ce = np.log(se[:, 0]) - t[np.arange(R), act]
    fwd, inv = mse.mean(), ce.mean()
    return dict(mse=mse, ce=ce, d_phi2_hat=s * w * d / R, d_phi2_fwd=-(s * w * d / R), d_act_hat=s * (1.0 - w) * (e / se - onehot) / R,
                forward_loss=fwd, inverse_loss=inv, loss=((1.0 - w) * inv + w * fwd) * s)


def join_grad(g_fwd, g_inv, d_phi2_fwd):
    """d_out [2R, F]: row 2r = g_fwd[r] + g_inv[r, :F], row 2r + 1 = g_inv[r, F:] + d_phi2_fwd[r], in the inputs' dtype."""
    g_fwd, g_inv, d_phi2_fwd = np.asarray(g_fwd), np.asarray(g_inv), np.asarray(d_phi2_fwd)
    R, Fd = g_fwd.shape
    out = np.empty((R, 2, Fd), g_fwd.dtype)
    out[:, 0] = g_fwd + g_inv[:, :Fd]
    out[:, 1] = g_inv[:, Fd:] + d_phi2_fwd
    return out.reshape(2 * R, Fd)


def x_fwd(phi, act, n_act: int):
    """[phi[2r] | one_hot(act[r])]; an action outside [0, n_act) gives an all-zero one-hot."""
    phi, act = np.asarray(phi), np.asarray(act, np.int64)
    R = act.size
    out = np.zeros((R, phi.shape[1] + n_act), phi.dtype)
    out[:, :phi.shape[1]] = phi[0::2]
    ok = (act >= 0) & (act < n_act)
    out[np.nonzero(ok)[0], phi.shape[1] + act[ok]] = 1
    return out


class IcmRestatement:
    """Three ReLU MLPs on one flat vector [feature_net | forward_model | inverse_model], each w0 b0 w1 b1 ...:
    feat_dims[0] -> .. -> feat_dims[-1] = F;  F + A -> hidden.. -> F;  2F -> hidden.. -> A."""

    def __init__(self, flat, feat_dims, n_act: int, hidden=(), lr: float = 1e-3, dtype=torch.float64) -> None:
        self.F, self.A, self.dtype, self.lr = int(feat_dims[-1]), int(n_act), dtype, lr
        self.dims = [[int(d) for d in feat_dims], [self.F + self.A, *hidden, self.F], [2 * self.F, *hidden, self.A]]
        flat = torch.as_tensor(np.asarray(flat, np.float64)).to(dtype)
        self.params, o = [], 0
        for dims in self.dims:
            ps = []
            for i in range(len(dims) - 1):
                for shp in ((dims[i + 1], dims[i]), (dims[i + 1],)):
                    n = int(np.prod(shp))
                    ps.append(flat[o:o + n].reshape(shp).clone().requires_grad_(True))
                    o += n
            self.params.append(ps)
        assert o == flat.numel()
        self.opt = torch.optim.Adam([p for ps in self.params for p in ps], lr=lr)
        self.kink = np.inf

    def _net(self, k: int, x):
        ps, L = self.params[k], len(self.dims[k]) - 1
        for i in range(L):
            x = F.linear(x, ps[2 * i], ps[2 * i + 1])
            if i < L - 1:
                self.kink = min(self.kink, float(x.detach().abs().min()))
                x = F.relu(x)
        return x

    def weights(self) -> np.ndarray:
        return torch.cat([p.detach().reshape(-1).to(torch.float64) for ps in self.params for p in ps]).numpy()

    def module(self, s1, act, s2) -> dict:
        """IntrinsicCuriosityModule.forward, the intermediate tensors kept (torch, with their graph)."""
        t = lambda v: torch.as_tensor(np.asarray(v)).to(self.dtype)  # noqa: E731
        act = torch.as_tensor(np.asarray(act, np.int64))
        phi1, phi2 = self._net(0, t(s1)), self._net(0, t(s2))
        phi2_hat = self._net(1, torch.cat([phi1, F.one_hot(act, num_classes=self.A).to(self.dtype)], dim=1))
        mse = 0.5 * ((phi2_hat - phi2) ** 2).sum(1)
        act_hat = self._net(2, torch.cat([phi1, phi2], dim=1))
        return dict(phi1=phi1, phi2=phi2, phi2_hat=phi2_hat, mse=mse, act_hat=act_hat, act=act)

    def loss_grads(self, s1, act, s2, forward_loss_weight: float, lr_scale: float) -> dict:
        """The module, the loss of _icm_update and its gradient over the whole vector (autograd), nothing stepped."""
        m = self.module(s1, act, s2)
        inv = F.cross_entropy(m["act_hat"], m["act"]).mean()
        fwd = m["mse"].mean()
        loss = ((1 - forward_loss_weight) * inv + forward_loss_weight * fwd) * lr_scale
        self.opt.zero_grad()
        loss.backward()
        n = lambda v: v.detach().to(torch.float64).numpy()  # noqa: E731
        grads = np.concatenate([n(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for ps in self.params for p in ps])
        return dict(mse=n(m["mse"]), act_hat=n(m["act_hat"]), phi=np.stack([n(m["phi1"]), n(m["phi2"])], 1).reshape(-1, self.F),
                    phi2_hat=n(m["phi2_hat"]), icm_loss=loss.item(), icm_forward_loss=fwd.item(), icm_inverse_loss=inv.item(),
                    grads=grads)

    def update(self, s1, act, s2, forward_loss_weight: float, lr_scale: float) -> dict:
        """`loss_grads`, then ONE Adam step."""
        r = self.loss_grads(s1, act, s2, forward_loss_weight, lr_scale)
        self.opt.step()
        return r
