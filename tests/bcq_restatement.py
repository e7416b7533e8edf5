"""Float64 restatement of BCQ (reference imitation/bcq.py:91-116, 188-263, utils/net/continuous.py:427-432, 478-513,
torch.optim.Adam) and of every kernel of csrc/bcq.hip -- the yardstick of the BCQ tests.  Written from the description of what
the reference computes, step by step, in numpy with closed-form gradients of everything between a network product and an
optimiser step (the networks themselves run in torch float64, as in tests/cac_restatement.py, whose mse and actor heads are
used as they are); pinned to the reference by tests/test_host_bcq.py against tests/golden/bcq.npz.

  `latent`          [obs | mean + exp(clamp(ls, -4, 15)) eps] and std
  `decode_rows`     [obs repeated | clamp(z, +-0.5)] for two groups of observations
  `action_rows`     [obs | max_action tanh(raw)]
  `target`          rew + not done * f32(gamma) * max_k(lmbda min(q1, q2) + (1 - lmbda) max(q1, q2))
  `vae_head`        mse(act, recon) + KL / 2 and its gradient at the decoder's raw output
  `latent_grad`     the decoder's input gradient -> the gradient at the encoder's [mean | raw log_std]
  `perturb`         clamp(a + phi max_action tanh(raw_p), +-max_action) and the factor of its backward
  `select`          the first maximal q per group and its candidate
  `BcqRestatement`  the nets on flat vectors (the VAE's as [encoder with the stacked mean / log_std layer | decoder]), their
                    Adams, the reference's order of steps, acting; `kink`: the smallest distance from any non-smooth point
"""
from __future__ import annotations

import numpy as np
import torch

from cac_restatement import CacRestatement, _Net, critic_head, det_actor_head, flat_of

LS_MIN, LS_MAX, Z_CLIP = -4.0, 15.0, 0.5


def _split_head(head, dtype):
    head = np.asarray(head, dtype)
    L = head.shape[1] // 2
    return head[:, :L], head[:, L:]


def latent(head, eps, obs, dtype=np.float64):
    mean, ls = _split_head(head, dtype)
    std = np.exp(np.clip(ls, dtype(LS_MIN), dtype(LS_MAX)))
    return np.concatenate([np.asarray(obs, dtype), mean + std * np.asarray(eps, dtype)], 1), std


def decode_rows(src_a, rep_a: int, src_b, z, dtype=np.float64):
    rows = np.repeat(np.asarray(src_a, dtype), rep_a, 0)
    if src_b is not None:
        rows = np.concatenate([rows, np.asarray(src_b, dtype)], 0)
    return np.concatenate([rows, np.clip(np.asarray(z, dtype), -dtype(Z_CLIP), dtype(Z_CLIP))], 1)


def action_rows(raw, x_dec, D: int, max_action=1.0, dtype=np.float64):
    return np.concatenate([np.asarray(x_dec, dtype)[:, :D], dtype(max_action) * np.tanh(np.asarray(raw, dtype))], 1)


def target(q1, q2, rew, vmask, K: int, gamma, lmbda, dtype=np.float64):
    """logical_not(done) * gamma is a float32 tensor in any run of the reference (bcq.py:235): gamma enters rounded to float32."""
    q1, q2 = np.asarray(q1, dtype).reshape(-1, K), np.asarray(q2, dtype).reshape(-1, K)
    tq = (dtype(lmbda) * np.minimum(q1, q2) + dtype(1.0 - lmbda) * np.maximum(q1, q2)).max(1)
    return np.asarray(rew, dtype).reshape(-1) + np.asarray(vmask, bool).astype(dtype) * dtype(np.float32(gamma)) * tq


def vae_head(raw, act, head, max_action=1.0, dtype=np.float64) -> dict:
    raw, act, M = np.asarray(raw, dtype), np.asarray(act, dtype), dtype(max_action)
    mean, ls = _split_head(head, dtype)
    B, Ad = raw.shape
    th = np.tanh(raw)
    diff = M * th - act
    c = np.clip(ls, dtype(LS_MIN), dtype(LS_MAX))
    std = np.exp(c)
    recon_loss, kl_loss = float((diff * diff).mean()), float((-c + (std * std + mean * mean - 1) / 2).mean())
    return dict(d_raw=2 * diff / dtype(B * Ad) * M * (1 - th * th), recon_loss=recon_loss, kl_loss=kl_loss,
                vae_loss=recon_loss + kl_loss / 2)


def latent_grad(dz, head, eps, dtype=np.float64):
    mean, ls = _split_head(head, dtype)
    dz, eps = np.asarray(dz, dtype), np.asarray(eps, dtype)
    B, L = dz.shape
    std = np.exp(np.clip(ls, dtype(LS_MIN), dtype(LS_MAX)))
    passm = ((ls >= LS_MIN) & (ls <= LS_MAX)).astype(dtype)
    inv = dtype(1.0) / dtype(2 * B * L)
    return np.concatenate([dz + mean * inv, passm * (dz * eps * std + (std * std - 1) * inv)], 1)


def perturb(raw_p, x_in, D: int, phi, max_action=1.0, dtype=np.float64):
    """-> (rows [obs | clamp(u, +-M)], factor, u = a + phi M tanh(raw_p))."""
    x_in, M = np.asarray(x_in, dtype), dtype(max_action)
    th = np.tanh(np.asarray(raw_p, dtype))
    u = x_in[:, D:] + dtype(phi) * M * th
    factor = dtype(phi) * (1 - th * th) * ((u >= -M) & (u <= M)).astype(dtype)
    return np.concatenate([x_in[:, :D], np.clip(u, -M, M)], 1), factor, u


def select(q, rows, S: int, col0: int, Ad: int):
    q, rows = np.asarray(q).reshape(-1, S), np.asarray(rows)
    index = q.argmax(1)   # numpy's, as torch's: the first maximum
    return rows[np.arange(q.shape[0]) * S + index, col0:col0 + Ad], index.astype(np.int32)


class BcqRestatement:
    """`init`: flat vectors pert, critic[, critic2], vae = [encoder whose last layer stacks mean over log_std | decoder]."""

    def __init__(self, init, D, Ad, L, pert_dims, critic_dims, enc_dims, dec_dims, tau, gamma, lr=1e-3, max_action=1.0, phi=0.05,
                 lmbda=0.75, num_sampled_action=10, forward_sampled_times=100) -> None:
        self.kink = np.inf
        self.D, self.Ad, self.L, self.M, self.phi = D, Ad, L, float(max_action), float(phi)
        self.tau, self.gamma, self.lmbda, self.K, self.S = float(tau), float(gamma), float(lmbda), num_sampled_action, forward_sampled_times
        n_enc = sum(a * b + b for a, b in zip(enc_dims, enc_dims[1:]))
        vae = np.asarray(init["vae"], np.float64)
        self.nets = {"pert": _Net(init["pert"], pert_dims, lr, self), "critic": _Net(init["critic"], critic_dims, lr, self),
                     "critic2": _Net(init.get("critic2", init["critic"]), critic_dims, lr, self),
                     "enc": _Net(vae[:n_enc], enc_dims, lr, self), "dec": _Net(vae[n_enc:], dec_dims, lr, self)}
        self.old = {n: self.nets[n].twin() for n in ("pert", "critic", "critic2")}
        self.clipped = self.below = 0.0   # of the last update: the share of perturbed actions at +-M, of raw log_std below -4

    _q_and_dqda = CacRestatement._q_and_dqda

    def weights(self, name: str) -> np.ndarray:
        if name.endswith("_old"):
            return flat_of(self.old[name[:-4]])
        if name == "vae":
            return np.concatenate([flat_of(self.nets["enc"].params), flat_of(self.nets["dec"].params)])
        return flat_of(self.nets[name].params)

    def _fwd(self, name, x, old=False, grad=False):
        net = self.nets[name]
        with torch.set_grad_enabled(grad):
            return net.fwd(self.old[name] if old else net.params, x)

    def _near(self, *dists) -> None:
        for d in dists:
            self.kink = min(self.kink, float(np.min(d)))

    def _decode_rows(self, src_a, rep_a, src_b, z):
        self._near(np.abs(np.abs(np.asarray(z, np.float64)) - Z_CLIP))   # every normal versus +-0.5
        return decode_rows(src_a, rep_a, src_b, z)

    def update(self, obs, act, rew, done, obs_next, z_vae, z_next, z_obs) -> dict:
        obs, act, obs_next = (np.asarray(v, np.float64) for v in (obs, act, obs_next))
        B, K, D, Ad = obs.shape[0], self.K, self.D, self.Ad
        enc, dec = self.nets["enc"], self.nets["dec"]
        # 1. the VAE's loss and step
        head = self._fwd("enc", np.concatenate([obs, act], 1), grad=True)
        h = head.detach().numpy()
        self._near(np.abs(h[:, self.L:] - LS_MIN), np.abs(h[:, self.L:] - LS_MAX))
        self.below = float((h[:, self.L:] < LS_MIN).mean())
        x_dec, _ = latent(h, z_vae, obs)
        x_dec_t = torch.as_tensor(x_dec).clone().requires_grad_(True)
        raw = dec.fwd(dec.params, x_dec_t)
        vh = vae_head(raw.detach().numpy(), act, h, self.M)
        g_dec = dec.step(raw, vh["d_raw"])
        g_enc = enc.step(head, latent_grad(x_dec_t.grad.numpy()[:, D:], h, z_vae))
        grads = dict(vae=np.concatenate([g_enc, g_dec]))
        # 2. one decode with the stepped VAE: K actions per obs_next, one per obs
        xd = self._decode_rows(obs_next, K, obs, np.concatenate([z_next, z_obs], 0))
        X = action_rows(self._fwd("dec", xd).numpy(), xd, D, self.M)
        # 3. the target on the decoded (not perturbed) actions
        tq1 = self._fwd("critic", X[:B * K], old=True).numpy().reshape(-1)
        tq2 = self._fwd("critic2", X[:B * K], old=True).numpy().reshape(-1)
        if not np.array_equal(tq1, tq2):
            self._near(np.abs(tq1 - tq2))
        tgt = target(tq1, tq2, rew, ~np.asarray(done, bool), K, self.gamma, self.lmbda)
        # 4. both critics' mse steps
        x = np.concatenate([obs, act], 1)
        q1, q2 = self._fwd("critic", x, grad=True), self._fwd("critic2", x, grad=True)
        ch = critic_head(q1.detach().numpy(), q2.detach().numpy(), tgt)
        grads.update(critic=self.nets["critic"].step(q1, ch["dq1"]), critic2=self.nets["critic2"].step(q2, ch["dq2"]))
        # 5. the perturbation net's step through critic 1 after its step
        x_s = X[B * K:]
        raw_p = self._fwd("pert", x_s, grad=True)
        x_pi, factor, u = perturb(raw_p.detach().numpy(), x_s, D, self.phi, self.M)
        self._near(np.abs(np.abs(u) - self.M))
        self.clipped = float((np.abs(u) > self.M).mean())
        q_pi, g = self._q_and_dqda("critic", x_pi[:, :D], x_pi[:, D:])
        ah = det_actor_head(g, factor, q_pi, self.M)
        grads["pert"] = self.nets["pert"].step(raw_p, ah["d_raw"])
        # 6. the Polyak moves
        for n in ("pert", "critic", "critic2"):
            for p, t in zip(self.nets[n].params, self.old[n]):
                t.copy_(self.tau * p.detach() + (1.0 - self.tau) * t)
        return dict(actor_loss=ah["loss"], critic1_loss=ch["loss1"], critic2_loss=ch["loss2"], vae_loss=vh["vae_loss"],
                    kl_loss=vh["kl_loss"], target=tgt, grads=grads)

    def act(self, obs, z) -> dict:
        """BCQPolicy.forward: obs [n, D], z [n S, L] -> act [n, Ad], index [n], the candidates and their q."""
        obs = np.asarray(obs, np.float64)
        xd = self._decode_rows(obs, self.S, None, z)
        x = action_rows(self._fwd("dec", xd).numpy(), xd, self.D, self.M)
        x_pi, _, u = perturb(self._fwd("pert", x).numpy(), x, self.D, self.phi, self.M)
        self._near(np.abs(np.abs(u) - self.M))
        q = self._fwd("critic", x_pi).numpy().reshape(-1)
        if self.S > 1:
            top = np.sort(q.reshape(-1, self.S), 1)
            self._near(top[:, -1] - top[:, -2])
        a, index = select(q, x_pi, self.S, self.D, self.Ad)
        return dict(act=a, index=index, rows=x_pi, q=q)
