"""GPU tests (`-m gpu`) of csrc/gauss.hip against tests/gauss_restatement.py (float64 torch.distributions + autograd).
Bars: gradients, folded sigma_param columns and finalized losses elementwise within rtol 1e-5 (the project's bar for losses and
gradients) + atol 1e-6 max |ref| of the array (the kernel is float64 inside: what remains is the float32 store); the draw z to
test_gpu_sampling.py's bar for cac_normal; exact zeros, equal bits between two runs and between the sample's logp and
`gauss_logp_entropy` of the stored action."""
import itertools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gauss_restatement as gr  # noqa: E402

from tianshou_marl_amd import _abi, ops  # noqa: E402

DEV = "cuda"
R = _abi.GAUSS_ROWS_PER_BLOCK
N_ROWS = 2 * R + 40          # the full batch the minibatches index into
EPS, MAX_ACTION = 0.2, 2.0
_d = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dt)  # noqa: E731
_np = lambda x: x.detach().cpu().numpy().astype(np.float64)  # noqa: E731


def _close(name, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref) / np.maximum(1e-6 * np.abs(ref).max() + 1e-5 * np.abs(ref), np.finfo(np.float64).tiny)
    print(f"PARITY {name}: max |hip - ref64| / (1e-6 max |ref| + 1e-5 |ref|) = {err.max() if err.size else 0:.3g}")
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max(), err_msg=name)


_inputs_cache = {}


def head_inputs(Ad: int, cond: bool, unbounded: bool):
    """Drawn once per (act_dim, sigma mode, unbounded) with a fixed seed: float32 arrays of N_ROWS rows.  logp_old is placed so
    that the float64 ratio of row i sits in one of four bands around the kinks at 1 -+ eps_clip and at dual_clip = 3."""
    key = (Ad, cond, unbounded)
    if key not in _inputs_cache:
        rng = np.random.default_rng(1000 * Ad + 2 * cond + unbounded)
        n = N_ROWS
        mu_raw = rng.uniform(-1.5, 1.5, (n, Ad)).astype(np.float32)
        if cond:   # below, inside and above the clamp [-20, 2]
            band = rng.integers(0, 8, (n, Ad))
            sigma_raw = np.where(band == 0, rng.uniform(-21.0, -20.2, (n, Ad)), np.where(band == 1, rng.uniform(2.2, 3.0, (n, Ad)),
                                                                                       rng.uniform(-2.0, 0.5, (n, Ad)))).astype(np.float32)
        else:
            sigma_raw = rng.uniform(-1.0, 0.5, Ad).astype(np.float32)
        d = gr.dist(torch.as_tensor(mu_raw).double(), torch.as_tensor(sigma_raw).double(), cond, unbounded, MAX_ACTION)
        act = (d.mean + d.stddev * torch.as_tensor(rng.standard_normal((n, Ad)))).numpy().astype(np.float32)
        lo, hi = np.array([0.5, 0.85, 1.25, 3.3]), np.array([0.75, 1.15, 1.6, 4.0])
        band = rng.integers(0, 4, n)
        ratio = rng.uniform(lo[band], hi[band])
        logp_old = (d.log_prob(torch.as_tensor(act).double()).numpy() - np.log(ratio)).astype(np.float32)
        adv = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)).astype(np.float32)   # (normalised, |A| stays above 0.1)
        perm = rng.permutation(n).astype(np.int64)
        _inputs_cache[key] = dict(mu_raw=mu_raw, sigma_raw=sigma_raw, act=act, logp_old=logp_old, adv=adv, perm=perm)
    return _inputs_cache[key]


def _assert_off_the_kinks(ref, sigma_raw, cond, dual_clip, whole_batch):
    """On the float64 reference: every ratio, dual-clip comparison and sigma_raw >= 1e-3 from its kink; over the whole drawn batch
    rows fall on each side of every kink."""
    r, A = ref["ratio"], ref["adv"]
    assert np.abs(r - (1 - EPS)).min() >= 1e-3 and np.abs(r - (1 + EPS)).min() >= 1e-3
    neg = A < 0
    if dual_clip and neg.any():
        assert np.abs(dual_clip * A[neg] - np.minimum(r * A, np.clip(r, 1 - EPS, 1 + EPS) * A)[neg]).min() >= 1e-3
    if cond:
        assert np.abs(sigma_raw + 20).min() >= 1e-3 and np.abs(sigma_raw - 2).min() >= 1e-3
    if whole_batch:
        assert (r < 1 - EPS).any() and ((r > 1 - EPS) & (r < 1 + EPS)).any() and (r > 1 + EPS).any()
        assert ((A < 0) & (r > 3)).any() and ((A < 0) & (r < 3)).any() and (A > 0).any()
        assert not cond or ((sigma_raw < -20).any() and (sigma_raw > 2).any() and ((sigma_raw > -20) & (sigma_raw < 2)).any())


@pytest.mark.parametrize("cond", [True, False], ids=["conditioned", "sigma_param"])
@pytest.mark.parametrize("M", [1, 2 * R - 1, 2 * R, 2 * R + 1])
@pytest.mark.parametrize("Ad", [1, 3, 8, 17, 64])
def test_ppo_head_matches_float64_autograd(Ad, M, cond):
    for unbounded, kind, dual, norm in itertools.product([False, True], [0, 1], [None, 3.0], [True, False]):
        x = head_inputs(Ad, cond, unbounded)
        rows = x["perm"][:M]
        opts = dict(cond=cond, unbounded=unbounded, max_action=MAX_ACTION, eps_clip=EPS, dual_clip=dual, loss_kind=kind)
        sg = x["sigma_raw"][rows] if cond else x["sigma_raw"]
        if kind == 0:   # (the whole drawn batch, then this minibatch with its own advantage statistics)
            every = gr.head(x["mu_raw"], x["sigma_raw"], x["act"], x["logp_old"], x["adv"], adv_norm=norm, **opts)
            _assert_off_the_kinks(every, x["sigma_raw"], cond, dual, True)
        cfg = ops.make_ppo_cfg(EPS, dual, False, norm, 0.5, 0.01, loss_kind=kind)
        raw = np.concatenate([x["mu_raw"][rows], sg], 1) if cond else x["mu_raw"][rows]
        kw = dict(max_action=MAX_ACTION, unbounded=unbounded, sigma_param=None if cond else _d(sg))
        perm = _d(rows, torch.int64)
        stats = ops.ppo_adv_stats(_d(x["adv"]), _d([0, M], torch.int64), perm=perm)[0] if norm else None
        run = lambda: ops.gauss_ppo_head(_d(raw), _d(x["act"]), _d(x["logp_old"]), _d(x["adv"]), cfg, adv_stats=stats, perm=perm, **kw)  # noqa: E731
        h, h2 = run(), run()
        name = f"Ad{Ad} M{M} {'cond' if cond else 'param'} unb{int(unbounded)} kind{kind} dual{dual} norm{int(norm)}"
        nb = h["n_blocks"]
        assert nb == -(-M // R) and h["partial"].shape == (nb, 4)
        assert torch.equal(h["partial"][:, 2], h2["partial"][:, 2]) and not h["partial"][:, 1::2].any()
        if M == 1 and norm:
            # torch.std of one row is NaN (ppo.py:185 on a minibatch of one): the reference has no finite gradient to hold to
            assert not np.isfinite(_np(h["d_raw"])[:, :Ad]).any()
            continue
        slabs = torch.full((3, Ad + 5), float("nan"), device=DEV)
        if not cond:
            ops.gauss_sigma_fold(h["col_partial"], nb, slabs[:, 2:2 + Ad])
            assert torch.equal(h["col_partial"], h2["col_partial"])
        assert torch.equal(h["d_raw"], h2["d_raw"]) and torch.equal(h["partial"], h2["partial"])
        ref = gr.head(x["mu_raw"][rows], sg, x["act"][rows], x["logp_old"][rows], x["adv"][rows], adv_norm=norm, **opts)
        if kind == 0:
            _assert_off_the_kinks(ref, sg, cond, dual, False)
        _close(name + " d_mu", _np(h["d_raw"])[:, :Ad], ref["d_mu"])
        if cond:
            _close(name + " d_sigma", _np(h["d_raw"])[:, Ad:], ref["d_sigma"])
            assert (_np(h["d_raw"])[:, Ad:][(sg < -20) | (sg > 2)] == 0).all()
        else:
            _close(name + " sigma_param columns", _np(slabs[0, 2:2 + Ad]), ref["d_sigma"])
            assert (slabs[1:, 2:2 + Ad] == 0).all() and torch.isnan(slabs[:, :2]).all() and torch.isnan(slabs[:, 2 + Ad:]).all()
        scal = torch.empty(1, 4, device=DEV)
        ops.ppo_finalize_many(h["partial"], nb * 4, _d([nb], torch.int32), _d([M], torch.int64), cfg, scal)
        _close(name + " clip_loss, ent_loss", _np(scal)[0, [1, 3]], [ref["clip_loss"], ref["ent_loss"]])


@pytest.mark.parametrize("B", [1, 5, 130])
@pytest.mark.parametrize("Ad", [1, 3, 64])
def test_sample_and_logp_match_the_restatement(Ad, B):
    rng = np.random.default_rng(Ad * 1000 + B)
    seed, off, off_dev = 0x1234567, 77, 2**33 + 5
    ctr = _d([off_dev], torch.int64)
    # the draw itself: mu = 0 (unbounded), sigma_param = 0 -> act = z
    zero = torch.zeros(B, Ad, device=DEV)
    got, _, _ = ops.gauss_sample(zero, seed, off, ctr, unbounded=True, sigma_param=torch.zeros(Ad, device=DEV))
    z64 = gr.normals(B, Ad, seed, off, [off_dev])
    e_ref = float(np.abs(z64 - gr.normals(B, Ad, seed, off, [off_dev], np.float32)).max())
    tol = 1e-5 * np.abs(z64).max() + e_ref   # test_gpu_sampling.py's bar for cac_normal (test_gpu_distq.py's `_bar`)
    print(f"PARITY gauss z Ad{Ad} B{B}: {np.abs(_np(got) - z64).max() / tol:.3g} of the bar")
    assert np.abs(_np(got) - z64).max() <= tol
    low, high = rng.uniform(-3.0, -1.0, Ad).astype(np.float32), rng.uniform(0.5, 4.0, Ad).astype(np.float32)
    for cond, unbounded, bound in itertools.product([True, False], [False, True], ["clip", "tanh", None]):
        mu_raw = rng.uniform(-1.5, 1.5, (B, Ad)).astype(np.float32)
        sg = rng.uniform(-1.5, 0.7, (B, Ad) if cond else Ad).astype(np.float32)
        raw = _d(np.concatenate([mu_raw, sg], 1) if cond else mu_raw)
        kw = dict(max_action=MAX_ACTION, unbounded=unbounded, sigma_param=None if cond else _d(sg))
        scale = bound is not None   # (action_scaling maps [-1, 1]: only behind a bound)
        act, logp, env = ops.gauss_sample(raw, seed, off, ctr, bound_method=bound, low=_d(low) if scale else None,
                                          high=_d(high) if scale else None, want_env_act=True, **kw)
        d = gr.dist(torch.as_tensor(mu_raw).double(), torch.as_tensor(sg).double(), cond, unbounded, MAX_ACTION)
        name = f"Ad{Ad} B{B} cond{int(cond)} unb{int(unbounded)} {bound}"
        _close(name + " act", _np(act), (d.mean + d.stddev * torch.as_tensor(z64)).numpy())
        _close(name + " logp", _np(logp), d.log_prob(act.cpu().double()).numpy())
        _close(name + " env_act", _np(env), gr.map_action(_np(act), bound, low if scale else None, high if scale else None))
        logp2, ent = ops.gauss_logp_entropy(raw, act, **kw)
        assert torch.equal(logp2, logp), name   # same arithmetic, same order: what lets the update reuse the stored logp
        _close(name + " entropy", _np(ent), d.entropy().numpy())
        # through a permutation of a longer batch of stored actions
        longer = torch.cat([torch.zeros(3, Ad, device=DEV), act.flip(0)])
        assert torch.equal(ops.gauss_logp_entropy(raw, longer, perm=_d(3 + np.arange(B)[::-1].copy(), torch.int64), **kw)[0], logp)
        mode, logp_m, _ = ops.gauss_sample(raw, seed, off, ctr, deterministic=True, **kw)
        _close(name + " mode", _np(mode), d.mean.numpy())
        _close(name + " logp(mode)", _np(logp_m), d.log_prob(mode.cpu().double()).numpy())
