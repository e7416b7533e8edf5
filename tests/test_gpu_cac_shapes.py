"""GPU tests (`-m gpu`) of csrc/cac.hip at the smallest shapes at which its kernels can go wrong, each against the float64
restatement (tests/cac_restatement.py) under test_gpu_distq.py's `_bar` with e_ref = 0: B around the rows of a workgroup and
over many workgroups, act_dim from 1 to TSM_CAC_MAX_ACT_DIM, critic rows whose width is no multiple of 4 written through a row
pointer that is not 16-byte aligned, weight present / absent, one critic / two, noise_clip <= 0, sigma_raw at and beyond both
clamp ends, vmask all zero, and act_dim = TSM_CAC_MAX_ACT_DIM + 1 refused on the host."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cac_restatement as R  # noqa: E402
from test_gpu_cac import DEV, _d, _final, _n, head_inputs  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops

ROWS = 16   # TSM_CAC_ROWS_PER_BLOCK
SHAPES = [(1, 1), (ROWS - 1, 2), (ROWS + 1, 5), (300, 64), (300, 3)]


def test_constants():
    assert _abi.CAC_ROWS_PER_BLOCK == ROWS and _abi.CAC_MAX_ACT_DIM == 64


@pytest.mark.parametrize("B,Ad", SHAPES)
def test_every_head_at_the_shape(B, Ad):
    d = head_inputs(None, B, Ad, seed=B + Ad)
    alpha = torch.tensor([0.2], device=DEV)
    # rows of D + Ad floats with D + Ad no multiple of 4, inside storage that starts 4 bytes off a 16-byte boundary
    D = 4 - (Ad % 4) + 1 if (Ad + 1) % 4 else 2
    W = D + Ad
    assert W % 4 != 0
    store = torch.zeros(B * W + 1, device=DEV)
    rows = store[1:].view(B, W)
    assert rows.data_ptr() % 16 != 0
    for clip in (0.5, 0.0, -1.0):   # noise_clip <= 0: no clip
        ref, omt2_ref = R.det_action(d["raw"], 2.0, d["z"], 0.7, clip)
        _, omt2 = ops.cac_det_action(_d(d["raw"]), 2.0, z=_d(d["z"]), policy_noise=0.7, noise_clip=clip, out=rows, col0=D,
                                     want_backward=True)
        _bar(f"det_action clip={clip}", _n(rows[:, D:]), ref, 0.0)
        assert not _n(rows[:, :D]).any() and float(store[0]) == 0.0
    _bar("1 - tanh^2", _n(omt2), omt2_ref, 0.0)
    rh = R.det_actor_head(d["g1"], omt2_ref, d["q1"], 2.0)
    ah = ops.cac_det_actor_head(_d(d["g1"]), omt2, _d(d["q1"]), 2.0)
    _bar("det d_raw", _n(ah["d_raw"]), rh["d_raw"], 0.0)
    _bar("det actor_loss", _final(ah["partial"], B)[0], rh["loss"], 0.0)
    raw = np.concatenate([d["raw"], d["sraw"]], 1)
    ref = R.sac_action(d["raw"], d["sraw"], d["z"], 1.0, False)
    rows.zero_()
    _, logp = ops.sac_action(_d(raw), _d(d["z"]), 1.0, False, out=rows, col0=D)
    _bar("sac act", _n(rows[:, D:]), ref["a"], 0.0)
    _bar("sac logp", _n(logp), ref["logp"], 0.0)
    assert not _n(rows[:, :D]).any() and float(store[0]) == 0.0
    for twin in (True, False):
        q2, g2 = (d["q2"], d["g2"]) if twin else (None, None)
        rh = R.sac_actor_head(d["raw"], d["sraw"], d["z"], d["q1"], q2, d["g1"], g2, np.float32(0.2), 1.0, False)
        ah = ops.sac_actor_head(_d(raw), _d(d["z"]), _d(d["q1"]), None if q2 is None else _d(q2), _d(d["g1"]),
                                None if g2 is None else _d(g2), alpha)
        _bar(f"sac d_raw twin={twin}", _n(ah["d_raw"]), np.concatenate([rh["d_mu"], rh["d_sigma"]], 1), 0.0)
        fin = _final(ah["partial"], B)
        _bar(f"sac actor_loss twin={twin}", fin[0], rh["loss"], 0.0)
        _bar(f"sac mean entropy twin={twin}", fin[1], rh["mean_entropy"], 0.0)
        for wt in (None, d["weight"]):
            rc = R.critic_head(d["q1"], q2, d["ret"], wt)
            ch = ops.cac_critic_head(_d(d["q1"]), None if q2 is None else _d(q2), _d(d["ret"]), None if wt is None else _d(wt))
            _bar("dq1", _n(ch["dq1"]), rc["dq1"], 0.0)
            _bar("prio", _n(ch["prio"]), rc["prio"], 0.0)
            fin = _final(ch["partial"], B)
            _bar("critic1_loss", fin[0], rc["loss1"], 0.0)
            if twin:
                _bar("dq2", _n(ch["dq2"]), rc["dq2"], 0.0)
                _bar("critic2_loss", fin[1], rc["loss2"], 0.0)
        for vm in (d["vmask"], np.zeros(B, bool)):   # vmask all zero: returns = mc
            rt = R.target(d["q1"], q2, d["lp"] if twin else None, np.float32(0.2), d["mc"], d["gpow"], vm)
            got = ops.cac_target(_d(d["q1"]), None if q2 is None else _d(q2), _d(d["mc"]), _d(d["gpow"]), _d(vm, torch.uint8),
                                 logp_next=_d(d["lp"]) if twin else None, alpha_dev=alpha if twin else None)
            _bar("target", _n(got), rt, 0.0)
            if not vm.any():
                assert np.array_equal(_n(got), d["mc"].astype(np.float64))
    z = ops.cac_normal(B * Ad, 11, offset=B, device=DEV)
    assert z.numel() == B * Ad and bool(torch.isfinite(z).all())
    assert torch.equal(z, ops.cac_normal(B * Ad + 3, 11, offset=B, device=DEV)[:B * Ad])


def test_sigma_raw_at_and_beyond_the_clamp_ends():
    B, Ad = 6, 4
    d = head_inputs(None, B, Ad, seed=1)
    s = d["sraw"]
    s[0], s[1], s[2], s[3] = 2.0, -20.0, 2.5, -23.0   # at both ends (the gradient passes), beyond both (it is zero)
    d["raw"][1], d["z"][1] = 0.1, 0.5                  # sigma = exp(-20): keep the row's action at the mean
    raw = np.concatenate([d["raw"], s], 1)
    alpha = torch.tensor([0.2], device=DEV)
    ref = R.sac_action(d["raw"], s, d["z"], 1.0, False)
    act, logp = ops.sac_action(_d(raw), _d(d["z"]))
    _bar("act", _n(act), ref["a"], 0.0)
    _bar("logp", _n(logp), ref["logp"], 0.0)
    rh = R.sac_actor_head(d["raw"], s, d["z"], d["q1"], d["q2"], d["g1"], d["g2"], np.float32(0.2), 1.0, False)
    ah = ops.sac_actor_head(_d(raw), _d(d["z"]), _d(d["q1"]), _d(d["q2"]), _d(d["g1"]), _d(d["g2"]), alpha)
    ds = _n(ah["d_raw"][:, Ad:])
    _bar("d_sigma", ds, rh["d_sigma"], 0.0)
    _bar("d_mu", _n(ah["d_raw"][:, :Ad]), rh["d_mu"], 0.0)
    assert not ds[2].any() and not ds[3].any() and ds[0].all() and ds[1].all()


def test_a_tie_of_the_critics_splits_the_gradient():
    B, Ad = 5, 3
    d = head_inputs(None, B, Ad, seed=2)
    raw = np.concatenate([d["raw"], d["sraw"]], 1)
    alpha = torch.tensor([0.2], device=DEV)
    rh = R.sac_actor_head(d["raw"], d["sraw"], d["z"], d["q1"], d["q1"], d["g1"], d["g2"], np.float32(0.2), 1.0, False)
    ah = ops.sac_actor_head(_d(raw), _d(d["z"]), _d(d["q1"]), _d(d["q1"]), _d(d["g1"]), _d(d["g2"]), alpha)
    _bar("d_raw at q1 = q2", _n(ah["d_raw"]), np.concatenate([rh["d_mu"], rh["d_sigma"]], 1), 0.0)


def test_one_more_action_component_than_the_limit_is_refused_on_the_host():
    n = _abi.CAC_MAX_ACT_DIM + 1
    with pytest.raises(ValueError, match=r"act_dim = 65 outside \[1, 64\]"):
        ops.cac_det_action(torch.zeros(2, n, device=DEV))
    with pytest.raises(ValueError, match=r"act_dim = 65 outside \[1, 64\]"):
        ops.sac_action(torch.zeros(2, 2 * n, device=DEV))
    with pytest.raises(ValueError, match="leave the row"):
        ops.cac_det_action(torch.zeros(2, 3, device=DEV), out=torch.zeros(2, 5, device=DEV), col0=3)
