"""GPU tests (`-m gpu`) of the ICM kernels alone (csrc/icm.hip: tsm_icm_rows, tsm_icm_head, tsm_icm_join_grad) at their shape
limits, against the float64 restatement (tests/icm_restatement.py, pinned to the reference by tests/test_icm_restatement.py).

Inputs sit on a lattice of eighths, exact in float32.  Bars: values rounded once from float64 (mse, the gradients, the two loss
sums): max |hip - ref64| <= 1e-5 max |ref64| per array, the project's bar; the one-hot rows, the shaped rewards (a float32
product and a float32 add of the kernel's own mse), untouched rewards, the zeros the formula gives and the joined gradient: bit
for bit."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

from icm_restatement import head, join_grad, x_fwd  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _rel(name, got, ref, bar=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), float(np.finfo(np.float32).tiny))
    ratio = float(np.abs(got - ref).max()) / (bar * scale)
    print(f"PARITY {name}: max |hip - ref64| / (1e-5 max |ref64|) = {ratio:.3g}")
    assert ratio <= 1.0, (name, ratio)


def inputs(R, Fd, A, seed=0):
    rs = np.random.RandomState(1000 * R + 10 * Fd + A + seed)
    lat = lambda *s: (rs.randint(-24, 25, s) / 8.0).astype(np.float32)  # noqa: E731
    return dict(phi=lat(2 * R, Fd), phi2_hat=lat(R, Fd), act_hat=lat(R, A), act=rs.randint(0, A, R).astype(np.int64),
                rew=lat(R))


def run_head(i, w=0.2, s=0.7, scale=0.125, rew_io=None, ids=None):
    out = ops.icm_head(_d(i["phi2_hat"]), _d(i["phi"]), _d(i["act_hat"]), _d(i["act"]), scale, w, s, rew_io=rew_io, ids=ids)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("A", [1, 64])
@pytest.mark.parametrize("Fd", [1, 15, 17, 512])
@pytest.mark.parametrize("R", [1, 15, 16, 17, 37])
def test_head_and_rows_at_shape_limits(R, Fd, A):
    i = inputs(R, Fd, A)
    rew = _d(i["rew"])
    o = run_head(i, rew_io=rew)
    h = head(i["phi2_hat"], i["phi"][1::2], i["act_hat"], i["act"], 0.2, 0.7)
    for k in ("mse", "d_phi2_hat", "d_phi2_fwd", "d_act_hat"):
        if np.abs(h[k]).max() > 0:
            _rel(f"R{R} F{Fd} A{A} {k}", o[k], h[k])
        else:
            assert not o[k].any(), k
    assert np.array_equal(o["d_phi2_fwd"], -o["d_phi2_hat"])
    nb = -(-R // 16)
    assert o["partial"].shape == (2 * nb,)
    _rel("sum mse", [o["partial"][0::2].sum()], [h["mse"].sum()])
    if A > 1:
        _rel("sum ce", [o["partial"][1::2].sum()], [h["ce"].sum()])
    else:
        assert np.abs(o["partial"][1::2]).max() == 0.0   # one action: softmax = 1, ce = 0, d_act_hat = 0
    for b in range(nb):   # per workgroup: its 16 rows
        _rel(f"partial of workgroup {b}", [o["partial"][2 * b]], [h["mse"][16 * b:16 * b + 16].sum()])
    # the shaped reward: a float32 product and a float32 add of the kernel's own mse
    assert np.array_equal(rew.cpu().numpy(), i["rew"] + o["mse"] * np.float32(0.125))
    out2 = torch.empty(2, device=DEV)
    ops.qmix_finalize(_d(o["partial"]), R, out2)
    _rel("finalize forward loss", out2.cpu().numpy()[:1], [h["forward_loss"]])
    if A > 1:
        _rel("finalize inverse loss", out2.cpu().numpy()[1:], [h["inverse_loss"]])
    else:
        assert out2.cpu().numpy()[1] == 0.0
    x = ops.icm_rows(_d(i["phi"]), _d(i["act"]), A).cpu().numpy()
    assert np.array_equal(x, x_fwd(i["phi"], i["act"], A))


def test_head_reward_ids_and_null():
    R, Fd, A = 37, 17, 5
    i = inputs(R, Fd, A)
    base = run_head(i)   # rew_io null: nothing stored, everything else as with it
    rs = np.random.RandomState(4)
    store0 = (rs.randint(-24, 25, 3 * R + 5) / 8.0).astype(np.float32)
    add = base["mse"] * np.float32(0.125)
    for name, ids in (("permutation", rs.permutation(R).astype(np.int64)), ("strided subset", (3 * np.arange(R) + 2).astype(np.int64))):
        store = _d(store0)
        o = run_head(i, rew_io=store, ids=_d(ids))
        want = store0.copy()
        want[ids] = store0[ids] + add
        assert np.array_equal(store.cpu().numpy(), want), name   # touched entries exact, untouched ones bit-identical
        for k in base:
            assert np.array_equal(o[k], base[k], equal_nan=True), (name, k)
    with pytest.raises(ValueError, match="ids"):
        ops.icm_head(_d(i["phi2_hat"]), _d(i["phi"]), _d(i["act_hat"]), _d(i["act"]), 0.1, 0.2, 0.7, ids=_d(np.arange(R)))


def test_head_poisons_an_action_outside_the_range():
    R, Fd, A = 37, 7, 5
    i = inputs(R, Fd, A)
    good = run_head(i, rew_io=None)
    bad = dict(i, act=i["act"].copy())
    bad["act"][18] = A
    rew = _d(i["rew"])
    o = run_head(bad, rew_io=rew)
    assert np.isnan(o["mse"][18]) and np.isnan(rew.cpu().numpy()[18])
    assert np.isnan(o["partial"][2]) and np.isnan(o["partial"][3]) and np.isfinite(np.delete(o["partial"], [2, 3])).all()
    for k in ("d_phi2_hat", "d_phi2_fwd", "d_act_hat"):
        assert not o[k][18].any(), k
    keep = np.arange(R) != 18
    for k in ("mse", "d_phi2_hat", "d_phi2_fwd", "d_act_hat"):
        assert np.array_equal(o[k][keep], good[k][keep]), k
    x = ops.icm_rows(_d(i["phi"]), _d(np.where(keep, i["act"], -1)), A).cpu().numpy()
    assert not x[18, Fd:].any() and np.array_equal(x, x_fwd(i["phi"], np.where(keep, i["act"], -1), A))


@pytest.mark.parametrize("w,s,zero", [(0.0, 0.7, ("d_phi2_hat", "d_phi2_fwd")), (1.0, 0.7, ("d_act_hat",)),
                                      (0.2, 0.0, ("d_phi2_hat", "d_phi2_fwd", "d_act_hat")), (0.3, 1.0, ())])
def test_loss_weights_at_zero_and_one(w, s, zero):
    i = inputs(37, 17, 5)
    o = run_head(i, w=w, s=s)
    h = head(i["phi2_hat"], i["phi"][1::2], i["act_hat"], i["act"], w, s)
    for k in ("d_phi2_hat", "d_phi2_fwd", "d_act_hat"):
        if k in zero:
            assert not o[k].any(), k
        else:
            _rel(f"w{w} s{s} {k}", o[k], h[k])
    _rel("mse", o["mse"], h["mse"])


@pytest.mark.parametrize("R,Fd", [(1, 1), (17, 15), (37, 512)])
def test_join_grad_is_the_written_float32_sums(R, Fd):
    rs = np.random.RandomState(R + Fd)
    a, b, c = (rs.standard_normal(s).astype(np.float32) for s in ((R, Fd), (R, 2 * Fd), (R, Fd)))
    want = join_grad(a, b, c)
    out = torch.empty(2 * R, Fd, device=DEV)
    got = ops.icm_join_grad(_d(a), _d(b), _d(c), out=out)
    assert np.array_equal(got.cpu().numpy(), want)
    g_inv = _d(b)
    got = ops.icm_join_grad(_d(a), g_inv, _d(c))   # in place: the inverse model's input gradient IS the feature net's d_out
    assert got.data_ptr() == g_inv.data_ptr() and np.array_equal(got.cpu().numpy(), want)


def test_bounds_are_refused_before_any_launch():
    i = inputs(4, 3, 2)
    with pytest.raises(ValueError, match="feature_dim = 513"):
        ops.icm_rows(torch.zeros(8, 513, device=DEV), _d(i["act"]), 2)
    with pytest.raises(ValueError, match="n_act = 65"):
        ops.icm_rows(_d(i["phi"]), _d(i["act"]), 65)
    with pytest.raises(ValueError, match="interleaved"):
        ops.icm_rows(torch.zeros(7, 3, device=DEV), _d(i["act"]), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.icm_rows(torch.zeros(8, 3), torch.zeros(4, dtype=torch.int64), 2)
