"""GPU tests (`-m gpu`) of the FQF kernels at their shape limits, as test_gpu_offpolicy_shapes.py has them for the other
heads: n_act = 64, num_fractions = 64, embedding_dim = 512, at B = 1 and at one row past a multiple of
TSM_IQN_ROWS_PER_BLOCK.  The reference is the float64 restatement (tests/fqf_restatement.py) on the same float32 inputs, under
test_gpu_distq.py's `_bar` with test_gpu_offpolicy_shapes.py's e_ref = max |restatement(float32) - restatement(float64)| at
that shape.  The inputs are seeded; the test asserts that their greedy actions are clear-cut (top-2 gap of q above 1e-4), so that
float32 cannot pick another a*."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

from fqf_restatement import fqf_head, fqf_values, fractions_of, propose  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_gpu_dqn import _d  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops

A, N, H = 64, 64, 512


def _rows():
    return [1, _abi.IQN_ROWS_PER_BLOCK + 1]


def _e(r32, r64):
    return float(np.abs(np.asarray(r32, np.float64) - np.asarray(r64, np.float64)).max())


@pytest.mark.parametrize("k", [0, 1])
def test_proposal_at_the_limits(k):
    B = _rows()[k]
    rs = np.random.RandomState(50 + B)
    f = rs.standard_normal((B, H)).astype(np.float32)
    Wf = rs.uniform(-0.05, 0.05, (N, H)).astype(np.float32)
    bf, d_logits = rs.uniform(-0.1, 0.1, N).astype(np.float32), rs.standard_normal((B, N)).astype(np.float32)
    r, r32 = propose(f, Wf, bf, True, d_logits), propose(f, Wf, bf, True, d_logits, dtype=torch.float32)
    got = ops.fqf_propose(_d(f), _d(Wf), _d(bf), relu_f=True)
    for name, x in zip(("taus", "tau_hats", "logp", "entropies"), got):
        _bar(f"limits B={B} {name}", x.cpu().numpy(), r[name], _e(r32[name], r[name]))
    slabs = ops.fqf_propose_backward(_d(d_logits), _d(f), 2, relu_f=True)
    total = slabs.double().sum(0).cpu().numpy()
    _bar(f"limits B={B} dWf", total[:N * H].reshape(N, H), r["dWf"], _e(r32["dWf"], r["dWf"]))
    _bar(f"limits B={B} dbf", total[N * H:], r["dbf"], _e(r32["dbf"], r["dbf"]))


@pytest.mark.parametrize("k", [0, 1])
def test_values_and_head_at_the_limits(k):
    B = _rows()[k]
    rs = np.random.RandomState(70 + B)
    out, on, tg = (rs.standard_normal((B, N, A)).astype(np.float32) for _ in range(3))
    out_tau = rs.standard_normal((B, N - 1, A)).astype(np.float32)
    xf, xf_next = (rs.standard_normal((B, N)).astype(np.float32) for _ in range(2))
    act = rs.randint(0, A, B).astype(np.int64)
    act[0] = A - 1
    mc, gpow = rs.standard_normal(B).astype(np.float32), np.full(B, 0.99 ** 2, np.float32)
    vmask, weight = np.ones(B, bool), (0.5 + rs.rand(B)).astype(np.float32)
    mask = rs.rand(B, A) > 0.5
    mask[:, 0] = True
    fr, fr_next = fractions_of(xf), fractions_of(xf_next)
    for m in (None, mask):
        top = np.sort(fqf_values(on, fr_next["taus"])["q"] if m is None else np.where(m, fqf_values(on, fr_next["taus"])["q"], -np.inf), 1)
        assert (top[:, -1] - top[:, -2]).min() > 1e-4
    q_next = ops.fqf_values(_d(on), _d(fr_next["taus"], torch.float32), A)
    rq = fqf_values(on, fr_next["taus"])["q"]
    _bar(f"limits B={B} q", q_next.cpu().numpy(), rq, _e(fqf_values(on, fr_next["taus"], dtype=torch.float32)["q"], rq))
    args = (out, out_tau, xf, on, fr_next["taus"], tg, mask, act, mc, gpow, vmask, weight, 0.01)
    r, r32 = fqf_head(*args), fqf_head(*args, dtype=torch.float32)
    assert np.array_equal(r["a_star"], r32["a_star"])
    h = ops.fqf_head(_d(out), _d(out_tau), q_next, _d(tg), _d(fr["taus"], torch.float32), _d(fr["tau_hats"], torch.float32), _d(fr["logp"], torch.float32),
                     _d(fr["entropies"], torch.float32), _d(act), _d(mc), _d(gpow), _d(vmask), mask_next=_d(mask), weight=_d(weight),
                     ent_coef=0.01)
    slot = torch.zeros(4, device=DEV)
    ops.qmix_finalize(h["partial"], B, slot[:2])
    ops.qmix_finalize(h["partial_frac"], B, slot[2:])
    got = slot.cpu().numpy()
    assert h["partial"].numel() == 2 * (k + 1)
    dout = h["d_out"].cpu().numpy()
    off = dout.copy()
    off[np.arange(B), :, act] = 0.0
    assert not off.any() and dout[np.arange(B), :, act].any()
    for name, x in (("returns", h["returns"].cpu().numpy()), ("prio", h["prio"].cpu().numpy()), ("d_out", dout),
                    ("d_logits", h["d_logits"].cpu().numpy()), ("quantile_loss", [got[0]]), ("fraction_loss", [got[2]]),
                    ("entropy_loss", [got[3]])):
        _bar(f"limits B={B} {name}", x, r[name], _e(r32[name], r[name]))
