"""CPU tests of the NPG / TRPO yardstick (tests/fisher_restatement.py): the closed-form Fisher head against the reference's own
double backward of mean KL(old || new) (npg.py:162-166, 195-200; torch autograd in float64 on bare logits), the KL / surrogate
head against torch.distributions and autograd -- on ordinary rows and on the rows with the documented edges -- the CG loop
against the closed-form solution of its diagonal system, and the condition that makes the GPU test's decisions safe."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fisher_restatement as fr  # noqa: E402

Cat, kl_div = torch.distributions.Categorical, torch.distributions.kl_divergence
CG_NS = (1, 1023, 1024, 1025, 65 * 1024 + 1)   # test_gpu_fisher_shapes.py runs the kernels at the same lengths


def close(got, ref, what, rel=1e-12):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.abs(got - ref).max() <= rel * np.abs(ref).max(), (what, np.abs(got - ref).max(), np.abs(ref).max())


@pytest.mark.parametrize("A", [1, 9, 64])
def test_fisher_head_is_the_double_backward_of_mean_kl(A):
    B = 5
    rs = np.random.RandomState(A)
    logits32, t32 = (rs.standard_normal((B, A)).astype(np.float32) for _ in range(2))
    u, vfv, p = fr.fisher_head(logits32, t32)
    lg = torch.tensor(logits32, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(t32, dtype=torch.float64)
    kl = kl_div(Cat(logits=lg.detach()), Cat(logits=lg)).mean()
    kg = torch.autograd.grad(kl, lg, create_graph=True)[0]
    Fv = torch.autograd.grad((kg * t).sum(), lg)[0]
    close(u, Fv.numpy(), "u")
    close(vfv.sum(), (t * Fv).sum().item(), "v F v")
    close(vfv, (t * Fv).sum(-1).numpy(), "v F v per row")
    close(p, torch.softmax(lg.detach(), -1).numpy(), "p")
    if A == 1:
        assert not u.any() and not vfv.any()


def test_block_sums_are_over_128_rows():
    rows = np.arange(257 * 2, dtype=np.float64).reshape(257, 2)
    got = fr.block_sums(rows)
    assert got.shape == (3, 2) and np.array_equal(got[0], rows[:128].sum(0)) and np.array_equal(got[1], rows[128:256].sum(0))
    assert np.array_equal(got[2], rows[256]) and fr.block_sums(np.ones(128)).tolist() == [128.0]


def _torch_kl_and_grad(c, kind, rows=None):
    """torch's per-row KL and, over `rows` (default: all), the per-row loss terms and the gradient of their sum / B."""
    B = c["lo"].shape[0]
    rows = np.arange(B) if rows is None else rows
    ln = torch.tensor(c["ln"], dtype=torch.float64, requires_grad=True)
    new = Cat(logits=ln)
    kl = kl_div(Cat(logits=torch.tensor(c["lo"], dtype=torch.float64)), new)
    logp = new.logits[torch.as_tensor(rows), torch.as_tensor(c["act"][rows].astype(np.int64))]
    adv, lpo = (torch.tensor(c[k][rows], dtype=torch.float64) for k in ("adv", "logp_old"))
    term = -((logp - lpo).exp() * adv) if kind == "ratio" else -(logp * adv)
    return kl.detach().numpy(), term.detach().numpy(), torch.autograd.grad(term.sum() / B, ln)[0].numpy()


@pytest.mark.parametrize("A,B", [(1, 3), (5, 50), (33, 129), (64, 7)])
@pytest.mark.parametrize("kind", ["ratio", "logp"])
def test_kl_surrogate_matches_torch_on_ordinary_rows(A, B, kind):
    c = fr.kl_rows(B, A, seed=5)
    kl, term, d = fr.kl_surrogate(kind=kind, **c)
    kl_t, term_t, d_t = _torch_kl_and_grad(c, kind)
    for got, ref, what in ((kl, kl_t, "kl"), (term, term_t, "term"), (d, d_t, "d_logits")):
        close(got, ref, what)
    if A == 1:
        assert not kl.any() and not d.any()


@pytest.mark.parametrize("A", [5, 33])
@pytest.mark.parametrize("kind", ["ratio", "logp"])
@pytest.mark.parametrize("edge", fr.EDGES)
def test_kl_surrogate_edge_rows_follow_torch_conventions(A, kind, edge):
    B = 129
    c = fr.kl_rows(B, A, seed=7, edge=edge)
    assert all(np.isfinite(c[k]).all() for k in ("lo", "ln", "logp_old", "adv"))
    kl, term, d = fr.kl_surrogate(kind=kind, **c)
    bad_act = edge in ("act_low", "act_high")
    kl_t, term_t, d_t = _torch_kl_and_grad(c, kind, np.arange(B - 1) if bad_act else None)
    po, pn = (torch.softmax(torch.tensor(c[k][-1], dtype=torch.float64), -1).numpy() for k in ("lo", "ln"))
    # the row's KL is torch's in every case: finite with a term dropped, +inf, or untouched by the action
    if edge == "p_old_zero":
        assert po[1] == 0.0 and pn[1] > 0.0 and np.isfinite(kl_t[-1])
    if edge == "p_new_zero":
        assert pn[A - 1] == 0.0 and po[A - 1] > 0.0 and kl_t[-1] == np.inf and kl[-1] == np.inf
        close(kl[:-1], kl_t[:-1], "kl")
    else:
        close(kl, kl_t, "kl")
    assert np.isfinite(kl[:-1]).all()
    if bad_act:
        assert np.isnan(term[-1]) and not d[-1].any()
        close(term[:-1], term_t, "term")
    else:
        assert np.isfinite(term).all()
        close(term, term_t, "term")
    assert np.isfinite(d).all()
    close(d, d_t, "d_logits")   # (torch leaves the row it was not given at zero, as the head does)


@pytest.mark.parametrize("n", CG_NS)
def test_cg_solve_reaches_the_closed_form_without_a_marginal_decision(n):
    r64, r32, g, diag = fr.cg_reference(n)     # asserts: every r.r outside [1e-6, 1], both runs of one length
    print(f"n {n}: float64 r.r {r64['rr']}, float32-state r.r {r32['rr']}")
    sol = g.astype(np.float64) / (diag.astype(np.float64) + fr.CG_DAMPING)
    close(r64["x"], sol, "x")
    assert np.abs(r64["r"]).max() <= 1e-12 * r64["r_scale"]
    assert r32["x"].dtype == np.float32 and np.abs(r32["x"] - sol).max() <= 1e-5 * np.abs(sol).max()
    # split into slabs whose sum is exact, the loop sees the same g
    w = np.array([0.5, 0.25, 0.25])[:, None]
    x3, _, _, rr3 = fr.cg_solve(w * g[None].astype(np.float64), diag, fr.CG_DAMPING, fr.CG_TOL, fr.CG_STEPS, np.float64)
    assert np.array_equal(x3, r64["x"]) and rr3 == r64["rr"]
    # homogeneous of degree 1, exactly so for a power of two
    x2, _, _, rr2 = fr.cg_solve(-2.0 * g[None], diag, fr.CG_DAMPING, fr.CG_TOL, fr.CG_STEPS, np.float32)
    assert np.array_equal(x2, -2.0 * r32["x"]) and rr2 == [4.0 * v for v in r32["rr"]]
