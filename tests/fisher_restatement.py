"""Float64 restatement of csrc/fisher.hip's row-wise heads and conjugate-gradient loop, in plain numpy on the CPU: what
tests/test_gpu_fisher_shapes.py holds the kernels to, itself held to torch autograd and torch.distributions by
tests/test_fisher_restatement.py.  It imports nothing of the package.

  fisher_head    the closed form of the kernel header: p = softmax(logits), u = p (t - <p, t>) / B, per row (<p, t^2> - <p, t>^2) / B
  kl_surrogate   per-row KL(old || new) in torch's Categorical convention (a term is 0 where p_old = 0, inf where p_new = 0 < p_old),
                 the per-row actor-loss term and d (mean loss) / d logits_new; an action outside [0, A) gives a NaN term and a zero
                 gradient row
  cg_solve       the reference's loop (npg.py:202-224) on the diagonal operator z = diag * p + damping * p
  cg_inputs      the synthetic system of period CG_CHUNK; cg_reference its float64 and float32 runs, conditioned
  kl_rows        the rows of the head tests, ordinary or with one documented edge in the last row"""
import functools

import numpy as np

ROWS_PER_BLOCK = 128   # TSM_FISHER_ROWS_PER_BLOCK: rows of one workgroup of the heads, hence of one partial
CG_CHUNK = 1024        # TSM_CG_CHUNK: elements of one workgroup of the CG kernels
CG_DAMPING, CG_TOL, CG_STEPS, CG_SEED = 0.1, 1e-3, 6, 3
ZERO_P = 1000.0        # a logit this far below its row's maximum has probability exactly 0 in float64 (exp underflows at -745.2)
EDGES = ("p_old_zero", "p_new_zero", "act_low", "act_high")


def block_sums(rows):
    """Per-row values [B, ...] -> [ceil(B / ROWS_PER_BLOCK), ...]: the sums over the rows [128 k, 128 (k + 1))."""
    rows = np.asarray(rows, np.float64)
    return np.stack([rows[k:k + ROWS_PER_BLOCK].sum(0) for k in range(0, rows.shape[0], ROWS_PER_BLOCK)])


def _categorical(logits):
    """-> (p, the normalised logits), float64, as Categorical(logits=..)."""
    t = np.asarray(logits, np.float64)
    t = t - t.max(-1, keepdims=True)
    e = np.exp(t)
    s = e.sum(-1, keepdims=True)
    return e / s, t - np.log(s)


def fisher_head(logits, t):
    """-> (u [B, A], the per-row terms of v^T F v [B], p [B, A])."""
    p, _ = _categorical(logits)
    t = np.asarray(t, np.float64)
    B = p.shape[0]
    pt = (p * t).sum(-1, keepdims=True)
    ptt = (p * t * t).sum(-1)
    return p * (t - pt) / B, (ptt - pt[:, 0] * pt[:, 0]) / B, p


def kl_surrogate(lo, ln, act, logp_old, adv, kind):
    """-> (KL(old || new) per row [B], the loss term per row [B], d (sum of the terms / B) / d ln [B, A]); kind "ratio":
    the term is -exp(logp_new - logp_old) adv, "logp": -logp_new adv."""
    assert kind in ("ratio", "logp")
    po, llo = _categorical(lo)
    pn, lln = _categorical(ln)
    B, A = pn.shape
    kl = np.where(po > 0, np.where(pn == 0, np.inf, po * (llo - lln)), 0.0).sum(-1)
    act = np.asarray(act, np.int64)
    ok = (act >= 0) & (act < A)
    a = np.where(ok, act, 0)
    logp = np.where(ok, lln[np.arange(B), a], np.nan)
    adv = np.asarray(adv, np.float64)
    with np.errstate(invalid="ignore"):
        ratio = np.exp(logp - np.asarray(logp_old, np.float64)) if kind == "ratio" else np.ones(B)
        term = -(ratio * adv) if kind == "ratio" else -(logp * adv)
    w = np.where(ok, -(np.where(ok, ratio, 0.0) * adv) / B, 0.0)
    onehot = (np.arange(A)[None, :] == a[:, None]) & ok[:, None]
    return kl, term, w[:, None] * (onehot.astype(np.float64) - pn)


def kl_rows(B, A, seed, edge=None):
    """float32 / int32 inputs of the KL / surrogate head -> dict(lo, ln, act, logp_old, adv); logp_old is the old policy's own
    log-probability of the action, rounded to float32.  `edge` (one of EDGES) rewrites the LAST row: "p_old_zero" puts old action
    1 ZERO_P below the maximum of the row's other logits while p_new stays positive there,
    "p_new_zero" does so to new action A - 1 and takes action 0, "act_low" / "act_high" set the action to -1 / A.  All logits
    are finite."""
    rs = np.random.RandomState(seed)
    lo, ln = (rs.standard_normal((B, A)).astype(np.float32) for _ in range(2))
    act = rs.randint(0, A, B).astype(np.int32)
    adv = rs.standard_normal(B).astype(np.float32)
    if edge == "p_old_zero":
        assert A >= 2
        lo[-1, 1] = np.float32(np.delete(lo[-1], 1).max() - ZERO_P)
    elif edge == "p_new_zero":
        assert A >= 2
        ln[-1, A - 1] = np.float32(ln[-1, :A - 1].max() - ZERO_P)
        act[-1] = 0
    elif edge is not None:
        assert edge in EDGES, edge
    good = act.copy()
    if edge in ("act_low", "act_high"):
        act[-1] = -1 if edge == "act_low" else A
    logp_old = _categorical(lo)[1][np.arange(B), good].astype(np.float32)
    return dict(lo=lo, ln=ln, act=act, logp_old=logp_old, adv=adv)


def cg_solve(g_slabs, diag, damping, tol, nsteps, dtype):
    """npg.py:202-224 with _MVP(p) = diag * p + damping * p, every figure in `dtype`; g is the sum of the rows of g_slabs.
    -> (x, r, p, [new_rdotr of every iteration run])."""
    dt = np.dtype(dtype).type
    g = np.asarray(g_slabs, dtype).reshape(-1, np.shape(g_slabs)[-1]).sum(0, dtype=dtype)
    diag, damping = np.asarray(diag, dtype), dt(damping)
    x, r, p, rr_all = np.zeros_like(g), g.copy(), g.copy(), []
    rdotr = r.dot(r)
    for _ in range(nsteps):
        z = diag * p + damping * p
        alpha = rdotr / p.dot(z)
        x += alpha * p
        r -= alpha * z
        new_rdotr = r.dot(r)
        rr_all.append(float(new_rdotr))
        if new_rdotr < tol:
            break
        p = r + new_rdotr / rdotr * p
        rdotr = new_rdotr
    assert x.dtype == r.dtype == p.dtype == np.dtype(dtype)
    return x, r, p, rr_all


def cg_inputs(n, seed=CG_SEED):
    """-> (g, diag) float32 [n], both of period CG_CHUNK: g standard normal, diag drawn from {1, 2, 4}.  Three distinct eigenvalues:
    CG converges at its third iteration, and every workgroup of the kernels sees the same numbers."""
    rs = np.random.RandomState(seed)
    g = rs.standard_normal(CG_CHUNK).astype(np.float32)
    diag = rs.choice(np.array([1.0, 2.0, 4.0], np.float32), CG_CHUNK)
    return np.resize(g, n), np.resize(diag, n)


@functools.lru_cache(maxsize=None)
def cg_reference(n, seed=CG_SEED):
    """The float64 and the float32 run of cg_solve on cg_inputs(n) -> (r64, r32, g, diag): dicts of x, r, p, rr and `r_scale` =
    max |g| (r ends near 0: it is compared on the scale it started from).  Asserts the condition the GPU test rests on -- no
    decision of either run is marginal: every new r.r lies outside [1e-6, 1] around CG_TOL = 1e-3, both runs stop at the same
    iteration, the third (the first for n = 1), well inside CG_STEPS."""
    g, diag = cg_inputs(n, seed)
    runs = []
    for dt in (np.float64, np.float32):
        x, r, p, rr = cg_solve(g[None], diag, CG_DAMPING, CG_TOL, CG_STEPS, dt)
        runs.append(dict(x=x, r=r, p=p, rr=rr, r_scale=float(np.abs(g).max())))
    r64, r32 = runs
    for run in runs:
        assert all(not 1e-6 <= v <= 1.0 for v in run["rr"]), (n, run["rr"])
    assert len(r64["rr"]) == len(r32["rr"]) == (1 if n == 1 else 3), (n, r64["rr"], r32["rr"])
    assert r64["rr"][-1] < 1e-6 and r32["rr"][-1] < 1e-6 and all(v > 1.0 for v in r64["rr"][:-1] + r32["rr"][:-1])
    return r64, r32, g, diag
