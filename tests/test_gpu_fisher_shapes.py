"""GPU tests (`-m gpu`) of csrc/fisher.hip at the shapes where its branches part, against the float64 restatement of
tests/fisher_restatement.py (itself held to torch by tests/test_fisher_restatement.py):

  a. the Fisher and KL / surrogate heads at every group width G = 8, 16, 32, 64 -- n_act on both sides of every `by_group`
     threshold and at both limits; one row, a ragged second workgroup, three workgroups with one row in the last -- each
     workgroup's partial on its own, `run_if` = 0, equal bits from two runs;
  b. the documented row edges of the KL / surrogate head: p_old = 0, p_new = 0 < p_old, an action outside [0, A);
  c. the CG vector kernels alone on a synthetic diagonal system of period TSM_CG_CHUNK: chunk edges, 66 and 130 partials (the
     second and third stride of `sum_partials`), three slabs of a pitch wider than n with NaN in the padding, the `done` flag, the
     frozen state behind it, equal bits in every workgroup, reuse of a finished state;
  d. the tangent forward at the edges of its own loaders (`load_cat`, `a_in` / `b_in` / `one_range`), every layer's block;
  e. `trpo_step_size` on a vector longer than its workgroup.

Bars: the heads and the tangent pass 1e-5 of max |reference| per output (test_gpu_fisher.py's `_close`; a vector of per-workgroup
partials is one output, so each partial is held to 1e-5 of the largest); the CG state max(1e-5, 4 e32) of max |reference|
(test_gpu_npg.py's `_check`), e32 the float32 run of the same reference loop, r on the scale of max |g|; `trpo_step_size`, float64
throughout, 1e-12.  Every figure is printed (pytest -s: profiles/fisher_shapes_parity.txt).

Measured on an MI355X (worst ratio to the bar): heads 0.006, CG state 0.030 (p, n = 1025), tangent pass 0.055 (2-5-16-64-3, layer
3); the 125 tests of the file take 1.7 s."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import fisher_restatement as fr  # noqa: E402
from test_gpu_fisher import _close, _forward  # noqa: E402
from test_gpu_npg import _check  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops
    from tianshou_marl_amd.utils.net import FlatMLP

N_ACTS = (1, 8, 9, 16, 17, 32, 33, 63, 64)
HEAD_ROWS = (1, 129, 257)
KIND = {"ratio": 0, "logp": 1}


def _d(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def test_constants_are_the_kernels():
    assert _abi.FISHER_ROWS_PER_BLOCK == fr.ROWS_PER_BLOCK and _abi.CG_CHUNK == fr.CG_CHUNK


# ---- a. heads at every group width ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", HEAD_ROWS)
@pytest.mark.parametrize("A", N_ACTS)
def test_fisher_head_at_every_group_width(A, B):
    rs = np.random.RandomState(1000 * A + B)
    logits, t = (rs.standard_normal((B, A)).astype(np.float32) for _ in range(2))
    u_ref, vfv, _ = fr.fisher_head(logits, t)
    u, part = ops.fisher_head(_d(logits), _d(t))
    assert part.numel() == ops.fisher_head_blocks(B) == -(-B // 128) and part.dtype == torch.float64
    _close(u, u_ref, f"fisher A {A} B {B} u")
    _close(part, fr.block_sums(vfv), f"fisher A {A} B {B} v F v partials")
    if A == 1:
        assert not u.any() and not part.any()
    u2, part2 = ops.fisher_head(_d(logits), _d(t))
    assert torch.equal(u2, u) and torch.equal(part2, part)


def _kl_head(c, kind, **kw):
    return ops.categorical_kl_surrogate(_d(c["lo"]), _d(c["ln"]), _d(c["act"]), _d(c["logp_old"]), _d(c["adv"]), kind, **kw)


@pytest.mark.parametrize("B", HEAD_ROWS)
@pytest.mark.parametrize("A", N_ACTS)
@pytest.mark.parametrize("kind", ["ratio", "logp"])
def test_kl_surrogate_head_at_every_group_width(kind, A, B):
    c = fr.kl_rows(B, A, seed=1000 * A + B)
    kl, term, d_ref = fr.kl_surrogate(kind=kind, **c)
    part, d_logits = _kl_head(c, kind, want_grad=True)
    assert part.numel() == 2 * ops.fisher_head_blocks(B)
    pairs = part.view(-1, 2)
    what = f"kl head {kind} A {A} B {B}"
    _close(pairs[:, 0], fr.block_sums(kl), what + " kl partials")
    _close(pairs[:, 1], fr.block_sums(term), what + " loss partials")
    _close(d_logits, d_ref, what + " d_logits")
    if A == 1:
        assert not pairs[:, 0].any() and not d_logits.any()
    part2, d2 = _kl_head(c, kind, want_grad=True)
    assert torch.equal(part2, part) and torch.equal(d2, d_logits)
    # run_if = 0: the launch leaves a pre-filled partial alone, at every group width
    fill = torch.arange(1, part.numel() + 1, dtype=torch.float64, device=DEV) * -7.25
    kept = fill.clone()
    _kl_head(c, kind, partial=fill, run_if=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert torch.equal(fill, kept)
    _kl_head(c, kind, partial=fill, run_if=torch.ones(1, dtype=torch.int32, device=DEV))
    assert torch.equal(fill, part)


# ---- b. documented row edges of the KL / surrogate head ------------------------------------------------------------------
@pytest.mark.parametrize("A", [5, 33])
@pytest.mark.parametrize("kind", ["ratio", "logp"])
@pytest.mark.parametrize("edge", fr.EDGES)
def test_kl_surrogate_row_edges(edge, kind, A):
    B = 129   # the special row is row 128: workgroup 1 holds it alone, workgroup 0 stays ordinary
    c = fr.kl_rows(B, A, seed=7, edge=edge)
    assert all(np.isfinite(c[k]).all() for k in ("lo", "ln", "logp_old", "adv"))
    kl, term, d_ref = fr.kl_surrogate(kind=kind, **c)
    part, d_logits = _kl_head(c, kind, want_grad=True)
    pairs = part.view(-1, 2).cpu()
    what = f"kl edge {edge} {kind} A {A}"
    kl_b, term_b = fr.block_sums(kl), fr.block_sums(term)
    _close(pairs[0, 0], kl_b[0], what + " block 0 kl")
    _close(pairs[0, 1], term_b[0], what + " block 0 loss")
    if edge == "p_new_zero":
        assert kl_b[1] == np.inf and pairs[1, 0].item() == float("inf")
    else:
        assert np.isfinite(kl_b[1])
        _close(pairs[1, 0], kl_b[1], what + " block 1 kl")
    if edge in ("act_low", "act_high"):
        assert np.isnan(term_b[1]) and torch.isnan(pairs[1, 1])
        assert not d_logits[128].any() and not d_ref[128].any()
        # workgroup 0 has the bits it has beside an ordinary last row
        good = dict(c, act=np.where(np.arange(B) == 128, 0, c["act"]).astype(np.int32))
        part_g, d_g = _kl_head(good, kind, want_grad=True)
        assert torch.equal(part_g[:2], part[:2]) and torch.equal(d_g[:128], d_logits[:128])
        assert torch.isfinite(part_g).all() and d_g[128].any()
    else:
        assert np.isfinite(term_b[1])
        _close(pairs[1, 1], term_b[1], what + " block 1 loss")
        assert d_ref[128].any()
        _close(d_logits[128], d_ref[128], what + " d_logits of the row")
    assert torch.isfinite(d_logits).all()
    _close(d_logits, d_ref, what + " d_logits")


# ---- c. CG kernels alone on the synthetic diagonal system ----------------------------------------------------------------
CG_NS = (1, 1023, 1024, 1025, 65 * 1024 + 1)
W3 = (0.5, 0.25, 0.25)   # exact in float32: the three slabs add up to the vector without rounding


def _slabs(v, n_slab, pitch):
    """v [n] f32 on the device -> [n_slab, pitch] slabs that sum to v exactly, NaN in the columns past n."""
    n = v.numel()
    out = torch.full((n_slab, pitch), float("nan"), dtype=torch.float32, device=DEV)
    for k in range(n_slab):
        out[k, :n] = v * (W3[k] if n_slab == 3 else 1.0)
    assert torch.equal(out[:, :n].sum(0), v)
    return out


def _head(p, diag, n_head):
    """p F p = sum_i diag_i p_i^2 in float64 as n_head partials over pieces of one length (zeros past n)."""
    q = p.double() ** 2 * diag.double()
    m = -(-q.numel() // n_head)
    return torch.nn.functional.pad(q, (0, m * n_head - q.numel())).view(n_head, m).sum(1)


def _same_in_every_chunk(st, what):
    """g and diag have the period of a workgroup's chunk and alpha / beta are formed from the same partials in one order: every
    chunk of x, r and p has the bits of chunk 0, and so has a shorter last chunk as far as it goes."""
    for k in ("x", "r", "p"):
        v = st[k]
        full = v.numel() // fr.CG_CHUNK
        if full > 1:
            rows = v[:full * fr.CG_CHUNK].view(full, fr.CG_CHUNK)
            assert torch.equal(rows, rows[:1].expand_as(rows)), f"{what}: {k} differs between workgroups"
        tail = v.numel() - full * fr.CG_CHUNK
        if full and tail:
            assert torch.equal(v[full * fr.CG_CHUNK:], v[:tail]), f"{what}: {k} of the last workgroup differs"


def _cg_run(g, diag, n_slab, pitch, n_head, stops_at, what, st=None):
    """CG_STEPS iterations of cg_update / cg_direction on z = diag * p, the flag and the per-workgroup bits checked after each
    -> (the state, its snapshot taken when the flag rose)."""
    n = g.numel()
    st = ops.cg_state(n, DEV) if st is None else st
    ops.cg_init(st, _slabs(g, n_slab, pitch))
    assert int(st["done"].item()) == 0 and st["it"] == 0
    assert torch.equal(st["r"], g) and torch.equal(st["p"], g) and not st["x"].any()
    snap = None
    for it in range(1, fr.CG_STEPS + 1):
        z = diag * st["p"]   # one float32 rounding per element
        ops.cg_update(st, _slabs(z, n_slab, pitch), _head(st["p"], diag, n_head), fr.CG_DAMPING)
        ops.cg_direction(st, fr.CG_TOL)
        assert int(st["done"].item()) == (it >= stops_at), f"{what}: flag after iteration {it}"
        _same_in_every_chunk(st, f"{what} iteration {it}")
        if it == stops_at:
            snap = {k: st[k].clone() for k in ("x", "r", "p", "pp")}
            snap["rr"] = [t.clone() for t in st["rr"]]
    # behind the flag the remaining launches ran and changed nothing
    assert snap is not None and stops_at < fr.CG_STEPS
    for k in ("x", "r", "p", "pp"):
        assert torch.equal(st[k], snap[k]), f"{what}: {k} moved behind the flag"
    assert all(torch.equal(a, b) for a, b in zip(st["rr"], snap["rr"])), f"{what}: r.r moved behind the flag"
    assert all(torch.isfinite(st[k]).all() for k in ("x", "r", "p")), f"{what}: padding was read"
    return st, snap


@pytest.mark.parametrize("n_head", [1, 130])
@pytest.mark.parametrize("n_slab,pad", [(1, 0), (3, 7)])
@pytest.mark.parametrize("n", CG_NS)
def test_cg_kernels_on_the_diagonal_system(n, n_slab, pad, n_head):
    r64, r32, g_np, diag_np = fr.cg_reference(n)   # asserts that no decision of either reference run is marginal
    stops_at = len(r64["rr"])
    what = f"cg n {n} slabs {n_slab} heads {n_head}"
    g, diag = _d(g_np), _d(diag_np)
    st, snap = _cg_run(g, diag, n_slab, n + pad, n_head, stops_at, what)
    assert ops.cg_chunks(n) == -(-n // 1024) == st["pp"].numel()
    _check(what, {k: st[k] for k in ("x", "r", "p")}, r64, r32)
    # two whole runs from fresh states: equal bits
    st2, _ = _cg_run(g, diag, n_slab, n + pad, n_head, stops_at, what + " again")
    assert all(torch.equal(st2[k], st[k]) for k in ("x", "r", "p", "pp", "done"))
    assert all(torch.equal(a, b) for a, b in zip(st2["rr"], st["rr"]))
    # reuse of the finished state: cg_init clears the flag; CG is homogeneous of degree 1 in g and a factor -2 is exact
    x1 = st["x"].clone()
    st3, _ = _cg_run(-2.0 * g, diag, n_slab, n + pad, n_head, stops_at, what + " reused", st=st)
    assert st3 is st and torch.equal(st["x"], -2.0 * x1)


# ---- d. tangent forward at its loader edges ------------------------------------------------------------------------------
def _offsets(dims):
    o, out = 0, []
    for k, n in zip(dims[:-1], dims[1:]):
        out.append(o)
        o += n * k + n
    return out


# (dims, B, act, per layer from layer 1 on: which operands may take the unconditional loader -- None: not claimed)
TANGENT_CASES = [
    # layer 2 (K 16, N 64): W / Vw at float 111, off 16-byte alignment -> guarded B beside a fast A; layer 3 the same at K 64
    ((2, 5, 16, 64, 3), 64, "tanh", {2: ("fast", "guarded"), 3: ("fast", "guarded")}),
    # acts + 65 * 5 is off alignment: a guarded A whose first row block is full, a ragged second row block
    ((2, 5, 16, 64, 3), 65, "relu", {2: ("guarded", "guarded"), 3: ("guarded", "guarded")}),
    # every K a multiple of 16, every offset aligned: two fast row blocks beside a one-row block, a ragged N in the last layer
    ((16, 64, 64, 4), 129, "tanh", {0: ("fast", "fast"), 1: ("fast", "fast"), 2: ("fast", "guarded")}),
    # two column blocks, the second on the fast path; K1 + K = 256 is sixteen double-buffer rounds
    ((16, 128, 5), 64, "relu", {0: ("fast", "fast"), 1: ("fast", "guarded")}),
    # K a multiple of 4, not of 16: the seam of layer 1 falls inside a k tile, on a 16-byte boundary
    ((20, 36, 4), 7, "tanh", {}),
    ((1, 1), 1, "relu", {}),
]


@pytest.mark.parametrize("dims,B,act,claims", TANGENT_CASES, ids=[f"{'-'.join(map(str, c[0]))}_B{c[1]}" for c in TANGENT_CASES])
def test_tangent_forward_at_loader_edges(dims, B, act, claims):
    g = torch.Generator().manual_seed(17)
    net = FlatMLP(dims, act, device=DEV, seed=6)
    x, v = torch.randn(B, dims[0], generator=g), torch.randn(net.flat.numel(), generator=g)
    xd, vd = x.to(DEV), v.to(DEV)
    net.forward(xd, save=True)
    x_saved, acts = net._saved
    jv, t_acts = ops.mlp_tangent_forward(net.desc, net.flat.data, vd, x_saved, acts)

    # the alignment each case is here for, asserted on the pointers the launch was given: a change of the flat layout or of the
    # activation layout fails here and does not quietly stop testing the path
    al = lambda p: p % 16 == 0  # noqa: E731
    offs, a_off = _offsets(dims), 0
    for l, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
        h_in = x_saved.data_ptr() if l == 0 else acts.data_ptr() + 4 * (a_off - B * k)
        t_in = t_acts.data_ptr() + 4 * (a_off - B * k)
        a_fast = k % 4 == 0 and al(h_in) and (l == 0 or al(t_in)) and B >= 64
        b_fast = k % 4 == 0 and al(net.flat.data.data_ptr() + 4 * offs[l]) and al(vd.data_ptr() + 4 * offs[l]) and n >= 64
        if l in claims:
            assert (("fast" if a_fast else "guarded"), ("fast" if b_fast else "guarded")) == claims[l], (l, a_fast, b_fast)
        a_off += B * n
    if dims == (2, 5, 16, 64, 3):
        assert offs[2] == 111 and not al(net.flat.data.data_ptr() + 4 * 111) and al(net.flat.data.data_ptr())
        assert al(acts.data_ptr() + 4 * B * 5) == (B == 64)

    theta, x64, v64 = net.flat.data.cpu().double(), x.double(), v.double()
    a_off = 0
    for l in range(len(dims) - 1):
        sub = dims[:l + 2]
        last = l + 2 == len(dims)
        n_sub = offs[l] + sub[-1] * sub[-2] + sub[-1]
        # (`_forward` leaves the last layer it is given linear: a hidden layer's block is the tangent behind its activation)
        outer = (lambda h: h) if last else torch.tanh if act == "tanh" else torch.relu
        fn = lambda th: outer(_forward(th, sub, act, x64))  # noqa: E731
        _, jv_ref = torch.autograd.functional.jvp(fn, theta[:n_sub], v64[:n_sub])
        got = t_acts[a_off:a_off + B * dims[l + 1]].view(B, dims[l + 1])
        _close(got, jv_ref, f"tangent {'-'.join(map(str, dims))} B {B} {act} layer {l} J v")
        a_off += B * dims[l + 1]
    assert a_off == t_acts.numel() and jv.data_ptr() == got.data_ptr() and tuple(jv.shape) == (B, dims[-1])


# ---- e. trpo_step_size with a long x -------------------------------------------------------------------------------------
def test_trpo_step_size_reduces_a_long_vector():
    rs = np.random.RandomState(4)
    x = rs.standard_normal(1500).astype(np.float32)   # five full strides of the 256 threads and a ragged sixth, four waves
    loss = rs.standard_normal(4)                      # two workgroups' {sum kl, sum loss}
    B, damping, max_kl = 200, 0.1, 0.01
    ls, run = ops.trpo_step_size(_d(np.array([0.125, 0.125])), _d(x), _d(loss), B, damping, max_kl)
    xx = float((x.astype(np.float64) ** 2).sum())
    want = [float(np.sqrt(2 * max_kl / (0.25 + damping * xx))), float(loss[1] + loss[3]) / B]
    got = ls.cpu().tolist()
    print(f"trpo_step_size: step {got[0]!r} want {want[0]!r}, loss {got[1]!r} want {want[1]!r}")
    assert got[:2] == pytest.approx(want, rel=1e-12, abs=0) and got[2:] == [0.0] * (len(got) - 2)
    assert int(run.item()) == 1
