"""GPU tests (`-m gpu`) of the host checks in front of the launches of ops.py, at the smallest shapes that show them:

* a caller's `out` is written in place or refused -- never copied: the entries that used to fill a contiguous copy of a strided
  `out` and hand the caller's tensor back unwritten now raise before any launch, and a contiguous `out` holds the bits of the
  `out=None` result;
* the weight gradients of `ens_mlp_backward`, `iqn_embed_backward` and `fqf_propose_backward` land inside `slabs` or the call
  is refused: a window of NaN-filled joint slabs is written and nothing around it, a window one float short is refused.

Every refusal is raised in Python before a launch, and every launch that runs writes inside its tensor."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")

if torch.cuda.is_available():
    from tianshou_marl_amd import ops

R, S, F, E, DIMS, B = 3, 2, 4, 2, [3, 4, 1], 5


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _ens():
    desc = ops.mlp_desc(DIMS, "relu")
    params = _rand(ops.ens_mlp_param_count(desc, E), seed=1) * 0.5
    x, d_out = _rand(B, DIMS[0], seed=2), _rand(E, B, DIMS[-1], seed=3)
    _, acts = ops.ens_mlp_forward(desc, E, params, x)
    return desc, params, x, acts, d_out


def _out_cases():
    """name -> (call(out), the out's shape, its dtype)"""
    desc, params, x, acts, d_out = _ens()
    phi, act = _rand(2 * R, F, seed=4), torch.tensor([0, 2, 1], device=DEV)
    mu, sigma = [_rand(E, 2, seed=5), _rand(E, 2, seed=6)], torch.full((1,), 0.3, device=DEV)
    return {
        "iqn_taus": (lambda out: ops.iqn_taus(R, S, 11, DEV, offset=5, out=out), (R, S), torch.float32),
        "icm_rows": (lambda out: ops.icm_rows(phi, act, 3, out=out), (R, F + 3), torch.float32),
        "maddpg_act": (lambda out: ops.maddpg_act(mu, sigma, 7, offset=2, out=out), (E * 2, 2), torch.float32),
        "ens_mlp_input_grad": (lambda out: ops.ens_mlp_input_grad(desc, E, params, x, acts, d_out, 0, 3, out=out), (B, 3),
                               torch.float32),
        "random_permutations": (lambda out: ops.random_permutations(5, 2, 13, counter=3, out=out, device=DEV), (2, 5), torch.int64),
    }


@pytest.mark.parametrize("name", ["iqn_taus", "icm_rows", "maddpg_act", "ens_mlp_input_grad", "random_permutations"])
def test_a_strided_out_is_refused_and_a_contiguous_one_is_written_in_place(name):
    call, shape, dtype = _out_cases()[name]
    want = call(None)
    assert tuple(want.shape) == shape and want.dtype == dtype
    backing = torch.full(shape[::-1], 77, dtype=dtype, device=DEV)
    with pytest.raises(ValueError, match="out must be"):
        call(backing.t())                                    # the right shape, transposed strides: used to fill a copy
    torch.cuda.synchronize()
    assert (backing == 77).all()                             # nothing was launched on it
    with pytest.raises(ValueError, match="out must be"):
        call(torch.zeros(shape, dtype=torch.float64, device=DEV))
    out = torch.full(shape, 77, dtype=dtype, device=DEV)
    assert call(out) is out
    assert torch.equal(out, want)


def _window_check(run, extent: int, n_split: int = 2):
    """`run(slabs, pitch)` must write columns [8, 8 + extent) of every row of a NaN-filled [n_split, extent + 16] with the bits
    of its own fresh slabs and leave the rest NaN; the same window one float short is refused before a launch."""
    want = run(None, 0)
    assert tuple(want.shape) == (n_split, extent)
    big = torch.full((n_split, extent + 16), NAN, device=DEV)
    pitch = big.shape[1]
    run(big[:, 8:], pitch)
    assert torch.equal(big[:, 8:8 + extent], want)
    assert big[:, :8].isnan().all() and big[:, 8 + extent:].isnan().all()
    short = torch.full((n_split * pitch,), NAN, device=DEV)[8:8 + (n_split - 1) * pitch + extent - 1]
    with pytest.raises(ValueError, match="slabs reach"):
        run(short, pitch)
    torch.cuda.synchronize()
    assert short.isnan().all()


def test_ens_mlp_backward_writes_inside_its_slabs_or_refuses():
    desc, params, x, acts, d_out = _ens()
    P = params.numel()
    run = lambda slabs, pitch, n_split=2: ops.ens_mlp_backward(desc, E, params, x, acts, d_out, n_split, slabs=slabs,  # noqa: E731
                                                               slab_stride=pitch)
    _window_check(run, P)
    with pytest.raises(ValueError, match="slabs reach"):
        run(torch.zeros(2 * P - 1, device=DEV), 0)           # one float short
    with pytest.raises(ValueError, match="n_split 3 exceeds the 2 rows of slabs"):
        run(torch.zeros(2, P, device=DEV), 0, n_split=3)
    with pytest.raises(ValueError, match=f"slab_stride {P - 1} smaller than the parameter count"):
        run(torch.zeros(2, P, device=DEV), P - 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        run(torch.zeros(2, P), 0)
    wide = run(None, P + 7)                                  # fresh slabs at the caller's pitch, as mlp_backward makes them
    assert tuple(wide.shape) == (2, P + 7)
    assert torch.equal(wide[:, :P], run(None, 0))


def test_iqn_embed_backward_writes_inside_its_slabs_or_refuses():
    H, C = 16, 4
    f, taus, We, be = _rand(R, H, seed=1), torch.rand(R, S, generator=torch.Generator().manual_seed(2)).to(DEV), \
        _rand(H, C, seed=3) * 0.5, _rand(H, seed=4) * 0.5
    d_e = _rand(R * S, H, seed=5)
    _, phi = ops.iqn_embed_forward(f, taus, We, be)
    _window_check(lambda slabs, pitch: ops.iqn_embed_backward(d_e, f, phi, taus, We, be, 2, slabs=slabs, slab_stride=pitch)[1],
                  H * C + H)


def test_fqf_propose_backward_writes_inside_its_slabs_or_refuses():
    H, N = 16, 3                                             # (three fractions: the fewest the FQF kernels take)
    f, d_logits = _rand(R, H, seed=1), _rand(R, N, seed=2)
    _window_check(lambda slabs, pitch: ops.fqf_propose_backward(d_logits, f, 2, slabs=slabs, slab_stride=pitch), N * H + N)
