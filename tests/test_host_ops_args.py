"""The three argument helpers every entry of ops.py shares -- `_out` (caller-supplied output buffers), `_slab_dest` (where weight
gradients land) and `_philox` (the counter arguments) -- on CPU tensors.  Their size, stride and dtype rules do not depend on
where a tensor lives; the one device requirement is `_dev_only`, which the fixture below takes out."""
import pytest

torch = pytest.importorskip("torch")

from tianshou_marl_amd import ops  # noqa: E402

F32 = torch.float32


@pytest.fixture(autouse=True)
def any_device(monkeypatch):
    monkeypatch.setattr(ops, "_dev_only", lambda name, *tensors: None)


# ---- _out ------------------------------------------------------------------------------------------------------------------
def test_out_returns_the_callers_tensor_itself_or_a_fresh_one():
    buf = torch.zeros(3, 2)
    assert ops._out("f", buf, (3, 2), F32, "cpu") is buf
    fresh = ops._out("f", None, (3, 2), torch.int64, "cpu")
    assert tuple(fresh.shape) == (3, 2) and fresh.dtype == torch.int64
    flat = torch.zeros(7)
    assert ops._out("f", flat, (3, 2), F32, "cpu", size="min") is flat        # at least 6 entries, any shape
    assert ops._out("f", flat[:6], (3, 2), F32, "cpu", size="numel") is not None   # exactly 6 entries, any shape


def test_out_refuses_what_a_launch_could_not_write_in_place():
    with pytest.raises(ValueError, match=r"f: out must be \[3, 2\], contiguous"):
        ops._out("f", torch.zeros(2, 3).t(), (3, 2), F32, "cpu")              # a transposed view of the right shape
    with pytest.raises(ValueError, match="out must be"):
        ops._out("f", torch.zeros(3, 2, dtype=torch.float64), (3, 2), F32, "cpu")
    with pytest.raises(ValueError, match="out must be"):
        ops._out("f", torch.zeros(2, 3), (3, 2), F32, "cpu")                  # as many entries, another shape
    with pytest.raises(ValueError, match="res must be at least 6 entries"):
        ops._out("f", torch.zeros(5), (3, 2), F32, "cpu", "res", "min")
    with pytest.raises(ValueError, match="out must be 6 entries"):
        ops._out("f", torch.zeros(7), (3, 2), F32, "cpu", size="numel")
    with pytest.raises(ValueError, match="contiguous"):
        ops._out("f", torch.zeros(6, 2)[:, 0], (3, 2), F32, "cpu", size="min")   # enough entries, strided


def test_out_requires_a_device_tensor(monkeypatch):
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops._out("f", torch.zeros(3, 2), (3, 2), F32, "cpu")


# ---- _slab_dest ------------------------------------------------------------------------------------------------------------
N_SPLIT, EXTENT = 3, 10


def _dest(slabs, n_split=N_SPLIT, pitch=EXTENT, rows=5):
    return ops._slab_dest("g", slabs, n_split, rows, pitch, EXTENT, "cpu")


def test_slab_dest_accepts_every_layout_whose_writes_stay_inside():
    n, fresh, pitch = _dest(None, pitch=EXTENT + 7)
    assert (n, pitch, tuple(fresh.shape), fresh.dtype) == (N_SPLIT, EXTENT + 7, (N_SPLIT, EXTENT + 7), F32)
    n, fresh, _ = _dest(None, n_split=0, rows=600)                             # n_split <= 0: the default for the rows
    assert n == ops.mlp_n_split(600) == fresh.shape[0] == 3
    exact = torch.zeros(N_SPLIT, EXTENT)
    assert _dest(exact)[1] is exact
    big = torch.zeros(N_SPLIT, EXTENT + 6)
    window = big[:, 6:]                                                        # a column window of wider joint slabs
    assert _dest(window, pitch=big.shape[1])[1] is window
    flat = torch.zeros(N_SPLIT * EXTENT)
    assert _dest(flat)[1] is flat
    assert _dest(exact, n_split=2)[0] == 2                                     # fewer slabs than rows


def test_slab_dest_refuses_every_layout_a_write_would_leave():
    exact = torch.zeros(N_SPLIT, EXTENT)
    with pytest.raises(ValueError, match="n_split 4 exceeds the 3 rows of slabs"):
        _dest(exact, n_split=4)
    with pytest.raises(ValueError, match=f"slab_stride {EXTENT - 1} smaller than the parameter count"):
        _dest(exact, pitch=EXTENT - 1)
    with pytest.raises(ValueError, match=f"slab_stride {EXTENT - 1} smaller than the parameter count"):
        _dest(None, pitch=EXTENT - 1)
    big = torch.zeros(N_SPLIT, EXTENT + 6)
    with pytest.raises(ValueError, match="slabs reach"):
        _dest(big[:, 7:], pitch=big.shape[1])                                  # the window ends one float short
    with pytest.raises(ValueError, match="slabs reach"):
        _dest(exact.view(-1)[1:])                                              # a flat view shifted by one
    with pytest.raises(ValueError, match="slabs reach"):
        _dest(exact, pitch=EXTENT + 1)
    with pytest.raises(ValueError, match="slabs must be"):
        _dest(torch.zeros(N_SPLIT, 2 * EXTENT)[:, ::2])                        # non-unit last stride
    with pytest.raises(ValueError, match="slabs must be"):
        _dest(exact.double())
    with pytest.raises(ValueError, match="slabs must be"):
        _dest(torch.zeros(0, EXTENT))
    with pytest.raises(ValueError, match=r"n_split 65536 outside \[1, 65535\]"):
        _dest(None, n_split=65536)


def test_slab_dest_requires_a_device_tensor(monkeypatch):
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="no CPU path"):
        _dest(torch.zeros(N_SPLIT, EXTENT))


# ---- _philox ---------------------------------------------------------------------------------------------------------------
def test_philox_wraps_seed_and_offset_modulo_two_to_the_64():
    assert ops._philox("h", 5, 7, None) == (5, 7, None)
    assert ops._philox("h", -1, -2, None) == (2**64 - 1, 2**64 - 2, None)
    assert ops._philox("h", 2**64 + 3, 2**65 + 9, None) == (3, 9, None)
    assert ops._philox("h", (1 << 40) ^ 0x5DEECE66D, 3 << 32, None) == ((1 << 40) ^ 0x5DEECE66D, 3 << 32, None)


def test_philox_requires_the_device_counter_in_device_memory(monkeypatch):
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops._philox("h", 0, 0, torch.zeros(1, dtype=torch.int64))
