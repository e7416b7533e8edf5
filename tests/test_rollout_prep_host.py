"""Host-side checks (no GPU) of the rollout launch's ride-along: the binding derived from tsmarl.h has its entry points, the
descriptor is the one the plain rollout entry point has always taken, the launcher's rule is callable on the host and declines where no CU
is idle."""
import ctypes as C

import pytest

from tianshou_marl_amd import _abi


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


def _extra(tiles, n_cu, n, n_perm):
    out = C.c_int32(-1)
    _abi.call("tsm_rollout_prep_extra", tiles, n_cu, n, n_perm, C.byref(out))
    return out.value


def test_binding_has_the_ride_along_entry_points(lib):
    sig, p, i32, i64, u64 = _abi.SIGNATURES, C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    assert sig["tsm_rollout_spread_prep"] == (C.c_int, [C.POINTER(_abi.tsm_rollout_desc), i64, i32, u64, p, i64, i32, i64, p, i32,
                                                         p, p])
    assert sig["tsm_rollout_prep_extra"] == (C.c_int, [i64, i32, i64, i32, p])
    # the request travels as arguments: the descriptor keeps its layout, so every caller of the plain entry point is untouched
    assert [f for f, _ in _abi.tsm_rollout_desc._fields_][-2:] == ["offset_inc", "done_ctr"]


def test_rule_gives_idle_cus_only(lib):
    # the headline launch: 205 eight-wave workgroups on 256 CUs, 3 permutations of 25 600 rows -> every idle CU
    assert _extra(205, 256, 25600, 3) == 51
    # never more workgroups than give each of their 512 threads an entry, never more than 64
    assert _extra(3, 256, 75, 1) == 1 and _extra(3, 256, 1200, 3) == 8 and _extra(3, 256, 25600, 6) == 64
    assert _extra(3, 256, 513, 1) == 2
    # no idle CU, or nothing to draw: declined
    assert _extra(256, 256, 25600, 3) == 0 and _extra(300, 256, 25600, 3) == 0 and _extra(3, 3, 1200, 3) == 0
    assert _extra(205, 256, 0, 3) == 0 and _extra(205, 256, 25600, 0) == 0
    with pytest.raises(ValueError):
        _extra(-1, 256, 75, 1)


def test_launcher_checks_its_request_on_the_host(lib):
    """A zeroed descriptor fails the plain launcher's own checks whether or not a request rides along; a request is checked first
    where it is malformed."""
    d, taken = _abi.tsm_rollout_desc(), C.c_int32(7)
    with pytest.raises(ValueError):   # no request: the plain entry point's path and message
        _abi.call("tsm_rollout_spread_prep", C.byref(d), 0, 0, 0, None, 1, 1, 0, None, 0, C.byref(taken), None)
    assert taken.value == 0
    with pytest.raises(ValueError, match="device counter"):
        _abi.call("tsm_rollout_spread_prep", C.byref(d), 75, 1, 0, None, 1, 1, 0, 1, 0, C.byref(taken), None)
    with pytest.raises(ValueError, match="perm_n"):
        _abi.call("tsm_rollout_spread_prep", C.byref(d), 1 << 30, 1, 0, 1, 1, 1, 0, 1, 0, C.byref(taken), None)
    with pytest.raises(ValueError, match="taken_out"):
        _abi.call("tsm_rollout_spread_prep", C.byref(d), 75, 1, 0, 1, 1, 1, 0, 1, 0, None, None)
