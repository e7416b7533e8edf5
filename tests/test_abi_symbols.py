"""CPU checks of the drop-in boundary: the C-ABI library loads here (no GPU) and exports every
symbol declared in include/tsmarl.h; argument validation that needs no device works."""
import ctypes as C
import os
import re

import pytest

from tianshou_marl_amd import _abi, _build


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _abi.load()


def test_every_header_symbol_is_exported_and_bound(lib):
    declared = _abi.header_symbols()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in tsmarl.h but not exported"
        assert name in _abi.SIGNATURES, f"{name} declared in tsmarl.h but not bound in _abi.SIGNATURES"
    for name in _abi.SIGNATURES:
        assert name in declared, f"{name} bound but not declared in tsmarl.h"


def test_abi_version_and_sizes(lib):
    # one number in three places: the header, the library, the binding (bumped with every signature / layout change)
    import re

    hdr = int(re.search(r"#define\s+TSM_ABI_VERSION\s+(\d+)", open(_abi.HEADER_PATH).read()).group(1))
    assert lib.tsm_abi_version() == hdr == _abi.ABI_VERSION == 4
    # ctypes mirrors of the header's structs keep their layout
    import ctypes

    assert ctypes.sizeof(_abi.tsm_slab_seg) == 64 and ctypes.sizeof(_abi.tsm_ppo_cfg) == 48
    assert lib.tsm_vrb_state_bytes(4, 1) == (6 * 4 + 4 + 1) * 8
    assert lib.tsm_vrb_state_bytes(8, 3) == (6 * 8 + 24 + 1) * 8
    assert lib.tsm_ppo_loss_partial_elems(0) == 0
    assert lib.tsm_ppo_loss_partial_elems(257) == 8


def c_layout_mismatches(structs, header_path, workdir):
    """The struct layouts the C compiler gives `header_path` against the ctypes classes `structs` {name: class}: a list of
    (what, ctypes figure, compiler's figure), empty when they agree.  `structs` supplies only the struct and field names that
    the generated program asks about; sizeof and every offsetof / member size are the compiler's."""
    import shutil
    import subprocess

    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{header_path}"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));'
                  for f, _ in cls._fields_]
    lines += ["    return 0;", "}"]
    cc = shutil.which("cc")
    src = os.path.join(workdir, "layout.c" if cc else "layout.cpp")   # no cc: hipcc compiles it as plain host C++
    exe = os.path.join(workdir, "layout")
    with open(src, "w") as f:
        f.write("\n".join(lines) + "\n")
    subprocess.run([cc or _build.HIPCC, src, "-o", exe], check=True, capture_output=True, text=True)
    seen = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        what, *figures = line.split()
        seen[what] = tuple(int(x) for x in figures)
    want = {}
    for name, cls in structs.items():
        want[name] = (C.sizeof(cls),)
        want.update({f"{name}.{f}": (getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_})
    return [(what, want.get(what), seen.get(what)) for what in sorted(set(want) | set(seen)) if want.get(what) != seen.get(what)]


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """Every ctypes struct that _abi derives from tsmarl.h has the size, and every field the offset and size, that the host
    C compiler gives the same header: a dropped, reordered or mistyped field moves what follows it or the total."""
    structs = {k: v for k, v in vars(_abi).items() if isinstance(v, type) and issubclass(v, C.Structure)}
    sizes = {"tsm_field": 24, "tsm_slab_reduce": 40, "tsm_noisy_layer": 40, "tsm_mlp_desc": 44, "tsm_ppo_cfg": 48,
             "tsm_slab_seg": 64, "tsm_gather_field": 72, "tsm_mpe_cfg": 88, "tsm_mpe_tag_cfg": 112, "tsm_qmix_agents": 320,
             "tsm_maddpg_agents": 320, "tsm_rollout_desc": 368, "tsm_rollout_tag_desc": 416, "tsm_noisy_net": 992}
    assert {k: C.sizeof(v) for k, v in structs.items()} == sizes   # ABI version 4: a change here bumps TSM_ABI_VERSION
    assert len(_abi.tsm_rollout_desc._fields_) == len(_abi.tsm_rollout_tag_desc._fields_) == 40
    assert c_layout_mismatches(structs, _abi.HEADER_PATH, str(tmp_path)) == []


def test_binding_follows_the_mapping_rules():
    """One or more literal cases per rule of _abi's docstring, read off the header by eye."""
    sig, p, i32, i64, f64 = _abi.SIGNATURES, C.c_void_p, C.c_int32, C.c_int64, C.c_double
    # scalars
    assert sig["tsm_ctde_td_head"][1][5] is C.c_float and sig["tsm_ctde_td_head"][0] is C.c_int
    assert sig["tsm_c51_head"][1][:15] == [p] * 10 + [i64, i32, i32, f64, f64] and len(sig["tsm_c51_head"][1]) == 20
    assert sig["tsm_categorical_sample"][1] == [p, i64, i32, C.c_uint64, C.c_uint64, p, C.c_int, p, p, p]
    assert sig["tsm_abi_version"] == (C.c_int, [])
    # char * as return and as argument
    assert sig["tsm_last_error"] == (C.c_char_p, [])
    assert sig["tsm_kernel_option_set"][1] == [C.c_char_p, i32]
    # a pointer to a struct of the header; every other pointer, `const float *const *` included
    assert sig["tsm_mlp_param_count"] == (i64, [C.POINTER(_abi.tsm_mlp_desc)])
    assert sig["tsm_adam_step_segs"][1][:3] == [p, C.POINTER(_abi.tsm_slab_seg), i32]
    assert sig["tsm_global_state"][1][0] is p and sig["tsm_kernel_option_get"][1] == [C.c_char_p, p]
    # members: any pointer is c_void_p, arrays by literal, macro and macro + 1, several declarators per line, nesting by value
    fields = {name: dict(cls._fields_) for name, cls in vars(_abi).items() if isinstance(cls, type) and issubclass(cls, C.Structure)}
    assert fields["tsm_qmix_agents"]["q"] is p * 8 and fields["tsm_rollout_tag_desc"]["params"] is p * 2
    assert fields["tsm_mlp_desc"]["dims"] is i32 * 9
    assert fields["tsm_rollout_tag_desc"]["offset"] is C.c_uint64 * 2 and fields["tsm_rollout_tag_desc"]["env"] is _abi.tsm_mpe_tag_cfg
    assert fields["tsm_noisy_net"]["layer"] is _abi.tsm_noisy_layer * 24 and fields["tsm_rollout_desc"]["done_ctr"] is p
    assert [f for f, _ in _abi.tsm_slab_seg._fields_] == ["slabs", "offset", "n", "stride", "n_slab", "frag_k1", "scale_dev",
                                                          "frag_image", "frag_kj", "_pad"]
    # constants come from their #defines and the enum
    assert (_abi.MAX_GATHER_FIELDS, _abi.DQN_ROWS_PER_BLOCK, _abi.NOISY_MAX_LAYERS, _abi.QMIX_MAX_AGENTS) == (12, 256, 24, 8)
    assert (_abi.TSM_OK, _abi.TSM_ERR_INVALID, _abi.TSM_ERR_HIP, _abi.TSM_ERR_MALFORMED_BUFFER, _abi.TSM_ERR_UNSUPPORTED) == (0, 1, 2, 3, 4)
    # value, not status: by return type, or an int that TSM_VALUE marks (13 marked + 24 by type today)
    assert {"tsm_abi_version", "tsm_vrb_state_bytes", "tsm_last_error", "tsm_ppo_update_grid"} <= _abi._NO_STATUS
    assert not {"tsm_vrb_init", "tsm_dqn_check", "tsm_distq_check"} & _abi._NO_STATUS and len(_abi._NO_STATUS) == 37


def test_header_reader_refuses_what_it_does_not_support(tmp_path):
    ok = _abi.read_header("#define TSM_N 3\ntypedef struct { const float *a, *b[TSM_N + 1]; int32_t n; } tsm_s;\n"
                          "TSM_VALUE int tsm_f(const tsm_s *s, void **out);\nint64_t tsm_g(void);")
    assert ok.signatures == {"tsm_f": (C.c_int, [C.POINTER(ok.structs["tsm_s"]), C.c_void_p]), "tsm_g": (C.c_int64, [])}
    assert ok.structs["tsm_s"]._fields_ == [("a", C.c_void_p), ("b", C.c_void_p * 4), ("n", C.c_int32)]
    assert ok.no_status == {"tsm_f", "tsm_g"} and ok.defines == {"TSM_N": 3}
    for bad in ("int tsm_f(void (*callback)(int), int n);",                      # a function-pointer parameter
                "typedef struct { int32_t a[TSM_UNKNOWN]; } tsm_s;",             # an array length it cannot resolve
                "#define TSM_N 2\ntypedef struct { int32_t a[2 * TSM_N]; } tsm_s;",
                "typedef struct { unsigned n; } tsm_s;",                         # a type outside the scalar list
                "int tsm_f(long n);",
                "#define TSM_N (1 << 4)"):
        with pytest.raises(ValueError, match="tsmarl.h reader"):
            _abi.read_header(bad)
    # no header: ImportError naming the path (a copy of the module in a tree without include/)
    import importlib.util
    import shutil

    os.makedirs(tmp_path / "pkg")
    shutil.copy(_abi.__file__, tmp_path / "pkg" / "_abi.py")
    spec = importlib.util.spec_from_file_location("_abi_without_header", tmp_path / "pkg" / "_abi.py")
    with pytest.raises(ImportError, match=re.escape(str(tmp_path / "include" / "tsmarl.h"))):
        spec.loader.exec_module(importlib.util.module_from_spec(spec))


def test_argument_validation_maps_to_python_errors(lib):
    # invalid sizes are rejected on the host before any device work (no GPU needed)
    with pytest.raises(ValueError):
        _abi.call("tsm_gae_lanes", None, None, None, None, None, 1, -1, 4, 1, None, None, 0.99, 0.95, 1.0,
                  None, None, None)
    with pytest.raises(ValueError):  # n_lane not a multiple of lanes_per_env
        _abi.call("tsm_gae_lanes", 1, 1, 1, 1, 1, 1, 5, 7, 3, None, None, 0.99, 0.95, 1.0, 1, 1, None)
    with pytest.raises(ValueError):
        _abi.call("tsm_vrb_init", None, 0, 5, 1, None)
    cfg = _abi.tsm_ppo_cfg(0.2, 0.5, 0.5, 0.01, 0, 1)  # dual_clip must be > 1 (ppo.py:124-126)
    with pytest.raises(ValueError, match="Dual-clip"):
        _abi.call("tsm_ppo_loss_fwd_bwd", 1, 1, 1, 1, 1, 1, None, None, 0, 8, 5, 1, C.byref(cfg), 1, 1, 1, None)


def test_kernel_options_are_host_state_with_validated_values(lib):
    """tsm_kernel_option_get / _set need no device: every option ops.KERNEL_OPTIONS names exists, starts at its rule value 0
    (no TSM_* override in the test environment), takes its documented values and refuses others and unknown names."""
    from tianshou_marl_amd import ops

    assert set(ops.KERNEL_OPTIONS) == {"actor_tile", "split_bf16", "generic_kernels", "rollout_form"}
    for name, good, bad in [("actor_tile", (32, 64, 0), 48), ("split_bf16", (1, 0), 2), ("generic_kernels", (1, 0), 128),
                            ("rollout_form", (1, 2, 0), 3)]:
        if os.environ.get("TSM_" + name.upper()) is None:
            assert ops.kernel_option(name) == 0
        for v in good:
            ops.set_kernel_option(name, v)
            assert ops.kernel_option(name) == v
        with pytest.raises(ValueError):
            ops.set_kernel_option(name, bad)
        assert ops.kernel_option(name) == 0
    with pytest.raises(ValueError, match="unknown option"):
        ops.kernel_option("no_such_option")
    with ops.kernel_override(rollout_form=2, actor_tile=64):
        assert ops.kernel_options() == (64, 0, 0, 2)
    assert ops.kernel_options() == (0, 0, 0, 0)


def test_new_host_entry_points_validate_without_a_device(lib):
    """tsm_gather_fields / tsm_gae_set_scan_workspace check their arguments on the host; the Python wrappers refuse CPU tensors
    (no CPU fallback) and do not register a scan workspace without a GPU."""
    import torch

    from tianshou_marl_amd import ops

    assert lib.tsm_gae_scan_workspace_bytes() >= 8 + 128 * 4 + 128 * 16
    with pytest.raises(ValueError):
        _abi.call("tsm_gae_set_scan_workspace", 1, 8)           # too small
    _abi.call("tsm_gae_set_scan_workspace", None, 0)            # withdrawing is always allowed
    fields = (_abi.tsm_gather_field * 1)(_abi.tsm_gather_field(None, None, 4, 0, 0, 1, 0, 1, 0, 0, 0))
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_gather_fields", fields, 1, None)
    with pytest.raises(ValueError, match="1..12 fields"):
        _abi.call("tsm_gather_fields", fields, 13, None)
    fields[0] = _abi.tsm_gather_field(1, 1, 6, 2, 2, 1, 0, 1, 0, 0, 0)   # n_rows != T * E
    with pytest.raises(ValueError, match="T \\* E"):
        _abi.call("tsm_gather_fields", fields, 1, None)
    fields[0] = _abi.tsm_gather_field(1, 1, 4, 0, 0, 1, 0, 1, 0, 1, 0)   # f32 -> i32 is not a conversion it does
    with pytest.raises(ValueError, match="f32 sources"):
        _abi.call("tsm_gather_fields", fields, 1, None)
    with pytest.raises(ValueError, match="device tensors"):
        ops.gather_fields([(torch.zeros(4), torch.zeros(4))])
    if not torch.cuda.is_available():
        assert ops.ensure_scan_workspace("cpu") is False


def test_product_has_no_oracle_import():
    """The product package must never import the oracle (test infrastructure)."""
    root = os.path.dirname(os.path.abspath(_abi.__file__))
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f
                assert "ref_shim" not in src, f


def test_ops_refuse_cpu_tensors():
    import torch

    from tianshou_marl_amd import ops

    x = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gae_lanes(x, x, x, x.to(torch.uint8), x.to(torch.uint8))


# Entry points that no test names, itself or through the ops function that calls it, with the test that reaches each one
# through a class.  Queries, one-time set-up and exports for outside callers only: no numerical kernel belongs here.
_REACHED_THROUGH_CLASSES = {
    # env and rollout kernels behind DeviceSimpleSpreadVectorEnv / DeviceSimpleTagVectorEnv / Collector
    "tsm_mpe_spread_reset": "test_gpu_pipeline.py", "tsm_mpe_spread_step": "test_gpu_pipeline.py",
    "tsm_mpe_tag_obs_dim": "test_gpu_tag.py", "tsm_mpe_tag_reset": "test_gpu_tag.py", "tsm_mpe_tag_step": "test_gpu_tag.py",
    "tsm_rollout_spread": "test_gpu_rollout.py", "tsm_rollout_spread_actor": "test_gpu_rollout.py",
    "tsm_rollout_tag": "test_gpu_tag.py",
    # the peer-memory gradient sum behind parallel.GradSync
    **{f"tsm_p2p_{s}": "test_gpu_parallel.py" for s in ("ipc_handle_bytes", "create", "export", "import", "all_reduce",
                                                        "adam_step", "set_timeout", "handshake", "failed", "error_async",
                                                        "destroy")},
    # support / grid / workspace queries and one-time set-up of the rows kernels
    "tsm_ppo_actor_rows_supported": "test_gpu_generic_ppo.py", "tsm_ppo_rows_init": "test_gpu_generic_ppo.py",
    "tsm_ppo_critic_rows_grid": "test_gpu_generic_ppo.py", "tsm_critic_rows_forward_supported": "test_gpu_generic_ppo.py",
    "tsm_critic_rows_init": "test_gpu_generic_ppo.py", "tsm_critic_rows_grad_grid": "test_gpu_generic_ppo.py",
    "tsm_critic_rows_dw1_chunks": "test_gpu_generic_ppo.py",
    # exports for ctypes callers and the runtime's own error path
    **{f"tsm_mem_{s}": "test_abi_symbols.py" for s in ("alloc", "free", "h2d", "d2h", "set")},
    "tsm_stream_sync": "test_abi_symbols.py", "tsm_stream_abort_capture": "test_abi_symbols.py",
}


def _ops_callers():
    """{C-ABI name: names of the ops functions / classes whose body calls it}."""
    import ast
    import re

    from tianshou_marl_amd import ops

    src = open(ops.__file__).read()
    callers = {}
    for node in ast.parse(src).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            for name in re.findall(r'"(tsm_\w+)"', ast.get_source_segment(src, node)):
                callers.setdefault(name, set()).add(node.name)
    return callers


def test_every_entry_point_is_named_by_a_test():
    """Every name in _abi.SIGNATURES appears in some tests/test_*.py, itself or as the ops function that calls it;
    the only other way through is the explicit list above.  A new entry point without a test fails here."""
    import glob
    import re

    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "test_*.py")))
    text = "\n".join(open(f).read() for f in files)
    text = re.sub(r"(?s)\n_REACHED_THROUGH_CLASSES = \{.*?\n\}\n", "\n", text)  # the list itself does not count
    callers = _ops_callers()

    def named(word):
        return re.search(r"\b" + re.escape(word) + r"\b", text) is not None

    untested = [s for s in _abi.SIGNATURES if not named(s) and not any(named(c) for c in callers.get(s, ()))]
    missing = sorted(set(untested) - set(_REACHED_THROUGH_CLASSES))
    assert not missing, f"C-ABI entry points that no test names (add a test, or list the test that reaches them): {missing}"
    stale = sorted(set(_REACHED_THROUGH_CLASSES) - set(untested))
    assert not stale, f"listed as reached through classes, but named by a test or no longer bound (drop them): {stale}"
    for name, test_file in _REACHED_THROUGH_CLASSES.items():
        assert os.path.exists(os.path.join(here, test_file)), (name, test_file)
