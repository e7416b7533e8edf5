"""CPU tests of GAIL's host side: the bounds of tsm_gail_check, the refusals of every tsm_gail_* entry before any launch (no
device is needed for them), the constructor's signature against the recorded reference signature, the refusal it makes before
anything is built, and the CPU tensors the ops refuse."""
import dataclasses
import inspect
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "gail.npz")

import gail_restatement as gr  # noqa: E402
from tianshou_marl_amd import _abi, ops  # noqa: E402
from tianshou_marl_amd.algorithm import GAIL, GailTrainingStats  # noqa: E402
from tianshou_marl_amd.algorithm.optim import AdamOptimizerFactory  # noqa: E402
from tianshou_marl_amd.data.stats import A2CTrainingStats  # noqa: E402
from tianshou_marl_amd.utils.net import FlatMLP, ref_layer_keys  # noqa: E402

POSITIONAL = ("POSITIONAL_OR_KEYWORD", "POSITIONAL_ONLY")
P = 4096   # any non-null address: every refusal below comes before a launch


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def test_gail_check_bounds():
    for D, A in ((1, 1), (18, 5), (4096, 64)):
        ops.gail_check(D, A)
        gr.check(D, A)
    for D, A, what in ((0, 5, "obs_dim = 0 below 1"), (-3, 5, "obs_dim = -3 below 1"), (18, 0, r"n_act = 0 outside \[1, 64\]"),
                       (18, 65, r"n_act = 65 outside \[1, 64\]")):
        with pytest.raises(ValueError, match="tsm_gail_check: " + what):
            ops.gail_check(D, A)
        with pytest.raises(ValueError):
            gr.check(D, A)
    assert _abi.GAIL_ROWS_PER_BLOCK == gr.ROWS_PER_BLOCK
    for name in ("gail_draw", "gail_rows", "gail_reward", "gail_head", "gail_finalize"):
        assert callable(getattr(ops, name))


def test_every_entry_refuses_null_pointers_and_sizes_naming_the_limit():
    call = _abi.call
    # tsm_gail_draw(valid, n_valid, n_agent, R, seed, counter, counter_dev, ids_out, stream): valid and counter_dev may be null
    with pytest.raises(ValueError, match="tsm_gail_draw: null pointer"):
        call("tsm_gail_draw", None, 3, 2, 5, 0, 0, None, None, None)
    for n_valid, n_agent in ((0, 1), (3, 0), (2 ** 31, 2), (2 ** 32, 1)):
        with pytest.raises(ValueError, match=r"tsm_gail_draw: n_valid n_agent = .* outside \[1, 2\^32\)"):
            call("tsm_gail_draw", None, n_valid, n_agent, 5, 0, 0, None, P, None)
    for R in (0, 2 ** 31):
        with pytest.raises(ValueError, match=r"tsm_gail_draw: R = \d+ outside \[1, 2\^31\)"):
            call("tsm_gail_draw", None, 3, 2, R, 0, 0, None, P, None)
    # tsm_gail_rows(obs, act, ids, R, obs_dim, n_act, x_out, stream): ids may be null
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        with pytest.raises(ValueError, match="tsm_gail_rows: null pointer"):
            call("tsm_gail_rows", args[0], args[1], None, 5, 3, 2, args[2], None)
    with pytest.raises(ValueError, match=r"tsm_gail_rows: R = 429496730 outside \[1, 429496729\]: R \(obs_dim \+ n_act\) stays below 2\^31"):
        call("tsm_gail_rows", P, P, None, 429496730, 3, 2, P, None)
    with pytest.raises(ValueError, match=r"tsm_gail_rows: R = 0 outside"):
        call("tsm_gail_rows", P, P, None, 0, 3, 2, P, None)
    with pytest.raises(ValueError, match=r"tsm_gail_rows: n_act = 65 outside \[1, 64\]"):
        call("tsm_gail_rows", P, P, None, 5, 3, 65, P, None)
    with pytest.raises(ValueError, match="tsm_gail_rows: obs_dim = 0 below 1"):
        call("tsm_gail_rows", P, P, None, 5, 0, 2, P, None)
    # tsm_gail_reward(logits, ids, R, rew_io, stream)
    for a, b in ((None, P), (P, None)):
        with pytest.raises(ValueError, match="tsm_gail_reward: null pointer"):
            call("tsm_gail_reward", a, None, 5, b, None)
    with pytest.raises(ValueError, match=r"tsm_gail_reward: R = 2147483648 outside \[1, 2\^31\)"):
        call("tsm_gail_reward", P, None, 2 ** 31, P, None)
    # tsm_gail_head(logits, Rp, Re, d_logits, partial, stream)
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        with pytest.raises(ValueError, match="tsm_gail_head: null pointer"):
            call("tsm_gail_head", args[0], 5, 5, args[1], args[2], None)
    for Rp, Re in ((0, 5), (5, 0)):
        with pytest.raises(ValueError, match=f"tsm_gail_head: Rp = {Rp}, Re = {Re}: each at least 1"):
            call("tsm_gail_head", P, Rp, Re, P, P, None)
    with pytest.raises(ValueError, match=r"tsm_gail_head: Rp \+ Re = 2147483648 outside \[1, 2\^31\)"):
        call("tsm_gail_head", P, 2 ** 30, 2 ** 30, P, P, None)
    # tsm_gail_finalize(partial, n_blocks, Rp, Re, out, stream)
    for a, b in ((None, P), (P, None)):
        with pytest.raises(ValueError, match="tsm_gail_finalize: null pointer"):
            call("tsm_gail_finalize", a, 1, 1, 1, b, None)
    for nb, Rp, Re in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError, match="tsm_gail_finalize: n_blocks = .* each at least 1"):
            call("tsm_gail_finalize", P, nb, Rp, Re, P, None)


def test_cpu_tensors_are_refused():
    obs, act = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32)
    for fn, args in ((ops.gail_rows, (obs, act, 2)), (ops.gail_reward, (torch.zeros(4), torch.zeros(4))),
                     (ops.gail_head, (torch.zeros(4), 2)), (ops.gail_finalize, (torch.zeros(4, dtype=torch.float64), 2, 2)),
                     (ops.gail_draw, (torch.zeros(3, dtype=torch.int64), 3, 1, 4, 0))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(*args)


def test_signatures_accept_the_reference_call_shape(g):
    """The rule of test_api_surface.py: every reference parameter is accepted under its name and kind with the same default;
    what the mirror adds has a default."""
    for cls in (GAIL, GailTrainingStats):
        ref = [(s.split("=", 1)[0], s.split("=", 1)[1], k) for s, k in zip(g[f"sig_{cls.__name__}"], g[f"sigkind_{cls.__name__}"])]
        ours = [q for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        by_name = {q.name: q for q in ours}
        var_kw = any(q.kind is inspect.Parameter.VAR_KEYWORD for q in ours)
        for name, default, kind in ref:
            if kind.startswith("VAR_"):
                continue
            assert name in by_name or var_kw, f"{cls.__name__}: `{name}` is not accepted"
            o = by_name[name]
            assert o.kind.name == kind or kind == "KEYWORD_ONLY", (cls.__name__, name)
            if default != "<required>":
                assert o.default is not inspect.Parameter.empty and repr(o.default) == default, (cls.__name__, name)
        names = {r[0] for r in ref}
        for o in ours:
            if o.name not in names and o.kind.name in POSITIONAL + ("KEYWORD_ONLY",):
                assert o.default is not inspect.Parameter.empty, f"{cls.__name__}: extra parameter `{o.name}` has no default"
    assert [f.name for f in dataclasses.fields(GailTrainingStats)][-3:] == ["disc_loss", "acc_pi", "acc_exp"]
    assert issubclass(GailTrainingStats, A2CTrainingStats)
    ref_names = [s.split("=")[0] for s in g["sig_GAIL"]]
    assert ref_names[:7] == ["policy", "critic", "optim", "expert_buffer", "disc_net", "disc_optim", "disc_update_num"]


def test_discriminator_exports_under_the_reference_mlp_keys(g):
    dims = [int(d) for d in g["disc_dims"]]
    disc = FlatMLP(dims, device="cpu", seed=0)
    sd = disc.export_layers(ref_layer_keys(disc.n_layers, "seq"), prefix="model.")
    assert list(sd.keys()) == list(g["sd_keys"])
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == list(g["sd_shapes"])
    assert disc.flat.numel() == g["up_init_disc"].size


def test_constructor_refuses_a_discriminator_without_a_hip_path():
    """Checked before anything is built, so it needs no device; the refusals that need a PPO are in tests/test_gpu_gail.py."""
    with pytest.raises(TypeError, match="no autograd fallback"):
        GAIL(net=None, expert_buffer=None, disc_net=torch.nn.Linear(23, 1), disc_optim=AdamOptimizerFactory(lr=1e-3))
    with pytest.raises(TypeError, match="expert_buffer"):
        GAIL(disc_net=FlatMLP([23, 32, 1], device="cpu", seed=0), disc_optim=None)   # required, as in the reference
