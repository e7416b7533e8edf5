"""GPU tests (`-m gpu`) that hold the optimizer kernels (csrc/adam.hip, csrc/adam_dev.h) to float64 Adam and to the exact slab
tree.  Restatement, case lists and seeded inputs: tests/adam_restatement.py; tests/test_host_adam.py pins the restatement to
torch's float64 Adam (1e-10), checks the preconditions, and shows that each of eight subtly wrong optimizers leaves the bar
used here on these very inputs.

  (a) the slab reduction (ops.reduce_slabs, ops.reduce_slabs_segs, and ops.adam_step seen through m with betas = (0, 0)) is
      bit-equal to `slab_tree_f32` on both sides of every tier's entry condition, for fewer slabs than lanes, with `scale`,
      pitch > n, col0 % 4 != 0 and a `scale_dev`; nothing outside [0, n) of `out` is written;
  (b) one step from a given state: per element |hip - ref64| / u, u = the float32 spacing at the largest magnitude among the
      operands and the result of the quantity's final addition; the maximum over each of p, m, v is at most
      max(1, 2 x the same maximum of torch.optim.Adam in float32 on the CPU from the same state).  coef64=True is held to
      the restatement with 1 - beta rounded once, coef64=False and adam_step_segs to the one with the float32 differences;
      the default path's deviation from the TRUE float64 Adam is printed and held to twice the host test's figure on p and
      v; on m, where that figure is of the size of float32 rounding itself, to max(2 x host, host + the bar of m): the exact
      deviation plus the rounding the kernel is allowed against its own restatement (the triangle inequality);
  (c) clipping: clipped cases under the bar of (b) (and, with weight decay, outside it against the decay-before-clip
      order); a norm below max_norm / 2 gives the bits of the call without clipping; the all-zero gradient; one norm over
      two segments of which one is scaled on the device;
  (d) step_dev / lr_dev give the bits of the host scalars; the parameter image receives exactly the stored bits;
  (e) five steps of FlatAdam.step (both coefficient forms) and FlatAdam.step_segs with a device step count, the bar of (b)
      after every step beside torch's float32 trajectory.
Every launch is made twice and must give the same bits.  Every comparison prints `PARITY adam ...`; the measured figures are
kept in profiles/adam_parity.txt.

The library is built with -ffp-contract=off, so beta * m + omb * g is NOT contracted into an fma: the kernel's roundings are
those of the written expression, and the factor 2 only has to cover torch's different forms (lerp_, addcmul_, its own sum
over the slabs and its own norm).  No discrepancy inherent to the summation tree or to contraction had to be recorded."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import adam_restatement as ar  # noqa: E402
from test_gpu_offpolicy_shapes import _same_bits  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.utils.net import FlatAdam

SENTINEL = -7.25


def _d(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _twice(name, fn):
    """Two launches from the same inputs: the same bits."""
    a, b = fn(), fn()
    _same_bits(name, a, b)
    return a


def _equal_bits(name, got, want):
    got, want = np.ascontiguousarray(_np(got) if torch.is_tensor(got) else got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, name
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    print(f"PARITY adam {name}: {got.size} entries, equal" if not len(bad) else f"PARITY adam {name}: DIFFERS at {bad[:8]} ({len(bad)} entries)")
    assert not len(bad), (name, bad[:8])


def _held(name, got, ref, r32):
    """max |hip - ref64| / u per array against max(1, 2 x torch float32's figure); prints all, then asserts."""
    figs = {k: ar.measure(_np(x).astype(np.float64), ref[k], ref["u"][k]) for k, x in zip("pmv", got)}
    for k, f in figs.items():
        print(f"PARITY adam {name} {k}: max |hip - ref64| / u = {f:.3g}, torch float32 {r32[k]:.3g}, bar {ar.bar_of(r32[k]):.3g}")
    for k, f in figs.items():
        assert f <= ar.bar_of(r32[k]), (name, k, f, r32[k])
    return figs


def _state(d):
    return _d(d["p"]), _d(d["m"]), _d(d["v"])


def _step(c, d, slabs_d, coef64=False, clip=True, **kw):
    p, m, v = _state(d)
    ops.adam_step(p, slabs_d, m, v, c["step"], **ar.hyper(c), max_grad_norm=c.get("max_norm") if clip else None, coef64=coef64, **kw)
    return p, m, v


def _segs_of(slabs_d, scale_dev=None):
    """Two segments over one slab array: a contiguous copy of the first SEG_SPLIT columns, and the rest as a view into the
    whole array (pitch n, col0 = SEG_SPLIT, which is no multiple of the 64-parameter block)."""
    n = slabs_d.shape[1]
    return [(slabs_d[:, :ar.SEG_SPLIT].contiguous(), 0, ar.SEG_SPLIT),
            (slabs_d, ar.SEG_SPLIT, n - ar.SEG_SPLIT, scale_dev, None, ar.SEG_SPLIT)]


def _step_segs(c, d, slabs_d, scale_dev=None, **kw):
    p, m, v = _state(d)
    ops.adam_step_segs(p, _segs_of(slabs_d, scale_dev), m, v, c["step"], **ar.hyper(c), max_grad_norm=c.get("max_norm"), **kw)
    return p, m, v


# ---- (a) the slab reduction: exact ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slab", ar.SLAB_COUNTS)
def test_slab_reduction_is_the_documented_tree(n_slab):
    sc, sd = np.float32(ar.SLAB_SCALE), np.float32(ar.SLAB_SCALE_DEV)
    scale_dev = _d(np.float32([ar.SLAB_SCALE_DEV]))
    for n in ar.SLAB_NS:
        tag = f"slabs {n_slab} x {n}"
        s = ar.slab_inputs(n_slab, n)
        want = ar.slab_tree_f32(s)
        bound = (n_slab - 1) * 2.0 ** -24 * np.abs(s.astype(np.float64)).sum(0)
        assert (np.abs(want.astype(np.float64) - ar.slab_sum_f64(s)) <= bound).all()
        s_d = _d(s)
        got = _twice(tag, lambda: ops.reduce_slabs(s_d))
        _equal_bits(f"{tag} reduce_slabs", got, want)
        assert (np.abs(_np(got).astype(np.float64) - ar.slab_sum_f64(s)) <= bound).all()
        _equal_bits(f"{tag} reduce_slabs scale", _twice(tag, lambda: ops.reduce_slabs(s_d, scale=ar.SLAB_SCALE)), want * sc)

        def through_m():
            p, m, v = (torch.zeros(n, device=DEV) for _ in range(3))
            ops.adam_step(p, s_d, m, v, 1, betas=(0.0, 0.0))
            return m
        _equal_bits(f"{tag} adam_step m", _twice(tag, through_m), want)
        # three segments: pitch > n; col0 = 3 with another slab count; a scale_dev
        wa, wb, wc = ar.slab_inputs(n_slab, n, n + 5, seed=1), ar.slab_inputs(n_slab + 2, 65, 70, seed=2), ar.slab_inputs(n_slab, n, seed=3)
        total = n + 65 + n
        segs = [(_d(wa), 0, n), (_d(wb), n, 65, None, None, 3), (_d(wc), n + 65, n, scale_dev)]
        want_s = np.concatenate([ar.slab_tree_f32(wa, (0, n)) * sc, ar.slab_tree_f32(wb, (3, 65)) * sc, (ar.slab_tree_f32(wc) * sc) * sd,
                                 np.full(9, SENTINEL, np.float32)])

        def segmented():
            out = torch.full((total + 9,), SENTINEL, device=DEV)
            ops.reduce_slabs_segs(segs, total, out=out, scale=ar.SLAB_SCALE)
            return out
        _equal_bits(f"{tag} reduce_slabs_segs (+ 9 sentinels behind)", _twice(tag, segmented), want_s)


# ---- (b) one step from a given state against float64 -------------------------------------------------------------------------
@pytest.mark.parametrize("c", ar.ADAM_CASES, ids=ar.case_id)
def test_one_step_against_float64(c):
    cid = ar.case_id(c)
    d, r32 = ar.inputs(c), ar.ref32_figures(c)
    ref, ref_d = ar.reference(c), ar.reference(c, omb=ar.omb_f32_differenced(c["betas"]))
    slabs_d = _d(d["slabs"])
    fails = []
    runs = (("coef64", lambda: _step(c, d, slabs_d, coef64=True), ref), ("default", lambda: _step(c, d, slabs_d), ref_d),
            ("segs", lambda: _step_segs(c, d, slabs_d), ref_d))
    got = {}
    for name, fn, rf in runs:
        got[name] = _twice(f"{cid} {name}", fn)
        try:
            _held(f"{cid} {name}", got[name], rf, r32)
        except AssertionError as e:   # (print every figure of the case before failing)
            fails.append(e)
    # the declared deviation of the default entry point from the TRUE float64 Adam (csrc/adam_dev.h: 1.f - beta), against the
    # host test's figure for the float32-differenced coefficients in exact arithmetic.  p (the step, which is what the header
    # documents) and v (where the deviation enters) are held to twice the host figure.  On m the host figure is of the size
    # of float32's own rounding, so twice it is no bound for a rounded result; m is held to the larger of that and the
    # triangle inequality's bound: the exact deviation plus the rounding the kernel is allowed against its own restatement.
    host = ar.default_path_deviation(c)
    dev = {k: ar.measure(_np(x).astype(np.float64), ref[k], ref["u"][k]) for k, x in zip("pmv", got["default"])}
    bound = {k: 2.0 * host[k] for k in "pv"}
    bound["m"] = max(2.0 * host["m"], host["m"] + ar.bar_of(r32["m"]))
    for k in "pmv":
        print(f"PARITY adam {cid} default path against the true float64 Adam {k}: {dev[k]:.3g} units, host figure {host[k]:.3g}, bound {bound[k]:.3g}")
    assert not fails, fails
    for k in "pmv":
        assert dev[k] <= bound[k], (k, dev[k], host[k], bound[k])


# ---- (c) clipping ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ar.CLIP_CASES, ids=ar.case_id)
def test_clipped_step_against_float64(c):
    cid = ar.case_id(c)
    d, r32 = ar.inputs(c), ar.ref32_figures(c)
    slabs_d = _d(d["slabs"])
    for name, coef64, rf in (("coef64", True, ar.reference(c)), ("default", False, ar.reference(c, omb=ar.omb_f32_differenced(c["betas"])))):
        got = _twice(f"{cid} {name}", lambda: _step(c, d, slabs_d, coef64=coef64))
        _held(f"{cid} {name}", got, rf, r32)
        if c["weight_decay"] and coef64:   # the decay was added AFTER the clip: against the other order the step is outside the bar
            ref, wrong = ar.reference(c), ar.variant_reference("decay_before_clip", c)
            off = {k: ar.measure(_np(x).astype(np.float64), wrong[k], ref["u"][k]) for k, x in zip("pmv", got)}
            print(f"PARITY adam {cid} against decay-before-clip:", {k: f"{f:.3g}" for k, f in off.items()}, "units")
            assert max(off[k] / ar.bar_of(r32[k]) for k in "pmv") > 1.0


@pytest.mark.parametrize("c", ar.NOOP_CASES, ids=ar.case_id)
def test_norm_below_the_bound_clips_nothing(c):
    cid = ar.case_id(c)
    d = ar.inputs(c)
    slabs_d = _d(d["slabs"])
    for coef64 in (False, True):
        a = _twice(cid, lambda: _step(c, d, slabs_d, coef64=coef64))
        b = _twice(cid, lambda: _step(c, d, slabs_d, coef64=coef64, clip=False))
        for k, x, y in zip("pmv", a, b):
            _equal_bits(f"{cid} coef64={coef64} {k}: clipped call against unclipped", x, _np(y))
    sa, sb = _twice(cid, lambda: _step_segs(c, d, slabs_d)), _twice(cid, lambda: _step_segs({**c, "max_norm": None}, d, slabs_d))
    for k, x, y in zip("pmv", sa, sb):
        _equal_bits(f"{cid} segs {k}: clipped call against unclipped", x, _np(y))


@pytest.mark.parametrize("c", ar.ZERO_CASES, ids=ar.case_id)
def test_all_zero_gradient_with_clipping(c):
    cid = ar.case_id(c)
    d = ar.inputs(c)
    slabs_d = _d(d["slabs"])
    assert not d["slabs"].any()
    for coef64 in (False, True):
        got = _twice(cid, lambda: _step(c, d, slabs_d, coef64=coef64))
        if c["weight_decay"] == 0.0:
            _equal_bits(f"{cid} coef64={coef64} p keeps its bits", got[0], d["p"])
            _equal_bits(f"{cid} coef64={coef64} m = 0", got[1], np.zeros(c["n"], np.float32))
            _equal_bits(f"{cid} coef64={coef64} v = 0", got[2], np.zeros(c["n"], np.float32))
        else:
            rf = ar.reference(c, omb=None if coef64 else ar.omb_f32_differenced(c["betas"]))
            _held(f"{cid} coef64={coef64}", got, rf, ar.ref32_figures(c))


@pytest.mark.parametrize("c", ar.SEGCLIP_CASES, ids=ar.case_id)
def test_segmented_clip_has_one_norm_over_the_scaled_gradient(c):
    cid = ar.case_id(c)
    d = ar.inputs(c)
    slabs_d, scale_dev = _d(d["slabs"]), _d(np.float32([ar.SEG_SCALE]))
    got = _twice(cid, lambda: _step_segs(c, d, slabs_d, scale_dev))
    _held(cid, got, ar.reference(c, omb=ar.omb_f32_differenced(c["betas"])), ar.ref32_figures(c))


# ---- (d) device scalars and the image: exact ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [ar.ADAM_CASES[0], ar.ADAM_CASES[5]], ids=ar.case_id)
def test_device_scalars_give_the_host_scalars_bits(c):
    cid = ar.case_id(c)
    assert c["step"] in (1, 1000)
    d = ar.inputs(c)
    slabs_d = _d(d["slabs"])
    step_dev, lr_dev = _d(np.int64([c["step"]])), _d(np.float64([c["lr"]]))
    other = {**c, "step": 7, "lr": 0.125}   # the host values that the device ones must override
    for name, fn in (("adam_step", lambda cc, **kw: _step(cc, d, slabs_d, **kw)), ("adam_step coef64", lambda cc, **kw: _step(cc, d, slabs_d, coef64=True, **kw)),
                     ("adam_step_segs", lambda cc, **kw: _step_segs(cc, d, slabs_d, **kw))):
        host = _twice(cid, lambda: fn(c))
        for what, kw, cc in (("step_dev", dict(step_dev=step_dev), {**c, "step": 7}), ("lr_dev", dict(lr_dev=lr_dev), {**c, "lr": 0.125}),
                             ("step_dev + lr_dev", dict(step_dev=step_dev, lr_dev=lr_dev), other)):
            dev = _twice(cid, lambda: fn(cc, **kw))
            for k, x, y in zip("pmv", dev, host):
                _equal_bits(f"{cid} {name} {what} {k}", x, _np(y))
    assert int(step_dev.item()) == c["step"] and float(lr_dev.item()) == c["lr"]


@pytest.mark.parametrize("c", [ar.ADAM_CASES[3], ar.CLIP_CASES[1]], ids=ar.case_id)
def test_parameter_image_receives_the_stored_bits(c):
    cid = ar.case_id(c)
    d, n = ar.inputs(c), c["n"]
    slabs_d = _d(d["slabs"])
    mp = ar.image_map(n)
    mp_d = _d(mp)
    rest = np.setdiff1d(np.arange(n + 37), mp)
    assert len(rest) == 37
    for coef64 in (False, True):
        def with_image():
            img = torch.full((n + 37,), SENTINEL, device=DEV)
            return (*_step(c, d, slabs_d, coef64=coef64, image=img, image_map=mp_d), img)
        p, m, v, img = _twice(cid, with_image)
        img = _np(img)
        _equal_bits(f"{cid} coef64={coef64} image[image_map] against p", img[mp], _np(p))
        _equal_bits(f"{cid} coef64={coef64} the image's 37 other slots", img[rest], np.full(37, SENTINEL, np.float32))
        plain = _twice(cid, lambda: _step(c, d, slabs_d, coef64=coef64))
        for k, x, y in zip("pmv", plain, (p, m, v)):
            _equal_bits(f"{cid} coef64={coef64} {k} without image against with", x, _np(y))


# ---- (e) a short trajectory --------------------------------------------------------------------------------------------------
def test_five_step_trajectory_against_float64():
    c = ar.TRAJ
    p0, slabs = ar.traj_inputs()
    n, hp = c["n"], ar.hyper(c)
    slabs_d = [_d(s) for s in slabs]

    def run(kind):
        p = _d(p0)
        opt = FlatAdam(p, coef64=(kind == "coef64"), **hp)
        step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
        out = []
        for s_d in slabs_d:
            if kind == "segs":
                step_dev += 1   # on the device
                opt.step_segs(_segs_of(s_d), step_dev=step_dev)
            else:
                opt.step(s_d)
            out.append((p.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()))
        return out

    got = {}
    for kind in ("coef64", "default", "segs"):
        a, b = run(kind), run(kind)
        for t, (x, y) in enumerate(zip(a, b)):
            _same_bits(f"traj {kind} step {t + 1}", x, y)
        got[kind] = a
    # float64 trajectories with both coefficient forms, torch's float32 trajectory beside them
    par = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt32 = torch.optim.Adam([par], amsgrad=False, foreach=False, **hp)
    st = {form: (p0.astype(np.float64), np.zeros(n), np.zeros(n)) for form in ("once", "diff")}
    omb = dict(once=None, diff=ar.omb_f32_differenced(c["betas"]))
    fails = []
    for t, s in enumerate(slabs):
        refs = {}
        for form in st:
            terms = {}
            st[form] = ar.adam_step(*st[form][:1], ar.slab_sum_f64(s), *st[form][1:], t + 1, omb=omb[form], terms=terms, **hp)
            refs[form] = dict(zip("pmv", st[form]), u=ar.units(terms))
        par.grad = torch.from_numpy(s.copy()).sum(0)
        opt32.step()
        t32 = (par.detach().double().numpy(), opt32.state[par]["exp_avg"].double().numpy(), opt32.state[par]["exp_avg_sq"].double().numpy())
        r32 = {k: ar.measure(x, refs["once"][k], refs["once"]["u"][k]) for k, x in zip("pmv", t32)}
        for kind, form in (("coef64", "once"), ("default", "diff"), ("segs", "diff")):
            try:
                _held(f"traj step {t + 1} {kind}", got[kind][t], refs[form], r32)
            except AssertionError as e:
                fails.append(e)
    assert not fails, fails
