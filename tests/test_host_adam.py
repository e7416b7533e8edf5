"""Host tests (no GPU) of tests/adam_restatement.py, the float64 yardstick of tests/test_gpu_adam.py:
  * the restatement is torch.optim.Adam (amsgrad off) after torch.nn.utils.clip_grad_norm_ in float64 on the CPU, to 1e-10 of
    each array's scale, on every Adam case of the GPU tests -- prefilled states written into optimizer.state;
  * every precondition the GPU tests rely on holds for the seeded inputs;
  * every deliberately wrong variant of the optimizer leaves the GPU tests' bar on these inputs: the proof, without a GPU,
    that those tests fail for a subtly wrong kernel.  If a variant were not caught, the inputs would have to change, not the bar.
Every comparison prints `PARITY adam ...`."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adam_restatement as ar  # noqa: E402

TINY = float(np.finfo(np.float32).tiny)


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("c", ar.CASES, ids=ar.case_id)
def test_restatement_is_torch_float64_adam(c):
    """round32=False: every scalar in float64, as torch's float64 Adam has them."""
    d = ar.inputs(c)
    g = ar.grad64(c)
    coef = ar.clip_coef(g, c["max_norm"]) if c.get("max_norm") else 1.0
    got = ar.adam_step(d["p"], g * coef, d["m"], d["v"], c["step"], round32=False, **ar.hyper(c))
    want = ar.torch_adam(d["p"], g, d["m"], d["v"], c["step"], max_norm=c.get("max_norm"), dtype="float64", **ar.hyper(c))
    worst = {k: _rel(x, y) for k, x, y in zip("pmv", got, want)}
    print(f"PARITY adam host {ar.case_id(c)}: max |restatement - torch64| / max |torch64| =", {k: f"{e:.3g}" for k, e in worst.items()})
    assert max(worst.values()) <= 1e-10


def test_rounded_scalars_are_the_kernels():
    """What round32 changes: the scalars the kernel receives as float, and the two coefficients it forms in double and rounds."""
    assert ar.omb_rounded_once((0.9, 0.999)) == (float(np.float32(0.1)), float(np.float32(0.001)))
    o1, o2 = ar.omb_f32_differenced((0.9, 0.999))
    assert o2 == float(np.float32(1) - np.float32(0.999)) and abs(o2 / 0.001 - 1) > 1e-5 and abs(o1 / 0.1 - 1) > 1e-8
    p, g, z = np.float32([0.5]), np.float32([0.25]), np.zeros(1, np.float32)
    t = {}
    ar.adam_step(p, g, z, z, 3, 1e-3, (0.9, 0.999), 1e-8, 0.01, terms=t)
    gg = 0.25 + float(np.float32(0.01)) * 0.5
    assert t["m"][1][0] == float(np.float32(0.1)) * gg and t["v"][1][0] == float(np.float32(0.001)) * gg * gg
    m, v = t["m"][2][0], t["v"][2][0]
    want = float(np.float32(1e-3 / (1 - 0.9 ** 3))) * (m / (np.sqrt(v) / float(np.float32(np.sqrt(1 - 0.999 ** 3))) + float(np.float32(1e-8))))
    assert t["p"][1][0] == want


def test_slab_tree_order():
    """The tree on values where the order of the additions decides the bits: 2^24 + 1 + 1 is 2^24 in one lane, 2^24 + 2 across."""
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    same_lane = np.array([[big], [0], [0], [0], [one], [0], [0], [0], [one]], np.float32)   # slabs 0, 4, 8: lane 0
    assert ar.slab_tree_f32(same_lane)[0] == big
    across = np.array([[big], [one], [0], [0], [0], [one]], np.float32)                     # lane 1 holds 1 + 1
    assert ar.slab_tree_f32(across)[0] == big + np.float32(2)
    last = np.array([[one], [0], [0], [big], [one]], np.float32)                            # (l0 + l1 + l2) = 2 meets l3 last
    assert ar.slab_tree_f32(last)[0] == big + np.float32(2)
    wide = np.arange(12, dtype=np.float32).reshape(2, 6)
    assert np.array_equal(ar.slab_tree_f32(wide, stride_view=(3, 2)), np.float32([3 + 9, 4 + 10]))
    for n_slab in ar.SLAB_COUNTS:
        s = ar.slab_inputs(n_slab, 65)
        err = np.abs(ar.slab_tree_f32(s).astype(np.float64) - ar.slab_sum_f64(s))
        assert (err <= (n_slab - 1) * 2.0 ** -24 * np.abs(s.astype(np.float64)).sum(0)).all()


@pytest.mark.parametrize("c", ar.CASES, ids=ar.case_id)
def test_preconditions(c):
    d = ar.inputs(c)
    g = ar.grad64(c)
    for k in ("p", "m", "v"):   # no subnormal input
        a = np.abs(d[k][d[k] != 0])
        assert a.size == 0 or a.min() >= TINY, k
    assert (d["v"] >= 0).all() and not d["m"][d["v"] == 0].any()
    if c["kind"] in ("step", "clip", "segclip", "noop"):
        assert (g == 0).sum() >= c["n"] // 8 and (d["p"] == 0).sum() >= c["n"] // 8
    if c["weight_decay"] == 0.0 and c["kind"] != "zero":   # without weight decay: gradients with and against the parameter ...
        gp = np.sign(g) * np.sign(d["p"])
        assert (gp < 0).sum() >= c["n"] // 4 and (gp > 0).sum() >= c["n"] // 4
        if c["n_slab"] >= 3:   # ... and in every column one slab that opposes the others
            assert ((np.sign(d["slabs"]) * np.sign(g) < 0).sum(0) == (g != 0)).all()
    coef = 1.0
    if c.get("max_norm"):   # at least a factor 2 between the norm and the bound, either way: no case sits on the clamp
        norm, mn = float(np.sqrt((g * g).sum())), c["max_norm"]
        coef = ar.clip_coef(g, mn)
        print(f"PARITY adam host {ar.case_id(c)}: norm / max_norm = {norm / mn:.4g}, coefficient {coef:.6g}")
        if c["kind"] in ("clip", "segclip"):
            assert norm >= 2.0 * mn and coef < 0.5
        elif c["kind"] == "noop":
            assert 0 < norm <= 0.5 * mn and coef == 1.0
        else:
            assert norm == 0.0 and coef == 1.0
    wp = float(np.float32(c["weight_decay"])) * d["p"].astype(np.float64)
    ge = g * coef + wp
    assert (np.abs(ge) >= np.maximum(np.abs(g * coef), np.abs(wp))).all()   # g + weight_decay p never cancels
    if c["step"] > 1:   # prefilled: m and g oppose each other on many elements, and nowhere cancel by more than a factor 2
        for omb in (None, ar.omb_f32_differenced(c["betas"])):
            m_a, m_b, m_new = ar.reference(c, omb=omb)["terms"]["m"]
            assert (np.maximum(np.abs(m_a), np.abs(m_b)) <= 2.0 * np.abs(m_new)).all()
            assert (m_a * m_b < 0).sum() >= c["n"] // 8
    nz = np.abs(ge[ge != 0])
    for o in (ar.omb_rounded_once(c["betas"])[1], ar.omb_f32_differenced(c["betas"])[1]):   # (omb2 g) g in the kernel's order
        assert nz.size == 0 or ((o * nz).min() >= TINY and (o * nz * nz).min() >= TINY)
    sl = np.abs(d["slabs"][d["slabs"] != 0])
    assert sl.size == 0 or sl.min() >= TINY


def test_case_lists_cover_the_issue():
    for kind_steps in ((1,), (2, 1000, 10 ** 6)):   # every value with each state kind
        cs = [c for c in ar.ADAM_CASES if c["step"] in kind_steps]
        assert {c["betas"] for c in cs} == {(0.9, 0.999), (0.8, 0.99)} and {c["eps"] for c in cs} == {1e-8, 1e-6}
        assert {c["weight_decay"] for c in cs} == {0.0, 0.01} and {c["lr"] for c in cs} == {3e-4, 1e-3}
    assert {c["step"] for c in ar.ADAM_CASES} == {1, 2, 1000, 10 ** 6}
    assert all(c["n"] == 4099 and c["n_slab"] == 5 for c in ar.ADAM_CASES)
    for cs in (ar.CLIP_CASES, ar.NOOP_CASES, ar.ZERO_CASES):
        assert {c["n"] for c in cs} == {4099, 16449} and {c["n_slab"] for c in cs} == {1, 33}
        assert {c["weight_decay"] for c in cs} == {0.0, 0.01}
    assert {c["max_norm"] for c in ar.CLIP_CASES} == {0.5, 40.0}
    mp = ar.image_map(4099)
    assert len(set(mp.tolist())) == 4099 and mp.min() >= 0 and mp.max() < 4099 + 37


def test_wrong_variants_leave_the_bar():
    """Each wrong optimizer, in exact float64 arithmetic, against the true float64 Adam on the GPU tests' inputs and under
    their bar max(1, 2 x torch float32's own figure): at least one array of at least one case must be outside."""
    caught = {}
    for name in ar.VARIANTS:
        best = (0.0, None, None)
        for c in ar.CASES:
            ref, bad, r32 = ar.reference(c), ar.variant_reference(name, c), ar.ref32_figures(c)
            for k in "pmv":
                ratio = ar.measure(bad[k], ref[k], ref["u"][k]) / ar.bar_of(r32[k])
                if ratio > best[0]:
                    best = (ratio, k, ar.case_id(c))
        caught[name] = best
        print(f"PARITY adam host variant {name}: worst error / bar = {best[0]:.3g} on {best[1]} of {best[2]}")
    for name, (ratio, k, cid) in caught.items():
        assert ratio > 1.0, f"{name} stays inside the bar on every case"
    # the two entry points need two restatements: the float32-differenced 1 - beta2 is outside the bar on v
    c = ar.ADAM_CASES[0]
    ref, bad = ar.reference(c), ar.variant_reference("omb2_f32_differenced", c)
    on_v = ar.measure(bad["v"], ref["v"], ref["u"]["v"])
    print(f"PARITY adam host variant omb2_f32_differenced on v of {ar.case_id(c)}: {on_v:.3g} units, bar {ar.bar_of(ar.ref32_figures(c)['v']):.3g}")
    assert on_v > ar.bar_of(ar.ref32_figures(c)["v"])
    # ... and the correct step passes its own bar trivially, so the variants are what is caught
    for c in ar.CASES:
        same = ar.variant_reference("none", c)
        ref = ar.reference(c)
        assert all(ar.measure(same[k], ref[k], ref["u"][k]) <= 1e-6 for k in "pmv"), ar.case_id(c)


def test_default_path_deviation_is_the_documented_one():
    """csrc/adam_dev.h: 1.f - 0.999f is 1.3e-5 below 0.001, which makes a step 6.4e-6 too long (the half of it, through the
    square root of v).  The figure the GPU test holds tsm_adam_step to is computed here."""
    o2 = ar.omb_f32_differenced((0.9, 0.999))[1]
    assert abs((1 - o2 / float(np.float32(0.001))) - 1.29e-5) < 2e-7
    c = ar.ADAM_CASES[0]
    ref, dev = ar.reference(c), ar.reference(c, omb=ar.omb_f32_differenced(c["betas"]))
    upd, upd_dev = ref["p"] - ar.inputs(c)["p"], dev["p"] - ar.inputs(c)["p"]
    big = np.abs(ar.grad64(c)) > 1e-6    # where eps does not matter: the whole 6.4e-6
    rel = np.abs(upd_dev[big] / upd[big] - 1)
    print(f"PARITY adam host default path: step too long by {rel.min():.3g} .. {rel.max():.3g}; in units", ar.default_path_deviation(c))
    assert 6.0e-6 < rel.min() and rel.max() < 6.9e-6
    for c in ar.ADAM_CASES:
        assert ar.default_path_deviation(c)["v"] > ar.bar_of(ar.ref32_figures(c)["v"])
