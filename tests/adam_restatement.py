"""Restatement of the optimizer kernels (csrc/adam.hip, csrc/adam_dev.h) in plain numpy, with the case lists and seeded inputs
of tests/test_gpu_adam.py.  tests/test_host_adam.py pins `adam_step` / `clip_coef` to torch.optim.Adam after clip_grad_norm_
in float64 (1e-10 of each array's scale), checks on the CPU every precondition the GPU tests rely on, and shows that every
wrong variant in `VARIANTS` leaves the bar on these inputs.

What is restated, and in which precision:
  * `slab_tree_f32`: the documented summation tree in float32 -- lane sl in 0..3 adds slabs sl, sl + 4, sl + 8, ... in that
    order starting from 0.f, then ((l0 + l1) + l2) + l3.  Additions only, so it is meant to be bit-exact with the kernels.
  * `slab_sum_f64`, `clip_coef`, `adam_step`: float64 on float32-valued inputs.  The scalars enter as the kernel receives
    them: beta1, beta2, eps and weight_decay as their float32 roundings; lr / (1 - beta1^t) and sqrt(1 - beta2^t) formed in
    float64 and rounded to float32 (torch's float32 Adam does the same with its python scalars).  `omb` = (1 - beta1,
    1 - beta2) as used: by default formed in float64 and rounded once (torch's form, the project's coef64 form);
    `omb_f32_differenced` gives float32(1) - float32(beta), the form of the default entry point tsm_adam_step.
    `round32=False` keeps every scalar in float64: the form that is pinned to torch's float64 Adam.

The measure (`units`, `measure`): per element |x - ref64| / u, u = the float32 spacing at the largest magnitude among the two
operands and the result of the quantity's final addition or subtraction (p: |p_old|, |update|, |p_new|; m: |beta1 m|,
|omb1 g|, |m_new|; v likewise), so that a cancelling element has the same unit for the kernel and for the reference.
The bar (`bar_of`): max(1, 2 x the same measure of torch's own float32 Adam on the CPU).

Plain numpy on the arithmetic path; torch appears only in `torch_adam`, which IS the reference.
"""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32
N_B = 4099          # 65 blocks of 64 parameters, the last with 3
N_C2 = 16449        # 258 blocks: the 256-strided sum of the blocks' squares takes a second trip with a ragged tail
SEG_SPLIT = 1500    # adam_step_segs: two segments [0, 1500) and [1500, n); 1500 is no multiple of the 64-parameter block
SEG_SCALE = 0.25    # the second segment's scale_dev in the clipped segmented case


# ---- the restatement ------------------------------------------------------------------------------------------------------
def slab_tree_f32(slabs, stride_view=None) -> np.ndarray:
    """float32 sum over the slabs (axis 0) in the kernels' order.  stride_view = (col0, n): the sum covers columns
    [col0, col0 + n) of every slab row (a segment that is a view into wider slabs)."""
    s = np.asarray(slabs)
    assert s.dtype == F32 and s.ndim == 2
    if stride_view is not None:
        s = s[:, stride_view[0]:stride_view[0] + stride_view[1]]
    lanes = [np.zeros(s.shape[1], F32) for _ in range(4)]
    for k in range(s.shape[0]):
        lanes[k & 3] = lanes[k & 3] + s[k]
    out = ((lanes[0] + lanes[1]) + lanes[2]) + lanes[3]
    assert out.dtype == F32
    return out


def slab_sum_f64(slabs) -> np.ndarray:
    return np.asarray(slabs, np.float64).sum(axis=0)


def clip_coef(g, max_norm) -> float:
    """clip_grad_norm_'s coefficient in float64."""
    g = np.asarray(g, np.float64)
    return float(min(1.0, float(max_norm) / (np.sqrt((g * g).sum()) + 1e-6)))


def omb_rounded_once(betas):
    return float(F32(1.0 - float(betas[0]))), float(F32(1.0 - float(betas[1])))


def omb_f32_differenced(betas):
    return float(F32(1) - F32(betas[0])), float(F32(1) - F32(betas[1]))


def adam_step(p, g, m, v, step, lr, betas, eps, weight_decay, omb=None, round32=True, terms=None):
    """One Adam step (amsgrad off) in float64 -> (p, m, v).  `g` is the gradient after clipping.  terms: a dict that receives
    the operands of every final addition (for `units`)."""
    r = (lambda x: float(F32(x))) if round32 else float
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    beta1, beta2, eps, wd = r(betas[0]), r(betas[1]), r(eps), r(weight_decay)
    if omb is None:
        omb = (r(1.0 - float(betas[0])), r(1.0 - float(betas[1])))
    step = int(step)
    assert step >= 1
    step_size = r(float(lr) / (1.0 - float(betas[0]) ** step))
    bc2_sqrt = r(np.sqrt(1.0 - float(betas[1]) ** step))
    if wd != 0.0:
        g = g + wd * p
    m_a, m_b = beta1 * m, omb[0] * g
    v_a, v_b = beta2 * v, omb[1] * g * g
    m_new, v_new = m_a + m_b, v_a + v_b
    update = step_size * (m_new / (np.sqrt(v_new) / bc2_sqrt + eps))
    p_new = p - update
    if terms is not None:
        terms.update(p=(p, update, p_new), m=(m_a, m_b, m_new), v=(v_a, v_b, v_new))
    return p_new, m_new, v_new


def units(terms) -> dict:
    """Per array the float32 spacing at max(|operand 1|, |operand 2|, |result|) of its final addition."""
    out = {}
    for key, ops3 in terms.items():
        big = np.maximum.reduce([np.abs(x) for x in ops3])
        out[key] = np.spacing(big.astype(F32)).astype(np.float64)
    return out


def measure(got, ref, u) -> float:
    return float((np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / u).max())


def bar_of(ref32_figure: float) -> float:
    """At most twice the reference's own float32 figure (another rounding order: torch's lerp_ / addcmul_ and its sum tree
    against the kernels'), with a floor of one unit (the half-unit rounding of the stored value, and the factor-2 ambiguity of
    the unit at a binade edge)."""
    return max(1.0, 2.0 * ref32_figure)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def torch_adam(p, g, m, v, step, lr, betas, eps, weight_decay, max_norm=None, dtype="float64"):
    """torch.optim.Adam (amsgrad off, single-tensor) after torch.nn.utils.clip_grad_norm_ on the CPU in `dtype`, from the
    state (m, v) before step `step`: a prefilled state is written into optimizer.state.  -> (p, m, v) as float64 arrays."""
    import torch

    dt = getattr(torch, dtype)
    par = torch.nn.Parameter(torch.tensor(np.asarray(p, np.float64), dtype=dt))
    opt = torch.optim.Adam([par], lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=False)
    if int(step) > 1 or np.any(m) or np.any(v):
        opt.state[par] = dict(step=torch.tensor(float(int(step) - 1)), exp_avg=torch.tensor(np.asarray(m, np.float64), dtype=dt),
                              exp_avg_sq=torch.tensor(np.asarray(v, np.float64), dtype=dt))
    par.grad = torch.tensor(np.asarray(g, np.float64), dtype=dt)
    if max_norm:
        torch.nn.utils.clip_grad_norm_([par], max_norm)
    opt.step()
    st = opt.state[par]
    assert int(st["step"]) == int(step)
    return tuple(x.detach().double().numpy() for x in (par, st["exp_avg"], st["exp_avg_sq"]))


# ---- cases -----------------------------------------------------------------------------------------------------------------
# (a) both sides of every tier's entry condition (s + 252, s + 60, s + 28 < n_slab, then the tail) for each of the four slab
# lanes, and fewer slabs than lanes
SLAB_COUNTS = [1, 2, 3, 4, 5, 28, 29, 32, 33, 60, 61, 64, 65, 124, 252, 253, 256, 257, 260, 516]
SLAB_NS = [1, 63, 64, 65, 129]
SLAB_SCALE = 0.3         # `scale`: the result is fl(sum * float32(0.3))
SLAB_SCALE_DEV = 0.37    # a segment's scale_dev: fl(fl(sum * scale) * float32(0.37))

DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-8)
OTHER = dict(betas=(0.8, 0.99), eps=1e-6)
# (b) every state kind (zero state at step 1; prefilled at steps 2, 1000, 10**6) meets both hyper-parameter sets, both weight
# decays and both learning rates
ADAM_CASES = [dict(kind="step", n=N_B, n_slab=5, step=t, seed=4100 + 2 * i + j, lr=lr, weight_decay=wd, **hp)
              for i, t in enumerate((1, 2, 1000, 10 ** 6))
              for j, (hp, wd, lr) in enumerate(((DEFAULTS, 0.0, 3e-4), (OTHER, 0.01, 1e-3)))]
# (c) `norm` = the gradient's norm as a multiple of max_norm: clipped (2.2: close enough to 1 / max_norm = 2 for the 1e-6 of
# the coefficient to show), the clamp (0.4), and the all-zero gradient
CLIP_CASES = [dict(kind="clip", n=n, n_slab=s, step=1, seed=4200 + i, lr=3e-4, weight_decay=wd, max_norm=mn, norm=2.2, **DEFAULTS)
              for i, (n, s, mn, wd) in enumerate(((N_B, 1, 0.5, 0.0), (N_B, 33, 40.0, 0.01), (N_C2, 33, 0.5, 0.01),
                                                  (N_C2, 1, 40.0, 0.0)))]
NOOP_CASES = [dict(kind="noop", n=n, n_slab=s, step=1, seed=4300 + i, lr=3e-4, weight_decay=wd, max_norm=mn, norm=0.4, **DEFAULTS)
              for i, (n, s, mn, wd) in enumerate(((N_B, 33, 0.5, 0.01), (N_C2, 1, 40.0, 0.0)))]
ZERO_CASES = [dict(kind="zero", n=n, n_slab=s, step=1, seed=4400 + i, lr=3e-4, weight_decay=wd, max_norm=0.5, norm=0.0, **DEFAULTS)
              for i, (n, s, wd) in enumerate(((N_B, 1, 0.0), (N_C2, 33, 0.01)))]
# adam_step_segs with clipping: ONE norm over both segments, the second scaled by SEG_SCALE on the device
SEGCLIP_CASES = [dict(kind="segclip", n=N_B, n_slab=5, step=1, seed=4500, lr=3e-4, weight_decay=0.01, max_norm=0.5, norm=2.2,
                      **DEFAULTS)]
CASES = ADAM_CASES + CLIP_CASES + NOOP_CASES + ZERO_CASES + SEGCLIP_CASES
# (e) a short trajectory
TRAJ = dict(kind="traj", n=N_B, n_slab=3, steps=5, seed=4600, lr=1e-3, weight_decay=0.01, **DEFAULTS)


def case_id(c: dict) -> str:
    s = f"{c['kind']}-n{c['n']}-s{c['n_slab']}-t{c['step']}-b{c['betas'][1]}-wd{c['weight_decay']}-lr{c['lr']}"
    return s + (f"-mn{c['max_norm']}" if "max_norm" in c else "")


def hyper(c: dict) -> dict:
    return dict(lr=c["lr"], betas=c["betas"], eps=c["eps"], weight_decay=c["weight_decay"])


def slab_inputs(n_slab: int, n: int, width: int | None = None, seed: int = 0) -> np.ndarray:
    """[n_slab, width or n] float32: N(0, 1) scaled per slab by 10^U(-3, 3), so that the order of the additions shows in the bits."""
    rs = np.random.RandomState(7000 + 1009 * seed + 31 * n_slab + n)
    w = n if width is None else width
    return (rs.standard_normal((n_slab, w)) * 10.0 ** rs.uniform(-3, 3, (n_slab, 1))).astype(F32)


def _populations(rs, n: int, weight_decay: float):
    """p: exact zeros; +-U(1e-4, 1e-3); N(0, 1).  g: exact zeros; random sign x 10^U(-12, 2).  Shuffled independently, so
    every population of p meets every population of g.  Without weight decay the sign of g is independent of p's: gradients
    oppose the parameter as often as not.  With weight decay the sign of g is p's where p is not zero: g + weight_decay p
    then never cancels.  (That sum is no final addition of p, m or v, so the measure's unit would not cover it: with
    independent signs the slab sum's rounding is amplified by |g| / |g + wd p|, thousands of units on the few elements where
    g is near -wd p, for torch's float32 Adam as for the kernel -- the comparison would hinge on those elements alone.)"""
    k = n // 8
    p = np.concatenate([np.zeros(k), rs.choice([-1.0, 1.0], 3 * k) * rs.uniform(1e-4, 1e-3, 3 * k), rs.standard_normal(n - 4 * k)])
    g = np.concatenate([np.zeros(k), rs.choice([-1.0, 1.0], n - k) * 10.0 ** rs.uniform(-12, 2, n - k)])
    p, g = rs.permutation(p), rs.permutation(g)
    if weight_decay != 0.0:
        g = np.where(p != 0, np.abs(g) * np.sign(p), g)
    return p.astype(F32), g.astype(F32)


def _split(rs, g: np.ndarray, n_slab: int, mixed: bool = False) -> np.ndarray:
    """Slabs [n_slab, n] float32 that sum to g up to rounding: shares U(0.2, 1) of every entry, so the float64 sum of the slabs
    has g's zeros and g's magnitudes.  mixed (the cases without weight decay, three slabs or more): per entry one slab's
    share is -0.25 U(0.2, 1), a slab that opposes the others, whose shares are raised to 0.5 at least.  The others then sum
    to 1 at least and the opposing one is 0.25 at most: sum |share| / |sum share| <= 1.25 / 0.75, so the sum's own rounding,
    which lies in front of the final addition that sets the unit, is amplified by less than 2."""
    w = rs.uniform(0.2, 1.0, (n_slab, g.size))
    if mixed and n_slab >= 3:
        opp = rs.randint(0, n_slab, g.size)
        w = np.maximum(w, 0.5)
        w[opp, np.arange(g.size)] = -0.25 * rs.uniform(0.2, 1.0, g.size)
        assert (np.abs(w).sum(axis=0) < 2.0 * w.sum(axis=0)).all()
    return (w / w.sum(axis=0) * g.astype(np.float64)).astype(F32)


@functools.lru_cache(maxsize=None)
def _inputs(key):
    c = dict(key)
    rs = np.random.RandomState(c["seed"])
    n = c["n"]
    p, g = _populations(rs, n, c["weight_decay"])
    if c["kind"] == "zero":
        g = np.zeros(n, F32)
    elif "norm" in c:   # the wanted norm (of the scaled gradient in the segmented case)
        eff = g.astype(np.float64)
        if c["kind"] == "segclip":
            eff[SEG_SPLIT:] *= SEG_SCALE
        g = (g.astype(np.float64) * (c["norm"] * c["max_norm"] / np.sqrt((eff * eff).sum()))).astype(F32)
    slabs = _split(rs, g, c["n_slab"], mixed=c["weight_decay"] == 0.0)
    if c["step"] == 1:
        m, v = np.zeros(n, F32), np.zeros(n, F32)
    else:   # v = 10^U(-24, 4) with a share of exact zeros where m = 0 too; m = U(-1, 1) sqrt(v)
        v = (10.0 ** rs.uniform(-24, 4, n)).astype(F32)
        v[rs.rand(n) < 0.1] = 0.0
        m = (rs.uniform(-1, 1, n) * np.sqrt(v.astype(np.float64))).astype(F32)
        # Where beta1 m and omb1 g cancel to less than 1 / 1.9 of the larger one, m takes the other sign.  The update is
        # proportional to m_new, so m_new's rounding reaches p amplified by max(|beta1 m|, |omb1 g|) / |m_new|, and where p is
        # zero or small p's unit is the update's own spacing, which does not cover that.  With factors of 20 to 200 on single
        # elements the maximum over p is set by those elements alone, for torch's float32 Adam as for the kernel, and which
        # of the two is hit harder there is chance.  Opposing m and g stay wherever the factor is below 1.9, and the host test
        # (tests/test_host_adam.py) asserts both that they occur and that no element exceeds 2.
        m_a = float(F32(c["betas"][0])) * m.astype(np.float64)
        m_b = omb_rounded_once(c["betas"])[0] * (slab_sum_f64(slabs) + float(F32(c["weight_decay"])) * p.astype(np.float64))
        m = np.where(np.maximum(np.abs(m_a), np.abs(m_b)) > 1.9 * np.abs(m_a + m_b), -m, m)
    out =dict(p=p, slabs=slabs, m=m, v=v)
    for a in out.values():
        a.setflags(write=False)
    return out


def inputs(c: dict) -> dict:
    """Seeded float32 inputs of a case: p, slabs [n_slab, n], m, v (read-only, shared)."""
    return _inputs(tuple(sorted((k, v) for k, v in c.items() if k in ("kind", "seed", "n", "n_slab", "step", "norm", "max_norm", "weight_decay", "betas"))))


def grad64(c: dict, slabs=None) -> np.ndarray:
    """The float64 sum of the slabs (times the second segment's scale in the segmented clip case), before clipping."""
    g = slab_sum_f64(inputs(c)["slabs"] if slabs is None else slabs)
    if c["kind"] == "segclip":
        g = g.copy()
        g[SEG_SPLIT:] *= SEG_SCALE
    return g


def reference(c: dict, omb=None, d=None, step_fn=adam_step, coef_fn=clip_coef):
    """Float64 restatement of the case -> dict(p, m, v, u, coef): clip (if the case has a max_norm), then `step_fn`."""
    d = inputs(c) if d is None else d
    g = grad64(c, d["slabs"])
    coef = coef_fn(g, c["max_norm"]) if c.get("max_norm") else 1.0
    terms = {}
    kw = dict(terms=terms) if step_fn is adam_step else {}
    p, m, v = step_fn(d["p"], g * coef, d["m"], d["v"], c["step"], omb=omb, **hyper(c), **kw)
    return dict(p=p, m=m, v=v, coef=coef, u=units(terms) if terms else None, terms=terms or None)


@functools.lru_cache(maxsize=None)
def _ref32(key):
    c = dict(key)
    c["betas"] = tuple(c["betas"])
    d, ref = inputs(c), reference(c)
    import torch

    g32 = torch.from_numpy(np.array(d["slabs"])).sum(0).numpy().astype(np.float64)   # torch's own float32 sum of the slabs
    if c["kind"] == "segclip":
        g32[SEG_SPLIT:] = (g32[SEG_SPLIT:].astype(F32) * F32(SEG_SCALE)).astype(np.float64)
    got = torch_adam(d["p"], g32, d["m"], d["v"], c["step"], max_norm=c.get("max_norm"), dtype="float32", **hyper(c))
    return {k: measure(x, ref[k], ref["u"][k]) for k, x in zip("pmv", got)}


def ref32_figures(c: dict) -> dict:
    """max |torch float32 Adam - ref64| / u per array: what float32 costs the reference itself on this case."""
    return dict(_ref32(tuple(sorted(c.items()))))


def default_path_deviation(c: dict) -> dict:
    """The float32-differenced coefficients against the true float64 Adam, per array in units: the declared deviation of
    tsm_adam_step (csrc/adam_dev.h), as the host test computes it."""
    ref, dev = reference(c), reference(c, omb=omb_f32_differenced(c["betas"]))
    return {k: measure(dev[k], ref[k], ref["u"][k]) for k in "pmv"}


def image_map(n: int, extra: int = 37, seed: int = 4700) -> np.ndarray:
    """A seeded injective map of n parameters into an image of n + extra floats."""
    return np.random.RandomState(seed).permutation(n + extra)[:n].astype(np.int32)


def traj_inputs():
    c = TRAJ
    rs = np.random.RandomState(c["seed"])
    p, _ = _populations(rs, c["n"], c["weight_decay"])
    # Fresh gradients per step: magnitudes 0.1 |N(0, 1)|, split into slabs of positive shares as in `_split`, with ONE sign per
    # element over the steps (p's where p is not zero).  The measure's unit covers the roundings of one step.  With
    # independent signs m = beta1 m + omb1 g cancels on some elements; what such an element inherits from the step before is
    # an error in the units of that step's much larger operands, and it showed as 20 to 35 units in m from step 3 on for
    # torch's float32 trajectory itself (100 where three raw N(0, 1) slabs cancel in the sum as well): the comparison would
    # hinge on a handful of elements.  With one sign per element no addition of m, v or g + weight_decay p cancels, and a
    # state read or written at the wrong index still shows at once: every element has its own magnitudes.
    sign = np.where(p != 0, np.sign(p), rs.choice([-1.0, 1.0], c["n"]))
    slabs = [_split(rs, (sign * 0.1 * np.abs(rs.standard_normal(c["n"]))).astype(F32), c["n_slab"]) for _ in range(c["steps"])]
    return p, slabs


# ---- deliberately wrong variants (tests/test_host_adam.py shows that each leaves the bar on CASES) ---------------------------
def _variant_step(which):
    def step_fn(p, g, m, v, step, lr, betas, eps, weight_decay, omb=None):
        r = lambda x: float(F32(x))  # noqa: E731
        p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
        beta1, beta2, eps_, wd = r(betas[0]), r(betas[1]), r(eps), r(weight_decay)
        o1, o2 = omb_rounded_once(betas) if omb is None else omb
        if which == "omb2_f32_differenced":
            o2 = omb_f32_differenced(betas)[1]
        bc1 = 1.0 - float(betas[0]) ** step
        step_size = r(float(lr) / bc1)
        bc2_sqrt = r(np.sqrt(1.0 - float(betas[1]) ** step))
        if which == "no_bias_correction2" and step >= 1000:
            bc2_sqrt = 1.0
        if wd != 0.0 and which != "decay_before_clip":   # (that variant adds the decay in front of the clip: `_decay_first`)
            g = g + wd * p
        m_new = beta1 * m + o1 * g
        gv = g / bc1 if which == "v_from_corrected_g" else g
        v_new = beta2 * v + o2 * gv * gv
        if which == "eps_before_bc2":
            denom = (np.sqrt(v_new) + eps_) / bc2_sqrt
        elif which == "eps_in_sqrt":
            denom = np.sqrt(v_new + eps_) / bc2_sqrt
        else:
            denom = np.sqrt(v_new) / bc2_sqrt + eps_
        return p - step_size * (m_new / denom), m_new, v_new
    return step_fn


def variant_reference(name: str, c: dict) -> dict:
    """The case through a wrong optimizer -> dict(p, m, v)."""
    d = inputs(c)
    if name == "clip_without_1e-6":
        return reference(c, step_fn=_variant_step(None), coef_fn=lambda g, mn: min(1.0, mn / np.sqrt((g * g).sum())) if np.any(g) else 1.0)
    if name == "clip_without_clamp":
        return reference(c, step_fn=_variant_step(None), coef_fn=lambda g, mn: mn / (np.sqrt((g * g).sum()) + 1e-6))
    if name == "decay_before_clip":
        g = grad64(c) + float(F32(c["weight_decay"])) * d["p"].astype(np.float64)
        coef = clip_coef(g, c["max_norm"]) if c.get("max_norm") else 1.0
        p, m, v = _variant_step(name)(d["p"], g * coef, d["m"], d["v"], c["step"], **hyper(c))
        return dict(p=p, m=m, v=v)
    return reference(c, step_fn=_variant_step(name))


VARIANTS = ["eps_before_bc2", "eps_in_sqrt", "no_bias_correction2", "decay_before_clip", "clip_without_1e-6", "clip_without_clamp",
            "v_from_corrected_g", "omb2_f32_differenced"]
