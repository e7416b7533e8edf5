"""GPU tests (`-m gpu`) of QMIX (csrc/qmix.hip + the dense Q-nets and hypernetworks under one HIP Adam).

Every array is compared with the float64 restatement (tests/qmix_restatement.py, pinned to the reference's float64 run by
tests/test_host_qmix.py) within  |hip - ref64| <= 4 max(e_ref, 8 ulp(max |ref64|)),  e_ref = the reference's own float32
error on that array (tests/golden/qmix.npz); weights after an Adam step also get the `adamcond` allowance of the CTDE
replays.  Each test prints the largest |hip - ref64| / tol per array."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden", "qmix.npz")
DEV = "cuda"

from qmix_restatement import QmixRestatement  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.multiagent.ctde import DecentralizedActor, QMIXMixer, QMIXPolicy
    from tianshou_marl_amd.data import Batch


class _Discrete:
    def __init__(self, n):
        self.n = n


def _ulp_floor(ref):
    m = float(np.abs(ref).max()) if np.size(ref) else 0.0
    return 8.0 * float(np.spacing(np.float32(m))) if m > 0 else 8.0 * float(np.finfo(np.float32).tiny)


def _load(name: str) -> dict:
    """The fixture arrays of a variant: qmix.npz, or for c3 qmix_c3.npz with its inputs from qmix_c3_rows.npz."""
    if name != "c3":
        return np.load(GOLD)
    d = dict(np.load(os.path.join(HERE, "golden", "qmix_c3.npz")))
    d.update(np.load(os.path.join(HERE, "golden", "qmix_c3_rows.npz")))
    return d


def _check(name, got, ref, e_ref, extra=0.0):
    """|got - ref| <= plain + extra everywhere, plain = 4 max(e_ref, 8 ulp(max |ref|)).  With an allowance `extra` (Adam
    steps on ill-conditioned parameters, test_gpu_dense.py:488-497) all but 0.1 % must also meet the plain bar alone."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    plain = 4.0 * max(float(e_ref), _ulp_floor(ref))
    tol = plain + extra
    err = np.abs(got - ref)
    ratio = float((err / tol).max())
    msg = f"PARITY {name}: max |hip - ref64| / tol = {ratio:.3g}"
    if np.ndim(extra) > 0:
        share = float((err <= plain).mean())
        msg += f", share within the plain bar {share:.6f}, max |hip - ref64| / plain = {float((err / plain).max()):.3g}"
        assert share > 0.999, (name, share)
    print(msg)
    assert np.all(err <= tol), (name, ratio)
    return ratio


def _policy(init, dims, mono=True, gamma=0.99, seed=0, epsilon=0.1):
    N, D, A, H, S, E, Hh = dims
    actors = [DecentralizedActor(D, A, H, device=DEV, seed=i) for i in range(N)]
    mixer = QMIXMixer(N, S, E, Hh, mono, device=DEV, seed=100)
    pol = QMIXPolicy(actors, mixer, None, _Discrete(A), N, discount_factor=gamma, epsilon=epsilon, seed=seed)
    t = torch.as_tensor(np.asarray(init, np.float32), device=DEV)
    pol.flat.copy_(t)
    pol.target_flat.copy_(t)
    return pol


def _batch(rows, N, B, D, device=False):
    conv = (lambda x: torch.as_tensor(x, device=DEV)) if device else (lambda x: x)
    b = Batch()
    for i in range(N):
        b[f"agent_{i}"] = Batch(obs=conv(rows["obs"][i]), act=conv(rows["act"][i]), rew=conv(rows["rew"][i]),
                                obs_next=conv(rows["obs_next"][i]), terminated=conv(rows["term"]))
    b["global_obs"] = conv(np.ascontiguousarray(rows["obs"].transpose(1, 0, 2).reshape(B, N * D)))
    b["global_obs_next"] = conv(np.ascontiguousarray(rows["obs_next"].transpose(1, 0, 2).reshape(B, N * D)))
    return b


def _draw_rows(R64, N, B, D, A, seed):
    """Joint rows drawn under the delta rule (every row redrawn while any kink of the f64 nets is within 1e-5)."""
    rs = np.random.RandomState(seed)
    S = N * D

    def draw():
        return dict(obs=rs.standard_normal((N, B, D)).astype(np.float32),
                    obs_next=rs.standard_normal((N, B, D)).astype(np.float32),
                    act=rs.randint(0, A, (N, B)).astype(np.int64), rew=rs.standard_normal((N, B)).astype(np.float32),
                    term=rs.rand(B) < 0.1)

    rows, share = draw(), None
    for _ in range(50):
        gs = rows["obs"].transpose(1, 0, 2).reshape(B, S)
        gsn = rows["obs_next"].transpose(1, 0, 2).reshape(B, S)
        bad = R64.kink_rows(rows["obs"], rows["obs_next"], gs, gsn, 1e-5)
        share = float(bad.mean()) if share is None else share
        if not bad.any():
            break
        fresh = draw()
        for k in rows:
            if k == "term":
                rows[k][bad] = fresh[k][bad]
            else:
                rows[k][:, bad] = fresh[k][:, bad]
    assert not bad.any()
    return rows, gs, gsn, share


def _grad_of(pol, B):
    return pol._ws[B]["slabs"].double().sum(0).cpu().numpy()


@pytest.mark.parametrize("name", ["small", "nonmono", "c3"])
def test_learn_matches_reference(name):
    g = _load(name)
    N, D, A, H, S, E, Hh, B, rounds, mono = (int(x) for x in g[f"{name}_dims"])
    dims = (N, D, A, H, S, E, Hh)
    pol = _policy(g[f"{name}_init"], dims, bool(mono), float(g["gamma"]))
    R = QmixRestatement(g[f"{name}_init"], dims, monotonic=bool(mono), gamma=float(g["gamma"]))
    lr = 1e-3
    cond = np.zeros(pol.flat.numel())
    grad_tol = None
    tau = float(g["tau"])
    extra_t = np.zeros(pol.flat.numel())
    for k in range(rounds):
        rows = {f: g[f"{name}_r{k}_{f}"] for f in ("obs", "obs_next", "act", "rew", "term")}
        gs = rows["obs"].transpose(1, 0, 2).reshape(B, S)
        gsn = rows["obs_next"].transpose(1, 0, 2).reshape(B, S)
        out = pol.learn(_batch(rows, N, B, D))
        r = R.learn(rows["obs"], rows["act"], rows["rew"], rows["obs_next"], rows["term"], gs, gsn)
        cond += R.adam_cond()
        for key in ("loss", "q_values"):
            ref64, ref32 = (float(x) for x in g[f"{name}_r{k}_{key}"])
            _check(f"{name} r{k} {key}", [out[key]], [r[key]], abs(ref32 - ref64))
        if k == 0:
            e = float(g[f"{name}_r0_grad_eref"])
            _check(f"{name} r0 grad", _grad_of(pol, B), r["grads"], e)
            grad_tol = 4.0 * max(e, _ulp_floor(r["grads"]))
        extra = np.minimum(cond * grad_tol, 2 * lr * (k + 1))
        _check(f"{name} r{k} weights", pol.flat.double().cpu().numpy(), R.weights(), float(g[f"{name}_r{k}_weights_eref"]),
               extra)
        pol.update_target_networks(tau)
        R.update_targets(tau)
        # a target takes tau x the weight's error per update: t_k = tau w_k + (1 - tau) t_{k-1}
        extra_t = tau * extra + (1 - tau) * extra_t
        _check(f"{name} r{k} targets", pol.target_flat.double().cpu().numpy(), R.targets(),
               float(g[f"{name}_r{k}_targets_eref"]), extra_t)


def test_mixer_forward_matches_restatement():
    g = np.load(GOLD)
    N, D, A, H, S, E, Hh, B, _, mono = (int(x) for x in g["small_dims"])
    dims = (N, D, A, H, S, E, Hh)
    pol = _policy(g["small_init"], dims)
    rs = np.random.RandomState(3)
    q = rs.standard_normal((B, N)).astype(np.float32)
    st = np.ascontiguousarray(g["small_r0_obs"].transpose(1, 0, 2).reshape(B, S))
    got = pol.mixer(torch.as_tensor(q, device=DEV), torch.as_tensor(st, device=DEV))
    assert tuple(got.shape) == (B, 1) and got.is_cuda
    outs = {}
    for dt in (torch.float64, torch.float32):
        R = QmixRestatement(g["small_init"], dims, dtype=dt)
        with torch.no_grad():
            outs[dt] = R._mixer(R.params, torch.as_tensor(q, dtype=dt), torch.as_tensor(st, dtype=dt)).double().numpy()
    _check("mixer forward", got.double().cpu().numpy(), outs[torch.float64],
           np.abs(outs[torch.float32] - outs[torch.float64]).max())


def test_learn_large_batch_against_f64_restatement():
    """configs[2] widths: N 8, D 48, H 128, B 4096, rows drawn under the delta rule, one learn.  Bar: 4 x the error of the
    same restatement in float32 through torch on this GPU, with the 8-ulp floor."""
    N, D, A, H, E, Hh, B = 8, 48, 5, 128, 64, 128, 4096
    S = N * D
    dims = (N, D, A, H, S, E, Hh)
    actors = [DecentralizedActor(D, A, H, device=DEV, seed=10 + i) for i in range(N)]
    mixer = QMIXMixer(N, S, E, Hh, device=DEV, seed=50)
    pol = QMIXPolicy(actors, mixer, None, _Discrete(A), N)
    init = pol.flat.double().cpu().numpy()
    R64 = QmixRestatement(init, dims)
    rows, gs, gsn, share = _draw_rows(R64, N, B, D, A, 8)
    print(f"large batch: redraw share {share:.4f}")
    assert share <= 0.25
    out = pol.learn(_batch(rows, N, B, D))
    r64 = R64.learn(rows["obs"], rows["act"], rows["rew"], rows["obs_next"], rows["term"], gs, gsn)
    R32 = QmixRestatement(init, dims, dtype=torch.float32, device=DEV)
    r32 = R32.learn(rows["obs"], rows["act"], rows["rew"], rows["obs_next"], rows["term"], gs, gsn)
    _check("large grad", _grad_of(pol, B), r64["grads"], np.abs(r32["grads"] - r64["grads"]).max())
    for key in ("loss", "q_values"):
        _check(f"large {key}", [out[key]], [r64[key]], abs(r32[key] - r64[key]))


def test_learn_is_deterministic():
    g = np.load(GOLD)
    N, D, A, H, S, E, Hh, B, _, mono = (int(x) for x in g["small_dims"])
    dims = (N, D, A, H, S, E, Hh)
    rows = {f: g[f"small_r0_{f}"] for f in ("obs", "obs_next", "act", "rew", "term")}
    flats = []
    for _ in range(2):
        pol = _policy(g["small_init"], dims)
        pol.learn(_batch(rows, N, B, D))
        pol.learn(_batch(rows, N, B, D))
        flats.append(pol.flat.cpu().numpy().copy())
    assert np.array_equal(flats[0].view(np.uint32), flats[1].view(np.uint32))


def test_host_forward_bitwise_equal_to_reference():
    g = np.load(GOLD)
    N, D, A, H, B = (int(x) for x in g["fwd_dims"])
    pol = _policy(g["fwd_init"], (N, D, A, H, N * D, 32, 64))
    obs = g["fwd_obs"]
    pol.epsilon = 0.0
    single = pol.forward(Batch(obs=obs[0])).act
    assert np.array_equal(single.numpy(), g["fwd_greedy_single"])
    multi = Batch(**{f"agent_{i}": Batch(obs=obs[i]) for i in range(N)})
    out = pol.forward(multi)
    assert np.array_equal(np.stack([out[f"agent_{i}"].act.numpy() for i in range(N)]), g["fwd_greedy_multi"])
    for tag, eps in (("eps1", 1.0), ("eps05", 0.5)):
        pol.epsilon = eps
        s_np, s_t = (int(x) for x in g[f"fwd_{tag}_seeds"])
        np.random.seed(s_np)
        torch.manual_seed(s_t)
        seq = []
        for _ in range(20):
            o = pol.forward(multi)
            seq.append(np.stack([o[f"agent_{i}"].act.numpy() for i in range(N)]))
        assert np.array_equal(np.stack(seq), g[f"fwd_{tag}"]), tag


def _chi2_crit(dof: int, p: float) -> float:
    """Upper p-quantile of chi^2 with an even number of degrees of freedom (closed-form survival function)."""
    def sf(x):
        term, s = 1.0, 1.0
        for k in range(1, dof // 2):
            term *= (x / 2) / k
            s += term
        return np.exp(-x / 2) * s
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if sf(mid) > p else (lo, mid)
    return hi


def test_act_device_greedy_uniform_coin_and_counter():
    g = np.load(GOLD)
    N, D, A, H, B = (int(x) for x in g["fwd_dims"])
    dims = (N, D, A, H, N * D, 32, 64)
    pol = _policy(g["fwd_init"], dims, seed=17)
    obs = torch.as_tensor(np.ascontiguousarray(g["fwd_obs"].transpose(1, 0, 2)), device=DEV)  # [B, N, D]
    # eps = 0: the f64 argmax of every agent's Q-net (rows drawn away from top-2 ties)
    pol.epsilon = 0.0
    act = pol.act_device(obs)["act"].view(B, N).cpu().numpy()
    R = QmixRestatement(g["fwd_init"], dims)
    with torch.no_grad():
        ref = np.stack([R._actor(R.params, i, torch.as_tensor(g["fwd_obs"][i], dtype=torch.float64)).argmax(1).numpy()
                        for i in range(N)], 1)
    assert np.array_equal(act, ref)
    # eps = 1: uniform actions, chi^2 over >= 1e5 draws at p = 1e-6
    pol.epsilon = 1.0
    big = obs.repeat(64, 1, 1)  # 4096 rows
    counts = np.zeros(A)
    n = 0
    while n < 100_000:
        a = pol.act_device(big)["act"].cpu().numpy()
        counts += np.bincount(a, minlength=A)
        n += a.size
    exp = n / A
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    crit = _chi2_crit(A - 1, 1e-6) if (A - 1) % 2 == 0 else _chi2_crit(A, 1e-6)
    print(f"eps=1: {n} draws, chi2 = {chi2:.2f}, critical {crit:.2f}")
    assert chi2 < crit
    # eps = 0.3: share of random (call, agent) pairs within 5 sigma of 0.3 (a random pair changes some of the B greedy actions)
    pol.epsilon = 0.3
    greedy = ref
    hits, calls = 0, 2000
    for _ in range(calls):
        a = pol.act_device(obs)["act"].view(B, N).cpu().numpy()
        hits += int((a != greedy).any(0).sum())
    m = calls * N
    sigma = np.sqrt(m * 0.3 * 0.7)
    print(f"eps=0.3: {hits} random pairs of {m} (expected {0.3 * m:.0f}, sigma {sigma:.1f})")
    assert abs(hits - 0.3 * m) <= 5 * sigma
    # the same device counter gives the same actions
    pol.epsilon = 0.5
    ctr = torch.tensor([123456], dtype=torch.int64, device=DEV)  # (read as u64)
    a1 = pol.act_device(obs, offset_dev=ctr)["act"].clone()
    a2 = pol.act_device(obs, offset_dev=ctr)["act"].clone()
    assert torch.equal(a1, a2)


def test_collector_epsilon_change_reaches_captured_replay_and_learn_on_buffer_rows():
    from tianshou_marl_amd.algorithm.multiagent import agent_batches_from_buffer
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv

    N, n_env, T = 3, 64, 5
    env = DeviceSimpleSpreadVectorEnv(n_env, N, max_cycles=25, device=DEV, seed=3)
    D, A = env.obs_dim, 5
    dims = (N, D, A, 64, N * D, 32, 64)

    def make():
        actors = [DecentralizedActor(D, A, 64, device=DEV, seed=i) for i in range(N)]
        return QMIXPolicy(actors, QMIXMixer(N, N * D, device=DEV, seed=7), None, _Discrete(A), N, epsilon=0.0, seed=5)

    pol = make()
    buf = DeviceVectorReplayBuffer(n_env * T * 3, n_env, N, D, device=DEV)
    col = Collector(pol, env, buf)
    col.reset()
    assert col._actor_of(pol) is None and not col._can_fuse()

    def collected(k):  # the rows of the k-th collect: slots [k T, (k + 1) T)
        obs = buf.obs_store[k * T:(k + 1) * T].reshape(-1, N, D)
        act = buf.act_store[k * T:(k + 1) * T].reshape(-1, N).long()
        greedy = torch.stack([pol.actors[i](obs[:, i].contiguous())[0].argmax(1) for i in range(N)], 1)
        return act, greedy

    col.collect(n_step=n_env * T)       # eager (first call of this size)
    col.collect(n_step=n_env * T)       # captured, replayed
    act, greedy = collected(1)
    assert torch.equal(act, greedy)
    pol.epsilon = 1.0
    col.collect(n_step=n_env * T)       # the same captured graph, replayed with the new epsilon
    act, greedy = collected(2)
    frac = float((act != greedy).double().mean())
    print(f"collector: share of non-greedy actions after eps 0 -> 1: {frac:.3f}")
    assert frac > 0.5
    # learn on the device batch equals learn on the same rows as numpy, bit for bit
    batches = agent_batches_from_buffer(buf, env.agents)
    pa, pb = make(), make()
    pb.flat.copy_(pa.flat)
    pb.target_flat.copy_(pa.target_flat)
    npb = Batch()
    for i, name in enumerate(env.agents):
        src = batches[name]
        npb[f"agent_{i}"] = Batch(**{k: src[k].cpu().numpy() for k in ("obs", "act", "rew", "obs_next", "terminated")})
        batches[f"agent_{i}"] = src
    npb["global_obs"] = batches.global_obs.cpu().numpy()
    npb["global_obs_next"] = batches.global_obs_next.cpu().numpy()
    ra, rb = pa.learn(batches), pb.learn(npb)
    assert np.array_equal(pa.flat.cpu().numpy().view(np.uint32), pb.flat.cpu().numpy().view(np.uint32))
    assert ra == rb


def test_state_dict_matches_reference_keys_and_round_trips():
    g = np.load(GOLD)
    N, D, A = 3, 18, 5
    actors = [DecentralizedActor(D, A, 64, device=DEV, seed=i) for i in range(N)]
    pol = QMIXPolicy(actors, QMIXMixer(N, N * D, device=DEV, seed=1), None, _Discrete(A), N)
    sd = pol.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g["sd_shapes"]]
    pol2 = QMIXPolicy([DecentralizedActor(D, A, 64, device=DEV, seed=9 + i) for i in range(N)],
                      QMIXMixer(N, N * D, device=DEV, seed=2), None, _Discrete(A), N)
    pol2.load_state_dict(sd)
    for k, v in pol2.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_optimizer_argument():
    N, D, A = 2, 6, 3
    actors = [DecentralizedActor(D, A, 16, device=DEV, seed=i) for i in range(N)]
    p = torch.nn.Parameter(torch.zeros(1))
    pol = QMIXPolicy(actors, QMIXMixer(N, N * D, device=DEV), None, _Discrete(A), N,
                     optimizer=torch.optim.Adam([p], lr=3e-4, betas=(0.8, 0.99), eps=1e-6))
    assert (pol.optimizer.lr, pol.optimizer.betas, pol.optimizer.eps) == (3e-4, (0.8, 0.99), 1e-6)
    with pytest.raises(TypeError):
        QMIXPolicy([DecentralizedActor(D, A, 16, device=DEV) for _ in range(N)], QMIXMixer(N, N * D, device=DEV), None,
                   _Discrete(A), N, optimizer=torch.optim.SGD([p], lr=0.1))
    assert ops.qmix_partial_elems(64, 64) == 2 * 4


@pytest.mark.parametrize("E", [32, 64])
def test_partial_last_workgroup(E):
    """B = 250 leaves a partial last workgroup in the mix kernel (16 or 32 rows each) and B = 37 in the epsilon-greedy kernel
    (16 rows each): learn, the mixer's forward and act_device against float64, and no store past the rows."""
    N, D, A, H, Hh, B = 3, 18, 5, 64, 64, 250
    S = N * D
    dims = (N, D, A, H, S, E, Hh)
    pol = QMIXPolicy([DecentralizedActor(D, A, H, device=DEV, seed=30 + i) for i in range(N)],
                     QMIXMixer(N, S, E, Hh, device=DEV, seed=60), None, _Discrete(A), N)
    init = pol.flat.double().cpu().numpy()
    R64 = QmixRestatement(init, dims)
    rows, gs, gsn, share = _draw_rows(R64, N, B, D, A, 9)
    assert share <= 0.25
    # the mixer alone on this batch
    q = torch.as_tensor(rows["rew"].T.copy(), device=DEV)  # any [B, N] values
    got = pol.mixer(q, torch.as_tensor(gs, device=DEV))
    R32 = QmixRestatement(init, dims, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        m64 = R64._mixer(R64.params, q.cpu().double(), torch.as_tensor(gs, dtype=torch.float64)).numpy()
        m32 = R32._mixer(R32.params, q, torch.as_tensor(gs, device=DEV)).double().cpu().numpy()
    _check(f"tail E{E} mixer forward", got.double().cpu().numpy(), m64, np.abs(m32 - m64).max())
    # acting on 37 envs; the action array carries a guard row behind them
    Bg = 37
    obs = torch.as_tensor(np.ascontiguousarray(rows["obs"][:, :Bg].transpose(1, 0, 2)), device=DEV)
    act = torch.full(((Bg + 1) * N,), -7, dtype=torch.int32, device=DEV)
    buf = dict(act=act[:Bg * N], logp=torch.empty(Bg * N, device=DEV), value=torch.empty(Bg * N, device=DEV))
    with torch.no_grad():  # (before the learn: the rows' top-2 gaps were kept clear of ties at these weights)
        ref = np.stack([R64._actor(R64.params, i, torch.as_tensor(rows["obs"][i, :Bg], dtype=torch.float64)).argmax(1).numpy()
                        for i in range(N)], 1)
    pol.epsilon = 0.0
    pol.act_device(obs, out=buf)
    assert np.array_equal(act[:Bg * N].view(Bg, N).cpu().numpy(), ref)
    pol.epsilon = 1.0
    pol.act_device(obs, out=buf)
    a = act.cpu().numpy()
    assert ((a[:Bg * N] >= 0) & (a[:Bg * N] < A)).all() and (a[Bg * N:] == -7).all()
    # one learn
    out = pol.learn(_batch(rows, N, B, D))
    r64 = R64.learn(rows["obs"], rows["act"], rows["rew"], rows["obs_next"], rows["term"], gs, gsn)
    r32 = R32.learn(rows["obs"], rows["act"], rows["rew"], rows["obs_next"], rows["term"], gs, gsn)
    _check(f"tail E{E} grad", _grad_of(pol, B), r64["grads"], np.abs(r32["grads"] - r64["grads"]).max())
    for key in ("loss", "q_values"):
        _check(f"tail E{E} {key}", [out[key]], [r64[key]], abs(r32[key] - r64[key]))


def test_policy_construction_draws_nothing_from_the_global_rng():
    """The reference deep-copies its targets (no draw): building the policy leaves the global torch RNG where it was, so a
    seeded script's later torch.randint (forward's random actions) and nn.Linear inits are the reference's."""
    N, D, A = 3, 18, 5
    actors = [DecentralizedActor(D, A, 64, device=DEV, seed=i) for i in range(N)]
    mixer = QMIXMixer(N, N * D, device=DEV, seed=1)
    torch.manual_seed(123)
    QMIXPolicy(actors, mixer, None, _Discrete(A), N)
    after = torch.rand(8)
    torch.manual_seed(123)
    assert torch.equal(after, torch.rand(8))
