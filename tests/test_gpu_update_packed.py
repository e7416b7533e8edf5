"""GPU tests (`-m gpu`) of the packed minibatch rows: `tsm_ppo_pack_minibatches` gathers every minibatch's rows once per update
into 16-row tile records (in the statistics launch), `tsm_ppo_update_fused_packed` reads a tile's record instead of row ids and
the rows behind them.  The records are a copy, so everything downstream must keep its bits: records against a torch gather,
gradient slabs and loss partials of the packed path against the `perm` path of the same kernel, and a whole `PPO.update`
with and without the workspace, captured and eager."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.algorithm.ppo import PPO, policy_within_training_step
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer
    from tianshou_marl_amd.data.collector import Collector
    from tianshou_marl_amd.env.mpe import DeviceSimpleSpreadVectorEnv
    from tianshou_marl_amd.utils.net import DiscreteActorCritic

DEV = "cuda"


def _rows(n, D, A, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(n, D, generator=g).to(DEV)
    act = torch.randint(0, A, (n,), generator=g, dtype=torch.int32).to(DEV)
    logp, adv, ret, v_old = (torch.randn(n, generator=g).to(DEV) for _ in range(4))
    return obs, act, logp * 0.3 - 1.5, adv, ret, v_old


# (obs_dim, n_act, rows of the buffer, rows of the minibatch, n_blocks or None = the grid rule)
_SHAPES = [
    (18, 5, 64, 5, None),       # fewer rows than one tile
    (18, 5, 64, 16, None),      # exactly one tile
    (18, 5, 300, 115, None),    # 16 * 7 + 3: ragged last tile; obs_dim 18 is a compiled-for width
    (18, 5, 1000, 200, 5),      # 13 tiles on 5 workgroups (3, 3, 3, 2, 2: the record prefetch), 200 rows chosen from 1000
    (16, 5, 300, 115, 3),       # the other compiled-for width, up to 3 tiles per workgroup
    (10, 5, 300, 115, None),    # a generic width (run-time dimensions)
    (10, 7, 1000, 200, 6),      # generic width and action count, several tiles per workgroup
]


@pytest.mark.parametrize("value_clip,adv_norm", [(False, True), (True, True), (False, False), (True, False)])
@pytest.mark.parametrize("shape", _SHAPES)
def test_packed_path_equals_perm_path_bit_for_bit(shape, value_clip, adv_norm):
    """The same kernel fed through `perm` and through the packed records: equal gradient slabs and loss partials."""
    D, A, n, M, n_blocks = shape
    obs, act, logp, adv, ret, v_old = _rows(n, D, A, seed=D * 1000 + M)
    net = DiscreteActorCritic(D, A, 64, device=DEV, seed=3)
    cfg = ops.make_ppo_cfg(value_clip=value_clip, adv_norm=adv_norm)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(M)).to(DEV)[:M].contiguous()
    mb_start = torch.tensor([0, M], device=DEV)
    ws = ops.ppo_pack_workspace([M], D, DEV)
    stats = ops.ppo_pack_minibatches(ws, adv, mb_start, perm, obs, act, logp, ret, v_old if value_clip else None)
    assert torch.equal(stats, ops.ppo_adv_stats(adv, mb_start, perm=perm))
    nb = n_blocks or ops.ppo_update_grid(M)
    out = []
    for packed in (None, ws["rows"](0)):
        partial = torch.full((nb * 4,), float("nan"), dtype=torch.float64, device=DEV)
        slabs, sc = ops.ppo_update_fused(net.flat.data, obs, act, logp, adv, ret, cfg, A, 64, adv_stats=stats[0] if adv_norm else None,
                                         perm=perm, M=M, v_s_old=v_old if value_clip else None, image=net.image, n_blocks=nb,
                                         partial=partial, packed=packed)
        torch.cuda.synchronize()
        out.append((slabs.clone(), partial, sc.clone()))
    assert torch.isfinite(out[0][0]).all() and out[0][0].abs().sum() > 0
    assert torch.equal(out[0][0], out[1][0]), "gradient slabs"
    assert torch.equal(out[0][1], out[1][1]), "loss partials"
    assert torch.equal(out[0][2], out[1][2]), "loss statistics"


@pytest.mark.parametrize("D,with_v_old,with_perm", [(18, True, True), (10, False, True), (33, True, False)])
def test_packed_records_equal_a_torch_gather(D, with_v_old, with_perm):
    """One launch, several minibatches of different (ragged) sizes out of a larger buffer: every record field against a torch
    gather of the same rows, the rows past a minibatch's end zero, the statistics those of `ppo_adv_stats`; nothing written
    past the last record."""
    n, sizes = 1000, [5, 16, 115, 200, 64]
    obs, act, logp, adv, ret, v_old = _rows(n, D, 5, seed=D)
    total = sum(sizes)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)[:total].contiguous() if with_perm else None
    starts = np.concatenate([[0], np.cumsum(sizes)])
    mb_start = torch.as_tensor(starts, dtype=torch.int64, device=DEV)
    ws = ops.ppo_pack_workspace(sizes, D, DEV)
    rec = ops.ppo_packed_record_elems(D)
    assert rec == 16 * D + 80 and rec % 4 == 0
    assert ws["tile_start_host"] == [0, 1, 2, 10, 23, 27] and tuple(ws["packed"].shape) == (27, rec)
    guard = torch.full((27 + 4, rec), 7.0, device=DEV)   # the workspace inside a larger allocation: records 27.. stay untouched
    ws["packed"] = guard[:27]
    stats = ops.ppo_pack_minibatches(ws, adv, mb_start, perm, obs, act, logp, ret, v_old if with_v_old else None)
    assert torch.equal(stats, ops.ppo_adv_stats(adv, mb_start, perm=perm))
    assert torch.equal(guard[27:], torch.full((4, rec), 7.0, device=DEV))
    for k, M in enumerate(sizes):
        ids = perm[starts[k]:starts[k + 1]] if with_perm else torch.arange(starts[k], starts[k + 1], device=DEV)
        r = ws["rows"](k)
        nt = (M + 15) // 16
        assert r.shape[0] == nt

        def padded(x):   # [M, ...] -> [nt, 16, ...] with zero rows behind the minibatch's end
            z = torch.zeros(nt * 16, *x.shape[1:], dtype=x.dtype, device=DEV)
            z[:M] = x
            return z.view(nt, 16, *x.shape[1:])

        assert torch.equal(r[:, :16 * D].view(nt, 16, D), padded(obs[ids]))
        f = r[:, 16 * D:].view(nt, 5, 16)
        assert torch.equal(f[:, 0].contiguous().view(torch.int32), padded(act[ids]))
        assert torch.equal(f[:, 1], padded(logp[ids])) and torch.equal(f[:, 2], padded(adv[ids]))
        assert torch.equal(f[:, 3], padded(ret[ids]))
        assert torch.equal(f[:, 4], padded((v_old if with_v_old else ret)[ids]))
    with pytest.raises(ValueError):   # a minibatch the one-workgroup statistics cannot hold
        ops.ppo_pack_workspace([8193], D, DEV)
    with pytest.raises(ValueError):   # too few records for the rows
        ops.ppo_update_fused(torch.zeros(8, device=DEV), obs, act, logp, adv, ret, ops.make_ppo_cfg(), 5, 64, perm=perm, M=115,
                             packed=ws["rows"](0))


@pytest.mark.parametrize("shuffle", ["numpy", "device"])
def test_ppo_update_with_and_without_packed_rows_graph_and_eager(shuffle):
    """64 envs x 3 agents x 5 steps, minibatches of 96 rows: the captured update and the eager one, each with and without the
    packed workspace -- parameters and Adam moments of all four agree bit for bit."""
    def run(use_graph, pack_rows):
        env = DeviceSimpleSpreadVectorEnv(64, 3, max_cycles=25, device=DEV, seed=11)
        net = DiscreteActorCritic(env.obs_dim, env.n_act, 64, device=DEV, seed=11)
        algo = PPO(net=net, seed=11, shuffle=shuffle, use_graph=use_graph, max_grad_norm=0.5)
        np.random.seed(5)   # (shuffle="numpy" draws its permutations from the global generator)
        algo.pack_rows = pack_rows
        buf = DeviceVectorReplayBuffer(64 * 5, 64, 3, env.obs_dim, device=DEV)
        col = Collector(algo, env, buf, use_graph=use_graph)
        col.reset()
        for _ in range(3):   # (the captured update replays from the second call on)
            with policy_within_training_step(algo):
                col.collect(n_step=64 * 5)
                algo.update(buf, 96, 2)
            col.reset_buffer(keep_statistics=True)
        packed = [v["packed"] for v in algo._ws.values() if isinstance(v, dict) and v.get("packed") is not None]
        packed += [v for k, v in algo._ws.items() if isinstance(k, tuple) and k[0] == "packed"]
        assert bool(packed) == pack_rows
        assert algo.opt_step >= 3 * 2 * 9   # (several minibatches per pass, two passes per update)
        return [x.clone() for x in (net.flat.data, algo.exp_avg, algo.exp_avg_sq)] + [torch.tensor(algo.opt_step)]

    ref = run(False, False)
    assert all(torch.isfinite(x).all() for x in ref[:3])
    for use_graph, pack_rows in [(False, True), (True, False), (True, True)]:
        for a, b in zip(ref, run(use_graph, pack_rows)):
            assert torch.equal(a, b), (use_graph, pack_rows)
