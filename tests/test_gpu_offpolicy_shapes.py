"""GPU tests (`-m gpu`) of the off-policy kernels at their shape limits: tsm_dqn_td_head (csrc/dqn.hip), tsm_distq_values /
tsm_c51_head / tsm_qrdqn_head (csrc/distq.hip), tsm_iqn_values / tsm_iqn_head / tsm_iqn_embed_forward / _backward
(csrc/iqn.hip), the three Discrete SAC heads (csrc/dsac.hip), the n-step walk (csrc/nstep.hip) and the sum tree
(csrc/segtree.hip) -- the row, lane, register, workgroup and strided-loop boundaries that the fixture tests (B = 37, n <= 300)
do not reach.  Cases, inputs and float64 yardsticks: tests/offpolicy_cases.py (the project's restatements, each pinned to the
reference to 1e-10 by its host test; tests/test_host_offpolicy_shapes.py checks the preconditions on the CPU).  Bars, all of
them the sibling files' own:
  * heads, values, embedding, losses and mean q (through tsm_qmix_finalize): test_gpu_distq._bar,
    max |hip - ref64| <= 1e-5 max |ref64| + e_ref, e_ref = max |restatement(float32) - restatement(float64)| at that shape;
  * a*, greedy actions, zeros of the gradient off the taken action, the embedding's gates, idx_n, vmask, leaf indices, the
    tree after a set (the same float64 additions): exact;
  * mc, gamma^m, leaves written from float32 TD errors, max / min priority, IS weights: test_gpu_dqn._rel (1e-5 of the
    array's scale); with alpha = 1 the leaves are bit-exact; every inner node is exactly the sum of its stored children.
Every variant of every case is launched twice and must give the same bits.  Every comparison prints `PARITY name: ...`."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import offpolicy_cases as oc  # noqa: E402
from distq_restatement import support_of, tau_hat_of  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_gpu_dqn import _d, _rel  # noqa: E402
from test_gpu_iqn import _bits  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import ops
    from tianshou_marl_amd.data import Batch
    from tianshou_marl_amd.data.buffer import DeviceVectorReplayBuffer


def _same_bits(name, a, b):
    """Two launches of one call: every output tensor bit for bit."""
    a, b = (x if isinstance(x, dict) else dict(enumerate(x if isinstance(x, (tuple, list)) else (x,))) for x in (a, b))
    for key in a:
        x, y = a[key], b[key]
        assert torch.equal(_bits(x), _bits(y)) if x.is_floating_point() else torch.equal(x, y), (name, key)


def _exact(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    bad = np.nonzero(got != ref)[0] if got.shape == ref.shape else None
    print(f"PARITY {name}: {got.size} entries, equal" if bad is not None and not len(bad) else f"PARITY {name}: DIFFERS at {bad}")
    assert got.shape == ref.shape and np.array_equal(got, ref), (name, bad)


def _finalized(partial, B, slot):
    ops.qmix_finalize(partial, B, slot)
    return slot.cpu().numpy().astype(np.float64)


def _worst(tag, worst):
    print(f"PARITY {tag} worst:", {k: f"{v:.3g}" for k, v in worst.items()})


# ---- DQN TD head ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.DQN_CASES, ids=oc.case_id)
def test_dqn_td_head(c):
    d, ref = oc.dqn_inputs(c), oc.dqn_reference(c)
    B, A = c["B"], c["A"]
    assert ref["greedy_margin"] > 1.0
    q, on, tg, act, vmask, weight, mask = (_d(d[k]) for k in ("q", "on", "tg", "act", "vmask", "weight", "mask"))
    mc, gpow = _d(d["mc"], torch.float32), _d(d["gpow"], torch.float32)
    slot = torch.zeros(2, device=DEV)
    rows, worst = np.arange(B), {}
    for v in oc.DQN_VARIANTS:
        dbl, tgt, loss, msk = v
        run = lambda: ops.dqn_td_head(q, on, tg if tgt else None, act, mc, gpow, vmask, mask_next=mask if msk else None,  # noqa: E731
                                      weight=weight if loss == "msew" else None, is_double=bool(dbl),
                                      huber_delta=oc.HUBER_DELTA if loss == "huber" else None)
        h = run()
        _same_bits(f"dqn {oc.case_id(c)} {v}", h, run())
        assert h["partial"].numel() == 2 * -(-B // 256)
        stat = _finalized(h["partial"], B, slot)
        r = ref["variants"][v]
        dq = h["dq"].cpu().numpy()
        off = dq.copy()
        off[rows, d["act"]] = 0.0
        assert not off.any(), v   # exactly zero off the taken action
        p = f"dqn {oc.case_id(c)} d{dbl}t{tgt}_{loss}_m{msk} "
        for key, got, want, e in (("returns", h["returns"].cpu().numpy(), r["returns"], r["e_ref"]["returns"]),
                                  ("td_error", h["td_error"].cpu().numpy(), r["td_error"], r["e_ref"]["td_error"]),
                                  ("dq", dq, r["dq"], r["e_ref"]["dq"]),
                                  ("loss", [stat[0]], [r["loss"]], r["e_ref"]["loss"]),
                                  ("mean_q", [stat[1]], [ref["mean_q"]], ref["mean_q_eref"])):
            worst[key] = max(worst.get(key, 0.0), _bar(p + key, got, want, e))
    _worst(f"dqn {oc.case_id(c)}", worst)


# ---- C51 / QR-DQN ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.DISTQ_CASES, ids=oc.case_id)
def test_distq_values_and_heads(c):
    d, ref = oc.distq_inputs(c), oc.distq_reference(c)
    B, A, N = c["B"], c["A"], c["N"]
    assert ref["greedy_margin"] > 1.0
    raw, on, tg, act, vmask, weight, mask = (_d(d[k]) for k in ("raw", "on", "tg", "act", "vmask", "weight", "mask"))
    mc, gpow = _d(d["mc"], torch.float32), _d(d["gpow"], torch.float32)
    eps0, slot = torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
    rows, worst = np.arange(B), {}
    for kind in ("c5", "qr"):
        aux = _d(support_of(oc.V_MIN, oc.V_MAX, N) if kind == "c5" else tau_hat_of(N), torch.float32)
        p = f"distq {oc.case_id(c)} {kind} "
        rv = ref["values"][kind]
        if kind == "c5":
            vals = lambda: ops.distq_values(on, A, N, support=aux, want_probs=True)  # noqa: E731
            q_next, probs = vals()
            assert probs.shape == (B, A, N)
            worst["probs"] = max(worst.get("probs", 0.0), _bar(p + "probs", probs.cpu().numpy(), rv["probs"], rv["e_ref"]["probs"]))
        else:
            vals = lambda: ops.distq_values(on, A, N)  # noqa: E731
            q_next = vals()
        _same_bits(p + "values", vals(), vals())
        worst["q"] = max(worst.get("q", 0.0), _bar(p + "q", q_next.cpu().numpy(), rv["q"], rv["e_ref"]["q"]))
        _exact(p + "greedy act", ops.dqn_egreedy(q_next, eps0, 0).cpu().numpy(), rv["act"])
        _exact(p + "greedy act (masked)", ops.dqn_egreedy(q_next, eps0, 0, mask=mask).cpu().numpy(), rv["act_masked"])
        for v in oc.HEAD_VARIANTS:
            tgt, wgt, msk = v
            args = (raw, q_next, tg if tgt else on, act, mc, gpow, vmask, aux)
            kw = dict(mask_next=mask if msk else None, weight=weight if wgt else None)
            run = (lambda: ops.c51_head(*args, oc.V_MIN, oc.V_MAX, **kw)) if kind == "c5" else (lambda: ops.qrdqn_head(*args, **kw))  # noqa: E731
            h = run()
            _same_bits(p + str(v), h, run())
            assert h["partial"].numel() == 2 * -(-B // 16)
            stat = _finalized(h["partial"], B, slot)
            r = ref["variants"][kind, v]
            dout = h["d_out"].cpu().numpy().reshape(B, A, N)
            off = dout.copy()
            off[rows, d["act"]] = 0.0
            assert not off.any(), v   # exactly zero off the taken action
            pv = p + f"t{tgt}w{wgt}m{msk} "
            # a* itself: the rows of the next distribution it selects show in the returns (QR-DQN) and the priorities (both)
            for key, got, want in (("returns", h["returns"].cpu().numpy(), r["returns"]), ("prio", h["prio"].cpu().numpy(), r["prio"]),
                                   ("d_out", dout, r["d_out"].reshape(B, A, N)), ("loss", [stat[0]], [r["loss"]]),
                                   ("mean_q", [stat[1]], [r["mean_q"]])):
                worst[key] = max(worst.get(key, 0.0), _bar(pv + key, got, want, r["e_ref"][key]))
    _worst(f"distq {oc.case_id(c)}", worst)


# ---- IQN values and head --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.IQN_CASES, ids=oc.case_id)
def test_iqn_values_and_head(c):
    d, ref = oc.iqn_inputs(c), oc.iqn_reference(c)
    B, A, N, Np = c["B"], c["A"], c["N"], c["Np"]
    assert ref["greedy_margin"] > 1.0
    out, on, tg, taus, act, vmask, weight, mask = (_d(d[k]) for k in ("out", "on", "tg", "taus", "act", "vmask", "weight", "mask"))
    mc, gpow = _d(d["mc"], torch.float32), _d(d["gpow"], torch.float32)
    eps0, slot = torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
    rows, worst = np.arange(B), {}
    p = f"iqn {oc.case_id(c)} "
    q_next = ops.iqn_values(on, N, A)
    _same_bits(p + "values", q_next, ops.iqn_values(on, N, A))
    rv = ref["values"]
    worst["q"] = _bar(p + "q", q_next.cpu().numpy(), rv["q"], rv["e_ref"]["q"])
    _exact(p + "greedy act", ops.dqn_egreedy(q_next, eps0, 0).cpu().numpy(), rv["act"])
    _exact(p + "greedy act (masked)", ops.dqn_egreedy(q_next, eps0, 0, mask=mask).cpu().numpy(), rv["act_masked"])
    for v in oc.HEAD_VARIANTS:
        tgt, wgt, msk = v
        run = lambda: ops.iqn_head(out, q_next, tg if tgt else on, taus, act, mc, gpow, vmask, mask_next=mask if msk else None,  # noqa: E731
                                   weight=weight if wgt else None)
        h = run()
        _same_bits(p + str(v), h, run())
        assert h["partial"].numel() == 2 * -(-B // 16)
        stat = _finalized(h["partial"], B, slot)
        r = ref["variants"][v]
        dout = h["d_out"].cpu().numpy()
        assert dout.shape == (B, N, A) and h["returns"].shape == (B, Np if tgt else N)
        off = dout.copy()
        off[rows, :, d["act"]] = 0.0
        assert not off.any(), v   # exactly zero off the taken action
        pv = p + f"t{tgt}w{wgt}m{msk} "
        for key, got, want in (("returns", h["returns"].cpu().numpy(), r["returns"]), ("prio", h["prio"].cpu().numpy(), r["prio"]),
                               ("d_out", dout, r["d_out"]), ("loss", [stat[0]], [r["loss"]]), ("mean_q", [stat[1]], [r["mean_q"]])):
            worst[key] = max(worst.get(key, 0.0), _bar(pv + key, got, want, r["e_ref"][key]))
    _worst(f"iqn {oc.case_id(c)}", worst)


# ---- IQN embedding --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.EMBED_CASES, ids=oc.case_id)
def test_iqn_embedding_forward_and_backward(c):
    d, r = oc.embed_inputs(c), oc.embed_reference(c)
    B, S, C, H, act_f = c["B"], c["S"], c["C"], c["H"], bool(c["relu_f"])
    assert r["min_abs_pre"] >= oc.MIN_ABS_PRE
    f, t, We, be, d_e = (_d(d[k]) for k in ("f", "taus", "We", "be", "d_e"))
    p = f"embed {oc.case_id(c)} "
    worst = {}
    e, phi = ops.iqn_embed_forward(f, t, We, be, relu_f=act_f)
    _same_bits(p + "forward", (e, phi), ops.iqn_embed_forward(f, t, We, be, relu_f=act_f))
    assert e.shape == (B * S, H) and phi.shape == (B * S, H)
    worst["e"] = _bar(p + "e", e.cpu().numpy(), r["e"], r["e_ref"]["e"])
    _exact(p + "gates", (phi.cpu().numpy() > 0).reshape(-1), (r["pre"] > 0).reshape(-1))
    nW = H * C

    def grads(tag, total, d_f):
        for key, got in (("d_f", d_f.cpu().numpy()), ("dWe", total[:nW].reshape(H, C)), ("dbe", total[nW:nW + H])):
            worst[key] = max(worst.get(key, 0.0), _bar(f"{p}{key} ({tag})", got, r[key], r["e_ref"][key]))

    for n_split in (1, 3, B + 2):   # one slab; uneven slabs; more slabs than batch rows: the empty ones are written as zeros
        run = lambda: ops.iqn_embed_backward(d_e, f, phi, t, We, be, n_split, relu_f=act_f)  # noqa: E731
        d_f, slabs = run()
        _same_bits(f"{p}backward n_split {n_split}", (d_f, slabs), run())
        assert slabs.shape == (n_split, nW + H)
        if n_split > B:
            assert not slabs[B:].any()
        grads(f"{n_split} slabs", slabs.double().sum(0).cpu().numpy(), d_f)
    # three slabs inside a wider joint layout whose other slots must stay
    n_split, P, w_off = 3, nW + H + 24, 16
    wide = torch.full((n_split, P), 7.0, device=DEV)
    d_f, _ = ops.iqn_embed_backward(d_e, f, phi, t, We, be, n_split, slabs=wide, slab_stride=P, w_off=w_off, relu_f=act_f)
    grads("joint slabs", wide.double().sum(0).cpu().numpy()[w_off:], d_f)
    assert (wide[:, :w_off] == 7.0).all() and (wide[:, w_off + nW + H:] == 7.0).all()
    _worst(f"embed {oc.case_id(c)}", worst)


# ---- Discrete SAC heads ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.DSAC_CASES, ids=oc.case_id)
def test_dsac_heads(c):
    d, ref = oc.dsac_inputs(c), oc.dsac_reference(c)
    B, A = c["B"], c["A"]
    lnext, q1n, q2n, logits, q1, q2, act, vmask, weight = (_d(d[k]) for k in ("lnext", "q1n", "q2n", "logits", "q1", "q2", "act",
                                                                                  "vmask", "weight"))
    mc, gpow = _d(d["mc"], torch.float32), _d(d["gpow"], torch.float32)
    slot = torch.zeros(2, 2, device=DEV)
    rows, worst = np.arange(B), {}
    for v in oc.DSAC_VARIANTS:
        wgt, auto = v
        r = ref[v]
        a_dev = torch.tensor([oc.DSAC_ALPHA[auto]], dtype=torch.float32, device=DEV)

        def run():
            ret = ops.dsac_target(lnext, q1n, q2n, a_dev, mc, gpow, vmask)
            ch = ops.dsac_critic_head(q1, q2, act, ret, weight if wgt else None)
            ah = ops.dsac_actor_head(logits, q1, q2, a_dev)
            return dict(returns=ret, **{"c_" + k: x for k, x in ch.items()}, **{"a_" + k: x for k, x in ah.items()})

        h = run()
        p = f"dsac {oc.case_id(c)} w{wgt}a{auto} "
        _same_bits(p, h, run())
        assert h["c_partial"].numel() == h["a_partial"].numel() == 2 * -(-B // 16)
        cstat, astat = _finalized(h["c_partial"], B, slot[0]), _finalized(h["a_partial"], B, slot[1])
        for k in ("c_dq1", "c_dq2"):
            off = h[k].cpu().numpy().copy()
            off[rows, d["act"]] = 0.0
            assert not off.any(), (v, k)   # exactly zero off the taken action
        checks = [("returns", h["returns"].cpu().numpy(), r["returns"]), ("dq1", h["c_dq1"].cpu().numpy(), r["dq1"]),
                  ("dq2", h["c_dq2"].cpu().numpy(), r["dq2"]), ("prio", h["c_prio"].cpu().numpy(), r["prio"]),
                  ("d_logits", h["a_d_logits"].cpu().numpy(), r["d_logits"]), ("entropy", h["a_entropy"].cpu().numpy(), r["entropy"]),
                  ("critic1_loss", [cstat[0]], [r["critic1_loss"]]), ("critic2_loss", [cstat[1]], [r["critic2_loss"]]),
                  ("actor_loss", [astat[0]], [r["actor_loss"]]), ("mean_entropy", [astat[1]], [r["mean_entropy"]])]
        if auto:   # AutoAlpha.update from the actor head's entropy partials, on device scalars
            outs = []
            for _ in range(2):
                la = torch.full((), oc.DSAC_LOG_ALPHA, device=DEV)
                m, s, t = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
                a_out, out = torch.ones(1, device=DEV), torch.zeros(2, device=DEV)
                ops.dsac_alpha_step(h["a_partial"], B, la, m, s, t, oc.DSAC_TARGET_ENTROPY, a_out, out, lr=oc.DSAC_LR)
                outs.append((la.reshape(1), out, a_out))
                assert int(t) == 1
            _same_bits(p + "alpha step", outs[0], outs[1])
            checks += [("log_alpha", [float(outs[0][0])], [r["log_alpha"]]), ("alpha_loss", [float(outs[0][1][0])], [r["alpha_loss"]]),
                       ("alpha", [float(outs[0][1][1])], [r["alpha"]])]
        for key, got, want in checks:
            worst[key] = max(worst.get(key, 0.0), _bar(p + key, got, want, r["e_ref"][key]))
    _worst(f"dsac {oc.case_id(c)}", worst)


# ---- n-step walk ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buffer_num,sub_size", oc.NSTEP_BUFFERS)
def test_nstep_walk(buffer_num, sub_size):
    rb, script, idx = oc.nstep_restated(buffer_num, sub_size)
    D = oc.NSTEP_REW_DIM
    buf = DeviceVectorReplayBuffer(buffer_num * sub_size, buffer_num, n_agent=D, obs_dim=3, device=DEV)
    z = np.zeros((1, D, 3), np.float32)
    for env, rew, term, trunc in script:   # agent k's lane carries reward column k
        buf.add(Batch(obs=z, act=np.zeros((1, D), np.int64), rew=rew[None], terminated=np.array([term]), truncated=np.array([trunc]),
                      obs_next=z), buffer_ids=[env])
    assert np.array_equal(buf.sample_indices(0), rb.sample_indices_all()) and np.array_equal(buf.unfinished_index(), rb.unfinished_index())
    idx_d = _d(idx)
    assert len(idx) > 256   # a second workgroup
    worst = {}
    for n_step in oc.nstep_horizons(sub_size):
        for gamma in oc.NSTEP_GAMMAS:
            for col in oc.NSTEP_COLS:
                r = oc.nstep_reference(rb, idx, n_step, gamma, col)
                run = lambda: ops.nstep_return(buf.index, buf.term_store, buf.rew_store, idx_d, n_step, gamma, rew_col=col, term_col=col)  # noqa: E731
                got = run()
                p = f"nstep ({buffer_num}, {sub_size}) n{n_step} g{gamma} c{col} "
                _same_bits(p, got, run())
                idx_n, mc, gpow, vmask = (x.cpu().numpy() for x in got)
                assert np.array_equal(idx_n, r["idx_n"]), p
                assert np.array_equal(vmask.astype(bool), r["vmask"]), p
                _rel(p + "mc", mc, r["mc"])
                _rel(p + "gpow", gpow, r["gpow"])
    print(f"PARITY nstep ({buffer_num}, {sub_size}): idx_n and vmask equal over {len(idx)} indices for every (n_step, gamma, column)")


# ---- sum tree -------------------------------------------------------------------------------------------------------------
def _tree_is_clean(t):
    assert (t.mark == -1).all()
    t.check()   # raises if a launch met an index outside [0, size)


@pytest.mark.parametrize("size", oc.TREE_SIZES)
def test_segtree_set_and_sample(size):
    t = ops.DeviceSegmentTree(size, device=DEV)
    for (idx, val), ref in zip(oc.tree_set_calls(size), oc.tree_after(size)):
        ops.segtree_set(t, _d(idx), _d(val))
        _exact(f"tree size {size} set n {len(idx)}: whole tree", t.tree.cpu().numpy(), ref)
        _tree_is_clean(t)
        ops.segtree_set(t, _d(idx), _d(val))   # the same call again: the same tree
        assert np.array_equal(t.tree.cpu().numpy(), ref)
        _tree_is_clean(t)
    if size == oc.TREE_SIZES[-1]:   # per_sample on the large, mostly empty tree: every draw lands on a leaf that holds weight
        n, seed = 4099, 77
        a = ops.per_sample(t, n, seed, offset=1000)
        an = a.cpu().numpy()
        leaves = t.tree.cpu().numpy()[t.bound:]
        assert an.dtype == np.int64 and an.min() >= 0 and an.max() < size and (leaves[an] > 0).all()
        assert (leaves[:size] == 0).sum() > size // 2 and len(np.unique(an)) > 1000
        assert torch.equal(ops.per_sample(t, n, seed, offset=1000), a)   # reproducible bit for bit
        assert not torch.equal(ops.per_sample(t, n, seed, offset=1001), a)
        print(f"PARITY tree size {size} per_sample: {n} draws, all on leaves with weight, equal on repeat")


def test_segtree_prefix_sum_idx_and_the_strict_comparison():
    ref = oc.prefix_tree()
    t = ops.DeviceSegmentTree(ref.size, device=DEV)
    for idx, val in oc.tree_set_calls(ref.size, lattice=True):
        ops.segtree_set(t, _d(idx), _d(val))
    _exact("prefix tree (lattice)", t.tree.cpu().numpy(), ref.tree)
    _tree_is_clean(t)
    vals, nodes, firsts = oc.prefix_values(ref)
    want = ref.prefix_sum_idx(vals)
    got = ops.segtree_prefix_sum_idx(t, _d(vals))
    assert torch.equal(got, ops.segtree_prefix_sum_idx(t, _d(vals)))
    _exact(f"prefix size {ref.size}: {len(vals)} values", got.cpu().numpy(), want)
    # a value equal to the sum left of a node's right child goes left (`<` is strict), as in the reference
    assert (got.cpu().numpy()[-len(nodes):] < firsts).all() and np.array_equal(want[-len(nodes):], firsts - 1)


@pytest.mark.parametrize("size", oc.TREE_SIZES)
@pytest.mark.parametrize("alpha", oc.PRIO_ALPHAS)
def test_priority_weights(size, alpha):
    ref, after = oc.prio_after(size, alpha)
    t = ops.DeviceSegmentTree(size, device=DEV)
    prio = torch.ones(2, dtype=torch.float64, device=DEV)
    bound = t.bound
    inner = np.arange(1, bound)
    for (kind, idx, td), (tree_ref, prio_ref) in zip(oc.prio_calls(size), after):
        if kind == "update":
            ops.per_update_weight(t, _d(idx), _d(td), alpha, prio)
        else:
            ops.per_init_weight(t, _d(idx), alpha, prio)
        tree = t.tree.cpu().numpy()
        p = f"prio size {size} alpha {alpha} {kind} n {len(idx)} "
        assert np.array_equal(tree[bound:] == 0, tree_ref[bound:] == 0), p
        _rel(p + "leaves", tree[bound:], tree_ref[bound:])
        if alpha == 1.0:
            _exact(p + "whole tree", tree, tree_ref)
        assert np.array_equal(tree[inner], tree[2 * inner] + tree[2 * inner + 1]), p    # exactly the sum of its children
        _rel(p + "max/min prio", prio.cpu().numpy(), prio_ref)
        _tree_is_clean(t)
    idx = oc.prio_calls(size)[-2][1]
    assert len(idx) == 4099
    for norm in (True, False):
        ref.weight_norm = norm
        want = ref.batch_weight(idx)
        run = lambda: ops.per_get_weight(t, _d(idx), oc.PRIO_BETA, norm, prio)  # noqa: E731
        w32, w64 = run()
        _same_bits(f"get_weight norm {norm}", (w32, w64), run())
        w32, w64 = w32.cpu().numpy(), w64.cpu().numpy()
        _rel(f"prio size {size} alpha {alpha} IS weights (norm {norm})", w64, want)
        assert w64.dtype == np.float64 and np.array_equal(w32, w64.astype(np.float32))
        assert not norm or w64.max() == 1.0
    _tree_is_clean(t)
