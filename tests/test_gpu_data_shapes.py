"""GPU tests (`-m gpu`) of the data-path kernels at their limits: the device VectorReplayBuffer's index algebra and payload
scatter (csrc/vrb.hip, vrb_dev.h), tsm_agent_index / tsm_gather_rows / tsm_scatter_rows (csrc/dispatch.hip),
tsm_gather_fields (csrc/gather_fields.hip) and tsm_categorical_logp_entropy (csrc/categorical.hip) -- a second and third chunk
of the 1024-wide scans, ragged fill at width, the float64 episode return, the malformed-buffer flag, every copy branch by row
size and by pointer alignment with guard bytes around every offset array, the field-count limits, more agents than a wave has
lanes, the grid-stride loop of gather_fields, and logits that underflow or sit at -inf; none of which the first-generation
cases of tests/test_gpu_kernels.py reach.  Cases, inputs and references: tests/data_cases.py (tests/test_host_data_shapes.py
checks their promises on the CPU).  Bars:
  * index algebra (against oracle.VectorReplayBufferIndex), payload bytes (numpy fancy indexing), dispatch (np.flatnonzero),
    gather_fields (torch indexing and .to(dtype)): exact, floats compared as raw bits;
  * categorical: test_gpu_distq._bar, max |hip - ref64| <= 1e-5 max |ref64| + e_ref, e_ref = max |Categorical(float32) -
    Categorical(float64)| on the same inputs, printed per case.
Every launch runs twice and must give the same bits.  Every comparison prints `PARITY name: ...`.

No test passes an index or an id that leaves an allocation: out-of-range cases are the ones the kernels define (ids that
tsm_agent_index drops, indices that wrap modulo maxsize, sizes refused on the host).  No test passes an out-of-range `act` to
tsm_categorical_logp_entropy, which indexes the logits with it unchecked; none adds one sub-buffer twice in one `add`."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

import data_cases as dc  # noqa: E402
from test_gpu_distq import _bar  # noqa: E402
from test_gpu_offpolicy_shapes import _same_bits, _worst  # noqa: E402

if torch.cuda.is_available():
    from tianshou_marl_amd import _abi, ops
    from tianshou_marl_amd._abi import call, ptr, stream_ptr


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _n(t):
    return t.cpu().numpy()


class _Tally:
    """Exact comparisons under one name: one PARITY line for all of them, one per comparison that differs."""

    def __init__(self, name):
        self.name, self.entries, self.count = name, 0, 0

    def exact(self, what, got, ref):
        got, ref = np.asarray(got), np.asarray(ref)
        assert got.shape == ref.shape and got.dtype == ref.dtype, (self.name, what, got.shape, ref.shape, got.dtype, ref.dtype)
        bad = np.flatnonzero(got.reshape(-1) != ref.reshape(-1))
        if len(bad):
            print(f"PARITY {self.name} {what}: DIFFERS at {bad[:8]} ({len(bad)} of {got.size} entries)")
        assert not len(bad), (self.name, what, bad[:8])
        self.entries, self.count = self.entries + got.size, self.count + 1

    def done(self, note=""):
        print(f"PARITY {self.name}: {self.count} comparisons, {self.entries} entries, equal{note}")


# ---- 1. replay-buffer index algebra ---------------------------------------------------------------------------------------
VRB_KEYS = ("ptr", "ep_rew", "ep_len", "ep_idx", "sample", "unfinished", "last_index", "lengths", "done")


def _snapshot(buf, out):
    return dict(ptr=out[0], ep_rew=out[1], ep_len=out[2], ep_idx=out[3], sample=buf.sample_indices_all().clone(),
                unfinished=buf.unfinished_index().clone(), last_index=buf.last_index.clone(), lengths=buf.lengths.clone(),
                done=buf.done_store.t().reshape(-1).clone())          # the reference's flat order env * S + slot


def _run_plan(c, plan, r):
    """The case's steps on two device buffers side by side (the same bits), every add against the oracle's snapshot."""
    bufs = [ops.VrbState(c["total"], c["B"], c["D"]) for _ in range(2)]
    assert bufs[0].sub_size == r["sub_size"] and bufs[0].maxsize == r["maxsize"]
    tally, k = _Tally(f"vrb {dc.case_id(c)}"), 0
    for step in plan:
        if step[0] == "reset":
            for b in bufs:
                b.reset(keep_statistics=step[1])
            continue
        _, ids, rew, done = step
        snaps = [_snapshot(b, b.add(_t(rew), _t(done), None if ids is None else _t(ids))) for b in bufs]
        _same_bits(f"{tally.name} add {k}", snaps[0], snaps[1])
        again = dict(sample=bufs[0].sample_indices_all(), unfinished=bufs[0].unfinished_index())     # the queries, launched again
        _same_bits(f"{tally.name} add {k} queries", again, {key: snaps[0][key] for key in again})
        want = r["adds"][k]
        for key in VRB_KEYS:
            tally.exact(f"add {k} {key}", _n(snaps[0][key]), want[key])
        assert len(bufs[0]) == len(bufs[1]) == want["len"], (tally.name, k)
        k += 1
    assert k == len(r["adds"])
    index = _t(r["index"])
    for name, fn in (("prev", lambda b: b.prev(index)), ("next", lambda b: b.next(index))):
        a = fn(bufs[0])
        _same_bits(f"{tally.name} {name}", a, fn(bufs[1]))
        tally.exact(name, _n(a), r[name])
    for b in bufs:
        b.check()                                                     # filled normally: no malformed-buffer flag
    tally.done(f" (len {r['adds'][-1]['len']} of {r['maxsize']}, {len(r['adds'][-1]['unfinished'])} unfinished)")


@pytest.mark.parametrize("c", dc.VRB_CASES, ids=dc.case_id)
def test_vrb_index_algebra(oracle, c):
    assert dc.vrb_conditions_hold(oracle, c)
    _run_plan(c, dc.vrb_plan(c), dc.vrb_replay(oracle, c))


def test_vrb_episode_return_is_accumulated_in_float64(oracle):
    """Rewards 2^24, 1, 1, 1 and a done row: 16777219 in float64 (a float32 accumulator stays at 16777216), in sub-buffers of all
    three scan chunks."""
    c, plan = dc.RETURN_CASE, dc.return_plan()
    r = dc.vrb_replay(oracle, c, plan)
    assert (r["adds"][-1]["ep_rew"][:, 0] == dc.RETURN_F64).all()
    _run_plan(c, plan, r)


def test_vrb_malformed_buffer_flag():
    c = dc.MALFORMED_CASE
    B, S = c["B"], c["S"]
    f = lambda R: (torch.ones(R, 1, device=DEV), torch.zeros(R, dtype=torch.bool, device=DEV))  # noqa: E731
    good = ops.VrbState(c["total"], B, c["D"])
    for _ in range(S + 1):
        good.add(*f(B))
    good.check()
    bad = ops.VrbState(c["total"], B, c["D"])
    assert bad.sub_size == S
    bad.add(*f(B))
    bad.check()
    bad._i64(3)[B - 1] = S + 1                     # ep_start_idx of the last sub-buffer, past every size it can have
    bad.add(*f(1), _t(np.array([B - 1], np.int64)))
    for _ in range(2):                             # the flag stays up
        with pytest.raises(_abi.MalformedBufferError, match="MalformedBufferError"):
            bad.check()
    good.check()
    print(f"PARITY vrb malformed B{B}-S{S}: ep_start_idx[{B - 1}] = {S + 1} raises MalformedBufferError, the buffer beside it passes")


# ---- 2. payload scatter and gather ----------------------------------------------------------------------------------------
class _Offset:
    """`nbytes` bytes `align` past a 16-byte boundary inside an allocation of guard bytes."""

    def __init__(self, nbytes, align, fill=None):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 96,), dc.GUARD, dtype=torch.uint8, device=DEV)
        self.lead = (-self.buf.data_ptr()) % 16 + 32 + align
        self.bytes = self.buf[self.lead:self.lead + nbytes]
        if fill is not None:
            self.bytes.copy_(_t(fill.reshape(-1)))
        assert self.bytes.data_ptr() % 16 == align and self.bytes.is_contiguous()

    def typed(self, dtype, *shape):
        t = self.bytes.view(getattr(torch, dtype)).view(*shape, -1)
        assert t.is_contiguous() and t.data_ptr() == self.bytes.data_ptr() and t.numel() * t.element_size() == self.nbytes
        return t

    def guards_intact(self):
        return bool((self.buf[:self.lead] == dc.GUARD).all()) and bool((self.buf[self.lead + self.nbytes:] == dc.GUARD).all())


class _PayloadBuffer:
    """A device buffer, the oracle beside it, and one store per field with its numpy image."""

    def __init__(self, oracle, fields, tag):
        p = dc.PAYLOAD_VRB
        self.B, self.S, self.R = p["B"], p["S"], p["R"]
        self.state = ops.VrbState(self.B * self.S, self.B, 1)
        self.orc = oracle.VectorReplayBufferIndex(self.B * self.S, self.B, 1)
        self.fields = fields                                            # [(row_bytes, (a_src, a_dst))]
        self.ref = [dc.payload_bytes(tag + 10 * i, self.S, self.B, rb) for i, (rb, _) in enumerate(fields)]
        self.stores = [_Offset(self.S * self.B * rb, a[1], self.ref[i]) for i, (rb, a) in enumerate(fields)]
        self.tag = tag

    def sources(self, k, fields=None):
        fields = self.fields if fields is None else fields
        src = [dc.payload_bytes(self.tag + 1000 * (k + 1) + 10 * i, self.R, rb) for i, (rb, _) in enumerate(fields)]
        return src, [_Offset(self.R * rb, a[0], src[i]) for i, (rb, a) in enumerate(fields)]

    def pairs(self, offs, stores, fields=None):
        fields = self.fields if fields is None else fields
        return [(o.typed(dc.payload_dtype(rb, a[0], i), self.R), s.typed(dc.payload_dtype(rb, a[1], i), self.S, self.B))
                for i, ((rb, a), o, s) in enumerate(zip(fields, offs, stores))]

    def add(self, k, tally):
        ids = dc.payload_ids(k)
        src, offs = self.sources(k)
        rew, done = np.zeros((self.R, 1), np.float32), np.zeros(self.R, bool)
        out = self.state.add(_t(rew), _t(done), _t(ids), fields=self.pairs(offs, self.stores))
        where = self.orc.add(rew.astype(np.float64), done, ids)[0]
        tally.exact(f"add {k} ptr", _n(out[0]), where)
        for i, (rb, a) in enumerate(self.fields):
            self.ref[i][where % self.S, where // self.S] = src[i]    # store[slot, env] = src
            tally.exact(f"add {k} store of {rb}-byte rows at {a}", _n(self.stores[i].bytes), self.ref[i].reshape(-1))
            assert self.stores[i].guards_intact() and offs[i].guards_intact(), (tally.name, k, rb, a)
            tally.exact(f"add {k} source of {rb}-byte rows at {a}", _n(offs[i].bytes), src[i].reshape(-1))

    def gather(self, tally):
        """Every index of [-maxsize, 2 maxsize) out of every store, into an output at the field's source offset."""
        index = dc.gather_index(self.B * self.S)
        idx = _t(index)
        for i, (rb, a) in enumerate(self.fields):
            want = dc.flat_order(self.ref[i])[index % (self.B * self.S)]
            outs = [_Offset(len(index) * rb, a[0]) for _ in range(2)]
            for o in outs:
                call("tsm_vrb_gather", ptr(self.stores[i].bytes), self.B, self.S, rb, ptr(idx), len(index), ptr(o.bytes), stream_ptr())
                assert o.guards_intact(), (tally.name, rb, a)
            assert torch.equal(outs[0].bytes, outs[1].bytes)
            tally.exact(f"gather of {rb}-byte rows, store at {a[1]}, output at {a[0]}", _n(outs[0].bytes), want.reshape(-1))
            if a == (0, 0):
                dt = dc.payload_dtype(rb, 0, i)
                got = self.state.gather(self.stores[i].typed(dt, self.S, self.B), idx)
                assert got.dtype == getattr(torch, dt) and got.shape[0] == len(index)
                tally.exact(f"VrbState.gather of {rb}-byte {dt} rows", _n(got.view(torch.uint8)).reshape(-1), want.reshape(-1))


@pytest.mark.parametrize("rb", dc.PAYLOAD_ROW_BYTES)
def test_vrb_payload_by_row_size_and_alignment(oracle, rb):
    fields = [(rb, a) for a in dc.payload_pairs(rb)]
    tally = _Tally(f"payload {rb}-byte rows")
    twins = [_PayloadBuffer(oracle, fields, tag=100 * rb) for _ in range(2)]
    for k in range(dc.PAYLOAD_VRB["adds"]):
        for b in twins:
            b.add(k, tally)
        for s0, s1 in zip(twins[0].stores, twins[1].stores):
            assert torch.equal(s0.bytes, s1.bytes)
    twins[0].gather(tally)
    words = sorted({dc.copy_branch(rb, *a) for _, a in fields}, reverse=True)
    tally.done(f" (copy words {words}, guards intact)")


def test_vrb_payload_twelve_fields_and_the_refusal_of_thirteen(oracle):
    tally = _Tally("payload twelve fields")
    twins = [_PayloadBuffer(oracle, dc.TWELVE_FIELDS, tag=7) for _ in range(2)]
    for k in range(2):
        for b in twins:
            b.add(k, tally)
    b = twins[0]
    thirteen = dc.TWELVE_FIELDS + [(5, (0, 0))]
    extra = _Offset(b.S * b.B * 5, 0, dc.payload_bytes(8, b.S, b.B, 5))
    src, offs = b.sources(9, thirteen)
    state = b.state.state.clone()
    with pytest.raises(ValueError, match="n_fields=13 exceeds 12"):
        b.state.add(torch.zeros(b.R, 1, device=DEV), torch.zeros(b.R, dtype=torch.bool, device=DEV), _t(dc.payload_ids(9)),
                    fields=b.pairs(offs, b.stores + [extra], thirteen))
    torch.cuda.synchronize()
    assert torch.equal(b.state.state, state)                          # refused before any launch: nothing moved
    for i, (rb, a) in enumerate(dc.TWELVE_FIELDS):
        tally.exact(f"store of {rb}-byte rows after the refusal", _n(b.stores[i].bytes), b.ref[i].reshape(-1))
    tally.exact("the thirteenth store", _n(extra.bytes), dc.payload_bytes(8, b.S, b.B, 5).reshape(-1))
    twins[0].gather(tally)
    tally.done()


@pytest.mark.parametrize("rb", dc.PAYLOAD_ROW_BYTES)
def test_gather_rows_and_scatter_rows_by_row_size_and_alignment(rb):
    tally = _Tally(f"rows {rb}-byte")
    for n in dc.ROWS_N:
        rs = np.random.RandomState(100 * rb + n)
        perm, n_src = rs.permutation(n).astype(np.int64), n + 3
        pick = rs.randint(0, n_src, n).astype(np.int64)
        src, old, pool = dc.payload_bytes(rb + n, n, rb), dc.payload_bytes(rb + n + 1, n, rb), dc.payload_bytes(rb + n + 2, n_src, rb)
        scattered = old.copy()
        scattered[perm] = src
        for i, a in enumerate(dc.payload_pairs(rb)):
            dts = dc.payload_dtype(rb, a[0], i), dc.payload_dtype(rb, a[1], i)
            s, p = _Offset(n * rb, a[0], src), _Offset(n_src * rb, a[0], pool)
            dsts, outs = [_Offset(n * rb, a[1], old) for _ in range(2)], [_Offset(n * rb, a[1]) for _ in range(2)]
            for d, o in zip(dsts, outs):
                ops.scatter_rows(s.typed(dts[0], n), _t(perm), d.typed(dts[1], n))
                call("tsm_gather_rows", ptr(p.bytes), ptr(_t(pick)), n, rb, ptr(o.bytes), stream_ptr())
                assert d.guards_intact() and o.guards_intact() and s.guards_intact() and p.guards_intact(), (rb, n, a)
            assert torch.equal(dsts[0].bytes, dsts[1].bytes) and torch.equal(outs[0].bytes, outs[1].bytes)
            tally.exact(f"scatter n{n} at {a}", _n(dsts[0].bytes), scattered.reshape(-1))
            tally.exact(f"gather n{n} at {a}", _n(outs[0].bytes), pool[pick].reshape(-1))
            if a == (0, 0):
                got = ops.gather_rows(p.typed(dts[0], n_src), _t(pick))
                tally.exact(f"ops.gather_rows n{n} {dts[0]}", _n(got.view(torch.uint8)).reshape(-1), pool[pick].reshape(-1))
    tally.done(f" (words {sorted({dc.word_branch(rb, *a) for a in dc.payload_pairs(rb)}, reverse=True)}, guards intact)")


# ---- 3. agent dispatch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", dc.DISPATCH_CASES, ids=dc.case_id)
def test_agent_index(c):
    ids, r = dc.dispatch_ids(c), dc.dispatch_reference(c)
    run = lambda: ops.agent_index(_t(ids), c["n_agent"])  # noqa: E731
    (index, offsets), (index2, offsets2) = run(), run()
    n_valid = int(r["offsets"][-1])
    tally = _Tally(f"dispatch {dc.case_id(c)}")
    tally.exact("offsets", _n(offsets), r["offsets"])
    assert torch.equal(offsets, offsets2) and torch.equal(index[:n_valid], index2[:n_valid])
    tally.exact("index", _n(index)[:n_valid], r["index"])         # ascending rows inside every agent; dropped rows leave the tail unwritten
    tally.done(f" ({n_valid} of {c['B']} rows kept)")


def test_agent_index_refuses_more_than_1024_agents():
    with pytest.raises(ValueError, match="bad sizes"):
        ops.agent_index(torch.zeros(5, dtype=torch.int32, device=DEV), 1025)


# ---- 4. gather_fields -----------------------------------------------------------------------------------------------------
GF_SENTINEL = 77


def _gf_launch(fields, devs, dsts):
    arr = (_abi.tsm_gather_field * len(fields))()
    for k, (f, s, d) in enumerate(zip(fields, devs, dsts)):
        arr[k] = _abi.tsm_gather_field(s.data_ptr(), d.data_ptr(), f["n_rows"], f["T"], f["E"], f["stride"], f["off"], f["width"],
                                       dc.KINDS[f["src_kind"]][0], dc.KINDS[f["dst_kind"]][0], 0)
    call("tsm_gather_fields", arr, len(fields), stream_ptr())


def _gf_dst(f):
    """[n_rows + 1, width]: the kernel writes n_rows rows, the last one is a guard."""
    return torch.full((f["n_rows"] + 1, f["width"]), GF_SENTINEL, dtype=dc.KINDS[f["dst_kind"]][1], device=DEV)


def _raw(t):
    t = t.contiguous()
    return _n(t.view(torch.int32) if t.dtype == torch.float32 else t)


def _gf_check(tally, fields, launch):
    devs = [f["src"].to(DEV) for f in fields]
    twice = []
    for _ in range(2):
        dsts = [_gf_dst(f) for f in fields]
        launch(fields, devs, dsts)
        twice.append(dsts)
    for f, d0, d1 in zip(fields, *twice):
        name = f"{f['src_kind']}->{f['dst_kind']} T{f['T']} E{f['E']} rows{f['n_rows']} width{f['width']} stride{f['stride']} off{f['off']}"
        assert np.array_equal(_raw(d0), _raw(d1)), name
        tally.exact(name, _raw(d0[:-1]), _raw(dc.gf_reference(f)))
        assert bool((d0[-1] == GF_SENTINEL).all()), name


def test_gather_fields_sweep():
    """Every allowed kind pair at five shapes, TSM_MAX_GATHER_FIELDS fields per launch; the remapped ones again through
    ops.gather_fields."""
    sweep, n_max = dc.gf_sweep(), _abi.MAX_GATHER_FIELDS
    tally = _Tally("gather_fields sweep")
    for k0 in range(0, len(sweep), n_max):
        _gf_check(tally, sweep[k0:k0 + n_max], _gf_launch)
    assert len(sweep) > n_max
    mapped = [f for f in sweep if f["T"]]

    def through_ops(fields, devs, dsts):
        ops.gather_fields([(s, d[:-1], f["T"], f["E"], f["stride"], f["off"]) for f, s, d in zip(fields, devs, dsts)])

    _gf_check(tally, mapped, through_ops)
    tally.done(f" ({len(sweep)} fields in launches of {n_max}, {len(mapped)} again through ops.gather_fields)")


def test_gather_fields_grid_stride_and_limits():
    b = dc.GF_BIG
    big = dc.gf_field("f32", "f32", b["T"], b["E"], b["width"], b["stride"], b["off"], 900)
    small = dc.gf_field("i64", "u8", 0, 0, 1, 1, 0, 901, n_rows=3)
    assert big["n_rows"] * big["width"] > 2048 * 256
    tally = _Tally("gather_fields grid-stride")
    _gf_check(tally, [big, small], _gf_launch)
    _gf_check(tally, [small, big], _gf_launch)
    tally.done(f" ({big['n_rows'] * big['width']} elements beside 3)")
    thirteen = [dc.gf_field("i32", "i32", 0, 0, 1, 1, 0, 950 + k, n_rows=4) for k in range(_abi.MAX_GATHER_FIELDS + 1)]
    devs, dsts = [f["src"].to(DEV) for f in thirteen], [_gf_dst(f) for f in thirteen]
    with pytest.raises(ValueError, match="1..12 fields"):
        _gf_launch(thirteen, devs, dsts)
    x = torch.ones(4, device=DEV)
    out = torch.full((4,), GF_SENTINEL, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="f32 sources"):
        ops.gather_fields([(x, out)])
    torch.cuda.synchronize()
    assert all(bool((d == GF_SENTINEL).all()) for d in dsts) and bool((out == GF_SENTINEL).all())       # refused before any launch


# ---- 5. categorical log-prob and entropy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", dc.CAT_CASES, ids=dc.case_id)
def test_categorical_logp_entropy(c):
    worst = {}
    for B in dc.CAT_B:
        d, r = dc.cat_inputs(c, B), dc.cat_reference(c, B)
        assert d["act"].min() >= 0 and d["act"].max() < c["A"]
        lg, act = _t(d["logits"]), _t(d["act"])
        h = ops.categorical_logp_entropy(lg, act)
        p = f"cat {dc.case_id(c)} B{B} "
        _same_bits(p, h, ops.categorical_logp_entropy(lg, act))
        print(f"PARITY {p}e_ref: logp {r['e_ref']['logp']:.3g}, ent {r['e_ref']['ent']:.3g}")
        for key, got in zip(("logp", "ent"), h):
            assert got.shape == (B,) and got.dtype == torch.float32
            worst[key] = max(worst.get(key, 0.0), _bar(p + key, _n(got), r[key], r["e_ref"][key]))
    _worst(f"cat {dc.case_id(c)}", worst)


def test_categorical_refuses_more_than_64_actions():
    with pytest.raises(ValueError, match="bad sizes"):
        ops.categorical_logp_entropy(torch.zeros(4, 65, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV))
