"""CPU tests of the shape sweeps that tests/test_gpu_data_shapes.py runs on the device (inputs and references:
tests/data_cases.py).  Every condition the cases promise is asserted here on the references alone: the replay-buffer cases are
the sweep asked for, their seeds are the first that put an empty, a full-and-wrapped, a done-ended and an unfinished sub-buffer
into every 1024-wide chunk, and the float64 episode return differs from a float32 one; every copy branch of the payload
kernels is reached by row size and by a pointer alone; the dispatch cases fill two scan chunks and split an agent over two row
blocks; the gather_fields references convert the way the header says; the categorical families underflow, hold -inf and keep
the taken action finite; and the C-ABI refuses the sizes past each limit before any launch."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import data_cases as dc  # noqa: E402
from test_host_offpolicy_shapes import _inside_bar  # noqa: E402


# ---- 1. replay-buffer index algebra ---------------------------------------------------------------------------------------
def test_vrb_cases_are_the_sweep_asked_for():
    assert {(c["B"], c["S"]) for c in dc.VRB_CASES} == {(B, S) for B in (1023, 1024, 1025, 2049, 3000) for S in (1, 2, 3)}
    assert len(dc.VRB_CASES) == 15 and {c["D"] for c in dc.VRB_CASES} == {1, 3, 8}
    assert any(c["total"] % c["B"] for c in dc.VRB_CASES if c["S"] > 1)
    for c in dc.VRB_CASES:
        assert -(-c["total"] // c["B"]) == c["S"] and c["total"] % c["B"]                  # the ceil of VrbState.__init__
        assert c["reset"] == (None if c["B"] <= 1024 else "plain" if c["S"] == 2 else "keep")
    for B in (1025, 2049, 3000):
        assert {c["reset"] for c in dc.VRB_CASES if c["B"] == B} == {"keep", "plain"}


@pytest.mark.parametrize("c", dc.VRB_CASES, ids=dc.case_id)
def test_vrb_case(oracle, c):
    plan, B = dc.vrb_plan(c), c["B"]
    adds = [s for s in plan if s[0] == "add"]
    assert len(adds) == 10 and [s[0] for s in plan].count("reset") == (1 if c["reset"] else 0)
    assert adds[0][1] is None and len(adds[0][3]) == B                                      # buffer_ids=None, R = B
    Rs = [len(s[3]) for s in adds]
    assert {1, 7, 8, 9} <= set(Rs) and any(R % dc.ROWS_PER_BLOCK for R in Rs if R > 9)
    assert (max(R for R in Rs[1:]) > 1024) == (B > 1024) and Rs[1] == (1025 if B > 1024 else B - 2)
    for _, ids, rew, done in adds:
        assert rew.dtype == np.float32 and rew.shape == (len(done), c["D"]) and done.dtype == bool
        if ids is not None:
            assert ids.dtype == np.int64 and len(set(ids.tolist())) == len(ids) and 0 <= ids.min() and ids.max() < B
            assert len(ids) < 20 or not np.array_equal(ids, np.sort(ids))                   # shuffled
    share = np.concatenate([s[3] for s in adds]).mean()
    assert 0.25 < share < 0.35
    if c["reset"]:   # in the middle of the running episodes
        i = [s[0] for s in plan].index("reset")
        assert 0 < i < len(plan) - 1 and not np.concatenate([s[3] for s in plan[:i]]).all()
    r = dc.vrb_replay(oracle, c)
    assert r["sub_size"] == c["S"] and r["maxsize"] == B * c["S"] and len(r["adds"]) == 10
    assert len(r["index"]) == r["maxsize"] + 4 and r["index"][0] == -2
    kinds = dc.vrb_chunk_kinds(c, r)
    assert [k[0] for k in kinds] == [min(1024, B - c0) for c0 in range(0, B, 1024)]
    if B > 1024:
        assert dc.vrb_conditions_hold(oracle, c)
        for n, empty, wrapped, on_done, not_done in kinds:
            assert wrapped and not_done, kinds
            assert n == 1 or (n >= 4 and empty and on_done), kinds
        # ragged fill: the sizes differ inside every wide chunk, so the offsets out of the scan are not e * size
        sample, lengths = r["adds"][-1]["sample"], r["adds"][-1]["lengths"]
        assert len(sample) == lengths.sum() and len(set(lengths[:1024].tolist())) > 1
        for k in range(200):   # the seed is the first of the sequence for which the conditions hold
            if dc.vrb_conditions_hold(oracle, dict(c, seed=dc._seed(k))):
                break
        assert c["seed"] == dc._seed(k), (dc.case_id(c), k)
    else:
        assert c["seed"] == dc._seed(0)
    print(f"vrb {dc.case_id(c)}: (members, empty, wrapped, on done, unfinished) per chunk {kinds}")


def test_float64_episode_return_differs_from_a_float32_one(oracle):
    c, plan = dc.RETURN_CASE, dc.return_plan()
    assert c["B"] > 2 * dc.CHUNK and {int(e) // dc.CHUNK for e in dc.RETURN_IDS} == {0, 1, 2} and c["B"] - 1 in dc.RETURN_IDS
    r = dc.vrb_replay(oracle, c, plan)
    last = r["adds"][-1]
    assert (last["ep_rew"] == np.array([dc.RETURN_F64, -dc.RETURN_F64, 5 * 0.25])).all() and (last["ep_len"] == 5).all()
    assert all(not a["ep_rew"].any() for a in r["adds"][:-1])
    acc = np.float32(0.0)
    for x in dc.RETURN_REW:
        acc = np.float32(acc + np.float32(x))
    assert float(acc) == dc.RETURN_F32 != dc.RETURN_F64 and all(np.float32(x) == x for x in dc.RETURN_REW)


# ---- 2. payload scatter and gather ----------------------------------------------------------------------------------------
def test_payload_cases_reach_every_copy_branch_by_size_and_by_pointer():
    assert dc.PAYLOAD_ROW_BYTES == (1, 2, 3, 4, 12, 16, 20, 48, 640, 33, 400)
    by_size, by_pointer, dtypes = {}, {}, set()
    for rb in dc.PAYLOAD_ROW_BYTES:
        pairs = dc.payload_pairs(rb)
        assert {(0, 0), (4, 0), (0, 4)} <= set(pairs) and (((1, 0) in pairs) == ((0, 1) in pairs) == (rb <= 48))
        for k, (a, b) in enumerate(pairs):
            for al in (a, b):
                d = dc.payload_dtype(rb, al, k)
                assert rb % dc.PAYLOAD_DTYPES[d] == 0 and al % dc.PAYLOAD_DTYPES[d] == 0
                dtypes.add(d)
            br = dc.copy_branch(rb, a, b)
            if (a, b) == (0, 0):
                by_size.setdefault(br, set()).add(rb)
            elif br != dc.copy_branch(rb, 0, 0):            # the same row size, another branch: the pointer alone decides
                by_pointer.setdefault((dc.copy_branch(rb, 0, 0), br), set()).add(rb)
    assert dtypes == set(dc.PAYLOAD_DTYPES)
    assert by_size == {16: {16, 48, 640, 400}, 4: {4, 12, 20}, 1: {1, 2, 3, 33}}
    assert {(16, 4), (16, 1), (4, 1)} == set(by_pointer) and 16 in by_pointer[(16, 4)] and 4 in by_pointer[(4, 1)]
    # the gather / row-copy kernels' two branches, by size and by pointer
    assert dc.word_branch(12, 0, 0) == 4 and dc.word_branch(33, 0, 0) == 1 and dc.word_branch(12, 0, 1) == 1 and dc.word_branch(16, 4, 0) == 4
    # a second trip through vrb_add_kernel's stride loop: more words per 8-row block than threads
    assert 640 // 16 * dc.ROWS_PER_BLOCK == 320 > dc.ADD_THREADS and 33 * dc.ROWS_PER_BLOCK == 264 > dc.ADD_THREADS
    assert dc.copy_branch(640, 0, 0) == 16 and dc.copy_branch(640, 4, 0) == 4 and 640 // 4 * dc.ROWS_PER_BLOCK > dc.ADD_THREADS
    p = dc.PAYLOAD_VRB
    assert p["R"] % dc.ROWS_PER_BLOCK and p["R"] > 2 * dc.ROWS_PER_BLOCK and p["R"] < p["B"] and p["adds"] > p["S"]
    for k in range(p["adds"]):
        ids = dc.payload_ids(k)
        assert len(set(ids.tolist())) == p["R"] and ids.max() < p["B"]
    # NaN payloads: the random bytes hold float32 and float64 NaNs
    x = dc.payload_bytes(0, 21, 640)
    assert np.isnan(x.view(np.float32)).any() and np.isnan(dc.payload_bytes(1, 4096, 8).view(np.float64)).any()
    idx = dc.gather_index(69)
    assert sorted(idx.tolist()) == list(range(-69, 138))
    assert len(dc.TWELVE_FIELDS) == 12 and {dc.copy_branch(rb, a, b) for rb, (a, b) in dc.TWELVE_FIELDS} == {16, 4, 1}
    assert len({rb for rb, _ in dc.TWELVE_FIELDS}) == 12 and dc.ROWS_N == (1, 255, 257)


def test_payload_reference_round_trip():
    """numpy's scatter `store[slot, env] = src` read back through the flat order env * S + slot gives the rows again."""
    S, B, rb = 3, 23, 33
    store, src, ids = dc.payload_bytes(2, S, B, rb), dc.payload_bytes(3, 21, rb), dc.payload_ids(0)
    slot = np.arange(21) % S
    store[slot, ids] = src
    assert np.array_equal(dc.flat_order(store)[(ids * S + slot) % (B * S)], src)
    assert np.array_equal(dc.flat_order(store)[(ids * S + slot - B * S) % (B * S)], src)       # a negative index wraps


# ---- 3. agent dispatch ----------------------------------------------------------------------------------------------------
def test_dispatch_cases_are_the_sweep_asked_for():
    shapes = [(c["B"], c["n_agent"], c["kind"]) for c in dc.DISPATCH_CASES]
    assert shapes[:5] == [(2049, 1024, "random"), (1025, 513, "random"), (200, 65, "random"), (4096, 300, "random"), (1000, 7, "one")]
    assert shapes[5][2] == "invalid" and len(shapes) == 6


@pytest.mark.parametrize("c", dc.DISPATCH_CASES, ids=dc.case_id)
def test_dispatch_case(oracle, c):
    ids, r, cnt = dc.dispatch_ids(c), dc.dispatch_reference(c), dc.dispatch_scan_counts(c)
    B, n = c["B"], c["n_agent"]
    assert ids.dtype == np.int32 and ids.shape == (B,) and cnt.sum() == r["offsets"][-1] == len(r["index"])
    for a in (0, n // 2, n - 1):
        rows = r["index"][r["offsets"][a]:r["offsets"][a + 1]]
        assert np.array_equal(rows, oracle.agent_index(ids, a)) and (np.diff(rows) > 0).all()
    entries = cnt.reshape(-1)
    chunks = [int(entries[k:k + dc.CHUNK].sum()) for k in range(0, len(entries), dc.CHUNK)]
    if len(entries) > dc.CHUNK:      # the chunked cases
        assert sum(1 for x in chunks if x) >= 2 and chunks[-1] > 0, chunks
        assert ((cnt > 0).sum(axis=1) > 1).any()                       # an agent with rows in more than one 1024-row block
    assert {(2049, 1024): 3, (1025, 513): 2, (4096, 300): 2}.get((B, n), 1) == len(chunks)
    if (B, n) == (1025, 513):
        assert len(entries) == 1026 and len(entries[dc.CHUNK:]) == 2 and entries[dc.CHUNK:].all()   # the second chunk holds two
    if c["kind"] == "one":
        assert (ids == 3).all() and r["offsets"].tolist() == [0, 0, 0, 0] + [B] * 4
    if c["kind"] == "invalid":
        assert (ids == -1).sum() > 100 and (ids == n).sum() > 100 and 0 < r["offsets"][-1] == ((ids >= 0) & (ids < n)).sum() < B
    else:
        assert r["offsets"][-1] == B and ids.min() >= 0 and ids.max() < n
    print(f"dispatch {dc.case_id(c)}: {len(entries)} scan entries, counts per chunk {chunks}")


# ---- 4. gather_fields -----------------------------------------------------------------------------------------------------
def test_gather_fields_cases_and_references():
    from tianshou_marl_amd import _abi

    assert _abi.MAX_GATHER_FIELDS == 12 and len(dc.KIND_PAIRS) == 13 and ("i64", "u8") in dc.KIND_PAIRS and ("f32", "i32") not in dc.KIND_PAIRS
    assert {k: v[0] for k, v in dc.KINDS.items()} == {"f32": _abi.TSM_KIND_F32, "i32": _abi.TSM_KIND_I32, "i64": _abi.TSM_KIND_I64,
                                                      "u8": _abi.TSM_KIND_U8}
    sweep = dc.gf_sweep()
    assert {(f["src_kind"], f["dst_kind"]) for f in sweep} == set(dc.KIND_PAIRS)
    assert {f["width"] for f in sweep} == {1, 3, 18} and {(f["T"], f["E"]) for f in sweep} >= {(1, 1), (0, 0), (5, 7)}
    assert any(f["off"] > 0 and f["stride"] > f["width"] for f in sweep)
    for f in sweep:
        ref = dc.gf_reference(f)
        assert ref.shape == (f["n_rows"], f["width"]) and ref.dtype == dc.KINDS[f["dst_kind"]][1]
        assert (f["n_rows"] - 1) * f["stride"] + f["off"] + f["width"] <= f["src"].numel()          # the mapping stays inside
        if f["dst_kind"] == "u8":
            assert set(ref.unique().tolist()) <= {0, 1}
    # I64 -> U8: any non-zero value, negatives and 256 included, becomes 1
    f = dict(dc.gf_field("i64", "u8", 0, 0, 1, 1, 0, 0, n_rows=5), src=torch.tensor([0, 256, -1, 1 << 32, -256]))
    assert dc.gf_reference(f).reshape(-1).tolist() == [0, 1, 1, 1, 1]
    f = dict(dc.gf_field("i64", "i32", 0, 0, 1, 1, 0, 0, n_rows=2), src=torch.tensor([(1 << 32) + 5, -7]))
    assert dc.gf_reference(f).reshape(-1).tolist() == [5, -7]
    assert all(float(np.float32(v)) == v for v in dc.GF_SPECIAL)
    # the remap: destination row e * T + t reads source row t * E + e
    f = dc.gf_field("i32", "i64", 5, 7, 3, 7, 2, 1)
    ref, store = dc.gf_reference(f), f["src"][:5 * 7 * 7].view(5, 7, 7)
    assert torch.equal(ref.view(7, 5, 3), store.transpose(0, 1)[:, :, 2:5].to(torch.int64))
    b = dc.GF_BIG
    assert b["T"] * b["E"] * b["width"] > 2048 * 256 and b["T"] * b["E"] * b["width"] * 4 < 8 << 20


def test_limits_are_refused_before_any_launch():
    """A = 65, n_agent = 1025, thirteen payload fields, thirteen gather fields and F32 -> I32: ValueError from the host checks
    (the pointers are never read)."""
    from tianshou_marl_amd import _abi

    with pytest.raises(ValueError, match="bad sizes"):
        _abi.call("tsm_categorical_logp_entropy", 1, 1, 4, 65, 1, 1, None)
    with pytest.raises(ValueError, match="null pointer"):       # 64 passes the size check
        _abi.call("tsm_categorical_logp_entropy", None, None, 4, 64, None, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        _abi.call("tsm_agent_index", 1, 5, 1025, 1, 1, 1, None)
    with pytest.raises(ValueError, match="null pointer"):
        _abi.call("tsm_agent_index", None, 5, 1024, None, None, None, None)
    farr = (_abi.tsm_field * 13)()
    with pytest.raises(ValueError, match="n_fields=13 exceeds 12"):
        _abi.call("tsm_vrb_add", 1, 4, 2, 1, None, 3, 1, 1, 1, farr, 13, 1, 1, 1, 1, None)
    with pytest.raises(ValueError, match="field 0 invalid"):    # 12 passes the count check
        _abi.call("tsm_vrb_add", 1, 4, 2, 1, None, 3, 1, 1, 1, farr, 12, 1, 1, 1, 1, None)
    garr = (_abi.tsm_gather_field * 13)()
    with pytest.raises(ValueError, match="1..12 fields"):
        _abi.call("tsm_gather_fields", garr, 13, None)
    garr[0] = _abi.tsm_gather_field(1, 1, 4, 0, 0, 1, 0, 1, _abi.TSM_KIND_F32, _abi.TSM_KIND_I32, 0)
    with pytest.raises(ValueError, match="f32 sources"):
        _abi.call("tsm_gather_fields", garr, 1, None)


# ---- 5. categorical -------------------------------------------------------------------------------------------------------
def test_categorical_cases_are_the_sweep_asked_for():
    assert dc.CAT_B == (1, 255, 256, 257) and dc.CAT_A == (1, 2, 63, 64)
    got = {(c["kind"], c["A"]) for c in dc.CAT_CASES}
    assert got == {(k, A) for k in dc.CAT_FAMILIES for A in dc.CAT_A} - {("spread", 1), ("neginf", 1)} and len(dc.CAT_CASES) == 18


@pytest.mark.parametrize("c", dc.CAT_CASES, ids=dc.case_id)
def test_categorical_case(c):
    A, worst = c["A"], 0.0
    for B in dc.CAT_B:
        d, r = dc.cat_inputs(c, B), dc.cat_reference(c, B)
        lg, act = d["logits"], d["act"]
        assert lg.dtype == np.float32 and lg.shape == (B, A) and act.dtype == np.int32 and act.min() >= 0 and act.max() < A
        assert not np.isnan(lg).any() and not np.isposinf(lg).any()
        assert np.isfinite(lg).any(axis=1).all()                                  # no row is all -inf
        assert np.isfinite(lg[np.arange(B), act]).all()                            # the taken action is finite
        assert np.isfinite(r["logp"]).all() and np.isfinite(r["ent"]).all() and (r["ent"] >= 0).all()
        if c["kind"] == "neginf":
            n_inf = np.isneginf(lg).sum(axis=1)
            assert n_inf.min() >= 1 and n_inf.max() <= A - 1 and (B < A - 1 or set(n_inf.tolist()) == set(range(1, A)))
        else:
            assert np.isfinite(lg).all()
        if c["kind"] == "spread":
            assert (lg.max(axis=1) - lg.min(axis=1) == dc.CAT_SPREAD).all()
            p32 = torch.softmax(torch.from_numpy(lg), dim=-1).numpy()
            assert (p32 == 0).any() and ((p32 == 0).sum(axis=1) >= 1).all()        # probabilities that underflow to 0 in float32
        if c["kind"] in ("plus1e4", "minus1e4"):
            assert abs(abs(float(lg.mean())) - 1e4) < 10
        if A == 1:
            assert not r["logp"].any() and not r["ent"].any()
        for k in ("logp", "ent"):
            worst = max(worst, _inside_bar(f"cat {k}", r["e_ref"][k], r[k]))
    print(f"cat {dc.case_id(c)}: worst e_ref / bar {worst:.3g}")
