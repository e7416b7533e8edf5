"""Inputs and references of the shape sweeps over the data-path kernels: the device VectorReplayBuffer's index algebra and
payload scatter (csrc/vrb.hip, vrb_dev.h), tsm_agent_index / tsm_gather_rows / tsm_scatter_rows (csrc/dispatch.hip),
tsm_gather_fields (csrc/gather_fields.hip) and tsm_categorical_logp_entropy (csrc/categorical.hip) -- the case lists, one
deterministic input builder per family and the references.  tests/test_gpu_data_shapes.py runs the kernels on these inputs;
tests/test_host_data_shapes.py checks on the CPU every condition promised below.  Plain numpy / torch-CPU module; the
references that need the project's C oracle take the `oracle` fixture's module as their first argument.

The references:
  * index algebra: oracle.VectorReplayBufferIndex (pinned to the reference's traces by tests/test_oracle_golden.py), exact;
  * payload: numpy fancy indexing on bytes -- scatter `store[slot, env] = src`, gather `store in env * S + slot order
    [index % maxsize]` --, exact on raw bytes (NaN payloads included);
  * dispatch: np.flatnonzero(ids == a), exact and ascending within an agent;
  * gather_fields: torch indexing and `.to(dtype)` (a uint8 destination takes `!= 0`), exact;
  * categorical: torch.distributions.Categorical(logits=...) in float64 on the float32 inputs cast up, with
    `e_ref = max |Categorical(float32) - Categorical(float64)|` on the same inputs.

Replay-buffer cases.  Every case starts with an add to all sub-buffers (`buffer_ids=None`, R = B) and an add of a shuffled
subset whose last block of 8 rows is ragged (R = 1025 where B > 1024, else B - 2).  Every case with B > 1024 then resets --
keep_statistics=True in the middle of the running episodes at S in {1, 3}, a plain reset() at S = 2 -- because an add to all
sub-buffers leaves none empty; eight more adds follow: R = 1, 7, 8, 9 between random subsets that hold each sub-buffer with
probability 0.7, rewards N(0, 1) in float32, done with probability 0.3.  At the final comparison every 1024-wide chunk of
sub-buffers with four or more members holds an empty sub-buffer, one that is full and has wrapped (more than S adds since the
reset), one that ends on a done row and one that does not.  The last chunk of B = 1025 and of B = 2049 is ONE sub-buffer, which
cannot be empty and full at once: it is full, has wrapped and ends on a row that is not done, so that both chunked scans write
an entry of that chunk at their carried `base`.  The seeds are the first of 1000 + 17 k for which this holds (run this file to
search them again); no case is dropped.

Not covered: duplicate ids within one `add`.  The kernel gives every row a thread of its own, two threads would own one
sub-buffer, and the result is undefined; nothing here tests it.  Sampling is pinned by tests/test_gpu_sampling.py.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from offpolicy_cases import _err, _seed, case_id  # noqa: E402,F401

CHUNK = 1024              # the scans of vrb.hip and dispatch.hip walk their input 1024 entries at a time
ROWS_PER_BLOCK = 8        # vrb_add_kernel's kRowsPerBlock
ADD_THREADS = 256
GUARD = 0xC3              # the byte around every offset store, source and output


# ---- 1. replay-buffer index algebra ---------------------------------------------------------------------------------------
VRB_B, VRB_S, VRB_D = (1023, 1024, 1025, 2049, 3000), (1, 2, 3), (1, 3, 8)
P_DONE, P_MEMBER = 0.3, 0.7
VRB_SEEDS = {(1025, 3): 1119, (2049, 1): 1051, (2049, 2): 1119, (2049, 3): 1068}     # every other case: 1000, the first


def _vrb_case(B, S, i):
    # total_size: the ceil of VrbState.__init__ rounds it up to B * S (no multiple of B, except where S = 1 allows none below B)
    reset = None if B <= CHUNK else ("plain" if S == 2 else "keep")
    return dict(family="vrb", B=B, S=S, D=VRB_D[i % 3], total=B * S - B // 2 if S > 1 else B - 5, reset=reset,
                seed=VRB_SEEDS.get((B, S), _seed(0)))


VRB_CASES = [_vrb_case(B, S, i + j) for i, B in enumerate(VRB_B) for j, S in enumerate(VRB_S)]
VRB_SMALL_R = (1, 7, 8, 9)


def vrb_plan(c: dict) -> list:
    """The case's steps: ("add", ids i64[R] | None, rew f32[R, D], done bool[R]) and ("reset", keep_statistics)."""
    rs = np.random.RandomState(c["seed"] + 7 * c["B"] + 131 * c["S"])
    B, D = c["B"], c["D"]

    def add(ids):
        R = B if ids is None else len(ids)
        return ("add", ids, rs.standard_normal((R, D)).astype(np.float32), rs.rand(R) < P_DONE)

    subset = lambda R: rs.permutation(B)[:R].astype(np.int64)  # noqa: E731  shuffled, no duplicates
    steps = [add(None), add(subset(1025 if B > CHUNK else B - 2))]
    if c["reset"]:
        steps.append(("reset", c["reset"] == "keep"))
    for R in (None, 1, 7, None, 8, None, 9, None):
        steps.append(add(subset(int(rs.binomial(B, P_MEMBER)) if R is None else R)))
    return steps


def vrb_replay(orc, c: dict, plan: list | None = None) -> dict:
    """The oracle's answers along a case: `adds`, one snapshot per add (ptr, ep_rew [R, D], ep_len, ep_idx, len, sample,
    unfinished, last_index, lengths, done in the reference's flat order), `prev` / `next` over arange(-2, maxsize + 2) after
    the last add, and `since`, the number of adds every sub-buffer received since the last reset."""
    ob = orc.VectorReplayBufferIndex(c["total"], c["B"], c["D"])
    out, since = [], np.zeros(c["B"], np.int64)
    for step in vrb_plan(c) if plan is None else plan:
        if step[0] == "reset":
            ob.reset(keep_statistics=step[1])
            since[:] = 0
            continue
        _, ids, rew, done = step
        ptr, ep_rew, ep_len, ep_idx = ob.add(rew.astype(np.float64), done, ids)
        since[np.arange(c["B"]) if ids is None else ids] += 1
        out.append(dict(ptr=ptr, ep_rew=np.asarray(ep_rew).reshape(len(ptr), c["D"]), ep_len=ep_len, ep_idx=ep_idx, len=len(ob),
                        sample=ob.sample_indices_all(), unfinished=ob.unfinished_index(), last_index=ob.last_index,
                        lengths=ob.lengths, done=ob.done.astype(np.uint8)))
    index = np.arange(-2, ob.maxsize + 2)
    return dict(adds=out, sub_size=ob.sub_size, maxsize=ob.maxsize, index=index, prev=ob.prev(index), next=ob.next(index), since=since)


def vrb_chunk_kinds(c: dict, r: dict) -> list:
    """Per 1024-wide chunk of sub-buffers, at the final comparison: (members, empty, full and wrapped, ending on a done row,
    ending on another) -- the last four as counts."""
    last = r["adds"][-1]
    S, lengths = r["sub_size"], last["lengths"]
    on_done = last["done"][last["last_index"]].astype(bool) & (lengths > 0)
    out = []
    for c0 in range(0, c["B"], CHUNK):
        s = slice(c0, min(c0 + CHUNK, c["B"]))
        out.append((s.stop - s.start, int((lengths[s] == 0).sum()), int(((lengths[s] == S) & (r["since"][s] > S)).sum()),
                    int(on_done[s].sum()), int(((lengths[s] > 0) & ~on_done[s]).sum())))
    return out


def vrb_conditions_hold(orc, c: dict) -> bool:
    if c["B"] <= CHUNK:
        return True
    for n, empty, wrapped, on_done, not_done in vrb_chunk_kinds(c, vrb_replay(orc, c)):
        if not (wrapped and not_done and (n < 4 or (empty and on_done))):
            return False
    return True


# the float64 episode return: rewards no float32 accumulator can add up.  Sub-buffers of every chunk, five adds.
RETURN_CASE = dict(family="vrb_return", B=2049, S=2, D=3, total=2049 * 2 - 1, reset=None, seed=_seed(0))
RETURN_IDS = np.array([2048, 3, 1024, 1023, 2047], np.int64)
RETURN_REW = (16777216.0, 1.0, 1.0, 1.0, 0.0)          # column 0; column 1 is its negative, column 2 is 0.25 every row
RETURN_F64, RETURN_F32 = 16777219.0, 16777216.0


def return_plan() -> list:
    R = len(RETURN_IDS)
    return [("add", RETURN_IDS, np.tile(np.array([[x, -x, 0.25]], np.float32), (R, 1)), np.full(R, k == len(RETURN_REW) - 1))
            for k, x in enumerate(RETURN_REW)]


MALFORMED_CASE = dict(family="vrb_malformed", B=1025, S=2, D=1, total=2050)


# ---- 2. payload scatter and gather ----------------------------------------------------------------------------------------
PAYLOAD_ROW_BYTES = (1, 2, 3, 4, 12, 16, 20, 48, 640, 33, 400)
PAYLOAD_DTYPES = {"uint8": 1, "int32": 4, "int64": 8, "float32": 4, "float64": 8}
# (bytes past a 16-byte boundary of the source, of the store / destination)
ALIGN_PAIRS = ((0, 0), (4, 0), (0, 4), (4, 4), (1, 0), (0, 1))
PAYLOAD_VRB = dict(B=23, S=3, R=21, adds=4)            # blocks of 8, 8 and 5 rows; the fourth add wraps
ROWS_N = (1, 255, 257)


def copy_branch(row_bytes: int, a_src: int, a_dst: int) -> int:
    """The word vrb_add_kernel copies a field with: 16, 4 or 1 bytes (by row size and by the alignment of both pointers)."""
    a = a_src | a_dst
    return 16 if row_bytes % 16 == 0 and a % 16 == 0 else 4 if row_bytes % 4 == 0 and a % 4 == 0 else 1


def word_branch(row_bytes: int, a_src: int, a_dst: int) -> int:
    """The word of vrb_gather_kernel and of rows_kernel: 4 bytes or 1."""
    return 4 if row_bytes % 4 == 0 and (a_src | a_dst) % 4 == 0 else 1


def payload_dtype(row_bytes: int, align: int, k: int = 0) -> str:
    """The element type a row of `row_bytes` bytes is held as `align` bytes past a 16-byte boundary: one whose size divides
    both (a byte past a boundary only uint8 can stand); k steps through the candidates."""
    ok = [d for d, n in PAYLOAD_DTYPES.items() if row_bytes % n == 0 and align % n == 0]
    return ok[(row_bytes + k) % len(ok)]


def payload_pairs(row_bytes: int) -> list:
    """The (source, store) offsets a row size is swept over: a byte past a boundary for rows that torch can hold as uint8."""
    return [p for p in ALIGN_PAIRS if 1 not in p or row_bytes <= 48]


def payload_bytes(tag: int, *shape) -> np.ndarray:
    return np.random.RandomState(9000 + tag).randint(0, 256, shape).astype(np.uint8)


def payload_ids(k: int) -> np.ndarray:
    p = PAYLOAD_VRB
    return np.random.RandomState(9100 + k).permutation(p["B"])[:p["R"]].astype(np.int64)


def gather_index(maxsize: int) -> np.ndarray:
    """Every index of [-maxsize, 2 maxsize), shuffled."""
    return np.random.RandomState(9200).permutation(np.arange(-maxsize, 2 * maxsize)).astype(np.int64)


def flat_order(store: np.ndarray) -> np.ndarray:
    """A [S, B, row_bytes] store in the reference's flat order env * S + slot."""
    S, B, rb = store.shape
    return store.transpose(1, 0, 2).reshape(B * S, rb)


TWELVE_FIELDS = [(1, (0, 1)), (2, (1, 0)), (3, (0, 0)), (4, (4, 4)), (12, (0, 4)), (16, (0, 0)), (20, (4, 0)), (48, (4, 0)), (640, (0, 0)),
                 (33, (0, 0)), (400, (0, 4)), (8, (0, 0))]


# ---- 3. agent dispatch ----------------------------------------------------------------------------------------------------
DISPATCH_CASES = [dict(family="dispatch", B=2049, n_agent=1024, kind="random"), dict(family="dispatch", B=1025, n_agent=513, kind="random"),
                  dict(family="dispatch", B=200, n_agent=65, kind="random"), dict(family="dispatch", B=4096, n_agent=300, kind="random"),
                  dict(family="dispatch", B=1000, n_agent=7, kind="one"), dict(family="dispatch", B=3000, n_agent=70, kind="invalid")]


def dispatch_ids(c: dict) -> np.ndarray:
    """int32 [B].  random: uniform over the agents, the last agent planted in the first and in the last row (so that the last
    scan chunk and two row blocks count it); one: every row agent 3; invalid: a fifth of the rows -1 or n_agent."""
    rs = np.random.RandomState(7000 + c["B"] + 3 * c["n_agent"])
    B, n = c["B"], c["n_agent"]
    if c["kind"] == "one":
        return np.full(B, 3, np.int32)
    ids = rs.randint(0, n, B).astype(np.int32)
    ids[0] = ids[-1] = n - 1
    if c["kind"] == "invalid":
        bad = rs.rand(B) < 0.2
        ids[bad] = rs.choice([-1, n], int(bad.sum()))
        ids[1], ids[-2] = -1, n
    return ids


def dispatch_reference(c: dict) -> dict:
    ids = dispatch_ids(c)
    rows = [np.flatnonzero(ids == a) for a in range(c["n_agent"])]
    return dict(index=np.concatenate(rows).astype(np.int64), offsets=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64))


def dispatch_scan_counts(c: dict) -> np.ndarray:
    """What hist_kernel hands the scan: the count of agent a in row block k at entry a * n_blocks + k."""
    ids = dispatch_ids(c)
    nb = -(-c["B"] // CHUNK)
    cnt = np.zeros((c["n_agent"], nb), np.int64)
    for k in range(nb):
        blk = ids[k * CHUNK:(k + 1) * CHUNK]
        blk = blk[(blk >= 0) & (blk < c["n_agent"])]
        cnt[:, k] = np.bincount(blk, minlength=c["n_agent"])
    return cnt


# ---- 4. gather_fields -----------------------------------------------------------------------------------------------------
KINDS = {"f32": (0, torch.float32), "i32": (1, torch.int32), "i64": (2, torch.int64), "u8": (3, torch.uint8)}
KIND_PAIRS = [("f32", "f32")] + [(s, d) for s in ("i32", "i64", "u8") for d in ("i32", "i64", "f32", "u8")]
GF_SPECIAL = (0, 1, -1, 255, 256, -256, 65536, 1 << 32, -(1 << 32))    # each exact in float32
GF_BIG = dict(T=19, E=9211, width=3, stride=4, off=1)                    # 525027 elements: more than 2048 * 256


def gf_source(kind: str, n: int, tag: int) -> torch.Tensor:
    rs = np.random.RandomState(6000 + tag)
    if kind == "f32":
        x = rs.standard_normal(n).astype(np.float32)
        x[::7] = np.float32("nan") if n > 7 else x[::7]
        return torch.from_numpy(x)
    v = rs.randint(-1000, 1000, n).astype(np.int64)
    v[rs.rand(n) < 0.3] = 0
    sp = rs.choice(len(GF_SPECIAL), n)
    v = np.where(rs.rand(n) < 0.3, np.array(GF_SPECIAL, np.int64)[sp], v)
    return torch.from_numpy(v).to(KINDS[kind][1])       # int32 / uint8 wrap the way a C cast does


def gf_field(src_kind, dst_kind, T, E, width, stride, off, tag, n_rows=None) -> dict:
    """A field's description and source.  T = 0: no remap, n_rows rows."""
    n_rows = T * E if T else n_rows
    return dict(src_kind=src_kind, dst_kind=dst_kind, T=T, E=E if T else 0, width=width, stride=stride, off=off, n_rows=n_rows,
                src=gf_source(src_kind, (n_rows - 1) * stride + off + width + 5, tag))


def gf_reference(f: dict) -> torch.Tensor:
    """dst [n_rows, width]: row r = e * T + t reads `width` elements at source row t * E + e (r itself without a remap)."""
    r = torch.arange(f["n_rows"])
    sr = (r % f["T"]) * f["E"] + r // f["T"] if f["T"] else r
    x = f["src"][(sr * f["stride"] + f["off"])[:, None] + torch.arange(f["width"])[None, :]]
    return (x != 0).to(torch.uint8) if f["dst_kind"] == "u8" else x.to(KINDS[f["dst_kind"]][1])


def gf_sweep() -> list:
    """Every kind pair at (T, E) = (1, 1), a remap (5, 7), a wide remap and no remap, widths 1 / 3 / 18, a column offset."""
    shapes = [(1, 1, 1, 1, 0, None), (5, 7, 3, 7, 2, None), (3, 4, 18, 40, 11, None), (0, 0, 3, 5, 1, 33), (0, 0, 1, 2, 1, 257)]
    return [gf_field(s, d, T, E, w, st, off, 100 * i + j, n) for i, (s, d) in enumerate(KIND_PAIRS)
            for j, (T, E, w, st, off, n) in enumerate(shapes)]


# ---- 5. categorical log-prob and entropy ------------------------------------------------------------------------------------
CAT_B, CAT_A = (1, 255, 256, 257), (1, 2, 63, 64)
CAT_FAMILIES = ("normal", "plus1e4", "minus1e4", "spread", "neginf")
CAT_CASES = [dict(family="cat", kind=k, A=A) for k in CAT_FAMILIES for A in CAT_A if A > 1 or k not in ("spread", "neginf")]
CAT_SPREAD = 200.0


def cat_inputs(c: dict, B: int) -> dict:
    """logits f32 [B, A] and act i32 [B] in [0, A).  spread: every row holds a 0 and a -200; neginf: row b has 1 + b % (A - 1)
    entries at -inf and its action on a finite one."""
    A, kind = c["A"], c["kind"]
    rs = np.random.RandomState(5000 + 1000 * CAT_FAMILIES.index(kind) + 10 * A + B)
    lg = (3.0 * rs.standard_normal((B, A))).astype(np.float32)
    act = rs.randint(0, A, B).astype(np.int32)
    if kind == "plus1e4":
        lg = (lg + np.float32(1e4)).astype(np.float32)
    elif kind == "minus1e4":
        lg = (lg - np.float32(1e4)).astype(np.float32)
    elif kind == "spread":
        lg = rs.uniform(-CAT_SPREAD, 0.0, (B, A)).astype(np.float32)
        for b in range(B):
            at = rs.choice(A, 2, replace=False)
            lg[b, at[0]], lg[b, at[1]] = 0.0, -CAT_SPREAD
    elif kind == "neginf":
        for b in range(B):
            cols = rs.permutation(A)
            n_inf = 1 + b % (A - 1)
            lg[b, cols[:n_inf]] = -np.inf
            act[b] = cols[n_inf + rs.randint(0, A - n_inf)]
    return dict(logits=lg, act=act)


def categorical(logits: np.ndarray, act: np.ndarray, dtype) -> dict:
    d = torch.distributions.Categorical(logits=torch.from_numpy(logits).to(dtype), validate_args=False)
    return dict(logp=d.log_prob(torch.from_numpy(act).to(torch.int64)).to(torch.float64).numpy(), ent=d.entropy().to(torch.float64).numpy())


def cat_reference(c: dict, B: int) -> dict:
    d = cat_inputs(c, B)
    r64, r32 = categorical(d["logits"], d["act"], torch.float64), categorical(d["logits"], d["act"], torch.float32)
    r64["e_ref"] = {k: _err(r32[k], r64[k]) for k in ("logp", "ent")}
    return r64


# ---- choosing the seeds -------------------------------------------------------------------------------------------------------
if __name__ == "__main__":   # print, per replay-buffer case with B > 1024, the first seed for which the conditions hold
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle as orc

    orc.build()
    for case in VRB_CASES:
        for k in range(400):
            trial = dict(case, seed=_seed(k))
            if vrb_conditions_hold(orc, trial):
                break
        print(case_id(case), "seed", trial["seed"], "(k = %d)" % k, "" if trial["seed"] == case["seed"] else "<-- differs",
              vrb_chunk_kinds(trial, vrb_replay(orc, trial)))
