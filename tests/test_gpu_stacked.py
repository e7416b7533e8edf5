"""GPU tests (`-m gpu`) of frame-stacked sampling: tsm_vrb_gather_stacked (csrc/vrb.hip) is bit-identical to rounds of
`index.prev` + `index.gather`, on the buffer state of fixture C (tests/golden/recurrent.npz: what the reference's
VectorReplayBuffer(stack_num=4) holds after a recorded add trace) and on a freshly wrapped buffer; `buf[idx]`, `get` and
`sample_indices(0)` with `sample_avail` equal what the reference recorded, exactly."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DEV = "cuda"

if torch.cuda.is_available():
    from tianshou_marl_amd.data.batch import Batch
    from tianshou_marl_amd.data.buffer import PrioritizedVectorReplayBuffer, VectorReplayBuffer

Z = np.load(os.path.join(HERE, "golden", "recurrent.npz"))


def _fixture_buffer(cls=None, **kw):
    buf = (cls or VectorReplayBuffer)(24, 3, device=DEV, **kw)
    for k in range(len(Z["c_env"])):
        buf.add(Batch(obs=Z["c_obs"][k:k + 1], act=np.zeros((1, 2), int), rew=np.zeros((1, 2)), terminated=Z["c_done"][k:k + 1],
                      truncated=np.zeros(1, bool), obs_next=Z["c_obs_next"][k:k + 1]), buffer_ids=[int(Z["c_env"][k])])
    return buf


def _wrapped_buffer():
    """2 sub-buffers of 5 slots, 13 joint steps each: wrapped more than twice, dones scattered, the last row done in env 1."""
    buf = VectorReplayBuffer(10, 2, device=DEV, stack_num=3)
    rs = np.random.RandomState(2)
    for k in range(13):
        done = np.array([k in (3, 9, 10), k in (7, 12)])
        buf.add(Batch(obs=rs.standard_normal((2, 3, 4)).astype(np.float32), act=np.zeros((2, 3), int), rew=np.zeros((2, 3)),
                      terminated=done, truncated=np.zeros(2, bool), obs_next=rs.standard_normal((2, 3, 4)).astype(np.float32)))
    return buf


def _by_rounds(buf, store, idx, L):
    cols, cur = [], idx
    for _ in range(L):
        cols.append(buf.index.gather(store, cur))
        cur = buf.index.prev(cur)
    return torch.stack(cols[::-1], dim=1)


@pytest.mark.parametrize("which", ["fixture", "wrapped"])
@pytest.mark.parametrize("L", [1, 2, 4])
def test_gather_stacked_is_rounds_of_prev_and_gather(which, L):
    buf = _fixture_buffer(stack_num=4) if which == "fixture" else _wrapped_buffer()
    S, B = buf.sub_size, buf.buffer_num
    # every slot of every sub-buffer: the oldest row, the rows right after a done, both edges of each sub-buffer, unfilled slots;
    # and indices outside [0, maxsize), which wrap as prev's do
    idx = torch.cat([torch.arange(S * B), torch.tensor([-1, S * B, S * B + S - 1])]).to(DEV)
    last, done = buf.index.last_index.cpu().numpy(), buf.done_store.cpu().numpy()
    assert done.any() and all(int(l) in idx.tolist() for l in last)
    for store in (buf.obs_store, buf.obs_next_store, buf.rew_store, buf.done_store.unsqueeze(-1)):
        want = _by_rounds(buf, store, idx, L)
        got = buf.index.gather_stacked(store, idx, L)
        assert got.shape == want.shape == (len(idx), L, *store.shape[2:]) and got.dtype == store.dtype
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    for lane in range(buf.n_agent):   # the lane form: one agent's column without a second pass
        got = buf.index.gather_stacked(buf.obs_store, idx, L, lane=lane)
        assert torch.equal(got, _by_rounds(buf, buf.obs_store, idx, L)[:, :, lane])
    with pytest.raises(ValueError, match="lane"):
        buf.index.gather_stacked(buf.obs_store, idx, L, lane=buf.n_agent)
    with pytest.raises(ValueError, match="stack_num"):
        buf.index.gather_stacked(buf.obs_store, idx, 0)


def test_fixture_c_items_and_available_indices():
    buf = _fixture_buffer(stack_num=4)
    assert np.array_equal(buf.index.insertion_idx.cpu().numpy(), Z["c_insertion_idx"])
    idx = Z["c_idx"]
    assert np.array_equal(buf.sample_indices(0), idx) and np.array_equal(buf.prev(idx), Z["c_prev"])
    got = buf[idx]
    assert got.obs.shape == (len(idx), 4, 2, 3)
    assert np.array_equal(got.obs, Z["c_stack_obs"]) and np.array_equal(got.obs_next, Z["c_stack_obs_next"])
    assert np.array_equal(buf.get(idx, "obs"), Z["c_stack_obs"])
    assert np.array_equal(buf.get(idx, "obs", stack_num=1), Z["c_stack_obs"][:, -1])
    assert np.array_equal(buf.get(idx, "obs_next", stack_num=2), Z["c_stack_obs_next"][:, -2:])
    assert np.array_equal(_fixture_buffer(stack_num=4, sample_avail=True).sample_indices(0), Z["c_avail"])
    # single frames are what they were
    one = _fixture_buffer()
    assert one[idx].obs.shape == (len(idx), 2, 3) and np.array_equal(one[idx].obs, Z["c_stack_obs"][:, -1])


def test_ignore_obs_next_stacks_obs_at_next():
    """buffer_base.py:612-616: without an obs_next store, obs_next is the stack of `obs` ending at next(index)."""
    buf = _fixture_buffer(stack_num=4, ignore_obs_next=True)
    idx = Z["c_idx"]
    want = buf.get(buf.next(idx), "obs")
    assert np.array_equal(buf[idx].obs_next, want) and want.shape == (len(idx), 4, 2, 3)


def test_prioritized_buffer_stacks_and_samples_by_priority():
    buf = _fixture_buffer(PrioritizedVectorReplayBuffer, alpha=0.6, beta=0.4, stack_num=4, sample_avail=True)
    assert buf.options == dict(stack_num=4, ignore_obs_next=False, save_only_last_obs=False, sample_avail=True, alpha=0.6, beta=0.4)
    assert np.array_equal(buf[Z["c_idx"]].obs, Z["c_stack_obs"])
    assert np.array_equal(buf.sample_indices(0), Z["c_avail"])
    drawn = buf.sample_indices(64)   # by priority, whatever sample_avail says (prio.py:62-67)
    assert set(drawn) <= set(Z["c_idx"]) and not set(drawn) <= set(Z["c_avail"])
