"""The replay window on the GPU (csrc/hive_replay.hip through hive_alphazero_amd/replay.py): whatever is appended comes back
from gather / sample as exactly the tensors records.dataset_tensors_gpu_packed builds from the same rows."""
import numpy as np
import pytest
import torch

from hive_alphazero_amd import records, replay
from test_replay_host import synthetic_games, synthetic_packed

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _dense(packed, dtype=torch.float32, layout="chw"):
    return records.dataset_tensors_gpu_packed(packed, dtype=dtype, layout=layout)


def _same(got, want):
    for g, w, name in zip(got, want, ("planes", "policies", "values")):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert torch.equal(g, w), name


@pytest.fixture(scope="module")
def six_games():
    """6 games of 1, 2, 3, 9, 30 and 55 rows, results +1 / -1 / 0 all there, policy supports of 0, 1 and 256 entries."""
    packed = synthetic_packed(11, [1, 2, 3, 9, 30, 55], [1, -1, 0, -1, 0, 1], supports=[0, 1, 256, 256, 0, 1, 255])
    widths = np.diff(packed["pol_ptr"])
    assert len(packed["meta"]) == 100 and {0, 1, 256} <= set(widths.tolist()) and widths.max() == 256
    buf = replay.ReplayBuffer(128)
    assert buf.add_packed(packed) == 100
    yield packed, buf
    buf.close()


@pytest.fixture(scope="module")
def window64():
    """Capacity 64 after batches of 40, 50 and 60 rows: the last 64 rows of the 150, as the dense fp32 reference."""
    rng = np.random.default_rng(23)
    batches = [records.pack_games(synthetic_games(rng, lens, res, first_id=10 * k))
               for k, (lens, res) in enumerate((([7, 33], [1, 0]), ([1, 20, 29], [-1, 1, 0]), ([45, 15], [0, -1])))]
    assert [len(b["meta"]) for b in batches] == [40, 50, 60]
    buf = replay.ReplayBuffer(64)
    for b in batches:
        buf.add_packed(b)
    dense = tuple(t[-64:].clone() for t in _dense(records.concat_packed(batches), layout="hwc"))
    yield buf, dense
    buf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_gather_all_equals_the_dense_dataset(six_games, dt, layout):
    packed, buf = six_games
    assert len(buf) == 100 and buf.rows_seen == 100 and buf.games_seen == 6 and buf.capacity == 128
    _same(buf.gather(torch.arange(100, device="cuda"), dtype=DTYPES[dt], layout=layout), _dense(packed, DTYPES[dt], layout))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gather_channels_last_view(six_games, dt):
    packed, buf = six_games
    planes, policies, values = buf.gather(np.arange(100), dtype=DTYPES[dt], layout="nchw_channels_last")
    want = _dense(packed, DTYPES[dt], "chw")
    assert planes.shape == (100, 56, 12, 12) and planes.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(planes, want[0]) and torch.equal(policies, want[1]) and torch.equal(values, want[2])
    assert planes.contiguous(memory_format=torch.channels_last).data_ptr() == planes.data_ptr()      # no copy for the trainer


@pytest.mark.gpu
def test_values_cover_every_result(six_games):
    packed, buf = six_games
    values = buf.gather(np.arange(100))[2].cpu().numpy()
    assert np.array_equal(values, records.packed_values(packed))
    assert (values > 0).any() and (values < 0).any() and (values[3:6] < 0).all()                  # game 2 is a draw: -1 for both


@pytest.mark.gpu
def test_wrap_around_keeps_the_last_rows_in_order(window64):
    buf, dense = window64
    assert len(buf) == 64 and buf.rows_seen == 150 and buf.games_seen == 7
    # (rows 86..149: the 4 last rows of the second batch's last game, whose earlier rows are gone, keep that game's values)
    _same(buf.gather(np.arange(64), layout="hwc"), dense)
    assert buf.add_packed(records.pack_games([])) == 0                                              # a zero-row batch: no-op
    assert len(buf) == 64 and buf.rows_seen == 150
    _same(buf.gather(np.arange(64), layout="hwc"), dense)
    with pytest.raises(IndexError):
        buf.gather([64])


@pytest.mark.gpu
def test_one_batch_longer_than_the_window_keeps_its_tail():
    packed = synthetic_packed(31, [60, 3, 90, 47], [1, 0, -1, 1])
    assert len(packed["meta"]) == 200
    buf = replay.ReplayBuffer(64)
    buf.add_packed(synthetic_packed(32, [10], [1]))                                                 # head is not at slot 0
    buf.add_packed(packed)
    assert len(buf) == 64 and buf.rows_seen == 210
    _same(buf.gather(np.arange(64), dtype=torch.bfloat16), tuple(t[-64:] for t in _dense(packed, torch.bfloat16)))
    buf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, replay.MAX_BLOCKS + 3])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_dirty_outputs_duplicates_and_shuffled_order(window64, n, dt):
    """Every output byte is written by the launch: buffers full of NaN / 0xFF come back as dense[idx].  n = 2051 is past the
    2048 workgroups of one launch, so the stride loop runs twice."""
    buf, dense = window64
    assert replay.MAX_BLOCKS == 2048
    g = torch.Generator().manual_seed(n)
    idx = torch.randint(0, 64, (n,), generator=g)
    if n == 7:
        idx[3] = idx[0]                                                                             # a duplicate for sure
    planes = torch.empty((n, 12, 12, 56), dtype=DTYPES[dt], device="cuda")
    planes.view(torch.uint8).fill_(0xFF)                                                            # NaN in f32, f16 and bf16
    policies = torch.full((n, 1584), float("nan"), device="cuda")
    values = torch.full((n,), float("nan"), device="cuda")
    out = buf.gather(idx.cuda(), dtype=DTYPES[dt], layout="hwc", out=(planes, policies, values))
    assert out[0].data_ptr() == planes.data_ptr() and out[1].data_ptr() == policies.data_ptr()
    j = idx.cuda()
    assert torch.equal(planes, dense[0][j].to(DTYPES[dt]))                                         # 0 / 1 / turn <= 255: exact
    assert torch.equal(policies, dense[1][j]) and torch.equal(values, dense[2][j])


@pytest.mark.gpu
def test_device_draw_matches_the_mirror(window64):
    buf, dense = window64
    a = buf.sample(300, step=5, seed=9, stream_id=2, layout="hwc", return_indices=True)
    want = replay.draw_indices(9, 5, 2, 300, 64)
    assert a[3].dtype == torch.int64 and np.array_equal(a[3].cpu().numpy(), want)
    _same(a[:3], buf.gather(a[3], layout="hwc"))
    _same(a[:3], tuple(t[torch.from_numpy(want).cuda()] for t in dense))
    b = buf.sample(300, step=5, seed=9, stream_id=2, layout="hwc", return_indices=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                                            # same keys, same batch
    c = buf.sample(300, step=6, seed=9, stream_id=2, return_indices=True)[3]
    d = buf.sample(300, step=5, seed=9, stream_id=3, return_indices=True)[3]
    assert not torch.equal(a[3], c) and not torch.equal(a[3], d)
    assert len(buf.sample(4, step=0)) == 3


@pytest.mark.gpu
def test_a_window_of_one_row_and_an_empty_one():
    packed = synthetic_packed(41, [1], [-1], supports=[3])
    buf = replay.ReplayBuffer(5)
    with pytest.raises(RuntimeError):
        buf.sample(4, step=0)
    buf.add_packed(packed)
    planes, policies, values, drawn = buf.sample(9, step=1, return_indices=True)
    assert not drawn.any()
    want = _dense(packed)
    assert torch.equal(planes, want[0].expand(9, -1, -1, -1)) and torch.equal(policies, want[1].expand(9, -1))
    assert torch.equal(values, want[2].expand(9))
    buf.close()


@pytest.mark.gpu
def test_state_dict_round_trip_and_appends_after_it(window64, tmp_path):
    buf, dense = window64
    state = buf.state_dict()
    assert state["feat"].shape == (64, 144) and state["pol_idx"].shape == (64, 256) and state["meta"].shape == (64, 3)
    np.savez(tmp_path / "window.npz", **state)
    with np.load(tmp_path / "window.npz") as z:
        state = {k: z[k] for k in z.files}
    twin = replay.ReplayBuffer(64)
    twin.load_state_dict(state)
    assert len(twin) == 64 and twin.rows_seen == buf.rows_seen and twin.games_seen == buf.games_seen
    _same(twin.gather(np.arange(64), layout="hwc"), dense)
    more = synthetic_packed(51, [4, 13], [1, 0])
    first = replay.ReplayBuffer(64)
    first.load_state_dict(state)
    for b in (first, twin):
        b.add_packed(more)
    want = tuple(torch.cat([d[17:], m]) for d, m in zip(dense, _dense(more, layout="hwc")))
    _same(twin.gather(np.arange(64), layout="hwc"), want)
    _same(first.gather(np.arange(64), layout="hwc"), want)
    small = replay.ReplayBuffer(10)                                                                 # a smaller buffer keeps the newest
    small.load_state_dict(state)
    _same(small.gather(np.arange(10), layout="hwc"), tuple(d[-10:] for d in dense))
    for b in (twin, first, small):
        b.close()

