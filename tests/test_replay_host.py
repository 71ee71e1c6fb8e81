"""The replay window's host side (hive_alphazero_amd/replay.py): ring bookkeeping and index-draw mirrors, the ABI surface,
and the checks add_packed makes before it touches the device.  No GPU."""
import itertools

import numpy as np
import pytest

from hive_alphazero_amd import _lib, records, replay


# ------------------------------------------------------------------ synthetic packed batches (shared with test_gpu_replay.py)
def synthetic_games(rng, lengths, results, supports=None, first_id=0):
    """Finished games as SelfPlay collects them, from a seeded generator: random 56-bit feature words with bits 31 and
    36..43 clear (the packed word never carries them), random history words, 0..4 valid history entries, a random turn byte
    and mover, a policy normalised over a random support.  `supports` = support sizes to use first, row by row."""
    supports = list(supports or [])
    clear = ~np.uint64((1 << 31) | (0xFF << 36))
    games = []
    for g, (length, result) in enumerate(zip(lengths, results)):
        plies = []
        for _ in range(length):
            words = (rng.integers(0, 1 << 56, size=144, dtype=np.uint64)) & clear
            hist = rng.integers(0, 1 << 32, size=(4, 2, 6), dtype=np.uint64).astype(np.uint32)
            size = supports.pop(0) if supports else int(rng.integers(0, 80))
            policy = np.zeros(1584, dtype=np.float32)
            if size:
                cols = rng.choice(1584, size=size, replace=False)
                w = rng.random(size) + 0.1
                policy[cols] = (w / w.sum()).astype(np.float32)
            plies.append((words, hist, int(rng.integers(0, 5)), int(rng.integers(0, 256)), policy, int(rng.integers(0, 2))))
        games.append((int(result), plies, first_id + g))
    return games


def synthetic_packed(seed, lengths, results, supports=None):
    return records.pack_games(synthetic_games(np.random.default_rng(seed), lengths, results, supports))


# ------------------------------------------------------------------ ring mirror against a brute-force list
@pytest.mark.parametrize("order", list(itertools.permutations([0, 1, 63, 64, 65, 200]))[::37] + [(200, 200, 1), (63, 1, 1, 64)])
def test_ring_model_matches_a_list(order):
    cap = 64
    ring, slots, window, serial = replay.RingModel(cap), [None] * cap, [], 0
    for rows in order:
        batch = list(range(serial, serial + rows))
        serial += rows
        written = ring.append(rows)
        assert [i for i, _ in written] == list(range(max(0, rows - cap), rows))
        assert len({s for _, s in written}) == len(written)            # every slot is written once per append
        for i, s in written:
            slots[s] = batch[i]
        window = (window + batch)[-cap:]
        assert ring.live == len(window) and ring.appended == serial
        assert [slots[ring.slot_of(k)] for k in range(ring.live)] == window
        assert ring.head == serial % cap
        with pytest.raises(IndexError):
            ring.slot_of(ring.live)
    ring.clear()
    assert ring.live == 0 and ring.head == 0 and ring.appended == serial


def test_ring_model_refuses_nonsense():
    with pytest.raises(ValueError):
        replay.RingModel(0)
    with pytest.raises(ValueError):
        replay.RingModel(4).append(-1)


# ------------------------------------------------------------------ the index draw
def _splitmix_int(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def test_draw_indices_is_the_generator_of_hive_rng():
    """Entry i, spelled out with Python integers after csrc/hive_rng.hpp (Rng(seed, a, b, c), then one splitmix step)."""
    m = (1 << 64) - 1
    seed, step, sid, live = 0xDEADBEEFCAFEF00D, 12345, 7, 1000003
    got = replay.draw_indices(seed, step, sid, 50, live)
    for i in range(50):
        s = _splitmix_int(seed ^ _splitmix_int((step * 0x100000001B3 + _splitmix_int((sid * 0x9E3779B1 + i) & m)) & m))
        assert got[i] == ((_splitmix_int(s) >> 32) * live) >> 32


def test_draw_indices_properties():
    a = replay.draw_indices(3, 10, 0, 4096, 64)
    assert a.dtype == np.int64 and a.shape == (4096,)
    assert np.array_equal(a, replay.draw_indices(3, 10, 0, 4096, 64))                      # deterministic
    assert np.array_equal(a[:100], replay.draw_indices(3, 10, 0, 100, 64))                 # entry i does not depend on n
    assert a.min() >= 0 and a.max() < 64
    assert set(a.tolist()) == set(range(64))                                               # 64 x 64 draws reach all 64 slots
    assert not np.array_equal(a, replay.draw_indices(3, 11, 0, 4096, 64))                  # step
    assert not np.array_equal(a, replay.draw_indices(3, 10, 1, 4096, 64))                  # stream_id (a DDP rank)
    assert not np.array_equal(a, replay.draw_indices(4, 10, 0, 4096, 64))                  # seed
    for live in (1, 2, 3, 63, 1000, (1 << 32) - 1):
        d = replay.draw_indices(0, 0, 0, 512, live)
        assert d.min() >= 0 and d.max() < live
    assert not replay.draw_indices(0, 0, 0, 512, 1).any()
    with pytest.raises(ValueError):
        replay.draw_indices(0, 0, 0, 4, 0)


def test_discount_table_is_what_packed_values_multiplies_by():
    t = replay.discount_table()
    assert t.dtype == np.float32 and t.shape == (256,) and t[0] == 1.0
    packed = synthetic_packed(5, [200], [1])
    packed["meta"][:, 2] = 0                                # one side moves 200 times: k = 199 .. 0
    assert np.array_equal(records.packed_values(packed), t[np.arange(199, -1, -1)])


# ------------------------------------------------------------------ ABI
REPLAY_SYMBOLS = ["hive_replay_create", "hive_replay_destroy", "hive_replay_clear", "hive_replay_stats", "hive_replay_append",
                  "hive_replay_import", "hive_replay_export", "hive_replay_sample"]


def test_replay_symbols_are_declared_and_exported():
    import hive_alphazero_amd as h
    h.build()
    L = h.load()
    for name in REPLAY_SYMBOLS:
        assert name in _lib.ABI_SYMBOLS
        assert getattr(L, name).argtypes, name


# ------------------------------------------------------------------ add_packed refuses before the device is involved
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"{name} called: the batch must be refused on the host")


def test_add_packed_refuses_257_entries_before_any_device_call(monkeypatch):
    packed = synthetic_packed(1, [3, 2], [1, -1], supports=[5, 257, 0])
    assert int(np.diff(packed["pol_ptr"]).max()) == 257
    monkeypatch.setattr(_lib, "load", lambda: _NoDevice())
    monkeypatch.setattr(replay.ReplayBuffer, "device", property(lambda self: (_ for _ in ()).throw(AssertionError("device asked"))))
    buf = replay.ReplayBuffer(64)
    with pytest.raises(ValueError, match="257"):
        buf.add_packed(packed)
    assert len(buf) == 0 and buf.rows_seen == 0 and buf.games_seen == 0
    ok = synthetic_packed(1, [3, 2], [1, -1], supports=[5, 256, 0])
    assert replay.check_packed(ok) == (5, 2)
    bad = dict(ok)
    bad["game_ptr"] = ok["game_ptr"][:-1]
    with pytest.raises(ValueError):
        buf.add_packed(bad)


def test_zero_row_batch_needs_no_device(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _NoDevice())
    buf = replay.ReplayBuffer(8)
    assert buf.add_packed(records.pack_games([])) == 0
    assert len(buf) == 0 and buf.rows_seen == 0
    with pytest.raises(RuntimeError):
        buf.sample(4, step=0)
    with pytest.raises(ValueError):
        replay.ReplayBuffer(0)
