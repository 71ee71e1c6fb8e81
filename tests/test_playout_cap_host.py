"""Playout-cap records on the host: the optional `full` key of a packed batch through every container, records.PlyLog
with flags against a naive double loop and datasets that keep the flagged rows with whole-game values.  Plain numpy: no GPU."""
import numpy as np

from hive_alphazero_amd import records

KEY = records.FULL_KEY


def _hand_batch(seed, lengths, flags=None):
    """A packed batch of len(lengths) games built row by row through records.pack_games (+ the flags)."""
    rng = np.random.default_rng(seed)
    games = []
    for g, n in enumerate(lengths):
        first = int(rng.integers(1, 3))
        plies = []
        for i in range(n):
            turn = first + i
            policy = np.zeros(1584, np.float32)
            k = int(rng.integers(0, 9))
            policy[rng.choice(1584, k, replace=False)] = rng.random(k).astype(np.float32) + np.float32(0.01)
            hist = rng.integers(0, 2 ** 32, (4, 2, 6), dtype=np.uint32) & np.uint32(0x0FFF0FFF)     # 12 columns per board row
            plies.append((rng.integers(0, 2 ** 56, 144, dtype=np.uint64), hist, int(rng.integers(0, 5)), turn, policy,
                          0 if turn % 2 == 1 else 1))
        games.append(((1, -1, 0)[g % 3], plies, 100 + g))
    packed = records.pack_games(games)
    if flags is not None:
        packed[KEY] = np.asarray(flags, dtype=np.uint8)
        assert len(packed[KEY]) == sum(lengths)
    return packed


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(a[k], b[k]), k


def _flags(seed, n):
    return (np.random.default_rng(seed).random(n) < 0.4).astype(np.uint8)


def test_full_key_survives_slice_concat_file_and_blob(tmp_path):
    lengths = [7, 3, 11, 5]
    flags = _flags(1, sum(lengths))
    assert 0 < flags.sum() < len(flags)
    packed = _hand_batch(2, lengths, flags)
    assert KEY not in records.PACKED_KEYS                      # the key is optional: the mandatory set is what it was
    # slice
    part = records.slice_packed(packed, 1, 3)
    assert np.array_equal(part[KEY], flags[7:21]) and len(part[KEY]) == len(part["meta"])
    # the slices concatenate back into the batch
    _same(records.concat_packed([records.slice_packed(packed, 0, 1), part, records.slice_packed(packed, 3, 4)]), packed)
    # a keyless batch counts as all ones, on either side
    plain = _hand_batch(3, [4, 6])
    assert KEY not in plain
    for order in ((packed, plain), (plain, packed)):
        both = records.concat_packed(list(order))
        want = np.concatenate([b[KEY] if KEY in b else np.ones(len(b["meta"]), np.uint8) for b in order])
        assert both[KEY].dtype == np.uint8 and np.array_equal(both[KEY], want)
        assert len(both[KEY]) == len(both["meta"]) == int(both["game_ptr"][-1])
    assert KEY not in records.concat_packed([plain, plain])    # keyless batches stay keyless
    # file
    path = records.save_packed(str(tmp_path / "play.npz"), packed)
    _same(records.load_packed(path), packed)
    path = records.save_packed(str(tmp_path / "plain.npz"), plain)
    _same(records.load_packed(path), plain)
    # blob
    layout = records.packed_to_blob(packed, str(tmp_path / "blob.bin"))
    assert [k for k, _, _, _ in layout] == list(records.PACKED_KEYS) + [KEY]
    _same(records.packed_from_blob(str(tmp_path / "blob.bin"), layout), packed)
    layout = records.packed_to_blob(plain, str(tmp_path / "blob2.bin"))
    assert [k for k, _, _, _ in layout] == list(records.PACKED_KEYS)
    # the tuple views ignore the key
    assert records.unpack_game(packed, 2)[2] == 102 and len(records.unpack_game(packed, 2)[1]) == 11


def test_dataset_keeps_flagged_rows_with_whole_game_values():
    lengths = [9, 6, 12]
    flags = _flags(5, sum(lengths))
    flags[9:15] = 0                                            # a game without a training row
    packed = _hand_batch(6, lengths, flags)
    keyless = {k: packed[k] for k in records.PACKED_KEYS}
    states_all, pol_all, val_all = records.dataset_from_packed(keyless)
    assert len(val_all) == sum(lengths) and np.array_equal(val_all, records.packed_values(packed))
    keep = np.flatnonzero(flags)
    assert np.array_equal(records.training_rows(packed), keep)
    states, pol, val = records.dataset_from_packed(packed)
    assert np.array_equal(states, states_all[keep]) and np.array_equal(pol, pol_all[keep])
    assert np.array_equal(val.view(np.uint32), val_all[keep].view(np.uint32))
    # the values are NOT those of a batch made of the flagged rows alone: the dropped plies still count as moves to come
    alone = records.pack_games([(v, [p for p, f in zip(plies, flags[lo:hi]) if f], gid)
                                for (v, plies, gid), lo, hi in ((records.unpack_game(packed, g), int(packed["game_ptr"][g]),
                                                                 int(packed["game_ptr"][g + 1])) for g in range(3))])
    assert not np.array_equal(records.packed_values(alone), val)
    # all zeros: an empty dataset, not an error
    packed[KEY] = np.zeros(sum(lengths), np.uint8)
    states, pol, val = records.dataset_from_packed(packed)
    assert states.shape == (0, 12, 12, 56) and pol.shape == (0, 1584) and val.shape == (0,)


SLOTS, PLIES = 4, 10
CLOSES = {3: [1], 5: [0, 3], 8: [1, 2], 10: [0, 1, 2, 3]}


def test_plylog_with_flags_cuts_what_a_naive_double_loop_cuts():
    """Four slots, ten plies, flags from ply 2 on (the plies before count as all ones), one entry left unsettled: every
    batch equals pack_games of the rows a double loop picks, and its `full` key the flags that loop collects."""
    rng = np.random.default_rng(8)
    plies = []
    for q in range(PLIES):
        boards = rng.integers(0, 256, (SLOTS, 64), dtype=np.uint8)
        boards[:, 33] = rng.integers(1, 55, SLOTS)
        boards[:, 35] = rng.integers(1, 5, SLOTS) | (rng.integers(1, 5, SLOTS) << 4)
        policy = np.zeros((SLOTS, 1584), np.float32)
        for s in range(SLOTS):
            k = int(rng.integers(0, 7))
            policy[s, rng.choice(1584, k, replace=False)] = rng.random(k).astype(np.float32) + np.float32(0.01)
        plies.append({"feat": rng.integers(0, 2 ** 56, (SLOTS, 144), dtype=np.uint64),
                      "hist": rng.integers(0, 2 ** 32, (SLOTS, 2, 4, 2, 6), dtype=np.uint32), "boards": boards, "policy": policy,
                      "moved": rng.random(SLOTS) < 0.85, "full": (rng.random(SLOTS) < 0.4).astype(np.int8) if q >= 2 else None})

    def row(p, s):
        turn = int(p["boards"][s, 33])
        mover = 0 if turn % 2 == 1 else 1
        nib = int(p["boards"][s, 35])
        return (p["feat"][s].copy(), p["hist"][s, mover].copy(), nib % 16 if mover == 0 else nib // 16, turn, p["policy"][s].copy(), mover)

    log = records.PlyLog(SLOTS)
    ids, next_id, start, seen = list(range(SLOTS)), SLOTS, [0] * SLOTS, 0
    for ply in range(PLIES + 1):
        if ply in CLOSES:
            slots = CLOSES[ply]
            winner = [(ply + s) % 3 for s in range(SLOTS)]
            want, want_flags = [], []
            for s in slots:
                qs = [q for q in range(start[s], ply) if plies[q]["moved"][s]]
                if qs:
                    want.append(({1: 1, 2: -1, 0: 0}[winner[s]], [row(plies[q], s) for q in qs], ids[s]))
                    want_flags += [1 if plies[q]["full"] is None else int(plies[q]["full"][s] != 0) for q in qs]
                start[s] = ply
            got = log.close_games(slots, winner, ids, ply)
            ref = records.pack_games(want)
            if ply >= 3:
                ref[KEY] = np.asarray(want_flags, dtype=np.uint8)
            _same(got, ref)
            seen += len(want_flags)
            for s in slots:
                ids[s], next_id = next_id, next_id + 1
        if ply == PLIES:
            break
        p = plies[ply]
        log.append(ply, p["feat"].copy(), p["policy"].copy(), p["boards"].copy(), p["hist"].copy(), p["moved"].copy(),
                   full=None if p["full"] is None else p["full"].copy())
        if len(log.entries) >= 2 and log.entries[-2]["ply"] != 6:
            log.settle(log.entries[-2])
    assert seen > 20


def test_new_symbols_are_declared_and_bound():
    from hive_alphazero_amd import _lib
    L = _lib.load()
    for name in ("hive_search_set_budgets", "hive_search_draw_budgets", "hive_arena_budget_launch", "hive_replay_append_ranked"):
        assert name in _lib.ABI_SYMBOLS
        assert getattr(L, name).argtypes, name


def test_selfplay_worker_says_it_has_no_playout_cap():
    from hive_alphazero_amd import self_play
    assert "playout_cap" in self_play.SelfPlayWorker.__doc__
