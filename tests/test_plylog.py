"""records.PlyLog -- the per-ply host log of mcts.SelfPlay and its one cutter -- against a naive cutter written here.
Plain numpy: no GPU, no torch."""
import warnings

import numpy as np

from hive_alphazero_amd import records

SLOTS, PLIES, KEPT = 5, 14, 8
# ply -> slots whose game ends before that ply is logged (as SelfPlay retires games at the start of play_ply)
CLOSES = {3: [1], 5: [0, 4], 6: [3], 7: [1], 9: [0, 2, 4], 14: [0, 1, 2, 3, 4]}
UNSETTLED = {4, 10}            # plies whose entry is never settled (besides the newest one at every close)


def _synthetic_plies():
    """Seeded whole-batch arrays of PLIES plies; the special cases are written in by hand below."""
    rng = np.random.default_rng(20)
    plies = []
    for _ in range(PLIES + 1):
        boards = rng.integers(0, 256, (SLOTS, 64), dtype=np.uint8)
        boards[:, 33] = rng.integers(1, 55, SLOTS)                           # turn: both parities
        boards[:, 35] = rng.integers(1, 5, SLOTS) | (rng.integers(1, 5, SLOTS) << 4)    # both nibbles in use, different
        policy = np.zeros((SLOTS, 1584), np.float32)
        for s in range(SLOTS):
            k = int(rng.integers(0, 13))
            policy[s, rng.choice(1584, k, replace=False)] = rng.random(k).astype(np.float32) + np.float32(0.01)
        plies.append({"feat": rng.integers(0, 2 ** 56, (SLOTS, 144), dtype=np.uint64),
                      "hist": rng.integers(0, 2 ** 32, (SLOTS, 2, 4, 2, 6), dtype=np.uint32),     # distinct per perspective
                      "boards": boards, "policy": policy, "moved": np.ones(SLOTS, dtype=bool)})
    plies[1]["policy"][0] = 0                       # a pass: no edge visited, but the game did move
    plies[11]["policy"][3] = 0
    plies[2]["moved"][0] = False                    # did not move in the middle of a game
    plies[4]["moved"][2] = False
    plies[12]["moved"][1] = False
    for p in (5, 6, 7, 8):
        plies[p]["moved"][4] = False                # the game slot 4 plays over plies 5..8 never logs a row
    assert {int(p["boards"][s, 33]) % 2 for p in plies for s in range(SLOTS)} == {0, 1}
    return plies


def _hand_row(p, s):
    """The six-tuple of slot s at one ply, straight from the ply's arrays (include/hive_abi.h: turn in byte 33, valid
    history entries of white's / black's perspective in the low / high nibble of byte 35; white moves on odd turns)."""
    turn = int(p["boards"][s, 33])
    mover = 0 if turn % 2 == 1 else 1
    nib = int(p["boards"][s, 35])
    hlen = nib % 16 if mover == 0 else nib // 16
    return (p["feat"][s].copy(), p["hist"][s, mover].copy(), hlen, turn, p["policy"][s].copy(), mover)


def _same_row(a, b):
    return len(a) == len(b) == 6 and all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(a, b))


def test_plylog_cuts_the_games_a_naive_double_loop_cuts():
    """Five slots, fourteen plies: a pass ply, plies on which a game did not move, a slot refilled twice, two games ending on
    one ply with the higher id in the lower slot, a game that never logged a row (leaves no entry), a slot whose opening was
    not logged (counted, no entry), more finished games waiting than `max_finished_kept` (one warning, the rest counted),
    and every close made while the newest entry -- and two older ones -- are still unsettled.  Every batch must equal
    records.pack_games of the rows a plain double loop picks, key by key, dtype by dtype."""
    plies = _synthetic_plies()
    log = records.PlyLog(SLOTS, max_finished_kept=KEPT)
    log.unlogged[3] = True                                   # (what SelfPlay.stagger marks)
    ids, next_id = list(range(SLOTS)), SLOTS
    # the naive side's own bookkeeping
    start, unlogged, waiting = [0] * SLOTS, [False, False, False, True, False], 0
    seen_ids, empty_games, trimmed, warned, tokens = [], 0, False, [], {}
    for ply in range(PLIES + 1):
        if ply in CLOSES:
            slots = CLOSES[ply]
            winner = [(ply + s) % 3 for s in range(SLOTS)]          # 1 = white, 2 = black, 0 = draw / cap
            want = []
            for s in slots:                                         # ---- the naive cutter
                if unlogged[s]:
                    unlogged[s] = False
                elif waiting + len(want) < KEPT:
                    rows = [_hand_row(plies[q], s) for q in range(start[s], ply) if plies[q]["moved"][s]]
                    if rows:
                        want.append(({1: 1, 2: -1, 0: 0}[winner[s]], rows, ids[s]))
                    else:
                        empty_games += 1                            # leaves no entry
                start[s] = ply
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                got = log.close_games(slots, winner, ids, ply, waiting)
            warned += [w for w in caught if "finished games are waiting" in str(w.message)]
            if want:
                ref = records.pack_games(want)
                assert got is not None and sorted(got) == sorted(records.PACKED_KEYS)
                for k in records.PACKED_KEYS:
                    assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (ply, k)
                waiting += len(want)
                seen_ids.append(got["game_id"].tolist())
            else:
                assert got is None, ply
            for s in slots:
                ids[s], next_id = next_id, next_id + 1
            assert log.start_ply == start
        if ply == PLIES:
            break
        p = plies[ply]
        tokens[ply] = object()                                   # (stands for the engine's pinned staging set)
        log.append(ply, p["feat"].copy(), p["policy"].copy(), p["boards"].copy(), p["hist"].copy(), p["moved"].copy(),
                   keepalive=tokens[ply])
        assert log.entries[-1]["ply"] == ply and log.entries[0]["ply"] >= min(start)     # nothing older than the oldest game
        assert [e["ply"] for e in log.entries] == list(range(max(min(start), 0), ply + 1))
        trimmed = trimmed or log.entries[0]["ply"] > 0
        # the newest entry, unsettled: every slot's row by hand == ply_record (CSR built on demand), before and after settle
        e = log.entries[-1]
        before = [records.PlyLog.ply_record(e, s) for s in range(SLOTS)]
        assert all(_same_row(before[s], _hand_row(p, s)) for s in range(SLOTS))
        if len(log.entries) >= 2 and log.entries[-2]["ply"] not in UNSETTLED:
            prev = log.entries[-2]
            had = [records.PlyLog.ply_record(prev, s) for s in range(SLOTS)]
            assert "policy" in prev and log.settle(prev) is tokens[prev["ply"]] and "policy" not in prev
            assert log.settle(prev) is None                                  # settled once
            assert all(_same_row(had[s], records.PlyLog.ply_record(prev, s)) for s in range(SLOTS))
            assert all(_same_row(had[s], _hand_row(plies[prev["ply"]], s)) for s in range(SLOTS))
    # what the scenario was built to contain
    assert seen_ids == [[1], [0, 4], [5], [6, 2], [10, 9]]          # [6, 2]: ascending slot, descending id; 7 left nothing
    assert empty_games == 1 and log.unrecorded_games == 1
    assert waiting == KEPT and log.dropped_games == 3 and len(warned) == 1
    assert trimmed
    for s in range(SLOTS):                                   # every slot idle: the log forgets everything
        log.idle(s)
    p = plies[PLIES]
    log.append(PLIES, p["feat"], p["policy"], p["boards"], p["hist"], p["moved"])
    assert log.entries == []
    # SelfPlay hands the staging buffers over as they are: features as int64 bits, the history as 384 bytes per slot
    p = plies[0]
    log = records.PlyLog(SLOTS)
    log.append(0, p["feat"].view(np.int64), p["policy"], p["boards"], p["hist"].view(np.uint8).reshape(SLOTS, 384), p["moved"])
    assert all(_same_row(records.PlyLog.ply_record(log.entries[0], s), _hand_row(p, s)) for s in range(SLOTS))
    got = log.close_games([0, 2], [1, 0, 2, 0, 0], [40, 41, 42, 43, 44], 1)
    ref = records.pack_games([(1, [_hand_row(p, 0)], 40), (-1, [_hand_row(p, 2)], 42)])
    for k in records.PACKED_KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
