"""Playout-cap self-play, the arena with unequal sides and the replay window's training-row filter, end to end on the GPU:
whole games whose records carry the full / fast flag of every ply, cap options that change nothing, each arena side
searched with its own simulations, and a window that takes the flagged rows with whole-game values."""
import numpy as np
import pytest
import torch

from hive_alphazero_amd import mcts, records, replay
from test_gpu_budgets import _bits, _lib, _outputs, _p, _roots, _same_rows, _stream, stub_evaluator
from test_replay_host import synthetic_packed

KEY = records.FULL_KEY


def other_evaluator(planes):
    """A second pure per-row function: the stub's policy reversed, its value negated."""
    p, v = stub_evaluator(planes)
    return p.flip(1).contiguous(), -v


def _play_out(engine, limit=400):
    plies = 0
    while engine.running():
        engine.play_ply()
        plies += 1
        assert plies < limit
    torch.cuda.synchronize()


def _by_game(packed):
    """{game id: that game as a packed batch of its own}."""
    return {int(gid): records.slice_packed(packed, g, g + 1) for g, gid in enumerate(packed["game_id"].tolist())}


def _same_packed(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------ 7. whole games
@pytest.mark.gpu
def test_capped_selfplay_plays_whole_games_and_flags_every_ply():
    cap = {"full": 8, "fast": 2, "p_full": 0.25}
    seed, runs = 21, {}
    for G, ids in ((32, list(range(32))), (48, list(reversed(range(48))))):
        sp = mcts.SelfPlay(G, 8, stub_evaluator, seed=seed, plane_dtype=torch.float32, game_ids=ids, packed_records=True,
                           playout_cap=cap)
        _play_out(sp)
        assert sp.env.illegal_count() == 0 and sp.finished == G and sp.dropped_games == 0
        packed = sp.drain_finished_packed()
        hist = sp.leaf_histogram()
        sp.close()
        rows = len(packed["meta"])
        assert KEY in packed and packed[KEY].dtype == np.uint8 and len(packed[KEY]) == rows
        assert sorted(packed["game_id"].tolist()) == sorted(ids)
        # one row per ply: the turns of a game count up from 1 to its last move
        for g in range(G):
            lo, hi = int(packed["game_ptr"][g]), int(packed["game_ptr"][g + 1])
            assert packed["meta"][lo:hi, 1].tolist() == list(range(1, hi - lo + 1))
        gid = np.repeat(packed["game_id"], np.diff(packed["game_ptr"]))
        want = mcts.playout_cap_draw(seed, gid, packed["meta"][:, 1].astype(np.int64), cap["p_full"])
        assert np.array_equal(packed[KEY], want.astype(np.uint8))
        assert 0.1 < want.mean() < 0.4
        # every simulation of every searched ply is one histogram entry: the budgets add up
        assert sum(hist.values()) == int(np.where(want, cap["full"], cap["fast"]).sum())
        runs[G] = _by_game(packed)
    for gid in range(32):                                       # the same ids as other slots of a larger engine
        _same_packed(runs[32][gid], runs[48][gid])


@pytest.mark.gpu
def test_capped_selfplay_refuses_what_it_cannot_record():
    with pytest.raises(ValueError):                             # the per-row tuples have no room for the flag
        mcts.SelfPlay(4, 8, stub_evaluator, plane_dtype=torch.float32, playout_cap={"full": 8, "fast": 2, "p_full": 0.25})
    with pytest.raises(ValueError):                             # sims is the number of rounds: max(full, fast)
        mcts.SelfPlay(4, 6, stub_evaluator, plane_dtype=torch.float32, packed_records=True,
                      playout_cap={"full": 8, "fast": 2, "p_full": 0.25})
    with pytest.raises(ValueError):
        mcts.SelfPlay(4, 8, stub_evaluator, plane_dtype=torch.float32, packed_records=True, playout_cap={"full": 8, "fast": 2})
    sp = mcts.SelfPlay(4, 8, stub_evaluator, plane_dtype=torch.float32, keep_records=False,
                       playout_cap={"full": 2, "fast": 8, "p_full": 0.5, "quiet_fast": False})
    sp.play_ply()
    assert sp.quiet is None and set(sp.budget.tolist()) <= {2, 8} and sp.env.illegal_count() == 0
    sp.close()


# ------------------------------------------------------------------------------------------ 8. options that change nothing
@pytest.mark.gpu
def test_cap_that_is_always_full_plays_the_plain_games():
    out = []
    for cap in (None, {"full": 8, "fast": 8, "p_full": 1.0}):
        sp = mcts.SelfPlay(16, 8, stub_evaluator, seed=5, plane_dtype=torch.float32, game_ids=range(16), packed_records=True,
                           playout_cap=cap)
        _play_out(sp)
        assert sp.env.illegal_count() == 0 and sp.finished == 16
        out.append((sp.drain_finished_packed(), sp.finished_turns, sp.leaf_histogram()))
        sp.close()
    (plain, turns0, hist0), (capped, turns1, hist1) = out
    assert KEY not in plain and capped[KEY].all() and len(capped[KEY]) == len(capped["meta"])
    _same_packed(plain, {k: capped[k] for k in records.PACKED_KEYS})
    assert turns0 == turns1 and hist0 == hist1


# ------------------------------------------------------------------------------------------ 9. unequal sides
@pytest.mark.gpu
def test_arena_sides_search_with_their_own_simulations():
    L, check = _lib()
    G, sims_a, sims_b = 16, 12, 3
    rb, rh = _roots(G, seed=37, games=4, skip=20)
    turn = rb[:, 33]
    assert int(turn.min()) > 4 and bool((turn % 2 == 1).any()) and bool((turn % 2 == 0).any())
    a_white = torch.tensor([1, 0, 0, 1] * 4, dtype=torch.int8, device="cuda")
    own_a = (a_white != 0) == (turn % 2 == 1)
    assert 0 < int(own_a.sum()) < G
    ids = torch.arange(G, device="cuda") * 3 + 50
    budget = torch.zeros((G,), dtype=torch.int32, device="cuda")
    check(L.hive_arena_budget_launch(_p(rb), _p(a_white), G, sims_a, sims_b, _p(budget), _stream()))
    assert torch.equal(budget, torch.where(own_a, sims_a, sims_b).to(torch.int32))
    ar = mcts.ArenaSearch(G, sims_a, stub_evaluator, other_evaluator, a_white, plane_dtype=torch.float32, seed=9, slots=2)
    ar.set_game_ids(ids)
    got = _outputs(ar, ar.search(rb, rh, budgets=budget))
    assert ar.leaf_histogram().sum(1).tolist() == budget.tolist()
    ar.close()
    for evaluator, sims, own in ((stub_evaluator, sims_a, own_a), (other_evaluator, sims_b, ~own_a)):
        ts = mcts.TreeSearch(G, sims, evaluator, plane_dtype=torch.float32, seed=9, slots=2)
        ts.set_game_ids(ids)
        want = _outputs(ts, ts.search(rb, rh))
        ts.close()
        _same_rows(got, want, torch.nonzero(own).view(-1), sims)
        assert not torch.equal(_bits(got[1])[~own], _bits(want[1])[~own])       # the other side's games are searched differently


@pytest.mark.gpu
def test_arena_with_unequal_sides_runs_to_the_end():
    from hive_alphazero_amd.alpha_net import ChessNet, InferenceNet
    from hive_alphazero_amd.arena import Arena
    ar = Arena(stub_evaluator, other_evaluator, pairs=8, sims=12, sims_b=3, seed=3)
    assert ar.search.sims == 12 and ar.budget is not None
    res = ar.run()
    assert ar.illegal_count() == 0 and res.games == 16 and sorted(ar.results) == list(range(16))
    assert len(res.pair_scores) == 8 and res.wins + res.losses + res.draws + res.caps == 16
    hist = ar.search.leaf_histogram().sum().item()
    assert 0 < hist < ar.search.evals_launched                  # B's games sat out most of every search
    ar.close()
    # two networks that take the row flags: each side's rows follow its own simulations
    torch.manual_seed(0)
    weights = ChessNet().cuda().eval()
    nets = [InferenceNet(weights, dtype=torch.bfloat16) for _ in range(2)]
    ar = Arena(nets[0], nets[1], pairs=8, sims=3, sims_b=12, seed=3)
    assert ar.search.sims == 12
    for _ in range(12):
        ar.play_ply()
    rows_a, rows_b = ar.rows_evaluated()
    print(f"rows evaluated: A (3 simulations) {rows_a}, B (12 simulations) {rows_b}")
    assert ar.illegal_count() == 0 and 0 < rows_a < rows_b
    ar.close()


# ------------------------------------------------------------------------------------------ 10. the window
def _flagged_batch():
    """5 games of 7..20 rows with random flags; game 1 is all zeros, game 3 all ones."""
    lengths = [12, 7, 20, 9, 15]
    packed = synthetic_packed(41, lengths, [1, -1, 0, 1, -1])
    flags = (np.random.default_rng(42).random(sum(lengths)) < 0.45).astype(np.uint8)
    gp = packed["game_ptr"]
    flags[gp[1]:gp[2]] = 0
    flags[gp[3]:gp[4]] = 1
    packed[KEY] = flags
    return packed, np.flatnonzero(flags)


def _check_rows(state, packed, keep):
    assert np.array_equal(state["feat"], packed["feat"][keep]) and np.array_equal(state["hist"], packed["hist"][keep])
    assert np.array_equal(state["meta"], packed["meta"][keep])
    width = np.diff(packed["pol_ptr"])[keep]
    assert np.array_equal(state["pol_cnt"], width)
    for i, r in enumerate(keep):
        lo = int(packed["pol_ptr"][r])
        assert np.array_equal(state["pol_idx"][i, :width[i]], packed["pol_idx"][lo:lo + width[i]])
        assert np.array_equal(state["pol_val"][i, :width[i]], packed["pol_val"][lo:lo + width[i]])
        assert not state["pol_val"][i, width[i]:].any()
    assert np.array_equal(state["values"].view(np.uint32), records.packed_values(packed)[keep].view(np.uint32))


@pytest.mark.gpu
def test_window_takes_the_flagged_rows_with_whole_game_values():
    packed, keep = _flagged_batch()
    assert 10 < len(keep) < len(packed["meta"]) - 10
    buf = replay.ReplayBuffer(128)
    buf.add_packed(synthetic_packed(43, [5], [1]))              # the head is not at slot 0
    assert buf.add_packed(packed) == len(keep)
    assert len(buf) == 5 + len(keep) and buf.rows_seen == 5 + len(keep) and buf.games_seen == 6
    state = buf.state_dict()
    _check_rows({k: (v[5:] if getattr(v, "ndim", 0) else v) for k, v in state.items()}, packed, keep)
    # the dataset route picks the same rows
    planes, policies, values = buf.gather(np.arange(5, 5 + len(keep)))
    want = records.dataset_tensors_gpu_packed(packed)
    assert torch.equal(planes, want[0]) and torch.equal(policies, want[1]) and torch.equal(values, want[2])
    # a batch whose flags are all zero adds nothing
    none = dict(packed)
    none[KEY] = np.zeros_like(packed[KEY])
    assert buf.add_packed(none) == 0 and len(buf) == 5 + len(keep) and buf.games_seen == 11
    buf.close()
    # a window smaller than the kept rows keeps the newest of them
    cap = len(keep) - 7
    small = replay.ReplayBuffer(cap)
    small.add_packed(synthetic_packed(43, [5], [1]))
    assert small.add_packed(packed) == len(keep) and len(small) == cap and small.rows_seen == 5 + len(keep)
    _check_rows(small.state_dict(), packed, keep[-cap:])
    small.close()
    # without the key the ring fills exactly as before: every row, in order
    keyless = {k: packed[k] for k in records.PACKED_KEYS}
    plain = replay.ReplayBuffer(128)
    assert plain.add_packed(keyless) == len(packed["meta"]) == len(plain)
    _check_rows(plain.state_dict(), packed, np.arange(len(packed["meta"])))
    ones = dict(keyless)
    ones[KEY] = np.ones(len(packed["meta"]), np.uint8)
    flagged = replay.ReplayBuffer(128)
    assert flagged.add_packed(ones) == len(packed["meta"])
    a, b = plain.state_dict(), flagged.state_dict()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    plain.close(); flagged.close()
