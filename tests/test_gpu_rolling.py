"""Rolling search on the GPU: per-game clocks against their numpy statement, a game searched on its own clock against the
lock-step search of its budget (trees bit for bit), restarts that touch only their games, the masked policy, and whole
self-play games whose records equal the lock-step engine's per game id -- capped and plain, stub and real network."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from hive_alphazero_amd import mcts, records
from test_gpu_budgets import _bits, _outputs, _p, _roots, _same_rows, _same_tree, stub_evaluator

KEY = records.FULL_KEY
BUDGETS = [3, 8, 1, 5, 0, 8, 2, 6]
ACTIVE = [1, 1, 1, 1, 1, 0, 1, 1]
SIMS = 8
CAP = {"full": 8, "fast": 2, "p_full": 0.25}


def _i8(x):
    return torch.tensor(x, dtype=torch.int8, device="cuda")


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def _ids(G):
    return torch.arange(G, device="cuda") * 5 + 300


def _rolling(G, slots, mode=mcts.PUCT, budgets=BUDGETS, seed=9):
    ts = mcts.TreeSearch(G, SIMS, stub_evaluator, plane_dtype=torch.float32, seed=seed, slots=slots, mode=mode, rolling=True)
    ts.set_game_ids(_ids(G))
    if budgets is not None:
        ts.set_budgets(_i32(budgets))
    return ts


def _lock_step(rb, rh, slots, mode=mcts.PUCT, budgets=BUDGETS, active=ACTIVE, seed=9):
    """TreeSearch(sims=8) run in lock step with the same budgets -> (handle, its outputs)."""
    G = rb.shape[0]
    ts = mcts.TreeSearch(G, SIMS, stub_evaluator, plane_dtype=torch.float32, seed=seed, slots=slots, mode=mode)
    ts.set_game_ids(_ids(G))
    out = _outputs(ts, ts.search(rb, rh, active=_i8(active), budgets=_i32(budgets)))
    return ts, out


def _play_out(engine, limit=600):
    turns = 0
    while engine.running():
        engine.play_ply()
        turns += 1
        assert turns < limit
    torch.cuda.synchronize()


def _by_game(packed):
    """{game id: that game as a packed batch of its own}."""
    return {int(gid): records.slice_packed(packed, g, g + 1) for g, gid in enumerate(packed["game_id"].tolist())}


def _same_packed(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------ 1. clocks
@pytest.mark.gpu
@pytest.mark.parametrize("slots", [1, 3])
def test_clocks_and_done_follow_the_numpy_statement(slots):
    G = len(BUDGETS)
    rb, rh = _roots(G, seed=17, games=4, skip=12)
    ts = _rolling(G, slots)
    ts.restart(torch.ones(G, dtype=torch.int8), rb, rh, _i8(ACTIVE))
    assert ts.clocks().tolist() == [0] * G
    clock = np.zeros(G, dtype=np.int64)
    took_part = np.zeros(G, dtype=np.int64)
    for r in range(mcts.rolling_quantum(SIMS, slots) + 1):
        part, clock, done = mcts.rolling_clock_step(clock, BUDGETS, ACTIVE, slots)
        took_part += part.sum(1)
        got = ts.run_rounds(1)
        assert ts.clocks().tolist() == clock.tolist(), (slots, r)
        assert got.tolist() == done.astype(np.int8).tolist(), (slots, r)
        # a game that does not take part leaves no leaf of any kind: one histogram entry per simulation it ran
        hist = ts.leaf_histogram().cpu().numpy()
        assert hist.sum(1).tolist() == took_part.tolist() == clock.tolist(), (slots, r)
    assert clock.tolist() == [b if a else 0 for b, a in zip(BUDGETS, ACTIVE)]
    assert ts.node_counts().tolist()[4:6] == [0, 0]             # budget 0 and the idle game: no tree
    ts.close()


# ------------------------------------------------------------------------------------------ 2. same trees as lock step
@pytest.mark.gpu
@pytest.mark.parametrize("mode,slots", [(mcts.PUCT, 1), (mcts.PUCT, 3), (mcts.UCT, 1), (mcts.UCT, 3)])
def test_own_clock_gives_the_lock_step_tree(mode, slots):
    G = len(BUDGETS)
    rb, rh = _roots(G, seed=17, games=4, skip=12)
    ref, want = _lock_step(rb, rh, slots, mode)
    ts = _rolling(G, slots, mode)
    ts.restart(torch.ones(G, dtype=torch.int8), rb, rh, _i8(ACTIVE))
    done = ts.run_rounds(mcts.rolling_quantum(SIMS, slots))
    assert done.tolist() == ACTIVE
    got = _outputs(ts, ts.policy_where(torch.ones(G, dtype=torch.int8)))
    _same_rows(got, want, torch.arange(G, device="cuda"), (mode, slots))
    assert (got[0][[0, 1, 3, 7]] >= -1).all() and got[0][[4, 5]].tolist() == [-2, -2]
    for g in range(G):
        _same_tree(ts.export_tree(g), ref.export_tree(g), (mode, slots, g))
    assert torch.equal(ts.leaf_histogram(), ref.leaf_histogram())
    if mode == mcts.PUCT:
        # the noise key matters: the same search under another seed differs
        other, diff = _lock_step(rb, rh, slots, mode, seed=10)
        assert not torch.equal(_bits(diff[3]), _bits(want[3]))
        other.close()
    ts.close(); ref.close()


# ------------------------------------------------------------------------------------------ 3. restart
def _whole_tree(ts, g):
    """Every array of export_tree as bytes, the rows past nedge included."""
    t = ts.export_tree(g)
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in t.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [1, 3])
def test_restart_touches_only_its_games(slots):
    G = len(BUDGETS)
    budgets = [5, 8, 3, 6, 8, 8, 4, 6]
    active = [1] * G
    rb, rh = _roots(G, seed=17, games=4, skip=12)
    rb2, rh2 = _roots(G, seed=41, games=4, skip=16)
    which = _i8([0, 1, 0, 0, 1, 0, 0, 0])
    assert not torch.equal(rb2[1], rb[1]) and not torch.equal(rb2[4], rb[4])
    ts = _rolling(G, slots, budgets=budgets)
    ts.restart(torch.ones(G, dtype=torch.int8), rb, rh, _i8(active))
    ts.run_rounds(2)
    clocks = ts.clocks().tolist()
    assert 0 < clocks[1] < 8 and 0 < clocks[4] < 8               # mid-search
    others = [g for g in range(G) if g not in (1, 4)]
    before = {g: _whole_tree(ts, g) for g in others}
    ts.restart(which, rb2, rh2, _i8(active))
    assert {g: _whole_tree(ts, g) for g in others} == before
    now = ts.clocks().tolist()
    assert now[1] == now[4] == 0 and [now[g] for g in others] == [clocks[g] for g in others]
    assert ts.node_counts()[[1, 4]].tolist() == [0, 0]
    done = ts.run_rounds(mcts.rolling_quantum(SIMS, slots))
    assert done.tolist() == [1] * G
    got = _outputs(ts, ts.policy_where(torch.ones(G, dtype=torch.int8)))
    # the six: the lock-step search of the first roots; the two: the lock-step search of their new roots, same game ids
    first, want_first = _lock_step(rb, rh, slots, budgets=budgets, active=active)
    mixed_rb = torch.where(which.bool().view(G, 1), rb2, rb)
    mixed_rh = torch.where(which.bool().view(G, 1), rh2, rh)
    second, want_second = _lock_step(mixed_rb, mixed_rh, slots, budgets=budgets, active=active)
    _same_rows(got, want_first, torch.tensor(others, device="cuda"), "kept")
    _same_rows(got, want_second, torch.tensor([1, 4], device="cuda"), "restarted")
    for g in range(G):
        _same_tree(ts.export_tree(g), (second if g in (1, 4) else first).export_tree(g), (slots, g))
    assert not torch.equal(_bits(want_first[1])[[1, 4]], _bits(want_second[1])[[1, 4]])      # the new roots are other searches
    ts.close(); first.close(); second.close()


# ------------------------------------------------------------------------------------------ 4. policy_where
@pytest.mark.gpu
@pytest.mark.parametrize("selfplay", [0, 1])
def test_policy_where_answers_its_games_like_hive_search_policy(selfplay):
    from hive_alphazero_amd._lib import check
    G = len(BUDGETS)
    rb, rh = _roots(G, seed=17, games=4, skip=2)                # early turns: the self-play resampling is on (turn <= 6)
    assert int(rb[:, 33].min()) <= 6
    ts = _rolling(G, 1)
    ts.restart(torch.ones(G, dtype=torch.int8), rb, rh, _i8(ACTIVE))
    ts.run_rounds(SIMS)
    policy = torch.full((G, 1584), 7.0, device="cuda")
    action = torch.full((G,), 7, dtype=torch.int32, device="cuda")
    sum_n = torch.full((G,), 7, dtype=torch.int32, device="cuda")
    check(ts.L.hive_search_policy(ts._h, _p(policy), _p(action), _p(sum_n), selfplay))
    which = [1, 0, 1, 1, 1, 1, 0, 1]
    a, p, n = ts.policy_where(_i8(which), selfplay=bool(selfplay))
    rows = torch.tensor([g for g in range(G) if which[g]], device="cuda")
    out = torch.tensor([g for g in range(G) if not which[g]], device="cuda")
    assert torch.equal(a[rows], action[rows]) and torch.equal(n[rows], sum_n[rows])
    assert torch.equal(_bits(p)[rows], _bits(policy)[rows])
    assert (action[out] >= -1).all() and (sum_n[out] > 0).all()  # games hive_search_policy does answer
    assert a[out].tolist() == [-2, -2] and n[out].tolist() == [0, 0] and not p[out].any()
    # NULL policy / sum_n are optional here as there
    a2 = torch.full((G,), 7, dtype=torch.int32, device="cuda")
    check(ts.L.hive_search_policy_where(ts._h, _p(_i8(which)), None, _p(a2), None, selfplay))
    assert torch.equal(a2, a)
    ts.close()


# ------------------------------------------------------------------------------------------ 5. whole games, capped
def _capped(G, ids, rolling, slots=1, evaluator=stub_evaluator, plane_dtype=torch.float32, seed=21):
    sp = mcts.SelfPlay(G, SIMS, evaluator, seed=seed, slots=slots, plane_dtype=plane_dtype, game_ids=ids, packed_records=True,
                       playout_cap=CAP, rolling=rolling)
    _play_out(sp)
    assert sp.env.illegal_count() == 0 and sp.finished == G and sp.dropped_games == 0
    out = (_by_game(sp.drain_finished_packed()), sp.leaf_histogram(), sp.plies)
    sp.close()
    return out


@pytest.fixture(scope="module")
def lock_step_games():
    """The lock-step capped engine's games 0..31, one and two leaves in flight: computed once, left unchanged."""
    return {slots: _capped(32, range(32), None, slots) for slots in (1, 2)}


@pytest.mark.gpu
def test_rolling_capped_games_equal_lock_step_games(lock_step_games):
    want, want_hist, plies = lock_step_games[1]
    got, hist, turnovers = _capped(32, range(32), True)
    assert sorted(got) == sorted(want) == list(range(32))
    for gid in range(32):
        assert KEY in got[gid]
        _same_packed(got[gid], want[gid])
    assert hist == want_hist
    assert turnovers > plies                                    # `plies` counts turn-overs: a full ply takes four of them
    flags = np.concatenate([want[g][KEY] for g in range(32)])
    assert 0.1 < flags.mean() < 0.4


@pytest.mark.gpu
def test_rolling_games_do_not_depend_on_the_batch(lock_step_games):
    want = lock_step_games[1][0]
    got = _capped(48, list(reversed(range(48))), True)[0]
    assert sorted(got) == list(range(48))
    for gid in range(32):
        _same_packed(got[gid], want[gid])


@pytest.mark.gpu
def test_rolling_two_slots_one_round_per_turnover(lock_step_games):
    """Two leaves in flight change the search itself (collisions, virtual loss): the lock-step reference has two as well."""
    want, want_hist, _ = lock_step_games[2]
    got, hist, _ = _capped(32, range(32), {"quantum": 1}, slots=2)
    for gid in range(32):
        _same_packed(got[gid], want[gid])
    assert hist == want_hist


# ------------------------------------------------------------------------------------------ 6. whole games, no cap
@pytest.mark.gpu
def test_rolling_without_a_cap_plays_the_plain_games():
    out = []
    for rolling in (None, True):
        sp = mcts.SelfPlay(16, SIMS, stub_evaluator, seed=5, plane_dtype=torch.float32, game_ids=range(16), packed_records=True,
                           rolling=rolling)
        _play_out(sp)
        assert sp.env.illegal_count() == 0 and sp.finished == 16
        packed = sp.drain_finished_packed()
        assert KEY not in packed
        out.append((_by_game(packed), sorted(sp.finished_turns), sp.leaf_histogram()))
        sp.close()
    (plain, turns0, hist0), (rolled, turns1, hist1) = out
    assert sorted(plain) == sorted(rolled) == list(range(16))
    for gid in range(16):
        _same_packed(rolled[gid], plain[gid])
    assert turns0 == turns1 and hist0 == hist1


# ------------------------------------------------------------------------------------------ 7. live share
@pytest.mark.gpu
def test_no_round_has_a_hole_while_every_slot_holds_a_game():
    """The default quantum is the shorter search's rounds (2 for fast = 2, one slot): every game is either mid-search or was
    restarted at the turn-over, so every round every game runs a simulation.  A property of the clock rule."""
    G = 32
    sp = mcts.SelfPlay(G, SIMS, stub_evaluator, seed=21, plane_dtype=torch.float32, game_ids=itertools.count(), packed_records=True,
                       playout_cap=CAP, rolling=True)
    q = sp.rolling["quantum"]
    assert q == 2
    for t in range(40):
        sp.play_ply()
        assert sp.running() == G
        assert sum(sp.leaf_histogram().values()) == (t + 1) * q * G, t      # q rounds, G participating rows in each
    clocks, budget = sp.search.clocks(), sp.budget
    assert bool(((clocks > 0) & (clocks <= budget)).all())
    assert sp.search.evals_launched == sum(sp.leaf_histogram().values()) == 40 * q * G
    assert sp.env.illegal_count() == 0 and set(sp.budget.tolist()) == {2, 8}
    sp.close()


# ------------------------------------------------------------------------------------------ 8. refusals
@pytest.mark.gpu
def test_what_rolling_refuses():
    from hive_alphazero_amd._lib import HiveError
    with pytest.raises(ValueError):
        mcts.TreeSearch(4, SIMS, stub_evaluator, plane_dtype=torch.float32, rolling=True, keep_tree=True)
    with pytest.raises(ValueError):
        mcts.SelfPlay(4, SIMS, stub_evaluator, plane_dtype=torch.float32, rolling=True, search_options={"keep_tree": True})
    with pytest.raises(ValueError):
        mcts.SelfPlay(4, SIMS, stub_evaluator, plane_dtype=torch.float32, rolling={"rounds": 2})
    with pytest.raises(ValueError):
        mcts.ArenaSearch(4, SIMS, stub_evaluator, stub_evaluator, torch.ones(4, dtype=torch.int8, device="cuda"),
                         plane_dtype=torch.float32, rolling=True)
    rb, rh = _roots(4, seed=17, games=2, skip=6)
    ts = _rolling(4, 1, budgets=None)
    ts.restart(torch.ones(4, dtype=torch.int8), rb, rh)
    E_ARG = -1
    assert ts.L.hive_search_select(ts._h, 0, _p(ts.leaf_boards), _p(ts.leaf_hist)) == E_ARG        # no budgets
    assert b"budget" in ts.L.hive_last_error()
    assert ts.L.hive_search_advance_roots(ts._h, None, _p(rb), _p(rh), None) == E_ARG              # moves all trees at once
    with pytest.raises(HiveError):
        ts.run_rounds(1)
    ts.set_budgets(_i32([2, 2, 2, 2]))
    assert ts.run_rounds(2).tolist() == [1, 1, 1, 1]
    ts.close()
    plain = mcts.TreeSearch(4, SIMS, stub_evaluator, plane_dtype=torch.float32, seed=9)
    plain.set_game_ids(_ids(4))
    with pytest.raises(ValueError):
        plain.run_rounds(1)
    assert plain.L.hive_search_round_end(plain._h, 1, _p(torch.zeros(4, dtype=torch.int8, device="cuda"))) == E_ARG
    # rolling switched off again: the handle searches in lock step, on the host counter, like one that never rolled
    back = _rolling(4, 1, budgets=None)
    assert back.L.hive_search_set_rolling(back._h, 0) == 0
    _same_rows(_outputs(back, back.search(rb, rh)), _outputs(plain, plain.search(rb, rh)), torch.arange(4, device="cuda"), "off")
    plain.close(); back.close()


# ------------------------------------------------------------------------------------------ 9. real network
@pytest.mark.gpu
def test_rolling_equals_lock_step_with_a_real_network():
    """Desynchronised games meet other neighbours in every leaf batch: the records only stay equal because the network gives
    a position the same bits at any row of any batch."""
    from hive_alphazero_amd.alpha_net import ChessNet, InferenceNet
    torch.manual_seed(0)
    net = InferenceNet(ChessNet().cuda().eval(), dtype=torch.bfloat16)
    assert getattr(net, "batch_independent_bits", False)
    want = _capped(16, range(16), None, evaluator=net, plane_dtype=None, seed=3)[0]
    got = _capped(16, range(16), True, evaluator=net, plane_dtype=None, seed=3)[0]
    assert sorted(got) == sorted(want) == list(range(16))
    for gid in range(16):
        _same_packed(got[gid], want[gid])
